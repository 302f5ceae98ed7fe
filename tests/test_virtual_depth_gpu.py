"""GPU (-m gpu): virtual depth planes (include/rtuf.h, VIRTUAL DEPTH; rtuf_render_batch*).

The expectation is bench_support/virtual_check.py on the CPU oracle's debug planes: num / (zwin - off) in numpy float32 where a
link's triangle won (prim >= 0), the empty value elsewhere; the 16UC1 form through the restated metres_to_u16.  tests/
test_virtual_depth_cpu.py shows that this arithmetic is the oracle's own.  Every comparison is bit for bit (NaN patterns
through isnan on both sides); labels are compared with labels_check.expected_labels.

Run as a script (RTUF_SMALL_LAUNCH=0 python tests/test_virtual_depth_gpu.py) the route checks go through the 256-thread tile
kernels: the threshold is read once per process, so test_every_route_256_thread_kernels starts one."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import realtime_urdf_filter_amd as R
from bench_support import configs as CF
from bench_support.labels_check import expected_labels, share_draws
from bench_support.virtual_check import bits_equal_f32, expected_virtual, metres_to_u16
from gpu_support import (Consumer, OracleScene, bits_equal, compare_labels, fixture_scene, label_planes, oracle_frames, params, quad, same_planes,
                         share_frames, tie_scene, torch_device, undrawn_scene, virtual_planes)

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -6
SENTINEL = -7.25            # fill of the f32 planes before a call (0x5a5a in the uint16 planes)

FIXTURES = ["soup_seed11_160x120", "soup_seed12_160x120", "soup_seed13_160x120", "mesh_links_seed21_160x120", "primitives_160x120",
            "near_range_ties_160x120", "far_plane_covers_160x120", "far_plane_covers_background_160x120", "near_large_shapes_517x389"]


def scene(name):
    return undrawn_scene() if name == "undrawn" else fixture_scene(name, 3)


def planes(sc, total=None, u16=False, labels=True):
    """Device planes of `total` streams with their sentinel fill."""
    torch, dev = torch_device()
    shape = (total or sc.n, sc.H, sc.W)
    v = torch.full(shape, 0x5a5a, dtype=torch.int16, device=dev) if u16 else torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)
    lab = torch.full(shape, 0x5a5a, dtype=torch.int16, device=dev) if labels else None
    torch.cuda.synchronize()          # the fills run on torch's stream, which the library's streams do not wait for: a late one would overwrite a batch's pixels
    return v, lab


def host(v, lab=None):
    a = v.cpu().numpy()
    return (a.view(np.uint16) if a.dtype == np.int16 else a), (lab.cpu().numpy().view(np.uint16) if lab is not None else None)


def render_device(ctx, sc, empty=0.0, u16=False, labels=True, n=None, total=None):
    v, lab = planes(sc, total, u16, labels)
    fn = ctx.render_batch_device_u16 if u16 else ctx.render_batch_device
    fn(n or sc.n, v.data_ptr(), lab.data_ptr() if labels else None, empty)
    ctx.sync()
    return host(v, lab)


# ---- every route ------------------------------------------------------------------------------------------------------------

def route_checks(name, lanes):
    sc = scene(name)
    ctx = sc.context(raster_lanes=lanes)
    want_lab = label_planes(sc)
    for rep in range(2):                       # (the second round runs after the cover pass has gone to sleep where no tile has a cover)
        for u16 in ((False, True) if sc.W % 4 == 0 else (False,)):
            for labels in (True, False):
                what = "%s lanes %d %s labels %d" % (name, lanes, "16UC1" if u16 else "f32", labels)
                v, lab = render_device(ctx, sc, empty=-1.5 if u16 else 0.25, u16=u16, labels=labels)
                same_planes(v, virtual_planes(sc, -1.5 if u16 else 0.25, u16), what + " device")
                if labels:
                    compare_labels(lab, want_lab, what + " device")
                v, lab = ctx.render_batch(sc.n, 3.0, labels=labels, u16=u16)
                same_planes(v, virtual_planes(sc, 3.0, u16), what + " host")
                if labels:
                    compare_labels(lab, want_lab, what + " host")
        assert ctx.stats()["batch_status"] == 0
    st = ctx.stats()
    if name.startswith("near_range_ties"):
        assert st["exact_tiles"] > 0, st
    # (at 160x120 no triangle of the far_plane_covers scenes covers a whole 64x32 tile: cover and cover-only tiles are met in
    # test_ties_go_to_the_earlier_draw's cover cases and in test_config3_256_streams)
    ctx.close()


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("name", FIXTURES)
def test_every_route(name, lanes):
    route_checks(name, lanes)


def test_every_route_256_thread_kernels():
    """The same checks with RTUF_SMALL_LAUNCH=0: every launch takes the 256-thread tile kernels."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=600,
                       env=dict(os.environ, RTUF_SMALL_LAUNCH="0"))
    assert r.returncode == 0 and "routes ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- empty values -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["soup_seed11_160x120", "undrawn"])
def test_empty_values(name):
    sc = scene(name)
    ctx = sc.context()
    drawn = sc.prim >= 0
    if name == "undrawn":                      # no link in view: undrawn pixels, and a background quad drawn as geometry -- empty, both
        assert (sc.prim == -1).any() and (sc.prim == -2).any()
    else:
        assert drawn.any() and (sc.prim == -2).any()
    first = {}
    for e in (0.0, -1.5, float("inf"), float("nan")):
        for u16 in (False, True):
            v, _ = render_device(ctx, sc, empty=e, u16=u16, labels=False)
            same_planes(v, virtual_planes(sc, e, u16), "%s empty %r u16 %d" % (name, e, u16))
            want_e = metres_to_u16(np.float32(e)) if u16 else np.float32(e)
            got_e = v[~drawn]
            assert (np.isnan(got_e).all() if (not u16 and np.isnan(e)) else (got_e == want_e).all()), (e, u16)
            ref = first.setdefault(u16, v)
            assert np.array_equal(ref[drawn], v[drawn]), (e, u16)       # the same virtual pixels whatever the empty value
    ctx.close()


# ---- agreement with the filter on the same context --------------------------------------------------------------------------

def far_quad_scene():
    """Two links in front of a third: a quad at 0.99 * far, the depth of the background quad, which is drawn first."""
    far = float(np.float32(0.99) * np.float32(8.0))
    tie = tie_scene([[quad(-0.5, -0.3, -0.3, 0.3, 1.2), quad(-0.2, 0.2, -0.15, 0.15, 1.0), quad(-20.0, 20.0, -20.0, 20.0, far)]])
    depth = np.linspace(0.5, 9.0, tie.W * tie.H, dtype=np.float32).reshape(1, tie.H, tie.W)
    return OracleScene(tie.wl, depth)


@pytest.mark.parametrize("far_quad", [False, True])
def test_agrees_with_the_filter_on_the_same_context(far_quad):
    torch, dev = torch_device()
    sc = far_quad_scene() if far_quad else scene("soup_seed12_160x120")
    ctx = sc.context()
    d = torch.from_numpy(sc.depth).to(dev)
    m, k = torch.empty_like(d), torch.empty(d.shape, dtype=torch.uint8, device=dev)
    _, flab = planes(sc)
    ctx.filter_batch_device_labels(sc.n, d.data_ptr(), m.data_ptr(), k.data_ptr(), flab.data_ptr())
    v, lab = render_device(ctx, sc, empty=float("nan"))
    flab, mask = flab.cpu().numpy().view(np.uint16), k.cpu().numpy()
    assert np.array_equal(flab, lab)
    compare_labels(lab, label_planes(sc), "labels")
    same_planes(v, virtual_planes(sc, float("nan")), "virtual")
    assert np.isnan(v[sc.prim < 0]).all()      # the background quad, drawn by the library or met at its own depth, reads the empty value
    with np.errstate(invalid="ignore"):
        robot = (lab > 0) & (sc.depth > v - np.float32(sc.wl.max_diff))
    plain = (lab == 0) & (sc.mask == 255)      # label 0: the plain filter (the oracle's) decides
    assert np.array_equal(mask == 255, robot | plain)
    assert np.array_equal(mask, sc.mask)
    ctx.close()


# ---- ties go to the earlier draw ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["links", "models", "cover_links", "cover_models", "near_links", "near_models"])
def test_ties_go_to_the_earlier_draw(case):
    if case.startswith("cover"):
        q = quad(-3.0, 3.0, -3.0, 3.0, 1.5)
    elif case.startswith("near"):
        q = quad(-0.02, 0.02, -0.015, 0.015, 0.100003)
    else:
        q = quad(-0.2, 0.2, -0.15, 0.15, 1.0)
    other = quad(-0.5, -0.3, -0.3, 0.3, 1.2)
    geo = [[other, q], [q]] if case.endswith("models") else [[other, q, q]]
    tie = tie_scene(geo)
    sc = OracleScene(tie.wl, tie.depth)
    ctx = sc.context()
    labels = [5, 7, 3]
    if case.endswith("models"):
        ctx.set_link_labels(sc.ids[0], np.array(labels[:2], np.uint16))
        ctx.set_link_labels(sc.ids[1], np.array(labels[2:], np.uint16))
    else:
        ctx.set_link_labels(sc.ids[0], np.array(labels, np.uint16))
    want = label_planes(sc, np.array(labels))
    assert (want == 7).sum() > 50 and not (want == 3).any()
    for u16 in (False, True):
        v, lab = render_device(ctx, sc, empty=0.0, u16=u16)
        same_planes(v, virtual_planes(sc, 0.0, u16), case)
        compare_labels(lab, want, case)
    st = ctx.stats()
    assert not case.startswith("near") or st["exact_tiles"] > 0, st
    assert not case.startswith("cover") or st["cover_tiles"] > 0, st
    ctx.close()


# ---- batch rules -------------------------------------------------------------------------------------------------------------

def test_partial_batch_leaves_the_other_planes_alone():
    sc = scene("mesh_links_seed21_160x120")
    ctx = sc.context(max_streams=5, n=3)
    for u16 in (False, True):
        v, lab = render_device(ctx, sc, empty=1.0, u16=u16, n=3, total=5)
        same_planes(v[:3], virtual_planes(sc, 1.0, u16), "partial")
        compare_labels(lab[:3], label_planes(sc), "partial")
        assert (v[3:] == (0x5a5a if u16 else np.float32(SENTINEL))).all() and (lab[3:] == 0x5a5a).all()
    ctx.close()


def test_pipelines_render_and_filter_batches_alternate():
    torch, dev = torch_device()
    sc = scene("soup_seed13_160x120")
    ctx = sc.context(pipelines=2)
    d = torch.from_numpy(sc.depth).to(dev)
    rounds = []
    for i in range(3):
        v, lab = planes(sc)
        m, k = torch.empty_like(d), torch.empty(d.shape, dtype=torch.uint8, device=dev)
        ctx.render_batch_device(sc.n, v.data_ptr(), lab.data_ptr(), float(i))          # two batches in flight, on two pipelines
        ctx.filter_batch_device(sc.n, d.data_ptr(), m.data_ptr(), k.data_ptr())
        rounds.append((v, lab, m, k))
    ctx.sync()
    for i, (v, lab, m, k) in enumerate(rounds):
        same_planes(v.cpu().numpy(), virtual_planes(sc, float(i)), "round %d" % i)
        compare_labels(lab.cpu().numpy().view(np.uint16), label_planes(sc), "round %d" % i)
        assert np.array_equal(k.cpu().numpy(), sc.mask) and bits_equal(m.cpu().numpy(), sc.masked), i
    ctx.close()


def test_regrown_bins_rerun_the_render_batch():
    sc = scene("mesh_links_seed21_160x120")
    ctx = sc.context(bin_capacity=1)
    v, lab = planes(sc)
    ctx.render_batch_device(sc.n, v.data_ptr(), lab.data_ptr(), -1.5)
    ctx.sync()
    st = ctx.stats()
    assert st["regrowths"] > 0 and st["batch_reruns"] > 0 and st["batch_status"] != 0, st
    v, lab = host(v, lab)
    same_planes(v, virtual_planes(sc, -1.5), "re-run")
    compare_labels(lab, label_planes(sc), "re-run")
    v, _ = ctx.render_batch(sc.n, 2.0, u16=True)
    same_planes(v, virtual_planes(sc, 2.0, True), "after the re-run")
    ctx.close()


def test_graph_replay_picks_up_a_new_empty_value_and_new_buffers():
    """One raster lane, pipelines = 2, one stream: small batches replay a captured graph.  TileArgs is hashed into the plan, so
    another empty value or buffer must capture anew and never write the old buffer."""
    sc = scene("primitives_160x120")
    ctx = sc.context(max_streams=1, n=1, raster_lanes=1, pipelines=2)
    want_lab = label_planes(sc)[:1]
    va, la = planes(sc, 1)
    vb, lb = planes(sc, 1)

    def run(v, lab, e, what):
        ctx.render_batch_device(1, v.data_ptr(), lab.data_ptr(), e)
        ctx.sync()
        gv, gl = host(v, lab)
        same_planes(gv, virtual_planes(sc, e)[:1], what)
        compare_labels(gl, want_lab, what)
    for i in range(6):
        run(va, la, 0.5, "repeat %d" % i)
    run(va, la, 4.0, "new empty value")
    run(va, la, 4.0, "new empty value, replayed")
    va.fill_(SENTINEL)
    run(vb, la, 4.0, "new virtual buffer")
    run(vb, la, 4.0, "new virtual buffer, replayed")
    assert (va.cpu().numpy() == np.float32(SENTINEL)).all()            # the old buffer is not written again
    la.fill_(0x5a5a)
    run(vb, lb, 4.0, "new label buffer")
    run(vb, lb, 4.0, "new label buffer, replayed")
    assert (la.cpu().numpy() == 0x5a5a).all()
    st = ctx.stats()
    assert st["graphs_enabled"] == 1 and st["graph_hits"] > 0, st
    ctx.close()


def test_status_word_is_zero_behind_a_final_render_batch():
    sc = scene("soup_seed11_160x120")
    ctx = sc.context()
    ctx.render_batch(sc.n)                     # (bins sized)
    v, lab = planes(sc)
    user = Consumer(ctx)
    ctx.render_batch_device(sc.n, v.data_ptr(), lab.data_ptr(), 0.0)
    word, early_v, early_lab, word_t = user.read(v, lab)
    assert word == 0, hex(word)
    same_planes(early_v, virtual_planes(sc, 0.0), "behind the batch")
    compare_labels(early_lab.view(np.uint16), label_planes(sc), "behind the batch")
    ctx.sync()
    st = ctx.stats()
    assert st["batch_status"] == 0 and st["batch_reruns"] == 0, st
    ctx.close()


def test_timings_land_in_ms_raster():
    sc = scene("soup_seed11_160x120")
    ctx = sc.context()
    ctx.enable_timing(1)
    ctx.render_batch(sc.n)
    st = ctx.stats()
    assert st["ms_raster"] > 0 and st["ms_compare"] == 0, st
    ctx.close()


# ---- refusals, and contexts whose filter batches take other routes ---------------------------------------------------------

def test_refusals_write_nothing_and_leave_the_context_usable():
    torch, dev = torch_device()
    sc = scene("soup_seed12_160x120")
    p = params(replace=sc.wl.replace_value, max_diff=sc.wl.max_diff)
    p.near_plane, p.far_plane = sc.wl.near, sc.wl.far
    ctx = R.Context(sc.W, sc.H, sc.n, 0, p)
    v, lab = planes(sc)

    def refused(code, call):
        with pytest.raises(R.RtufError) as e:
            call()
        assert e.value.code == code, e.value
    refused(STATE, lambda: ctx.render_batch_device(sc.n, v.data_ptr(), lab.data_ptr(), 0.0))        # before finalize
    ids = sc.wl.load_into(ctx)
    sc.wl.stage(ctx, ids)
    refused(INVALID, lambda: ctx.render_batch_device(sc.n, None, lab.data_ptr(), 0.0))             # NULL plane
    refused(INVALID, lambda: ctx.render_batch_device_u16(sc.n, None, None, 0.0))
    refused(INVALID, lambda: ctx.render_batch_device(0, v.data_ptr(), lab.data_ptr(), 0.0))        # n out of range
    refused(INVALID, lambda: ctx.render_batch_device(sc.n + 1, v.data_ptr(), lab.data_ptr(), 0.0))
    refused(INVALID, lambda: ctx.render_batch(sc.n + 1))
    p.silhouette_dilation_px = 2
    ctx.set_params(p)
    refused(INVALID, lambda: ctx.render_batch_device(sc.n, v.data_ptr(), lab.data_ptr(), 0.0))     # silhouette dilation: not supported yet
    refused(INVALID, lambda: ctx.render_batch_device_u16(sc.n, v.data_ptr(), None, 0.0))
    refused(INVALID, lambda: ctx.render_batch(sc.n, labels=True))
    ctx.sync()
    torch.cuda.synchronize()
    assert (v.cpu().numpy() == np.float32(SENTINEL)).all() and (lab.cpu().numpy() == 0x5a5a).all()
    p.silhouette_dilation_px = 0
    ctx.set_params(p)
    gv, gl = render_device(ctx, sc, empty=0.0)
    same_planes(gv, virtual_planes(sc, 0.0), "after the refusals")
    compare_labels(gl, label_planes(sc), "after the refusals")
    masked, mask = ctx.filter_batch(sc.depth)
    assert np.array_equal(mask, sc.mask) and bits_equal(masked, sc.masked)
    ctx.close()


@pytest.mark.parametrize("kind", ["two_kernel", "link_thresholds"])
def test_contexts_with_other_filter_routes_render_and_filter_as_before(kind):
    sc = scene("soup_seed13_160x120")
    ctx = sc.context(flags=R.FLAG_TWO_KERNEL if kind == "two_kernel" else 0)
    if kind == "link_thresholds":
        ctx.set_link_thresholds(sc.ids[0], np.linspace(-0.1, 0.3, ctx.num_links(sc.ids[0])).astype(np.float32))
    before = ctx.filter_batch(sc.depth)
    zs = ctx.read_zsurface(sc.n) if kind == "two_kernel" else None
    if kind == "two_kernel":
        assert np.array_equal(before[1], sc.mask) and bits_equal(before[0], sc.masked)
    for u16 in (False, True):
        v, lab = render_device(ctx, sc, empty=0.0, u16=u16)
        same_planes(v, virtual_planes(sc, 0.0, u16), kind)
        compare_labels(lab, label_planes(sc), kind)
    v, lab = ctx.render_batch(sc.n, 1.0, labels=True)
    same_planes(v, virtual_planes(sc, 1.0), kind + " host")
    if zs is not None:                         # the z-surface still shows the last filter batch
        assert bits_equal_f32(ctx.read_zsurface(sc.n), zs)
    after = ctx.filter_batch(sc.depth)
    assert np.array_equal(after[1], before[1]) and bits_equal(after[0], before[0])
    ctx.close()


# ---- real size ---------------------------------------------------------------------------------------------------------------

def test_config3_256_streams():
    share = CF.build("c3", 1, 0)
    n = share.n
    wl0 = share.wl0
    ctx = R.Context(share.width, share.height, n, 0, params(replace=wl0.replace_value, max_diff=wl0.max_diff))
    share.load(ctx)
    share.stage(ctx, 0)
    torch, dev = torch_device()
    v = torch.full((n, share.height, share.width), SENTINEL, dtype=torch.float32, device=dev)
    lab = torch.full((n, share.height, share.width), 0x5a5a, dtype=torch.int16, device=dev)
    ctx.render_batch_device(n, v.data_ptr(), lab.data_ptr(), -1.0)
    ctx.sync()                                 # (a context's first batch sizes its bins: the planes are final once it is retired)
    sample = [0, 1, 85, 170, n - 1]
    depth = np.ascontiguousarray(share.depth_host(0), np.float32)
    frames = share_frames(share, ctx, n)
    zwin, prim = oracle_frames([frames[s] for s in sample], depth[sample])
    gv, gl = v[sample].cpu().numpy(), lab[sample].cpu().numpy().view(np.uint16)
    want_v = expected_virtual(zwin, prim, wl0.near, wl0.far, -1.0)
    want_l = np.stack([expected_labels(p, *share_draws(share, s)) for p, s in zip(prim, sample)])
    same_planes(gv, want_v, "C3")
    compare_labels(gl, want_l, "C3")
    assert (want_l > 0).any() and (want_v == -1.0).any()
    ctx.close()


if __name__ == "__main__":
    for fixture in FIXTURES:
        route_checks(fixture, 1)
    print("routes ok")
