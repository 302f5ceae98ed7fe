"""GPU (-m gpu): link label planes (include/rtuf.h, LINK LABELS; rtuf_filter_batch*_labels, rtuf_set_link_labels).

The expectation maps the CPU oracle's winning source triangle (`prim`) through the draw list it was given: draw -> link ->
label, 0 where the background quad won or nothing was drawn (bench_support/labels_check.py).  Every pixel of every stream is
compared, 0 mismatches.  The planes the label calls write are compared bit for bit with their counterparts' output."""
import numpy as np
import pytest

import golden_io
import realtime_urdf_filter_amd as R
from bench_support import configs as CF
from bench_support import workloads as WL
from bench_support.labels_check import expected_labels, share_draws
from gpu_support import OracleScene, compare_labels, label_planes, oracle_frames, params, quad, share_frames, soup_scene, tie_scene, torch_device
from realtime_urdf_filter_amd.filter import depth_f32_to_u16

pytestmark = pytest.mark.gpu
INVALID = -1


def run_host(ctx, depth, u16=False, want_mask=True):
    """(labels call, counterpart) on host planes: planes bit for bit equal, returns the labels."""
    d = depth_f32_to_u16(depth) if u16 else depth
    m, k, lab = ctx.filter_batch_labels(d, want_mask=want_mask)
    m0, k0 = (ctx.filter_batch_u16 if u16 else ctx.filter_batch)(d, want_mask=want_mask)
    assert np.array_equal(np.asarray(m).view(np.uint16 if u16 else np.uint32), np.asarray(m0).view(np.uint16 if u16 else np.uint32))
    assert (k is None and k0 is None) or np.array_equal(k, k0)
    return lab


def run_device(ctx, depth, u16=False, with_mask=True):
    torch, dev = torch_device()
    n = depth.shape[0]
    if u16:
        d = torch.from_numpy(depth_f32_to_u16(depth).view(np.int16)).to(dev)
    else:
        d = torch.from_numpy(depth).to(dev)
    outs = []
    for labels in (True, False):
        m = torch.empty_like(d)
        k = torch.empty(d.shape, dtype=torch.uint8, device=dev) if with_mask else None
        if labels:
            lab = torch.full(d.shape, 0x5a5a, dtype=torch.int16, device=dev)
            ctx.filter_batch_device_labels(n, d.data_ptr(), m.data_ptr(), k.data_ptr() if with_mask else None, lab.data_ptr(), u16=u16)
        elif u16:
            ctx.filter_batch_device_u16(n, d.data_ptr(), m.data_ptr(), k.data_ptr() if with_mask else None)
        else:
            ctx.filter_batch_device(n, d.data_ptr(), m.data_ptr(), k.data_ptr() if with_mask else None)
        ctx.sync()
        outs.append((m.cpu().numpy(), k.cpu().numpy() if with_mask else None, lab.cpu().numpy().view(np.uint16) if labels else None))
    (m1, k1, lab), (m0, k0, _) = outs
    assert np.array_equal(m1.view(np.uint16 if u16 else np.uint32), m0.view(np.uint16 if u16 else np.uint32)), "device planes differ"
    assert (k1 is None) or np.array_equal(k1, k0)
    return lab


# ---- golden fixtures ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("two_kernel", [False, True])
@pytest.mark.parametrize("name", golden_io.fixture_names())
def test_golden_fixture_labels(name, two_kernel):
    """One link per draw (golden_io.Fixture.load_into): label = 1 + draw index.  The masked / mask planes of the label call
    are still the reference's."""
    fx = golden_io.Fixture(name)
    p = params(fx.replace_value, fx.max_diff, near_plane=fx.z_near, far_plane=fx.z_far)
    if two_kernel:
        p.flags |= R.FLAG_TWO_KERNEL
    ctx = R.Context(fx.width, fx.height, 1, 0, p)
    m, tfs = fx.load_into(ctx)
    ctx.set_camera(0, fx.projection, fx.offset_inv, fx.cam_tf)
    if len(tfs):
        ctx.set_link_poses(0, m, tfs)
    masked, mask, lab = ctx.filter_batch_labels(fx.depth[None])
    fx.check(masked[0], mask[0])
    prim = oracle_frames([(fx.projection, fx.draws, fx.offset_inv, fx.cam_tf, fx.z_near, fx.z_far)], fx.depth[None])[1]
    want = expected_labels(prim[0], np.arange(1, len(fx.draws) + 1), [len(d[4]) for d in fx.draws])[None]
    compare_labels(lab, want, name)
    ctx.close()


# ---- the matrix: routes, element types, entry points, lanes --------------------------------------------------------------

_scenes = {}


def scene(name):
    if name not in _scenes:
        if name == "c1_640x480":
            wl = WL.example_workload(640, 480)
            _scenes[name] = OracleScene(wl, wl.depth_batch())
        elif name == "soup_517x389":
            _scenes[name] = soup_scene(2, 517, 389, n=2)
        elif name == "pr2_near_walls":
            wl = WL.pr2_workload(3, 640, 480, total_triangles=40000, near_arm=True, walls=True)
            _scenes[name] = OracleScene(wl, wl.depth_batch())
    return _scenes[name]


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("two_kernel", [False, True])
@pytest.mark.parametrize("name", ["c1_640x480", "soup_517x389", "pr2_near_walls"])
def test_labels_every_route(name, two_kernel, lanes):
    sc = scene(name)
    ctx = sc.context(flags=R.FLAG_TWO_KERNEL if two_kernel else 0, raster_lanes=lanes)
    want = label_planes(sc)
    compare_labels(run_host(ctx, sc.depth), want, "%s host f32" % name)
    compare_labels(run_host(ctx, sc.depth, want_mask=False), want, "%s host f32 without mask" % name)
    compare_labels(run_device(ctx, sc.depth), want, "%s device f32" % name)
    compare_labels(run_device(ctx, sc.depth, with_mask=False), want, "%s device f32 without mask" % name)
    if sc.W % 4 == 0:
        compare_labels(run_host(ctx, sc.depth, u16=True), want, "%s host 16UC1" % name)
        compare_labels(run_device(ctx, sc.depth, u16=True), want, "%s device 16UC1" % name)
    assert ctx.stats()["batch_status"] == 0
    if name == "pr2_near_walls":
        st = ctx.stats()
        assert st["exact_tiles"] > 0 and st["cover_tiles"] > 0, st
    ctx.close()


@pytest.mark.parametrize("two_kernel", [False, True])
def test_pipelines_and_partial_batches(two_kernel):
    """pipelines = 2 (the child contexts take turns), and a partial batch: max_streams 64, max_inflight_streams 8, n = 49."""
    wl = WL.pr2_workload(49, 320, 240, total_triangles=20000, near_arm=True)
    sc = OracleScene(wl, wl.depth_batch())
    want = label_planes(sc)
    flags = R.FLAG_TWO_KERNEL if two_kernel else 0
    ctx = sc.context(flags=flags, pipelines=2)
    for _ in range(3):
        compare_labels(run_device(ctx, sc.depth), want, "pipelines=2 device")
        compare_labels(run_host(ctx, sc.depth), want, "pipelines=2 host")
    ctx.close()
    ctx = sc.context(max_streams=64, n=49, flags=flags, max_inflight_streams=8)
    compare_labels(run_device(ctx, sc.depth), want, "partial batch device")
    compare_labels(run_host(ctx, sc.depth, u16=True), want, "partial batch host 16UC1")
    ctx.close()


# ---- BASELINE configs ---------------------------------------------------------------------------------------------------

def run_share(share, n, two_kernel=False, link_label=None, custom=None):
    """Loads a RankShare, filters step 0 through the device labels call, returns (labels, expected labels)."""
    p = params(replace=share.wl0.replace_value, max_diff=share.wl0.max_diff)
    if two_kernel:
        p.flags |= R.FLAG_TWO_KERNEL
    ctx = R.Context(share.width, share.height, n, 0, p)
    share.load(ctx)
    if custom:
        custom(ctx)
    share.stage(ctx, 0)
    depth = np.ascontiguousarray(share.depth_host(0), np.float32)
    lab = run_device(ctx, depth)
    prim = oracle_frames(share_frames(share, ctx, n), depth)[1]
    want = np.stack([expected_labels(prim[s], *share_draws(share, s, link_label)) for s in range(n)])
    st = ctx.stats()
    ctx.close()
    return lab, want, st


def test_config3_256_streams():
    share = CF.build("c3", 1, 0)
    lab, want, _ = run_share(share, share.n)
    compare_labels(lab, want, "C3")
    assert len(np.unique(want)) > 20


@pytest.mark.parametrize("two_kernel", [False, True])
def test_config3_near_arm(two_kernel):
    share = CF.build("c3", 1, 0, streams=16, near_arm=True)
    lab, want, st = run_share(share, share.n, two_kernel)
    compare_labels(lab, want, "C3 near-arm")
    assert st["exact_tiles"] > 0


def test_config4_share_720p_walls():
    share = CF.build("c4", 8, 0, streams=64)
    lab, want, st = run_share(share, share.n)
    compare_labels(lab, want, "C4 share")
    assert st["cover_tiles"] > 0
    # the walls are links of their own models: their labels show
    wall_models = share.groups[0].model_ids[1:]
    wall_labels = [1 + share.link_base[m] + li for m in wall_models for li in range(len(share.groups[0].variants[0].models[share.groups[0].model_ids.index(m)]))]
    assert np.isin(want, wall_labels).any()


def test_config5_share_several_models():
    share = CF.build("c5", 8, 0, per_urdf=8)
    lab, want, _ = run_share(share, share.n)
    compare_labels(lab, want, "C5 share")
    # every stream shows only its own robot's links
    for g in share.groups:
        lo = 1 + share.link_base[g.model_ids[0]]
        hi = lo + len(g.variants[0].models[0])
        v = want[g.first:g.first + g.count]
        assert ((v == 0) | ((v >= lo) & (v < hi))).all()


def test_config5_custom_labels_group_links_per_robot():
    """rtuf_set_link_labels on every model: all links of robot i share label 100 + i."""
    share = CF.build("c5", 8, 0, per_urdf=4)

    def custom(ctx):
        for i, g in enumerate(share.groups):
            ctx.set_link_labels(g.model_ids[0], np.full(len(g.variants[0].models[0]), 100 + i, np.uint16))
    lab, _, _ = run_share(share, share.n, custom=custom)
    link_label = np.zeros(share.n_links_total, np.int64)
    for i, g in enumerate(share.groups):
        link_label[share.link_base[g.model_ids[0]]:share.link_base[g.model_ids[0]] + len(g.variants[0].models[0])] = 100 + i
    # (the context's labels against the same oracle prims mapped through the custom table: the default-label run above
    # already pinned the prims, so here the robot of every stream is checked to carry its group's label only)
    for s in range(share.n):
        i = share.groups.index(share.group_of(s))
        assert set(np.unique(lab[s])) <= {0, 100 + i}
        assert (lab[s] > 0).any()


# ---- ties: identical triangles, the earlier draw's label wins -------------------------------------------------------------

@pytest.mark.parametrize("two_kernel", [False, True])
@pytest.mark.parametrize("case", ["links", "models", "cover_links", "cover_models", "near_links", "near_models"])
def test_ties_go_to_the_earlier_draw(case, two_kernel):
    if case.startswith("cover"):
        q = quad(-3.0, 3.0, -3.0, 3.0, 1.5)              # covers every tile of the image
    elif case.startswith("near"):
        q = quad(-0.02, 0.02, -0.015, 0.015, 0.100003)   # just beyond the near plane: winners need the exact-z pass
    else:
        q = quad(-0.2, 0.2, -0.15, 0.15, 1.0)
    other = quad(-0.5, -0.3, -0.3, 0.3, 1.2)
    geo = [[other, q], [q]] if case.endswith("models") else [[other, q, q]]
    sc = tie_scene(geo)
    flags = R.FLAG_TWO_KERNEL if two_kernel else 0
    ctx = sc.context(flags=flags)
    n_links = 3
    for labels in ([5, 7, 3], [5, 3, 7]):
        if case.endswith("models"):
            ctx.set_link_labels(sc.ids[0], np.array(labels[:2], np.uint16))
            ctx.set_link_labels(sc.ids[1], np.array(labels[2:], np.uint16))
        else:
            ctx.set_link_labels(sc.ids[0], np.array(labels, np.uint16))
        want = label_planes(sc, np.array(labels))
        assert (want == labels[1]).sum() > 50 and not (want == labels[2]).any()
        compare_labels(run_device(ctx, sc.depth), want, "%s labels %s" % (case, labels))
        compare_labels(run_host(ctx, sc.depth), want, "%s labels %s host" % (case, labels))
    st = ctx.stats()
    if case.startswith("near"):
        assert st["exact_tiles"] > 0, st
    if case.startswith("cover"):
        assert st["cover_tiles"] > 0, st
    assert n_links == 3
    ctx.close()


# ---- re-runs --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("two_kernel", [False, True])
def test_regrown_bins_rerun_the_labels(two_kernel):
    sc = scene("pr2_near_walls")
    ctx = sc.context(flags=R.FLAG_TWO_KERNEL if two_kernel else 0, bin_capacity=1)
    masked, mask, lab = ctx.filter_batch_labels(sc.depth)
    st = ctx.stats()
    assert st["regrowths"] >= 1 and st["batch_reruns"] >= 1 and st["batch_status"] != 0
    compare_labels(lab, label_planes(sc), "re-run")
    compare_labels(run_device(ctx, sc.depth), label_planes(sc), "after the re-run")
    ctx.close()


# ---- rtuf_set_link_labels ---------------------------------------------------------------------------------------------------

def test_set_link_labels_custom_zero_grouping_and_changes():
    sc = scene("pr2_near_walls")
    ctx = sc.context()
    n_links = [ctx.num_links(m) for m in sc.ids]
    total = sum(n_links)
    rng = np.random.default_rng(3)
    tables = [None,
              rng.integers(1, 65536, total),                          # any value
              np.where(np.arange(total) % 3 == 0, 0, 9 + np.arange(total) % 4),   # 0 and grouping
              np.full(total, 65535)]
    for t in tables + tables[:2]:
        if t is None:
            t = np.arange(1, total + 1)
        base = 0
        for m, nl in zip(sc.ids, n_links):
            ctx.set_link_labels(m, np.asarray(t[base:base + nl], np.uint16))
            base += nl
        want = label_planes(sc, t)
        compare_labels(run_device(ctx, sc.depth), want, "device, table %s" % t[:4])
        compare_labels(run_host(ctx, sc.depth), want, "host, table %s" % t[:4])
    ctx.close()


def test_graph_replay_picks_up_new_labels_and_buffers():
    """One raster lane, pipelines = 2, batches of one stream: graph replay is on.  Two label buffers alternate and the
    labels change between batches; every batch must carry its own labels into its own buffer."""
    torch, dev = torch_device()
    sc = scene("c1_640x480")
    ctx = sc.context(max_streams=1, n=1, raster_lanes=1, pipelines=2)
    n_links = ctx.num_links(sc.ids[0])
    d = torch.from_numpy(sc.depth[:1]).to(dev)
    m = torch.empty_like(d)
    bufs = [torch.zeros(d.shape, dtype=torch.int16, device=dev) for _ in range(2)]
    seq = [0, 0, 1, 1, 0, 2, 2, 2, 1, 0, 0, 0, 2, 1]
    for i, t in enumerate(seq):
        labels = np.arange(1, n_links + 1) * (t + 1) + t
        ctx.set_link_labels(sc.ids[0], labels.astype(np.uint16))
        buf = bufs[i % 2]
        buf.fill_(-1)
        ctx.filter_batch_device_labels(1, d.data_ptr(), m.data_ptr(), None, buf.data_ptr())
        ctx.sync()
        got = buf.cpu().numpy().view(np.uint16)
        compare_labels(got, label_planes(sc, labels)[:1], "batch %d" % i)
    st = ctx.stats()
    assert st["graphs_enabled"] == 1 and st["graph_hits"] > 0
    ctx.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_refusals():
    torch, dev = torch_device()
    sc = scene("c1_640x480")
    ctx = sc.context()
    n = sc.n
    d = torch.from_numpy(sc.depth).to(dev)
    m = torch.empty_like(d)
    lab = torch.empty(d.shape, dtype=torch.int16, device=dev)
    with pytest.raises(R.RtufError) as e:                       # NULL label plane
        ctx.filter_batch_device_labels(n, d.data_ptr(), m.data_ptr(), None, None)
    assert e.value.code == INVALID
    with pytest.raises(R.RtufError) as e:                       # bad model
        ctx.set_link_labels(len(sc.ids), np.ones(2, np.uint16))
    assert e.value.code == INVALID
    with pytest.raises(R.RtufError) as e:                       # bad link count
        ctx.set_link_labels(sc.ids[0], np.ones(ctx.num_links(sc.ids[0]) + 1, np.uint16))
    assert e.value.code == INVALID
    p = params(replace=sc.wl.replace_value, max_diff=sc.wl.max_diff, silhouette_dilation_px=2)
    ctx.set_params(p)
    with pytest.raises(R.RtufError) as e:                       # silhouette dilation: not supported yet
        ctx.filter_batch_device_labels(n, d.data_ptr(), m.data_ptr(), None, lab.data_ptr())
    assert e.value.code == INVALID
    with pytest.raises(R.RtufError) as e:
        ctx.filter_batch_labels(sc.depth)
    assert e.value.code == INVALID
    # the context still works, labels included, once the radius is 0 again
    ctx.set_params(params(replace=sc.wl.replace_value, max_diff=sc.wl.max_diff))
    compare_labels(run_host(ctx, sc.depth), label_planes(sc), "after the refusals")
    ctx.close()
