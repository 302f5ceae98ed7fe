"""GPU (-m gpu, except the expectation's self-check): silhouette dilation, rtuf_params.silhouette_dilation_px = r.

Expected outputs come from the CPU oracle's debug planes: its window z where something was drawn (NaN where prim == -1),
the clipped (2r+1)^2 NaN-ignoring minimum of that per stream, and the shader's compare in numpy float32 with the host's
shade_num / shade_off order of operations.  At r = 0 that restatement reproduces the oracle's own outputs bit for bit
(test_expectation_reproduces_the_oracle_at_r0), which pins the expectation itself.  One analytic case (a square on a flat
sensor plane) checks the geometry of the dilation without the numpy shading."""
import numpy as np
import pytest

import scenes as S
import realtime_urdf_filter_amd as R
from bench_support import workloads as WL
from bench_support.dilation_check import window_min
from gpu_support import (DeviceWord, OracleScene, bits_equal, border_scene, cached, centred_projection, compare_labels, compare_planes, filter_expected, neighbour_scene,
                         pack_bits, params, quad, set_radius, soup_scene, undrawn_at, undrawn_scene, workload_of)
from realtime_urdf_filter_amd.filter import depth_f32_to_u16

RADII = (1, 2, 5, 16)
STATUS_UNCOVERED = 1 << 20
gpu = pytest.mark.gpu


# ---- scenes (the expectation at radius r is gpu_support.filter_expected: point clouds and clearance tables expect it too) ----------

def example_scene():
    wl = WL.example_workload(640, 480)
    return OracleScene(wl, wl.depth_batch(), "example_urdf_640x480")


def pr2_scene():
    wl = WL.pr2_workload(3, 640, 480, near_arm=True, walls=True)
    return OracleScene(wl, wl.depth_batch(), "pr2_near_arm_walls_3x640x480")


BUILDERS = {
    "soup_160x120": lambda: soup_scene(1, 160, 120),
    "odd_517x389": lambda: soup_scene(2, 517, 389, n=2),
    "example_640x480": example_scene,
    "pr2_640x480": pr2_scene,
    "borders_160x120": border_scene,
    "neighbours_160x120": neighbour_scene,
    "undrawn_160x120": undrawn_scene,
}


@cached
def scene(name):
    return BUILDERS[name]()


def check(sc, r, masked, mask, u16=False, what=""):
    em, ek = filter_expected(sc, r, u16)
    if mask is not None:
        compare_labels(mask, ek, "%s r=%d %s" % (sc.name, r, what), "mask")
    compare_planes(masked, em, "%s r=%d %s" % (sc.name, r, what), "16UC1 masked depth" if u16 else "masked depth")


# ---- the expectation itself -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_expectation_reproduces_the_oracle_at_r0(name):
    sc = scene(name)
    em, ek = filter_expected(sc, 0)
    for s in range(sc.n):
        om, ok = sc.masked[s], sc.mask[s]
        assert np.array_equal(ok, ek[s]), "%s stream %d: %d mask px" % (name, s, int((ok != ek[s]).sum()))
        assert bits_equal(om, em[s]), name
    if name in ("soup_160x120", "pr2_640x480", "borders_160x120", "neighbours_160x120"):
        # the scenes are not trivial for the dilation: the mask grows
        assert (filter_expected(sc, 1)[1] > 0).sum() > (ek > 0).sum(), name


def test_window_min_clips_instead_of_padding():
    z = np.full((5, 6), np.nan, np.float32)
    z[0, 0] = 0.5
    z[4, 5] = 0.25
    d = window_min(z, 1)
    assert d[1, 1] == np.float32(0.5) and np.isnan(d[2, 2]) and d[3, 4] == np.float32(0.25) and np.isnan(d[0, 2])
    assert np.all(window_min(z, 16) == np.float32(0.25))


# ---- every output form, both flag settings, one and three lanes ---------------------------------------------------------

@gpu
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("two_kernel", [False, True])
@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_dilated_outputs_match_the_expectation(name, two_kernel, lanes):
    import torch
    sc = scene(name)
    flags = R.FLAG_TWO_KERNEL if two_kernel else 0
    ctx = sc.context(flags=flags, raster_lanes=lanes)
    dev = torch.device("cuda:0")
    d_depth = torch.from_numpy(sc.depth).to(dev)
    u16_ok = sc.W % 4 == 0
    depth16 = depth_f32_to_u16(sc.depth)
    d_depth16 = torch.from_numpy(depth16.view(np.int16)).to(dev)
    words = ctx.mask_bits_words()
    ctx.filter_batch(sc.depth)                    # (sizes the bins: the batches below are final at once)
    for r in RADII:
        set_radius(ctx, sc, r, flags=flags, raster_lanes=lanes)
        masked, mask = ctx.filter_batch(sc.depth)
        check(sc, r, masked, mask, what="host planes")
        assert ctx.stats()["batch_status"] == 0
        masked_nm, none = ctx.filter_batch(sc.depth, want_mask=False)
        assert none is None
        check(sc, r, masked_nm, None, what="host planes without mask")
        d_masked = torch.empty_like(d_depth)
        d_mask = torch.empty(d_depth.shape, dtype=torch.uint8, device=dev)
        ctx.filter_batch_device(sc.n, d_depth.data_ptr(), d_masked.data_ptr(), d_mask.data_ptr())
        ctx.sync()
        check(sc, r, d_masked.cpu().numpy(), d_mask.cpu().numpy(), what="device planes")
        if not u16_ok:
            continue
        m16, k16 = ctx.filter_batch_u16(depth16)
        check(sc, r, m16, k16, u16=True, what="16UC1")
        d_m16 = torch.empty_like(d_depth16)
        ctx.filter_batch_device_u16(sc.n, d_depth16.data_ptr(), d_m16.data_ptr(), None)
        ctx.sync()
        check(sc, r, d_m16.cpu().numpy().view(np.uint16), None, u16=True, what="16UC1 device")
        if two_kernel:
            with pytest.raises(R.RtufError):          # the rule stays: no mask bits under RTUF_FLAG_TWO_KERNEL
                ctx.filter_batch_bits_async(sc.depth, np.zeros((sc.n, words), np.uint32))
            continue
        undrawn = undrawn_at(sc, r)
        for u16 in (False, True):
            bits = np.zeros((sc.n, words), np.uint32)
            ctx.filter_batch_bits_async(depth16 if u16 else sc.depth, bits)
            if undrawn:
                with pytest.raises(R.RtufError) as e:
                    ctx.sync()
                assert "background quad" in str(e.value)
                assert ctx.stats()["batch_status"] & STATUS_UNCOVERED
                continue
            ctx.sync()
            em, ek = filter_expected(sc, r, u16)
            for s in range(sc.n):
                assert np.array_equal(bits[s], pack_bits(ek[s])), "%s r=%d bits (u16=%s) stream %d" % (name, r, u16, s)
                xm, xk = R.expand_mask_bits(depth16[s] if u16 else sc.depth[s], bits[s], sc.wl.replace_value)
                assert np.array_equal(xk, ek[s])
                if u16:
                    assert np.array_equal(xm, em[s])
                else:
                    assert bits_equal(xm, em[s])
            d_bits = torch.zeros((sc.n, words), dtype=torch.int32, device=dev)
            ctx.filter_batch_device_bits(sc.n, (d_depth16 if u16 else d_depth).data_ptr(), d_bits.data_ptr(), u16=u16)
            ctx.sync()
            db = d_bits.cpu().numpy().view(np.uint32)
            for s in range(sc.n):
                assert np.array_equal(db[s], pack_bits(ek[s])), "%s r=%d device bits (u16=%s) stream %d" % (name, r, u16, s)
    ctx.close()


# ---- context shapes ---------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("r", RADII)
def test_single_stream_filter_call(r):
    sc = scene("example_640x480")
    ctx = sc.context(silhouette_dilation_px=r)
    md, mk = ctx.filter(sc.depth[0], sc.wl.projection[0])
    check(sc, r, md[None], mk[None], what="rtuf_filter")
    ctx.close()


@gpu
def test_partial_batch():
    """A batch of 3 streams in a context of 8 (groups of a full batch differ from a partial one's)."""
    sc = scene("soup_160x120")
    ctx = sc.context(max_streams=8)
    for r in (2, 5):
        set_radius(ctx, sc, r)
        masked, mask = ctx.filter_batch(sc.depth)
        check(sc, r, masked, mask, what="partial batch")
    ctx.close()


@gpu
@pytest.mark.parametrize("bits", [False, True])
def test_regrown_bins_rerun_the_batch_with_its_radius(bits):
    sc = scene("pr2_640x480")
    ctx = sc.context(bin_capacity=1, silhouette_dilation_px=5)
    if bits:
        out = np.zeros((sc.n, ctx.mask_bits_words()), np.uint32)
        ctx.filter_batch_bits_async(sc.depth, out)
        ctx.sync()
        for s in range(sc.n):
            assert np.array_equal(out[s], pack_bits(filter_expected(sc, 5)[1][s]))
    else:
        masked, mask = ctx.filter_batch(sc.depth)
        check(sc, 5, masked, mask, what="re-run")
    st = ctx.stats()
    assert st["regrowths"] >= 1 and st["batch_reruns"] >= 1 and st["batch_status"] != 0
    masked, mask = ctx.filter_batch(sc.depth)           # the next batch is final at once
    check(sc, 5, masked, mask, what="after the re-run")
    assert ctx.stats()["batch_status"] == 0
    ctx.close()


@gpu
def test_graph_replay_follows_the_radius():
    """pipelines = 2, batches of one stream: graph replay is on.  The radius changes between batches, and every batch must
    match its own radius (the captured graph of an earlier radius is never replayed for another)."""
    sc = scene("soup_160x120")
    ctx = sc.context(max_streams=1, pipelines=2)
    seq = [0, 3, 0, 3, 5, 5, 5, 5, 0, 0, 3, 3, 3, 3, 1, 16, 16, 16, 16, 0, 0, 0, 0, 5, 3, 0]
    for i, r in enumerate(seq):
        set_radius(ctx, sc, r, pipelines=2)
        s = i % sc.n
        ctx.set_cameras(0, sc.wl.projection[s:s + 1], sc.wl.offset_inv[s:s + 1], sc.wl.cam_tf[s:s + 1])
        ctx.set_link_poses_batch(0, 0, sc.wl.link_tf[0][s:s + 1])
        masked, mask = ctx.filter_batch(sc.depth[s:s + 1])
        em, ek = filter_expected(sc, r)
        assert np.array_equal(mask[0], ek[s]), "batch %d (r=%d): %d mask px" % (i, r, int((mask[0] != ek[s]).sum()))
        assert bits_equal(masked[0], em[s]), "batch %d (r=%d)" % (i, r)
    st = ctx.stats()
    assert st["graphs_enabled"] == 1 and st["graph_hits"] > 0
    ctx.close()


# ---- switching and validation -----------------------------------------------------------------------------------------

@gpu
def test_back_to_zero_is_the_unmodified_filter():
    sc = scene("pr2_640x480")
    ctx = sc.context(silhouette_dilation_px=5)
    masked, mask = ctx.filter_batch(sc.depth)
    check(sc, 5, masked, mask)
    set_radius(ctx, sc, 0)
    masked, mask = ctx.filter_batch(sc.depth)
    for s in range(sc.n):
        om, ok = sc.masked[s], sc.mask[s]
        assert np.array_equal(mask[s], ok) and bits_equal(masked[s], om)
    bits = np.zeros((sc.n, ctx.mask_bits_words()), np.uint32)
    ctx.filter_batch_bits_async(sc.depth, bits)
    ctx.sync()
    for s in range(sc.n):
        assert np.array_equal(bits[s], pack_bits(sc.mask[s]))
    ctx.close()


@gpu
def test_radius_above_16_is_refused_and_the_previous_params_stay():
    sc = scene("soup_160x120")
    p = params(silhouette_dilation_px=17)
    with pytest.raises(R.RtufError) as e:
        R.Context(sc.W, sc.H, sc.n, 0, p)
    assert e.value.code == -1
    ctx = sc.context(silhouette_dilation_px=16)
    set_radius(ctx, sc, 2)
    with pytest.raises(R.RtufError) as e:
        set_radius(ctx, sc, 17)
    assert e.value.code == -1
    masked, mask = ctx.filter_batch(sc.depth)
    check(sc, 2, masked, mask, what="after a refused radius")
    ctx.close()


@gpu
def test_status_word_of_final_dilated_batches_is_zero():
    import torch
    sc = scene("soup_160x120")
    ctx = sc.context(silhouette_dilation_px=3)
    dev = torch.device("cuda:0")
    d = torch.from_numpy(sc.depth).to(dev)
    m = torch.empty_like(d)
    ctx.filter_batch(sc.depth)                    # (sizes the bins)
    for _ in range(3):
        ctx.filter_batch_device(sc.n, d.data_ptr(), m.data_ptr(), None)
        ctx.sync()
        word = torch.as_tensor(DeviceWord(ctx.batch_status_device()), device=dev)
        assert int(word.cpu().numpy()[0]) == 0
        assert ctx.stats()["batch_status"] == 0
    check(sc, 3, m.cpu().numpy(), None)
    ctx.close()


# ---- the analytic case ------------------------------------------------------------------------------------------------

def _chebyshev_dilate(mask, r):
    H, W = mask.shape
    p = np.zeros((H + 2 * r, W + 2 * r), bool)
    p[r:r + H, r:r + W] = mask > 0
    out = np.zeros((H, W), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[dy:dy + H, dx:dx + W]
    return out


@gpu
def test_square_on_a_plane_grows_by_r_pixels_and_keeps_the_occluder():
    """A square at 1 m over a flat sensor plane at 1.5 m: the mask at r is the r = 0 mask dilated by r in Chebyshev distance.
    A block of sensor pixels at 0.5 m (in front of the square, nearer than its depth minus the threshold) across the
    square's right edge stays unfiltered at every r."""
    W, H = 160, 128
    P = centred_projection(W, H)
    wl = workload_of("square", W, H, [quad(-0.15, 0.15, -0.12, 0.12, 1.0)], np.tile(S.gl(np.eye(4)), (1, 1, 1)), P[None])
    depth = np.full((1, H, W), 1.5, np.float32)
    ctx = R.Context(W, H, 1, 0, params(replace=5.0, max_diff=0.05))
    ids = wl.load_into(ctx)
    wl.stage(ctx, ids)
    _, mask0 = ctx.filter_batch(depth)
    ys, xs = np.nonzero(mask0[0])
    assert len(ys) > 100
    x1, yc = xs.max(), (ys.min() + ys.max()) // 2
    occ = np.zeros((H, W), bool)
    occ[yc - 6:yc + 6, x1 - 4:x1 + 24] = True
    depth[0][occ] = 0.5
    for r in (0,) + RADII:
        ctx.set_params(params(replace=5.0, max_diff=0.05, silhouette_dilation_px=r))
        masked, mask = ctx.filter_batch(depth)
        want = _chebyshev_dilate(mask0[0], r) & ~occ
        assert np.array_equal(mask[0] > 0, want), "r=%d: %d px differ" % (r, int(((mask[0] > 0) != want).sum()))
        assert not (mask[0][occ]).any()
        assert np.all(masked[0][want] == np.float32(5.0)) and bits_equal(masked[0][~want], depth[0][~want])
    ctx.close()
