"""GPU (-m gpu, except the expectation's self-check): filtered point clouds (include/rtuf.h, FILTERED POINT CLOUDS).

The expectation is bench_support/cloud_check.py applied to the mask the dilation tests expect (gpu_support.filter_expected(sc, r)[1], built
from the CPU oracle's planes; with per-link thresholds link_thresholds_check.expected_planes) and the scene's sensor plane --
never the library's own mask.  Organized planes are compared as uint32 bit patterns; compacted output for equality on
[:count], together with counts and index.  Every stream has intrinsics of its own, so a point computed with another stream's
would show."""
import numpy as np
import pytest

import realtime_urdf_filter_amd as R
from bench_support import cloud_check as CC
from bench_support.link_thresholds_check import expected_planes
from bench_support.link_thresholds_check import workload_draws as thr_draws
from gpu_support import CLOUD_SENTINEL as SENTINEL
from gpu_support import (CloudBuffers, CloudExpect, Consumer, OracleScene, border_scene, cached, check_comp, check_org, cloud_context, cloud_enqueue,
                         cloud_expect, filter_expected, intrinsics, neighbour_scene, params, sensor_of, set_radius, soup_scene, torch_device,
                         undrawn_scene, upload)
from oracle import bindings as O
from realtime_urdf_filter_amd.filter import depth_f32_to_u16

gpu = pytest.mark.gpu
INVALID, STATE = -1, -6
STATUS_UNCOVERED = 1 << 20


# ---- scenes and expectations -------------------------------------------------------------------------------------------------

def _neighbours_with_invalid_pixels():
    """neighbour_scene with a few pixels of streams 0 and 2 without a reading (stream 1 still keeps every pixel)."""
    nb = neighbour_scene()
    depth = nb.depth.copy()
    depth[0, 50:54, 7:90] = np.nan
    depth[2, 60, :] = 0.0
    depth[2, 61, 3:40] = np.inf
    return OracleScene(nb.wl, depth, nb.name)


BUILDERS = {"soup_160x120": lambda: soup_scene(1, 160, 120), "soup_100x75": lambda: soup_scene(3, 100, 75), "neighbours": _neighbours_with_invalid_pixels,
            "borders": border_scene, "undrawn": undrawn_scene}


@cached
def scene(name):
    return BUILDERS[name]()


def expect(name, r=0, u16=False, streams=None):
    return cloud_expect(scene(name), r, u16, streams)


def device_forms(ctx, sc, ex, u16, what, n=None, total=None):
    """The organized and the compacted device form of one sensor batch against ex."""
    n, total = n or sc.n, total or sc.n
    d = upload(depth_f32_to_u16(sc.depth) if u16 else sc.depth)
    org = CloudBuffers(sc, total)
    cloud_enqueue(ctx, d, n, org, u16)
    comp = CloudBuffers(sc, total, sc.W * sc.H)
    cloud_enqueue(ctx, d, n, comp, u16)
    ctx.sync()
    assert ctx.stats()["batch_status"] == 0
    check_org(org.host()[0][:n], ex, what + " organized", n)
    p, i, c = comp.host()
    check_comp(p, i, c, ex, sc.W * sc.H, what + " compacted", n)
    return org, comp


# ---- the expectation itself (CPU) ----------------------------------------------------------------------------------------------

def test_expected_counts_of_the_soup_scenes():
    ex = expect("soup_160x120")
    assert ex.counts.tolist() == [9976, 117, 7727]
    sc = scene("soup_160x120")
    inv = [CC.classes(sc.depth[s], filter_expected(sc, 0)[1][s])[2] for s in range(sc.n)]
    assert all(591 <= v <= 636 for v in inv), inv
    rows = CC.kept(sc.depth[1], filter_expected(sc, 0)[1][1]).any(axis=1)
    assert int((~rows).sum()) == 112                         # stream 1: 112 rows without a kept pixel
    assert expect("soup_100x75").counts.tolist() == [5045, 4757, 4715]
    assert expect("soup_100x75", 2).counts.tolist() == [4561, 3744, 3453]
    assert expect("neighbours").counts[1] == 19200


# ---- every form on the smallest shapes -------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", ["soup_160x120", "soup_100x75"])
def test_all_forms_match_the_expectation(name):
    sc = scene(name)
    ctx = cloud_context(sc)
    depth16 = depth_f32_to_u16(sc.depth)
    ctx.filter_batch(sc.depth)                    # (sizes the bins: the batches below are final at once)
    for r in (0, 2):
        set_radius(ctx, sc, r)
        for u16 in (False, True):
            ex = expect(name, r, u16)
            device_forms(ctx, sc, ex, u16, "%s r=%d u16=%s device" % (name, r, u16))
            if r and name == "soup_160x120":
                continue
            sensor = depth16 if u16 else sc.depth
            check_org(ctx.cloud_batch(sensor), ex, "%s r=%d u16=%s host organized" % (name, r, u16))
            p, i, c = ctx.cloud_compact_batch(sensor, sc.W * sc.H)
            check_comp(p, i, c, ex, sc.W * sc.H, "%s r=%d u16=%s host compacted" % (name, r, u16))
            p, i, c = ctx.cloud_compact_batch(sensor, 4000, want_index=False)
            assert i is None
            check_comp(p, None, c, ex, 4000, "%s r=%d u16=%s host compacted, capacity 4000, no index" % (name, r, u16))
    ctx.close()


@gpu
def test_capacity_filled_exactly_and_exceeded():
    sc = scene("neighbours")
    ex = expect("neighbours")
    assert ex.counts[1] == sc.W * sc.H
    ctx = cloud_context(sc)
    d = upload(sc.depth)
    full = CloudBuffers(sc, sc.n, sc.W * sc.H)
    cloud_enqueue(ctx, d, sc.n, full)
    small = CloudBuffers(sc, sc.n, 1000)
    cloud_enqueue(ctx, d, sc.n, small, index=False)
    ctx.sync()
    p, i, c = full.host()
    check_comp(p, i, c, ex, sc.W * sc.H, "capacity = W*H")
    assert np.array_equal(i[1], np.arange(sc.W * sc.H, dtype=np.uint32))
    p, i, c = small.host()
    assert c.tolist() == ex.counts.tolist() and c[1] == 19200          # the counts stay full
    check_comp(p, None, c, ex, 1000, "capacity = 1000")
    assert (i == SENTINEL).all()                                        # no index asked for: none written
    p, i, c = ctx.cloud_compact_batch(sc.depth, 1000)
    check_comp(p, i, c, ex, 1000, "capacity = 1000, host planes")
    check_org(ctx.cloud_batch(sc.depth), ex, "organized")
    ctx.close()


@gpu
def test_per_link_thresholds_are_honoured():
    sc = scene("borders")
    wl = sc.wl
    link_thr = np.array([np.nan, 0.3, 0.0, -0.2], np.float32)
    thr, nt = thr_draws(wl, link_thr)
    masks = {}
    for u16 in (False, True):
        sensor = sensor_of(sc, u16)
        planes = []
        for s in range(sc.n):
            _, _, zwin, prim, _ = O.filter_frame(sensor[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], z_near=wl.near,
                                                 z_far=wl.far, max_diff=wl.max_diff, replace_value=wl.replace_value, want_debug=True)
            planes.append(expected_planes(zwin, prim, sensor[s], thr, nt, wl.max_diff, wl.near, wl.far, wl.replace_value)[1])
        masks[u16] = np.stack(planes)
    assert (masks[False] != filter_expected(sc, 0)[1]).any()                    # the thresholds change the mask
    ctx = cloud_context(sc)
    ids = list(range(len(wl.models)))
    ctx.set_link_thresholds(ids[0], link_thr)
    for u16 in (False, True):
        ex = CloudExpect(sc, masks[u16], u16, range(sc.n))
        device_forms(ctx, sc, ex, u16, "thresholds u16=%s" % u16)
    check_org(ctx.cloud_batch(sc.depth), CloudExpect(sc, masks[False], False, range(sc.n)), "thresholds, host planes")
    ctx.clear_link_thresholds(ids[0])
    device_forms(ctx, sc, expect("borders"), False, "after clear")
    ctx.close()


@gpu
def test_uncovered_image_fails_when_the_batch_is_retired():
    sc = scene("undrawn")
    ctx = cloud_context(sc)
    d = upload(sc.depth)
    for buf in (CloudBuffers(sc, sc.n), CloudBuffers(sc, sc.n, 500)):
        cloud_enqueue(ctx, d, sc.n, buf)
        with pytest.raises(R.RtufError) as e:
            ctx.sync()
        assert e.value.code == STATE and "background quad" in str(e.value)
        assert ctx.stats()["batch_status"] & STATUS_UNCOVERED
    with pytest.raises(R.RtufError) as e:
        ctx.cloud_batch(sc.depth)
    assert e.value.code == STATE
    ctx.close()


@gpu
def test_refusals_enqueue_nothing_and_a_good_call_still_matches():
    sc = scene("soup_160x120")
    ex = expect("soup_160x120")
    d = upload(sc.depth)
    org, comp = CloudBuffers(sc, sc.n), CloudBuffers(sc, sc.n, 3000)

    def refused(code, call):
        with pytest.raises(R.RtufError) as e:
            call()
        assert e.value.code == code, e.value

    def untouched():
        ctx.sync()
        torch_device()[0].cuda.synchronize()
        for buf in (org, comp):
            for t in (buf.points, buf.index, buf.counts):
                assert t is None or bool((t == SENTINEL).all())

    p = params(replace=sc.wl.replace_value, max_diff=sc.wl.max_diff)
    p.near_plane, p.far_plane = sc.wl.near, sc.wl.far
    ctx = R.Context(sc.W, sc.H, sc.n, 0, p)
    refused(STATE, lambda: cloud_enqueue(ctx, d, sc.n, org))                  # before finalize
    ids = sc.wl.load_into(ctx)
    sc.wl.stage(ctx, ids)
    refused(STATE, lambda: cloud_enqueue(ctx, d, sc.n, org))                  # no intrinsics at all
    refused(STATE, lambda: ctx.cloud_batch(sc.depth))
    ctx.set_cloud_intrinsics(0, [intrinsics(sc, i) for i in range(2)])
    refused(STATE, lambda: cloud_enqueue(ctx, d, sc.n, comp))                 # stream 2 has none yet
    for bad in ((0.0, 100.0, 1.0, 1.0), (100.0, -2.0, 1.0, 1.0), (np.nan, 100.0, 1.0, 1.0), (100.0, np.inf, 1.0, 1.0)):
        refused(INVALID, lambda: ctx.set_cloud_intrinsics(1, [intrinsics(sc, 1), bad]))      # ... and a refused set changes nothing
    refused(INVALID, lambda: ctx.set_cloud_intrinsics(2, [intrinsics(sc, 2)] * 2))           # beyond max_streams
    refused(STATE, lambda: cloud_enqueue(ctx, d, sc.n, comp))
    ctx.set_cloud_intrinsics(2, intrinsics(sc, 2))
    for cap in (0, sc.W * sc.H + 1, -5):
        comp.cap = cap
        refused(INVALID, lambda: cloud_enqueue(ctx, d, sc.n, comp))
        refused(INVALID, lambda: ctx.cloud_compact_batch(sc.depth, cap))
    comp.cap = 3000
    refused(INVALID, lambda: ctx.cloud_batch_device(sc.n, None, org.points.data_ptr()))      # NULL planes
    refused(INVALID, lambda: ctx.cloud_batch_device(sc.n, d.data_ptr(), None))
    refused(INVALID, lambda: ctx.cloud_compact_batch_device(sc.n, d.data_ptr(), comp.points.data_ptr(), None, None, 3000))
    refused(INVALID, lambda: ctx.cloud_batch_device(sc.n, d.data_ptr() + 4, org.points.data_ptr()))            # organized: 16-byte alignment
    refused(INVALID, lambda: ctx.cloud_batch_device(sc.n, d.data_ptr(), org.points.data_ptr() + 8))
    refused(INVALID, lambda: ctx.cloud_batch_device(sc.n, d.data_ptr() + 4, org.points.data_ptr(), u16=True))  # (16UC1: 8 bytes)
    refused(INVALID, lambda: cloud_enqueue(ctx, d, 0, org))                   # n out of range
    refused(INVALID, lambda: cloud_enqueue(ctx, d, sc.n + 1, comp))
    untouched()
    cloud_enqueue(ctx, d, sc.n, org)
    cloud_enqueue(ctx, d, sc.n, comp)
    ctx.sync()
    check_org(org.host()[0], ex, "after the refusals")
    pp, ii, cc = comp.host()
    check_comp(pp, ii, cc, ex, 3000, "after the refusals")
    ctx.close()


@gpu
def test_width_that_is_no_multiple_of_4_is_refused():
    sc = soup_scene(2, 517, 389, n=1)
    ctx = cloud_context(sc)
    d = upload(sc.depth)
    buf = CloudBuffers(sc, 1)
    with pytest.raises(R.RtufError) as e:
        cloud_enqueue(ctx, d, 1, buf)
    assert e.value.code == INVALID and "multiple of 4" in str(e.value)
    with pytest.raises(R.RtufError) as e:
        ctx.cloud_compact_batch(sc.depth, 100)
    assert e.value.code == INVALID
    ctx.sync()
    assert bool((buf.points == SENTINEL).all())
    masked, mask = ctx.filter_batch(sc.depth)                           # the context still filters
    assert np.array_equal(mask, filter_expected(sc, 0)[1])
    ctx.close()


# ---- batch machinery ---------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("kw", [dict(raster_lanes=1), dict(raster_lanes=3), dict(flags=R.FLAG_TWO_KERNEL), dict(pipelines=2)],
                         ids=["one_lane", "three_lanes", "two_kernel_flag", "two_pipelines"])
def test_lanes_flags_and_pipelines(kw):
    sc = scene("soup_160x120")
    ctx = cloud_context(sc, **kw)
    for r in (0, 2):
        set_radius(ctx, sc, r, **kw)
        for u16 in (False, True):
            device_forms(ctx, sc, expect("soup_160x120", r, u16), u16, "%s r=%d u16=%s" % (kw, r, u16))
    if "flags" in kw:                             # the context filters in two-kernel mode as before, and the cloud again behind it
        masked, mask = ctx.filter_batch(sc.depth)
        assert np.array_equal(mask, filter_expected(sc, 2)[1])
        device_forms(ctx, sc, expect("soup_160x120", 2), False, "behind a two-kernel filter batch")
    ctx.close()


@gpu
def test_partial_batch_leaves_the_other_streams_alone():
    sc = scene("soup_160x120")
    ctx = cloud_context(sc)
    ex = expect("soup_160x120")
    org, comp = device_forms(ctx, sc, ex, False, "2 of 3 streams", n=2, total=3)
    assert bool((org.points[2] == SENTINEL).all()) and bool((comp.points[2] == SENTINEL).all())
    assert bool((comp.index[2] == SENTINEL).all()) and int(comp.counts[2]) == SENTINEL
    ctx.close()


@gpu
def test_several_launch_groups():
    sc = scene("soup_160x120")
    ctx = cloud_context(sc, max_inflight_streams=1, raster_lanes=3)
    device_forms(ctx, sc, expect("soup_160x120"), False, "three groups")
    assert ctx.stats()["groups_last_batch"] == 3
    ctx.close()


@gpu
def test_two_batches_in_flight_with_outputs_of_their_own():
    sc = scene("soup_160x120")
    ctx = cloud_context(sc)
    ctx.filter_batch(sc.depth)
    d, d16 = upload(sc.depth), upload(depth_f32_to_u16(sc.depth))
    a, b = CloudBuffers(sc, sc.n), CloudBuffers(sc, sc.n, 8000)
    cloud_enqueue(ctx, d, sc.n, a)
    cloud_enqueue(ctx, d16, sc.n, b, u16=True)
    ctx.sync()
    check_org(a.host()[0], expect("soup_160x120"), "first in flight")
    p, i, c = b.host()
    check_comp(p, i, c, expect("soup_160x120", 0, True), 8000, "second in flight")
    ctx.close()


@gpu
def test_regrown_bins_rerun_rewrites_counts_and_points():
    sc = scene("soup_160x120")
    ctx = cloud_context(sc, bin_capacity=1, silhouette_dilation_px=2)
    d = upload(sc.depth)
    org, comp = CloudBuffers(sc, sc.n), CloudBuffers(sc, sc.n, sc.W * sc.H)
    cloud_enqueue(ctx, d, sc.n, comp)
    ctx.sync()
    st = ctx.stats()
    assert st["regrowths"] >= 1 and st["batch_reruns"] >= 1 and st["batch_status"] != 0, st
    ex = expect("soup_160x120", 2)
    p, i, c = comp.host()
    check_comp(p, i, c, ex, sc.W * sc.H, "re-run")
    cloud_enqueue(ctx, d, sc.n, org)                    # the next batch is final at once
    ctx.sync()
    assert ctx.stats()["batch_status"] == 0
    check_org(org.host()[0], ex, "after the re-run")
    ctx.close()


@gpu
def test_regrown_bins_rerun_host_planes():
    sc = scene("soup_160x120")
    ctx = cloud_context(sc, bin_capacity=1)
    p, i, c = ctx.cloud_compact_batch(sc.depth, sc.W * sc.H)
    assert ctx.stats()["batch_reruns"] >= 1
    check_comp(p, i, c, expect("soup_160x120"), sc.W * sc.H, "re-run, host planes")
    ctx.close()


@gpu
def test_graph_replay_follows_the_sensor():
    """One raster lane, pipelines = 2, one stream: small batches replay a captured graph, the cloud kernels included.  The
    same buffers every time; sensor plane and poses change in between."""
    torch, dev = torch_device()
    sc = scene("soup_160x120")
    ctx = cloud_context(sc, n=1, max_streams=1, raster_lanes=1, pipelines=2)
    d = torch.empty((1, sc.H, sc.W), dtype=torch.float32, device=dev)
    org, comp = CloudBuffers(sc, 1), CloudBuffers(sc, 1, 9000)
    for i in range(15):
        s = i % sc.n
        ctx.set_cameras(0, sc.wl.projection[s:s + 1], sc.wl.offset_inv[s:s + 1], sc.wl.cam_tf[s:s + 1])
        ctx.set_link_poses_batch(0, 0, sc.wl.link_tf[0][s:s + 1])
        d.copy_(torch.from_numpy(sc.depth[s:s + 1]))
        torch.cuda.synchronize()
        ex = expect("soup_160x120", 0, False, (s,))
        if i % 5 == 4:
            cloud_enqueue(ctx, d, 1, org)
            ctx.sync()
            check_org(org.host()[0], ex, "replay %d" % i)
        else:
            cloud_enqueue(ctx, d, 1, comp)
            ctx.sync()
            p, ix, c = comp.host()
            check_comp(p, ix, c, ex, 9000, "replay %d" % i)
    st = ctx.stats()
    assert st["graphs_enabled"] == 1 and st["graph_hits"] >= 3, st
    ctx.close()


@gpu
def test_status_word_is_zero_behind_a_final_cloud_batch():
    sc = scene("soup_160x120")
    ctx = cloud_context(sc)
    ctx.filter_batch(sc.depth)                    # (bins sized)
    d = upload(sc.depth)
    comp = CloudBuffers(sc, sc.n, sc.W * sc.H)
    user = Consumer(ctx)
    cloud_enqueue(ctx, d, sc.n, comp)
    word, early_points, early_counts, _ = user.read(comp.points, comp.counts)
    assert word == 0, hex(word)
    ex = expect("soup_160x120")
    check_comp(np.ascontiguousarray(early_points).view(np.float32), None, np.ascontiguousarray(early_counts).view(np.uint32), ex, sc.W * sc.H,
               "behind the batch")
    ctx.sync()
    st = ctx.stats()
    assert st["batch_status"] == 0 and st["batch_reruns"] == 0, st
    ctx.close()


@gpu
def test_counts_shrink_when_the_second_call_keeps_fewer_pixels():
    sc = scene("soup_160x120")
    ctx = cloud_context(sc)
    d = upload(sc.depth)
    comp = CloudBuffers(sc, sc.n, sc.W * sc.H)
    cloud_enqueue(ctx, d, sc.n, comp)
    ctx.sync()
    p, i, c = comp.host()
    first = expect("soup_160x120")
    check_comp(p, i, c, first, sc.W * sc.H, "first call")
    set_radius(ctx, sc, 2)
    cloud_enqueue(ctx, d, sc.n, comp)
    ctx.sync()
    p, i, c = comp.host()
    second = expect("soup_160x120", 2)
    assert (second.counts < first.counts).all()
    check_comp(p, i, c, second, sc.W * sc.H, "second call, same buffers")
    ctx.close()


@gpu
def test_scratch_is_counted_in_device_bytes_and_timings_land_in_ms_compare():
    sc = scene("soup_160x120")
    ctx = cloud_context(sc)
    ctx.filter_batch(sc.depth)
    before = ctx.stats()["device_bytes"]
    ctx.enable_timing(2)
    ctx.cloud_compact_batch(sc.depth, 100)
    st = ctx.stats()
    words = ctx.mask_bits_words()
    assert st["device_bytes"] - before >= sc.n * (words * 4 + 2 * sc.H * 4), (before, st["device_bytes"])
    assert st["ms_compare"] > 0 and st["ms_raster"] > 0, st
    ctx.close()
