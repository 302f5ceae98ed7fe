"""GPU (-m gpu): point list batches (include/rtuf.h, POINT LIST BATCHES).

The expectation is bench_support/points_check.py applied to gpu_support.virtual_planes(sc, empty=np.inf), built from the CPU
oracle's planes -- never the library's own render.  Equality everywhere: verdict bytes, pixels, summaries, and the sentinel past
min(count, capacity).  Every stream has intrinsics of its own (gpu_support.intrinsics), so a point projected with another
stream's pinhole would show."""
import numpy as np
import pytest

import realtime_urdf_filter_amd as R
from bench_support import points_check as PC
from gpu_support import (CloudBuffers, Consumer, cached, cloud_context, cloud_enqueue, filter_expected, intrinsics, neighbour_scene, params,
                         soup_scene, torch_device, upload, virtual_planes)

gpu = pytest.mark.gpu
INVALID, STATE = -1, -6
SENT8, SENT32 = 0x5A, 0x5A5A5A5A
F = np.float32

BUILDERS = {"soup_100x75": lambda: soup_scene(3, 100, 75), "soup_160x120": lambda: soup_scene(1, 160, 120), "neighbours": neighbour_scene}


@cached
def scene(name):
    return BUILDERS[name]()


@cached
def virt(name):
    return virtual_planes(scene(name), empty=np.inf)


@cached
def grid_lists(name):
    sc = scene(name)
    return tuple(PC.grid_points(sc.depth[s], intrinsics(sc, s)) for s in range(sc.n))


@cached
def mixed_lists(name):
    """Per stream: every triple of the edge values and 3,000 random points of the box; streams 0 and 2 get a rigid transform,
    stream 1 none."""
    sc = scene(name)
    rng = np.random.default_rng(23)
    lists = tuple(np.concatenate([PC.edge_points(), PC.random_points(rng, 3000)]) for _ in range(sc.n))
    return lists, tuple(None if s == 1 else PC.rigid_transform(rng) for s in range(sc.n))


def expected(name, lists, r, matrices=None, streams=None):
    """Per slot (verdict, pixel) of the lists: slot i shows stream streams[i] of the scene through slot i's intrinsics."""
    sc = scene(name)
    streams = range(len(lists)) if streams is None else streams
    return [PC.verdicts(p, intrinsics(sc, i), virt(name)[s], sc.wl.max_diff, r, None if matrices is None else matrices[i])
            for i, (p, s) in enumerate(zip(lists, streams))]


class PointBuffers:
    """Device inputs and outputs of one points batch: the lists packed into [total][cap][3] (entries past a list's end hold
    NaN), counts as given (default: the lists' lengths), outputs filled with a sentinel.  offset_words: d_points starts that
    many floats behind a 256-byte boundary."""

    def __init__(self, lists, total=None, cap=None, counts=None, offset_words=0):
        torch, dev = torch_device()
        total = total or len(lists)
        self.cap = cap = cap or max(max(len(p) for p in lists), 1)
        host = np.full((total, cap, 3), np.nan, F)
        for s, p in enumerate(lists):
            host[s, :min(len(p), cap)] = p[:cap]
        self.counts_host = np.array([len(p) for p in lists] + [0] * (total - len(lists)), np.uint32) if counts is None else np.asarray(counts, np.uint32)
        self._store = torch.empty(host.size + offset_words, dtype=torch.float32, device=dev)
        self.points = self._store[offset_words:]
        self.points.copy_(torch.from_numpy(host.reshape(-1)))
        self.counts = torch.from_numpy(self.counts_host.view(np.int32)).to(dev)
        self.verdict = torch.full((total, cap), SENT8, dtype=torch.uint8, device=dev)
        self.pixel = torch.full((total, cap), SENT32, dtype=torch.int32, device=dev)
        self.summary = torch.full((total, 4), SENT32, dtype=torch.int32, device=dev)

    def enqueue(self, ctx, n, r, pixel=True, summary=True):
        ctx.points_batch_device(n, self.points.data_ptr(), self.counts.data_ptr(), self.cap, r, self.verdict.data_ptr(),
                                self.pixel.data_ptr() if pixel else None, self.summary.data_ptr() if summary else None)

    def host(self):
        return (self.verdict.cpu().numpy(), np.ascontiguousarray(self.pixel.cpu().numpy()).view(np.uint32),
                np.ascontiguousarray(self.summary.cpu().numpy()).view(np.uint32))

    def untouched(self):
        return bool((self.verdict == SENT8).all()) and bool((self.pixel == SENT32).all()) and bool((self.summary == SENT32).all())


def check(out, ex, counts, cap, what, n=None, pixel=True, summary=True):
    """Streams 0 .. n-1 of (verdict, pixel, summary) against ex on their first min(count, capacity) entries; everything else
    still holds the sentinel."""
    verdict, pix, summ = out
    n = n or len(ex)
    for s in range(n):
        m = min(int(counts[s]), cap)
        v, p = ex[s][0][:m], ex[s][1][:m]
        bad = verdict[s, :m] != v
        assert not bad.any(), "%s stream %d: %d verdicts differ, first at %d: %d instead of %d" % (
            what, s, int(bad.sum()), int(np.argmax(bad)), verdict[s, :m][np.argmax(bad)], v[np.argmax(bad)])
        assert (verdict[s, m:] == SENT8).all(), "%s stream %d: verdicts written past min(count, capacity)" % (what, s)
        if pixel:
            assert np.array_equal(pix[s, :m], p), "%s stream %d: pixels" % (what, s)
            assert (pix[s, m:] == SENT32).all(), "%s stream %d: pixels written past min(count, capacity)" % (what, s)
        if summary:
            assert summ[s].tolist() == PC.summary(v).tolist(), "%s stream %d: summary %s instead of %s" % (what, s, summ[s], PC.summary(v))
    assert (verdict[n:] == SENT8).all() and (summ[n:] == SENT32).all(), "%s: streams beyond the batch were written" % what
    if pixel:
        assert (pix[n:] == SENT32).all(), "%s: pixels of streams beyond the batch were written" % what
    else:
        assert (pix == SENT32).all(), "%s: pixels written though none were asked for" % what
    if not summary:
        assert (summ == SENT32).all(), "%s: a summary written though none was asked for" % what


def run(ctx, lists, r, ex, what, **kw):
    buf = PointBuffers(lists, **kw)
    buf.enqueue(ctx, len(lists), r)
    ctx.sync()
    check(buf.host(), ex, buf.counts_host, buf.cap, what)
    return buf


def check_host_form(ctx, lists, r, ex, what):
    verdict, pixel, summ = ctx.points_batch(lists, r)
    for s, p in enumerate(lists):
        assert np.array_equal(verdict[s], ex[s][0]) and np.array_equal(pixel[s], ex[s][1]), "%s stream %d" % (what, s)
        assert summ[s].tolist() == PC.summary(ex[s][0]).tolist(), "%s stream %d: summary" % (what, s)


# ---- pixel-grid, boundary, edge and random points ----------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", ["soup_100x75", "soup_160x120"])
def test_pixel_grid_points(name):
    sc = scene(name)
    lists = grid_lists(name)
    ctx = cloud_context(sc)
    for r in (0, 2):
        ex = expected(name, lists, r)
        buf = run(ctx, lists, r, ex, "%s r=%d device" % (name, r))
        check_host_form(ctx, lists, r, ex, "%s r=%d host" % (name, r))
        verdict, pixel, _ = buf.host()
        mask = filter_expected(sc, r)[1]
        for s in range(sc.n):
            judged = verdict[s] != PC.OUTSIDE
            assert np.array_equal(pixel[s][judged], np.flatnonzero(judged).astype(np.uint32)), "every judged point's pixel is its own index"
            assert judged.sum() > 0.9 * judged.size and (~judged).sum() > 0
            # wherever a link holds the window minimum the verdict is the (dilated) filter's mask bit
            link = np.isfinite(PC.window_min(virt(name)[s], r)).ravel() & judged
            assert link.sum() > 1000
            assert np.array_equal(verdict[s][link] == PC.FILTERED, mask[s].ravel()[link] != 0), "%s r=%d stream %d" % (name, r, s)
    ctx.close()


@gpu
@pytest.mark.parametrize("name", ["soup_100x75", "soup_160x120"])
def test_boundary_points(name):
    """For every link pixel z = V - t exactly and its two float neighbours: kept, kept below, filtered above."""
    sc = scene(name)
    made = [PC.boundary_points(virt(name)[s], sc.wl.max_diff, intrinsics(sc, s)) for s in range(sc.n)]
    lists = [m[0] for m in made]
    ex = expected(name, lists, 0)
    for s in range(sc.n):
        assert len(lists[s]) >= 3 * 1000 and np.array_equal(ex[s][0], made[s][1]), "the expectation itself: kept / kept / filtered"
    ctx = cloud_context(sc)
    buf = run(ctx, lists, 0, ex, name + " boundary")
    verdict = buf.host()[0]
    for s in range(sc.n):
        assert np.array_equal(verdict[s, :len(lists[s])], made[s][1])
    ctx.close()


@gpu
@pytest.mark.parametrize("name", ["soup_100x75", "soup_160x120"])
def test_edge_and_random_points_with_transforms(name):
    sc = scene(name)
    lists, matrices = mixed_lists(name)
    ctx = cloud_context(sc)
    for s, m in enumerate(matrices):
        if m is not None:
            ctx.set_point_transforms(s, m)
    for r in (0, 3):
        ex = expected(name, lists, r, matrices)
        sums = np.array([PC.summary(ex[s][0]) for s in range(sc.n)])
        assert (sums[:, 1] > 100).all() and (sums[:, 2] > 100).all() and sums[:, 0].sum() > 500, sums      # (a vacuous pass must not hide)
        run(ctx, lists, r, ex, "%s mixed r=%d" % (name, r))
        check_host_form(ctx, lists, r, ex, "%s mixed r=%d host" % (name, r))
    # ... taken away again, the points are taken as given
    ctx.set_point_transforms(0, None, n_streams=sc.n)
    run(ctx, lists, 0, expected(name, lists, 0), name + " mixed, transforms taken away")
    with pytest.raises(R.RtufError) as e:
        ctx.set_point_transforms(0, np.full(16, np.nan))
    assert e.value.code == INVALID
    with pytest.raises(R.RtufError) as e:
        ctx.set_point_transforms(sc.n, np.eye(4).reshape(16))
    assert e.value.code == INVALID
    ctx.close()


# ---- capacities, counts, alignment -----------------------------------------------------------------------------------------------

@gpu
def test_capacities_counts_and_an_odd_aligned_list():
    name = "soup_100x75"
    sc = scene(name)
    lists = grid_lists(name)
    full = expected(name, lists, 1)
    ctx = cloud_context(sc)
    for cap in (1, 63, 65, 1000, sc.W * sc.H):
        # stream 0: no point at all; stream 1: exactly the capacity; stream 2: a count above the capacity
        cut = [lists[0][:0], lists[1][:cap], lists[2][:cap]]
        counts = [0, cap, cap + 7]
        ex = [(full[s][0][:len(cut[s])], full[s][1][:len(cut[s])]) for s in range(sc.n)]
        for offset in (0, 1):                     # (1: d_points starts 4 bytes behind a 16-byte boundary)
            buf = PointBuffers(cut, cap=cap, counts=counts, offset_words=offset)
            assert buf.points.data_ptr() % 16 == 4 * offset
            buf.enqueue(ctx, sc.n, 1)
            ctx.sync()
            out = buf.host()
            check(out, ex, counts, cap, "capacity %d offset %d" % (cap, offset))
            assert out[2][:, 3].tolist() == [0, cap, cap]
    # the lists' own lengths differ: the sentinel stays past each stream's count
    cut = [lists[0][:777], lists[1][:2], lists[2][:4001]]
    ex = [(full[s][0][:len(cut[s])], full[s][1][:len(cut[s])]) for s in range(sc.n)]
    run(ctx, cut, 1, ex, "uneven counts")
    buf = PointBuffers(cut)
    buf.enqueue(ctx, sc.n, 1, pixel=False, summary=False)
    ctx.sync()
    check(buf.host(), ex, buf.counts_host, buf.cap, "no pixels, no summary", pixel=False, summary=False)
    ctx.close()


@gpu
def test_neighbouring_streams_do_not_leak_at_radius_4():
    name = "neighbours"
    sc = scene(name)
    lists = grid_lists(name)
    ex = expected(name, lists, 4)
    assert PC.summary(ex[1][0]).tolist() == [sc.W * sc.H, 0, 0, sc.W * sc.H]
    assert PC.summary(ex[0][0])[1] > 1000 and PC.summary(ex[2][0])[1] > 1000
    ctx = cloud_context(sc)
    buf = run(ctx, lists, 4, ex, "neighbours r=4")
    assert buf.host()[2][1].tolist() == [sc.W * sc.H, 0, 0, sc.W * sc.H]
    ctx.close()


@gpu
def test_round_trip_of_the_compacted_cloud():
    """rtuf_cloud_compact_batch_device's output fed straight back, device counts and all: every point is kept and lands on the
    pixel the cloud's index names."""
    name = "soup_160x120"
    sc = scene(name)
    ctx = cloud_context(sc)
    cap = sc.W * sc.H
    cloud = CloudBuffers(sc, sc.n, cap)
    d = upload(sc.depth)                          # (kept alive while the cloud batch reads it)
    cloud_enqueue(ctx, d, sc.n, cloud)
    torch, dev = torch_device()
    verdict = torch.full((sc.n, cap), SENT8, dtype=torch.uint8, device=dev)
    pixel = torch.full((sc.n, cap), SENT32, dtype=torch.int32, device=dev)
    summary = torch.full((sc.n, 4), SENT32, dtype=torch.int32, device=dev)
    ctx.sync()                                    # (the points batch reads what the cloud batch wrote: ordered by the host here)
    ctx.points_batch_device(sc.n, cloud.points.data_ptr(), cloud.counts.data_ptr(), cap, 0, verdict.data_ptr(), pixel.data_ptr(), summary.data_ptr())
    ctx.sync()
    _, index, counts = cloud.host()
    v, p, sm = verdict.cpu().numpy(), np.ascontiguousarray(pixel.cpu().numpy()).view(np.uint32), np.ascontiguousarray(summary.cpu().numpy()).view(np.uint32)
    for s in range(sc.n):
        m = int(counts[s])
        assert m > 100
        assert (v[s, :m] == PC.KEPT).all() and (v[s, m:] == SENT8).all(), "stream %d" % s
        assert np.array_equal(p[s, :m], index[s, :m]), "stream %d: pixels" % s
        assert sm[s].tolist() == [m, 0, 0, m]
    ctx.close()


# ---- batch machinery ---------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("kw", [dict(raster_lanes=1), dict(raster_lanes=3), dict(pipelines=2), dict(max_inflight_streams=1, raster_lanes=3),
                                dict(flags=R.FLAG_TWO_KERNEL)],
                         ids=["one_lane", "three_lanes", "two_pipelines", "three_groups", "two_kernel_flag"])
def test_lanes_pipelines_and_launch_groups(kw):
    name = "soup_160x120"
    sc = scene(name)
    lists, matrices = mixed_lists(name)
    ctx = cloud_context(sc, **kw)
    for s, m in enumerate(matrices):
        if m is not None:
            ctx.set_point_transforms(s, m)
    for r in (0, 2):
        run(ctx, lists, r, expected(name, lists, r, matrices), "%s r=%d" % (kw, r))
    if "max_inflight_streams" in kw:
        assert ctx.stats()["groups_last_batch"] == 3
    ctx.close()


@gpu
def test_partial_batch_leaves_the_other_streams_alone():
    name = "soup_160x120"
    sc = scene(name)
    lists = grid_lists(name)
    ctx = cloud_context(sc)
    buf = PointBuffers(lists[:2], total=3)
    buf.counts_host[2] = 5                        # (a count beyond the batch: never read)
    buf.counts.copy_(torch_device()[0].from_numpy(buf.counts_host.view(np.int32)))
    buf.enqueue(ctx, 2, 0)
    ctx.sync()
    check(buf.host(), expected(name, lists[:2], 0), buf.counts_host, buf.cap, "2 of 3 streams", n=2)
    ctx.close()


@gpu
def test_two_batches_in_flight_with_outputs_of_their_own():
    name = "soup_160x120"
    sc = scene(name)
    grid, (mixed, matrices) = grid_lists(name), mixed_lists(name)
    ctx = cloud_context(sc)
    ctx.filter_batch(sc.depth)                    # (sizes the bins: the batches below are final at once)
    a, b = PointBuffers(grid), PointBuffers(mixed)
    a.enqueue(ctx, sc.n, 0)
    b.enqueue(ctx, sc.n, 2)
    ctx.sync()
    assert ctx.stats()["batch_reruns"] == 0
    check(a.host(), expected(name, grid, 0), a.counts_host, a.cap, "first in flight")
    check(b.host(), expected(name, mixed, 2), b.counts_host, b.cap, "second in flight")
    ctx.close()


@gpu
def test_regrown_bins_rerun_rewrites_verdicts_and_summary():
    name = "soup_160x120"
    sc = scene(name)
    lists = grid_lists(name)
    ctx = cloud_context(sc, bin_capacity=1)
    ex = expected(name, lists, 2)
    buf = PointBuffers(lists)
    buf.enqueue(ctx, sc.n, 2)
    ctx.sync()
    st = ctx.stats()
    assert st["regrowths"] >= 1 and st["batch_reruns"] >= 1 and st["batch_status"] != 0, st
    check(buf.host(), ex, buf.counts_host, buf.cap, "re-run")          # (the summary is that of one run)
    buf.enqueue(ctx, sc.n, 2)                     # the next batch is final at once
    ctx.sync()
    assert ctx.stats()["batch_status"] == 0
    check(buf.host(), ex, buf.counts_host, buf.cap, "after the re-run")
    ctx2 = cloud_context(sc, bin_capacity=1)
    check_host_form(ctx2, lists, 0, expected(name, lists, 0), "re-run, host form")
    assert ctx2.stats()["batch_reruns"] >= 1
    ctx2.close()
    ctx.close()


@gpu
def test_graph_replay_follows_new_contents_of_the_same_buffers():
    """One raster lane, pipelines = 2, one stream: small batches replay a captured graph, the summary's zeroing and the points
    kernel included.  The same buffers every time; points, counts and poses change in between."""
    torch, dev = torch_device()
    name = "soup_160x120"
    sc = scene(name)
    lists = grid_lists(name)
    ctx = cloud_context(sc, n=1, max_streams=1, raster_lanes=1, pipelines=2)
    buf = PointBuffers([lists[0]])
    for i in range(12):
        s = i % sc.n
        ctx.set_cameras(0, sc.wl.projection[s:s + 1], sc.wl.offset_inv[s:s + 1], sc.wl.cam_tf[s:s + 1])
        ctx.set_link_poses_batch(0, 0, sc.wl.link_tf[0][s:s + 1])
        count = buf.cap - 37 * i
        pts = np.full((buf.cap, 3), np.nan, F)
        pts[:count] = PC.grid_points(sc.depth[s], intrinsics(sc, 0))[:count]      # (slot 0's pinhole shows stream s)
        buf.points.copy_(torch.from_numpy(pts.reshape(-1)))
        buf.counts.copy_(torch.from_numpy(np.array([count], np.int32)))
        buf.verdict.fill_(SENT8)
        buf.pixel.fill_(SENT32)
        torch.cuda.synchronize()
        buf.enqueue(ctx, 1, 1)
        ctx.sync()
        ex = expected(name, [pts[:count]], 1, streams=(s,))
        check(buf.host(), ex, [count], buf.cap, "replay %d" % i)
    st = ctx.stats()
    assert st["graphs_enabled"] == 1 and st["graph_hits"] >= 3, st
    ctx.close()


@gpu
def test_status_word_is_zero_behind_a_final_points_batch():
    name = "soup_160x120"
    sc = scene(name)
    lists = grid_lists(name)
    ctx = cloud_context(sc)
    ctx.filter_batch(sc.depth)                    # (bins sized)
    buf = PointBuffers(lists)
    user = Consumer(ctx)
    buf.enqueue(ctx, sc.n, 0)
    word, early_verdict, early_summary, _ = user.read(buf.verdict, buf.summary)
    assert word == 0, hex(word)
    ex = expected(name, lists, 0)
    for s in range(sc.n):
        assert np.array_equal(early_verdict[s], ex[s][0]), "behind the batch, stream %d" % s
        assert np.ascontiguousarray(early_summary).view(np.uint32)[s].tolist() == PC.summary(ex[s][0]).tolist()
    ctx.sync()
    st = ctx.stats()
    assert st["batch_status"] == 0 and st["batch_reruns"] == 0, st
    ctx.close()


# ---- refusals and statistics ----------------------------------------------------------------------------------------------------------

@gpu
def test_refusals_enqueue_nothing_and_a_good_call_still_matches():
    name = "soup_100x75"
    sc = scene(name)
    lists = grid_lists(name)
    buf = PointBuffers(lists)

    def refused(code, call):
        with pytest.raises(R.RtufError) as e:
            call()
        assert e.value.code == code, e.value

    def device_call(n=sc.n, points=True, counts=True, verdict=True, cap=None, r=0):
        ctx.points_batch_device(n, buf.points.data_ptr() if points else None, buf.counts.data_ptr() if counts else None,
                                buf.cap if cap is None else cap, r, buf.verdict.data_ptr() if verdict else None, buf.pixel.data_ptr(), buf.summary.data_ptr())

    def base_params(**kw):
        p = params(replace=sc.wl.replace_value, max_diff=sc.wl.max_diff, **kw)
        p.near_plane, p.far_plane = sc.wl.near, sc.wl.far
        return p

    ctx = R.Context(sc.W, sc.H, sc.n, 0, base_params())
    refused(STATE, device_call)                                               # before finalize
    ids = sc.wl.load_into(ctx)
    sc.wl.stage(ctx, ids)
    refused(STATE, device_call)                                               # no intrinsics at all
    refused(STATE, lambda: ctx.points_batch(lists))
    ctx.set_cloud_intrinsics(0, [intrinsics(sc, i) for i in range(2)])
    refused(STATE, device_call)                                               # stream 2 has none yet
    ctx.set_cloud_intrinsics(2, intrinsics(sc, 2))
    refused(INVALID, lambda: device_call(points=False))                       # NULL arrays
    refused(INVALID, lambda: device_call(counts=False))
    refused(INVALID, lambda: device_call(verdict=False))
    refused(INVALID, lambda: device_call(n=0))                                # n out of range
    refused(INVALID, lambda: device_call(n=sc.n + 1))
    for cap in (0, -3, (1 << 24) + 1):
        refused(INVALID, lambda: device_call(cap=cap))
    for r in (-1, 5):
        refused(INVALID, lambda: device_call(r=r))
        refused(INVALID, lambda: ctx.points_batch(lists, r))
    ctx.set_params(base_params(silhouette_dilation_px=2))                     # not supported yet: dilation ...
    refused(INVALID, device_call)
    refused(INVALID, lambda: ctx.points_batch(lists))
    ctx.set_params(base_params())
    ctx.set_link_padding(ids[0], np.full(sc.n_links, 0.02, F))                # ... link padding ...
    refused(INVALID, device_call)
    ctx.clear_link_padding(ids[0])
    ctx.set_link_thresholds(ids[0], np.full(sc.n_links, 0.1, F))              # ... and per-link thresholds
    refused(INVALID, device_call)
    ctx.clear_link_thresholds(ids[0])
    ctx.sync()
    torch_device()[0].cuda.synchronize()
    assert buf.untouched()
    ex = expected(name, lists, 0)
    buf.enqueue(ctx, sc.n, 0)
    ctx.sync()
    check(buf.host(), ex, buf.counts_host, buf.cap, "after the refusals")
    ctx.close()


@gpu
def test_the_plane_is_counted_in_device_bytes_and_timings_land_in_ms_compare():
    name = "soup_160x120"
    sc = scene(name)
    lists = grid_lists(name)
    ctx = cloud_context(sc)
    ctx.filter_batch(sc.depth)
    before = ctx.stats()["device_bytes"]
    ctx.enable_timing(2)
    buf = PointBuffers(lists)
    buf.enqueue(ctx, sc.n, 0)
    ctx.sync()
    st = ctx.stats()
    assert st["device_bytes"] - before >= sc.n * sc.W * sc.H * 4, (before, st["device_bytes"])
    assert st["ms_compare"] > 0 and st["ms_raster"] > 0, st
    check(buf.host(), expected(name, lists, 0), buf.counts_host, buf.cap, "timed")
    ctx.close()
