"""GPU (-m gpu): batches of fewer streams than the context was created for (1 <= n < max_streams).

Every rtuf_filter_batch* entry takes the first n of up to max_streams streams.  A partial batch is split into launch groups by
its own n -- and can make MORE groups than a full batch (3 lanes, groups of 8, max_streams 64: a full batch makes 8 groups, a
batch of 49 makes 9; tests/launch_groups_check.cpp).  These tests run partial batches through every entry point and every
split: each frame is the CPU oracle's bit for bit, streams n .. max_streams - 1 of the caller's buffers stay untouched, every
batch reports no more launch groups than its slot has counter blocks, and the status word read from a consumer's stream is 0
when the planes it saw were final.  Streams beyond n are staged with cameras and depth of their own, so a launch group that
renders the wrong stream -- an uneven last group's offset into the planes, a stale upload -- shows up."""
import ctypes
import functools

import numpy as np
import pytest

import launch_groups as LG
import scenes as S
import realtime_urdf_filter_amd as R
from gpu_support import Consumer, OracleScene, bits_equal, unpack_bits, workload_of
from realtime_urdf_filter_amd.filter import depth_f32_to_u16, depth_u16_to_f32

pytestmark = pytest.mark.gpu

SENTINEL_F32 = np.uint32(0x7FC0A5A5)          # a NaN bit pattern no kernel writes
SENTINEL_U8 = 0xA5
RTUF_ERR_INVALID = -1


class Scene(OracleScene):
    """A soup model and M streams, each with its own camera, link poses and sensor plane; the oracle's frames for all M."""

    def want(self, s):
        return self.masked[s], self.mask[s]

    @functools.cached_property
    def _u16(self):
        sc = OracleScene(self.wl, depth_u16_to_f32(self.mm))
        return depth_f32_to_u16(sc.masked), sc.mask

    def want16(self, s):
        return self._u16[0][s], self._u16[1][s]

    def exact(self, n, masked, mask, u16=False):
        """Streams 0 .. n-1 of (masked, mask) are the oracle's frames (mask None: not checked)."""
        for s in range(n):
            om, ok = self.want16(s) if u16 else self.want(s)
            if mask is not None and not np.array_equal(ok, mask[s]):
                return False
            if not (np.array_equal(om, masked[s]) if u16 else bits_equal(om, masked[s])):
                return False
        return True

    def check(self, n, masked, mask, u16=False, what=""):
        for s in range(n):
            om, ok = self.want16(s) if u16 else self.want(s)
            if mask is not None:
                assert np.array_equal(ok, mask[s]), "%s stream %d of %d: mask differs in %d pixels" % (what, s, n, int((ok != mask[s]).sum()))
            same = np.array_equal(om, masked[s]) if u16 else bits_equal(om, masked[s])
            assert same, "%s stream %d of %d: masked depth differs" % (what, s, n)


def scene(W, H, M, seed, **pkw):
    """The scene with its context (sc.ctx, parameters pkw) of M streams, every one of them staged."""
    rng = np.random.default_rng(seed)
    P = S.projection(525.0 * W / 640, 525.0 * W / 640, (W - 1) / 2, (H - 1) / 2, W, H)
    geo = S.soup_geometry(rng, n_links=7, tris_per_link=50)
    tfs, cams = [], []
    for s in range(M):
        tfs.append(np.stack(S.random_link_poses(rng, len(geo), near=(s % 3 == 1), far=(s % 3 == 2))))
        cams.append(S.random_camera(rng, small=bool(s & 1)))
    wl = workload_of("partial_%dx%d_%d" % (W, H, M), W, H, geo, np.stack(tfs), np.tile(P, (M, 1)), np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
    sc = Scene(wl, np.stack([S.sensor_depth(W, H, 0.3 * s + seed) for s in range(M)]))
    sc.M = M
    sc.mm = depth_f32_to_u16(np.nan_to_num(sc.depth, nan=0.0, posinf=0.0))
    sc.ctx = sc.context(**pkw)
    return sc


def untouched(a, n, what):
    """Streams n.. of a buffer pre-filled with the sentinel still hold it, byte for byte."""
    rest = np.ascontiguousarray(a[n:]).view(np.uint8).reshape(-1)
    if a.dtype == np.float32:
        want = np.full(a[n:].shape, SENTINEL_F32, np.uint32).view(np.uint8).reshape(-1)
    else:
        want = np.full(rest.shape, SENTINEL_U8, np.uint8)
    assert np.array_equal(rest, want), "%s: streams %d.. were written" % (what, n)


def fill(a):
    if a.dtype == np.float32:
        a.view(np.uint32)[...] = SENTINEL_F32
    else:
        a.view(np.uint8)[...] = SENTINEL_U8


def check_groups(ctx, n):
    """The last batch made the launch groups the rule gives for n at the context's launch group, within its counter blocks."""
    st = ctx.stats()
    lanes, group = st["raster_lanes"], st["launch_group"]
    assert st["counter_blocks"] == LG.counter_blocks_for(ctx.max_streams, group, lanes), st
    assert st["groups_last_batch"] == LG.groups_for(n, group, lanes) <= st["counter_blocks"], (n, st)
    return st


def host_call(ctx, fn, n, depth, masked, mask):
    """The synchronous host-plane entries with planes 0 .. n-1 of larger arrays (the Python wrapper allocates its own)."""
    PP = ctypes.c_void_p * n
    din = PP(*[depth[i].ctypes.data for i in range(n)])
    mout = PP(*[masked[i].ctypes.data for i in range(n)])
    kout = PP(*[mask[i].ctypes.data for i in range(n)]) if mask is not None else None
    ctx._check(getattr(ctx._lib, fn)(ctx._h, n, din, mout, kout))


def torch_sentinel(torch, shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda:0")
    if dtype == torch.float32:
        t.view(torch.int32).fill_(int(np.array(SENTINEL_F32).view(np.int32)))
    else:
        t.view(torch.uint8).fill_(SENTINEL_U8)
    return t


def device_batch(sc, n, user=None):
    """One batch of n streams through device planes of M streams; returns (status word seen by the consumer or None,
    early planes ok or None) after checking the retired batch."""
    import torch
    ctx, M, H, W = sc.ctx, sc.M, sc.H, sc.W
    d = torch.from_numpy(sc.depth).to("cuda:0")
    masked = torch_sentinel(torch, (M, H, W), torch.float32)
    mask = torch_sentinel(torch, (M, H, W), torch.uint8)
    torch.cuda.synchronize()
    ctx.filter_batch_device(n, d.data_ptr(), masked.data_ptr(), mask.data_ptr())
    word = early_ok = None
    if user is not None:
        word, early_m, early_k, _ = user.read(masked, mask)
        early_ok = sc.exact(n, early_m, early_k)
    ctx.sync()
    torch.cuda.synchronize()
    got_m, got_k = masked.cpu().numpy(), mask.cpu().numpy()
    sc.check(n, got_m, got_k, what="device n=%d" % n)
    untouched(got_m, n, "masked"); untouched(got_k, n, "mask")
    return word, early_ok


# ---------------------------------------------------------------------------------------------
# (lanes, max_inflight_streams, M, n): the partial batches that made more groups than a full one (lanes 3 group 8 M 64 n 49:
# 9 > 8; group 6: 12 > 11; M 128 n 121: 18 > 16; 2 lanes M 72 n 65: 10 > 9; group 5 M 33 n 32: 8 > 7), n = 1,
# kSplitMin - 1, kSplitMin and M - 1, and one lane with a group set by the caller
SPLITS = [(3, 8, 64, 49), (3, 6, 64, 56), (3, 6, 64, 60), (3, 8, 128, 121), (2, 8, 72, 65), (2, 5, 33, 32),
          (3, 8, 64, 1), (3, 8, 64, LG.SPLIT_MIN - 1), (3, 8, 64, LG.SPLIT_MIN), (3, 8, 64, 63),
          (1, 5, 40, 37), (1, 5, 40, 11)]


@pytest.mark.parametrize("lanes,group,M,n,size", [sp + ((128, 96),) for sp in SPLITS] +
                         [sp + ((131, 77),) for sp in ((3, 8, 64, 49), (2, 5, 33, 32), (1, 5, 40, 37))])
def test_partial_batch_split_matrix(lanes, group, M, n, size):
    """131 x 77: the last tile row and column are partial."""
    sc = scene(size[0], size[1], M, seed=1000 + 7 * n + M + lanes, max_inflight_streams=group, raster_lanes=lanes)
    ctx = sc.ctx
    st = ctx.stats()
    assert st["launch_group"] == group and st["counter_blocks"] == LG.counter_blocks_for(M, group, lanes), st
    user = Consumer(ctx)
    device_batch(sc, n)                                 # (bins and grid estimates settled by a batch of this split)
    check_groups(ctx, n)
    word, early_ok = device_batch(sc, n, user)
    st = check_groups(ctx, n)
    assert word == 0 and early_ok, hex(word)
    assert st["batch_status"] == 0 and st["batch_reruns"] == 0, st
    ctx.close()


def test_memory_limit_shrink_then_partial_batches():
    """3 lanes, 64 streams, bins of one record under a 1 MiB limit: the context starts at launch groups of 6 streams (12
    counter blocks: 56 .. 60 streams make 12 groups, a full batch 11), and the first batch -- one of those -- overflows, grows
    the bins and shrinks the launch group again, so the counter blocks are allocated anew under a batch in flight.  Then a
    full batch, up to five of the partial batches that need more groups than a full one at the new launch group (there may
    be none: groups of 2 streams have none), and a full batch after them."""
    M, lanes = 64, 3
    sc = scene(128, 96, M, seed=79, bin_capacity=1, memory_limit_mb=1, raster_lanes=lanes)
    ctx = sc.ctx
    before = ctx.stats()
    g0 = before["launch_group"]
    assert before["counter_blocks"] == LG.counter_blocks_for(M, g0, lanes), before
    over = [n for n in range(1, M) if LG.groups_for(n, g0, lanes) > LG.groups_for(M, g0, lanes)]
    assert g0 == 6 and over == [56, 57, 58, 59, 60], (before, over)      # 3 lanes x 6 streams x 6 tiles x (32 + 1024 x 8) B = 0.85 MiB
    device_batch(sc, over[0])
    st = check_groups(ctx, over[0])
    assert st["regrowths"] >= 1 and st["launch_group"] < g0, st
    device_batch(sc, M)                                 # (bins grown for the streams the first batch did not have)
    g1 = check_groups(ctx, M)["launch_group"]
    over = [n for n in range(1, M) if LG.groups_for(n, g1, lanes) > LG.groups_for(M, g1, lanes)]
    print("launch group %d -> %d; partial batches that need more groups than a full one: %s" % (g0, g1, over))
    for n in over[:: max(1, len(over) // 4)] + [M]:
        device_batch(sc, n)
        st = check_groups(ctx, n)
        assert st["launch_group"] == g1, st
    ctx.close()


def test_every_entry_point_at_a_partial_batch():
    """3 lanes, groups of 8, M = 64, n = 49: nine launch groups, one more than a full batch makes.  Every entry takes planes
    0 .. 48 of buffers sized for 64 streams and pre-filled with a sentinel; streams 49 .. 63 stay untouched."""
    import torch
    M, n = 64, 49
    sc = scene(128, 96, M, seed=80, max_inflight_streams=8, raster_lanes=3)
    ctx, H, W = sc.ctx, sc.H, sc.W
    assert LG.groups_for(n, 8, 3) == 9 > LG.groups_for(M, 8, 3) and ctx.stats()["counter_blocks"] == 9
    words = ctx.mask_bits_words()

    def bits_ok(bits, u16):
        for s in range(n):
            ok = (sc.want16(s) if u16 else sc.want(s))[1]
            assert np.array_equal(unpack_bits(bits[s], W, H), ok > 0), s
        untouched(bits, n, "bits")

    # synchronous host planes, float and 16UC1 (plain numpy arrays)
    for fn, src, dt, u16 in (("rtuf_filter_batch", sc.depth, np.float32, False), ("rtuf_filter_batch_u16", sc.mm, np.uint16, True)):
        masked = np.empty((M, H, W), dt); mask = np.empty((M, H, W), np.uint8)
        fill(masked); fill(mask)
        host_call(ctx, fn, n, src, masked, mask)
        check_groups(ctx, n)
        sc.check(n, masked, mask, u16=u16, what=fn)
        untouched(masked, n, fn); untouched(mask, n, fn)
    # asynchronous host planes (pinned), float and 16UC1, and the bits output, all three in flight two at a time
    pin = {}
    for dt in (np.float32, np.uint16):
        pin[dt] = (ctx.host_alloc((M, H, W), dt), ctx.host_alloc((M, H, W), dt), ctx.host_alloc((M, H, W), np.uint8))
        pin[dt][0][...] = sc.depth if dt == np.float32 else sc.mm
        fill(pin[dt][1]); fill(pin[dt][2])
    bits = ctx.host_alloc((M, words), np.uint32)
    bits.view(np.uint8)[...] = SENTINEL_U8
    ctx.filter_batch_async(pin[np.float32][0][:n], pin[np.float32][1][:n], pin[np.float32][2][:n])
    ctx.filter_batch_async(pin[np.uint16][0][:n], pin[np.uint16][1][:n], pin[np.uint16][2][:n])
    ctx.wait_oldest()
    check_groups(ctx, n)
    ctx.filter_batch_bits_async(pin[np.float32][0][:n], bits[:n])
    ctx.sync()
    check_groups(ctx, n)
    for dt, u16 in ((np.float32, False), (np.uint16, True)):
        _, masked, mask = pin[dt]
        sc.check(n, masked, mask, u16=u16, what="async %s" % np.dtype(dt).name)
        untouched(masked, n, "async masked"); untouched(mask, n, "async mask")
    bits_ok(np.array(bits), False)
    # device planes: float, 16UC1, bits
    user = Consumer(ctx)
    word, early_ok = device_batch(sc, n, user)
    assert word == 0 and early_ok, hex(word)
    st = check_groups(ctx, n)
    assert st["batch_status"] == 0, st
    d16 = torch.from_numpy(sc.mm.view(np.int16)).to("cuda:0")
    m16 = torch.empty((M, H, W), dtype=torch.int16, device="cuda:0"); m16.view(torch.uint8).fill_(SENTINEL_U8)
    k16 = torch_sentinel(torch, (M, H, W), torch.uint8)
    d32 = torch.from_numpy(sc.depth).to("cuda:0")
    dbits = torch.empty((M, words), dtype=torch.int32, device="cuda:0"); dbits.view(torch.uint8).fill_(SENTINEL_U8)
    torch.cuda.synchronize()
    ctx.filter_batch_device_u16(n, d16.data_ptr(), m16.data_ptr(), k16.data_ptr())
    ctx.filter_batch_device_bits(n, d32.data_ptr(), dbits.data_ptr())
    ctx.sync()
    check_groups(ctx, n)
    torch.cuda.synchronize()
    got16, gotk = m16.cpu().numpy().view(np.uint16), k16.cpu().numpy()
    sc.check(n, got16, gotk, u16=True, what="device u16")
    untouched(got16, n, "device u16 masked"); untouched(gotk, n, "device u16 mask")
    bits_ok(dbits.cpu().numpy().view(np.uint32), False)
    ctx.close()


def test_batch_size_changes_between_batches_in_flight():
    """One context (3 lanes, groups of 8, M = 64) through n = 64, 49, 1, 33, 64, 7, 49, two batches in flight, retired by
    wait_oldest.  A batch's per-group grid estimates come from the last retired batch, which may have been split otherwise:
    a grid that turns out short is run again (allowed), but the status word a consumer reads must then be non-zero -- and
    0 exactly when the planes it saw were the oracle's.  After retirement every frame is exact."""
    import torch
    M = 64
    sc = scene(128, 96, M, seed=81, max_inflight_streams=8, raster_lanes=3)
    ctx, H, W = sc.ctx, sc.H, sc.W
    d = torch.from_numpy(sc.depth).to("cuda:0")
    user = Consumer(ctx)
    inflight, seen = [], []
    for i, n in enumerate((M, 49, 1, 33, M, 7, 49)):
        masked = torch_sentinel(torch, (M, H, W), torch.float32)
        mask = torch_sentinel(torch, (M, H, W), torch.uint8)
        torch.cuda.synchronize()
        if len(inflight) == 2:
            ctx.wait_oldest()
            retire(sc, *inflight.pop(0))
        ctx.filter_batch_device(n, d.data_ptr(), masked.data_ptr(), mask.data_ptr())
        word, early_m, early_k, _ = user.read(masked, mask)
        early_ok = sc.exact(n, early_m, early_k)
        assert (word & R.STATUS_PENDING_MASK) == 0 and (word == 0) == early_ok, (i, n, hex(word), early_ok)
        seen.append((n, word))
        inflight.append((n, masked, mask))
    while inflight:
        ctx.wait_oldest()
        retire(sc, *inflight.pop(0))
    print("n, status word:", [(n, hex(w)) for n, w in seen])
    ctx.close()


def retire(sc, n, masked, mask):
    import torch
    torch.cuda.synchronize()
    st = check_groups(sc.ctx, n)
    got_m, got_k = masked.cpu().numpy(), mask.cpu().numpy()
    sc.check(n, got_m, got_k, what="n=%d" % n)
    untouched(got_m, n, "masked n=%d" % n); untouched(got_k, n, "mask n=%d" % n)
    return st


def test_graph_cache_never_replays_another_batch_size():
    """Small batches of one-lane pipelines replay a captured hipGraph keyed by the batch's plan.  n alternates 5, 7, 5, 7 on
    every batch slot with the same buffers, three times: the repeats must be replays (graph_hits rises), and each replay must be of its
    own size -- the outputs are exact and streams beyond n untouched, so a graph of 5 streams never stands in for 7."""
    import torch
    M = 8
    sc = scene(128, 96, M, seed=82, pipelines=2)
    ctx, H, W = sc.ctx, sc.H, sc.W
    d = torch.from_numpy(sc.depth).to("cuda:0")
    masked = torch.empty((M, H, W), dtype=torch.float32, device="cuda:0")
    mask = torch.empty((M, H, W), dtype=torch.uint8, device="cuda:0")
    # two pipelines take the batches in turn and each has two slots: batch i lands on pipeline i % 2, slot (i // 2) % 2
    sizes = [5 if (i // 4) % 2 == 0 else 7 for i in range(24)]
    hits = []
    for n in sizes:
        masked.view(torch.int32).fill_(int(np.array(SENTINEL_F32).view(np.int32))); mask.fill_(SENTINEL_U8)
        torch.cuda.synchronize()
        ctx.filter_batch_device(n, d.data_ptr(), masked.data_ptr(), mask.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        got_m, got_k = masked.cpu().numpy(), mask.cpu().numpy()
        sc.check(n, got_m, got_k, what="n=%d" % n)
        untouched(got_m, n, "masked n=%d" % n); untouched(got_k, n, "mask n=%d" % n)
        st = ctx.stats()
        assert st["groups_last_batch"] == 1 and st["counter_blocks"] == 1 and st["graphs_enabled"] == 1, st
        hits.append(st["graph_hits"])
    print("graph hits after each batch:", hits, "misses:", st["graph_misses"])
    assert st["graph_hits"] + st["graph_misses"] == len(sizes), st
    # every (pipeline, slot) has seen both sizes after the first 8 batches (both cover-pass states after 16: it switches off
    # after three batches without whole-tile triangles); the third round of 8 is replays only
    assert hits[15] > hits[7] and hits[23] - hits[15] == 8, hits
    ctx.close()


@pytest.mark.parametrize("bad", ["zero", "over"])
def test_batch_sizes_outside_1_to_max_streams_are_refused(bad):
    """n = 0 and n = max_streams + 1 are refused by every entry (buffers for max_streams + 1 streams: nothing is written
    out of bounds even if one were not), and the context filters exactly afterwards."""
    import torch
    M = 40
    sc = scene(128, 96, M, seed=83, max_inflight_streams=8, raster_lanes=3)
    ctx, H, W = sc.ctx, sc.H, sc.W
    n = 0 if bad == "zero" else M + 1
    N = M + 1
    depth = np.concatenate([sc.depth, sc.depth[:1]])
    mm = np.concatenate([sc.mm, sc.mm[:1]])
    masked = np.empty((N, H, W), np.float32); mask = np.empty((N, H, W), np.uint8); masked16 = np.empty((N, H, W), np.uint16)
    words = ctx.mask_bits_words()
    bits = np.empty((N, words), np.uint32)
    dd = torch.from_numpy(depth).to("cuda:0"); d16 = torch.from_numpy(mm.view(np.int16)).to("cuda:0")
    dm = torch.empty((N, H, W), dtype=torch.float32, device="cuda:0"); dk = torch.empty((N, H, W), dtype=torch.uint8, device="cuda:0")
    dm16 = torch.empty((N, H, W), dtype=torch.int16, device="cuda:0"); db = torch.empty((N, words), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    calls = {
        "filter_batch": lambda: ctx.filter_batch(depth[:n]),
        "filter_batch_u16": lambda: ctx.filter_batch_u16(mm[:n]),
        "filter_batch_async": lambda: ctx.filter_batch_async(depth[:n], masked[:n], mask[:n]),
        "filter_batch_async_u16": lambda: ctx.filter_batch_async(mm[:n], masked16[:n], mask[:n]),
        "filter_batch_bits_async": lambda: ctx.filter_batch_bits_async(depth[:n], bits[:n]),
        "filter_batch_device": lambda: ctx.filter_batch_device(n, dd.data_ptr(), dm.data_ptr(), dk.data_ptr()),
        "filter_batch_device_u16": lambda: ctx.filter_batch_device_u16(n, d16.data_ptr(), dm16.data_ptr(), dk.data_ptr()),
        "filter_batch_device_bits": lambda: ctx.filter_batch_device_bits(n, dd.data_ptr(), db.data_ptr()),
        "filter_batch_device_bits_u16": lambda: ctx.filter_batch_device_bits(n, d16.data_ptr(), db.data_ptr(), u16=True),
    }
    for name, call in calls.items():
        with pytest.raises(R.RtufError) as e:
            call()
        assert e.value.code == RTUF_ERR_INVALID, (name, e.value)
    device_batch(sc, 33)
    check_groups(ctx, 33)
    ctx.close()
