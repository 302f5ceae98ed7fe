"""GPU (-m gpu, except the check of the order itself): batches of different kinds behind each other in the same two batch slots.

A context keeps two batch slots, and the batch enqueued two calls later takes the slot over.  The tests of each kind -- filter
(masked / mask planes, with and without link labels, f32 and 16UC1), mask bits, render, link residuals, point clouds -- run that
kind alone; here every kind follows every other one in a slot, with device buffers and with host planes, across a re-run after
a bin regrowth, and through captured graphs.

One scene, soup_scene(1, 160, 120), three streams.  Every expectation comes from the CPU oracle through the kinds' shared
helpers (tests/gpu_support.py) and bench_support/{cloud,residuals,virtual,labels}_check.py, never from the library; every comparison is bit for bit."""
import numpy as np
import pytest

import gpu_support as K
from gpu_support import pack_bits, soup_scene, torch_device
from realtime_urdf_filter_amd.filter import depth_f32_to_u16

gpu = pytest.mark.gpu
KINDS = ("filter", "bits", "render", "residual", "cloud")
LINK_LABEL = (3, 7, 7, 1, 12, 5)             # of the scene's six links: two share a label, the order is not the links'
N_LABELS = 13
SENT16, SENT32, SENT64 = 0x5a5a, 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a
EMPTY = 0.25
CAP = 9000                                    # compacted clouds: below stream 0's 9976 kept pixels, above the others'


class World:
    """The scene with the expectations of every kind, built once."""

    def __init__(self):
        self.sc = soup_scene(1, 160, 120)
        sc = self.sc
        assert sc.n == 3 and len(LINK_LABEL) == sum(len(links) for links in sc.wl.models)
        self.depth16 = depth_f32_to_u16(sc.depth)
        self.virtual, self.labels = K.virtual_planes(sc, EMPTY), K.label_planes(sc, LINK_LABEL)
        self.table = {u16: K.residual_tables(sc, self.sensor(u16), N_LABELS, link_label=LINK_LABEL) for u16 in (False, True)}
        self.bits = {u16: np.stack([pack_bits(m) for m in K.filter_expected(sc, 0, u16)[1]]) for u16 in (False, True)}

    def sensor(self, u16):
        return self.depth16 if u16 else self.sc.depth

    def context(self, **kw):
        ctx = K.cloud_context(self.sc, **kw)
        ctx.set_link_labels(0, np.array(LINK_LABEL, np.uint16))
        return ctx

    # -- expectations of streams `streams` against host arrays ---------------------------------------------------------------
    def check_filter(self, masked, mask, labels, u16, what, streams=(0, 1, 2)):
        em, ek = K.filter_expected(self.sc, 0, u16)
        for i, s in enumerate(streams):
            view = np.uint16 if u16 else np.uint32
            assert np.array_equal(np.ascontiguousarray(masked[i]).view(view), em[s].view(view)), "%s stream %d: masked depth" % (what, s)
            assert mask is None or np.array_equal(mask[i], ek[s]), "%s stream %d: mask" % (what, s)
            assert labels is None or np.array_equal(labels[i], self.labels[s]), "%s stream %d: labels" % (what, s)

    def check_bits(self, bits, u16, what, streams=(0, 1, 2)):
        for i, s in enumerate(streams):
            assert np.array_equal(np.asarray(bits[i]).reshape(-1), self.bits[u16][s]), "%s stream %d: mask bits" % (what, s)

    def check_render(self, virt, labels, what, streams=(0, 1, 2)):
        K.same_planes(np.asarray(virt), self.virtual[list(streams)], what)
        if labels is not None:
            K.compare_labels(labels, self.labels[list(streams)], what)

    def check_table(self, table, u16, what, streams=(0, 1, 2)):
        K.check_tables(table, self.table[u16][list(streams)], what)

    def check_cloud(self, points, index, counts, u16, cap, what, streams=(0, 1, 2)):
        ex = K.cloud_expect(self.sc, 0, u16, streams)
        if cap is None:
            K.check_org(points, ex, what)
        else:
            K.check_comp(points, index, counts, ex, cap, what)


_world = []


def world():
    if not _world:
        _world.append(World())
    return _world[0]


def slot_order():
    """Kinds in an order in which every ordered pair of different kinds is two calls apart somewhere: the four Hamiltonian cycles
    0, d, 2d, .. (mod 5) visit every ordered pair once as neighbours, and every entry is enqueued twice in a row."""
    walk = [(i * d) % 5 for d in (1, 2, 3, 4) for i in range(5)] + [0]
    return [KINDS[k] for k in walk for _ in range(2)]


def pairs_two_apart(order):
    return {(a, b) for a, b in zip(order, order[2:]) if a != b}


def test_the_order_puts_every_kind_behind_every_other():
    assert len(pairs_two_apart(slot_order())) == 20 == len(KINDS) * (len(KINDS) - 1)


# ---- device buffers ----------------------------------------------------------------------------------------------------------------

class DeviceJob:
    """One batch of `kind` (variant `v` of it) on device buffers of its own for all three streams, sentinel-filled; n streams of
    them are computed."""

    def __init__(self, w, kind, v, n):
        torch, dev = torch_device()
        self.w, self.kind, self.n = w, kind, n
        sc = w.sc
        self.u16 = bool(v & 1)
        self.with_labels = kind in ("filter", "render") and bool(v & 2)
        self.cap = CAP if kind == "cloud" and v & 2 else None
        self.what = "%s variant %d n=%d" % (kind, v, n)
        shape = (3, sc.H, sc.W)
        full = lambda sh, val, dt: torch.full(sh, val, dtype=dt, device=dev)
        self.d = K.upload(w.sensor(self.u16))
        self.out = {}
        if kind == "filter":
            self.out["masked"] = full(shape, SENT16, torch.int16) if self.u16 else full(shape, SENT32, torch.int32)
            self.out["mask"] = full(shape, 0x5a, torch.uint8)
        if kind == "bits":
            self.out["bits"] = full((3, w.bits[False].shape[1]), SENT32, torch.int32)
        if kind == "render":
            self.u16 = False
            self.out["virtual"] = full(shape, SENT32, torch.int32)
        if self.with_labels:
            self.out["labels"] = full(shape, SENT16, torch.int16)
        if kind == "residual":
            self.out["table"] = full((3, N_LABELS, 8), SENT64, torch.int64)
        if kind == "cloud":
            self.buf = K.CloudBuffers(sc, 3, self.cap)
            self.out = {k: t for k, t in (("points", self.buf.points), ("index", self.buf.index), ("counts", self.buf.counts)) if t is not None}

    def enqueue(self, ctx):
        o, n, d = self.out, self.n, self.d.data_ptr()
        lab = o["labels"].data_ptr() if self.with_labels else None
        if self.kind == "filter" and self.with_labels:
            ctx.filter_batch_device_labels(n, d, o["masked"].data_ptr(), o["mask"].data_ptr(), lab, u16=self.u16)
        elif self.kind == "filter":
            (ctx.filter_batch_device_u16 if self.u16 else ctx.filter_batch_device)(n, d, o["masked"].data_ptr(), o["mask"].data_ptr())
        elif self.kind == "bits":
            ctx.filter_batch_device_bits(n, d, o["bits"].data_ptr(), u16=self.u16)
        elif self.kind == "render":
            ctx.render_batch_device(n, o["virtual"].data_ptr(), lab, EMPTY)
        elif self.kind == "residual":
            (ctx.link_residuals_batch_device_u16 if self.u16 else ctx.link_residuals_batch_device)(n, d, o["table"].data_ptr(), N_LABELS)
        else:
            K.cloud_enqueue(ctx, self.d, n, self.buf, self.u16)

    def check(self):
        w, n, what = self.w, self.n, self.what
        streams = tuple(range(n))
        host = {k: t.cpu().numpy() for k, t in self.out.items()}
        for k, a in host.items():                # the streams the batch did not have: untouched
            sent = {1: 0x5a, 2: SENT16, 4: SENT32, 8: SENT64}[a.dtype.itemsize]
            assert (a[n:] == sent).all(), "%s: %s of a stream beyond n was written" % (what, k)
        labels = host["labels"][:n].view(np.uint16) if self.with_labels else None
        if self.kind == "filter":
            w.check_filter(host["masked"][:n], host["mask"][:n], labels, self.u16, what, streams)
        elif self.kind == "bits":
            w.check_bits(host["bits"][:n].view(np.uint32), self.u16, what, streams)
        elif self.kind == "render":
            w.check_render(host["virtual"][:n].view(np.float32), labels, what, streams)
        elif self.kind == "residual":
            w.check_table(K.table_host(self.out["table"])[:n], self.u16, what, streams)
        else:
            p, i, c = self.buf.host()
            w.check_cloud(p[:n], None if i is None else i[:n], None if c is None else c[:n], self.u16, self.cap, what, streams)


@gpu
def test_every_kind_behind_every_other_device_buffers():
    w = world()
    order = slot_order()
    assert len(pairs_two_apart(order)) == 20
    ctx = w.context()
    ctx.filter_batch(w.sc.depth)                  # (sizes the bins: no batch below is run twice)
    seen = {k: 0 for k in KINDS}
    jobs = []
    for i, kind in enumerate(order):
        jobs.append(DeviceJob(w, kind, seen[kind], 2 if i % 3 == 2 else 3))
        seen[kind] += 1
    for job in jobs:                              # nothing waits in between: the ring retires its oldest batch as needed
        job.enqueue(ctx)
    ctx.sync()
    torch_device()[0].cuda.synchronize()
    assert ctx.stats()["batch_status"] == 0
    for job in jobs:
        job.check()
    ctx.close()


# ---- host planes -------------------------------------------------------------------------------------------------------------------

def host_call(w, ctx, kind, v, n):
    """One call of `kind` on host planes of the first n streams; returns the check of its results, to be run once the batch is
    retired (the filter and mask-bits calls only enqueue)."""
    sc = w.sc
    u16 = bool(v & 1)
    what = "host planes: %s variant %d n=%d" % (kind, v, n)
    streams = tuple(range(n))
    sensor = np.ascontiguousarray(w.sensor(u16)[:n])
    if kind == "filter" and v & 2:
        masked, mask, labels = ctx.filter_batch_labels(sensor)
        return lambda: w.check_filter(masked, mask, labels, u16, what, streams)
    if kind == "filter":
        masked, mask = np.full_like(sensor, 77), np.full(sensor.shape, 0x5a, np.uint8)
        ctx.filter_batch_async(sensor, masked, mask)
        return lambda: w.check_filter(masked, mask, None, u16, what, streams)
    if kind == "bits":
        bits = np.full((n, ctx.mask_bits_words()), SENT32, np.uint32)
        ctx.filter_batch_bits_async(sensor, bits)
        return lambda: w.check_bits(bits, u16, what, streams)
    if kind == "render":
        virt, labels = ctx.render_batch(n, EMPTY, labels=bool(v & 1))
        return lambda: w.check_render(virt, labels, what, streams)
    if kind == "residual":
        table = ctx.link_residuals_batch(sensor, N_LABELS)
        return lambda: w.check_table(table, u16, what, streams)
    if v & 2:
        p, i, c = ctx.cloud_compact_batch(sensor, CAP, want_index=bool(v & 4))
        return lambda: w.check_cloud(p, i, c, u16, CAP, what, streams)
    p = ctx.cloud_batch(sensor)
    return lambda: w.check_cloud(p, None, None, u16, None, what, streams)


@gpu
def test_every_kind_behind_every_other_host_planes():
    w = world()
    order = slot_order()
    assert len(pairs_two_apart(order)) == 20
    ctx = w.context()
    ctx.filter_batch(w.sc.depth)
    seen = {k: 0 for k in KINDS}
    inflight = []
    for kind in order + [None]:
        if kind is not None:
            inflight.append(host_call(w, ctx, kind, seen[kind], 3))
            seen[kind] += 1
            if kind in ("filter", "bits") and len(inflight) < 2:
                continue                          # stays in flight: the next call takes the other slot
        ctx.sync()                                # (the other kinds' host-plane calls have synchronised already)
        for check in inflight:
            check()
        inflight = []
    assert ctx.stats()["batch_status"] == 0
    # two of the three streams: the staging of both slots only grows, so nothing is allocated again
    before = ctx.stats()["device_bytes"]
    for v in range(8):
        for kind in KINDS:
            check = host_call(w, ctx, kind, v, 2)
            ctx.sync()
            check()
    after = ctx.stats()["device_bytes"]
    print("device_bytes after the host-plane sequence: %d" % after)
    assert after == before, (before, after)
    ctx.close()


# ---- two kinds in flight when the bins are regrown ---------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("pair", ["residual_then_compacted_cloud", "render_with_labels_then_host_filter"])
def test_rerun_of_two_kinds_in_flight(pair):
    """bin_capacity = 1: the first batch overflows its bins, and both batches in flight are run again from their slots' records.
    (rtuf_stats.batch_reruns is that of the batch retired last, so it is read behind each of the two.)"""
    w = world()
    ctx = w.context(bin_capacity=1)
    if pair == "residual_then_compacted_cloud":
        first, second = DeviceJob(w, "residual", 0, 3), DeviceJob(w, "cloud", 2, 3)
        first.enqueue(ctx)
        second.enqueue(ctx)
        checks = [first.check, second.check]
    else:
        first = DeviceJob(w, "render", 2, 3)
        first.enqueue(ctx)
        checks = [first.check, host_call(w, ctx, "filter", 0, 3)]
    ctx.wait_oldest()
    reruns = ctx.stats()["batch_reruns"]
    ctx.sync()
    torch_device()[0].cuda.synchronize()
    st = ctx.stats()
    assert max(reruns, st["batch_reruns"]) >= 1 and st["regrowths"] >= 1, (reruns, st)
    for f in checks:
        f()
    ctx.close()


# ---- captured graphs -----------------------------------------------------------------------------------------------------------------

@gpu
def test_graph_replay_across_kinds():
    """One raster lane, pipelines = 2, one stream: small batches replay captured graphs.  Filter, render, residual and organized
    cloud batches alternate on the same buffers, the order turned by one every round, so that every slot of both pipelines
    meets every kind again and again; the stream's sensor plane and poses change from call to call."""
    torch, dev = torch_device()
    w = world()
    sc = w.sc
    ctx = w.context(n=1, max_streams=1, raster_lanes=1, pipelines=2)
    d = torch.empty((1, sc.H, sc.W), dtype=torch.float32, device=dev)
    masked, mask = torch.empty_like(d), torch.empty((1, sc.H, sc.W), dtype=torch.uint8, device=dev)
    virt, labels = torch.empty_like(d), torch.empty((1, sc.H, sc.W), dtype=torch.int16, device=dev)
    table = torch.empty((1, N_LABELS, 8), dtype=torch.int64, device=dev)
    cloud = K.CloudBuffers(sc, 1)
    kinds = ["filter", "render", "residual", "cloud"]
    for i in range(48):
        kind = kinds[(i + i // 4) % 4]
        s = i % sc.n
        ctx.set_cameras(0, sc.wl.projection[s:s + 1], sc.wl.offset_inv[s:s + 1], sc.wl.cam_tf[s:s + 1])
        ctx.set_link_poses_batch(0, 0, sc.wl.link_tf[0][s:s + 1])
        d.copy_(torch.from_numpy(sc.depth[s:s + 1]))
        torch.cuda.synchronize()
        what = "replay %d: %s" % (i, kind)
        if kind == "filter":
            ctx.filter_batch_device(1, d.data_ptr(), masked.data_ptr(), mask.data_ptr())
            ctx.sync()
            w.check_filter(masked.cpu().numpy(), mask.cpu().numpy(), None, False, what, (s,))
        elif kind == "render":
            ctx.render_batch_device(1, virt.data_ptr(), labels.data_ptr(), EMPTY)
            ctx.sync()
            w.check_render(virt.cpu().numpy(), labels.cpu().numpy().view(np.uint16), what, (s,))
        elif kind == "residual":
            ctx.link_residuals_batch_device(1, d.data_ptr(), table.data_ptr(), N_LABELS)
            ctx.sync()
            w.check_table(K.table_host(table), False, what, (s,))
        else:
            K.cloud_enqueue(ctx, d, 1, cloud)
            ctx.sync()
            w.check_cloud(cloud.host()[0], None, None, False, None, what, (s,))
    st = ctx.stats()
    assert st["graphs_enabled"] == 1 and st["graph_hits"] >= 3, st
    ctx.close()
