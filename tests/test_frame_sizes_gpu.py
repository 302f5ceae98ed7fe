"""GPU (-m gpu): every batch kind at the smallest, thinnest and widest frames a context accepts (rtuf_create: 1 x 1 to
2048 x 2048) -- tests/frame_sizes.py holds the thirteen frames with the reason for each, the inputs and the expectations;
tests/test_frame_sizes_cpu.py asserts that those inputs tell a right kernel from a wrong one.  The frames aim at what depends
on the frame: the tile kernel's partial last tiles, compare_kernel's tail, shade_window_tile's row pairs and scalar paths, the
dilation and padding halos around an image smaller than the window, the cloud kernels' partial chunk and the scan's carry, the
points and carve windows at a border that is everywhere, the scene kernels' partial words.

One test per (frame, context configuration), three streams; a context serves every kind its configuration admits:
  plain       filter with and without a label plane, mask bits, render with labels, residual table, organized and compacted
              cloud, clearance table, point lists at window radius 0 and 4, one synchronous host-plane filter call
  thresh      per-link thresholds: filter, mask bits, residual table, organized cloud
  two_kernel  RTUF_FLAG_TWO_KERNEL: filter with and without labels
  dilate2     silhouette radius 2: filter, mask bits, organized cloud, clearance table
  dilate16    silhouette radius kMaxDilation: filter and mask bits (the eight frames up to 68 x 33, and 2048 x 3)
  pad         link padding: filter and mask bits
  scene       scene planes learned from one frame, then filter and mask bits with the scene enabled
  voxels      one insert from device planes with counts and summary, one carve at radius 1 with summary (five frames)
Every kind runs in float32 and, where include/rtuf.h admits it at the frame's width, in 16UC1.  At the five frames whose width
is no multiple of 4 every call the header documents as needing one is asserted to fail with RTUF_ERR_INVALID and to leave its
sentinel-filled outputs untouched, and a good call on the same context afterwards still matches.

Every expectation comes from the CPU oracle's planes through tests/gpu_support.py, tests/link_padding_scenes.py and
bench_support/*_check.py, never from the library; every comparison is for equality, of bit patterns where the output is a
float.  Every device output lies inside a larger allocation with 1 KiB of sentinel in front of it and behind it, which must
still be there afterwards -- a store past a row or past the last stream shows -- and every element a call must not write still
holds the sentinel.  The sensor planes lie between 1 KiB of NaN (16UC1: 65,535 mm), so that a read past the frame changes a
result.

In this process the launches take the 1,024-thread tile kernels; run as a script (RTUF_SMALL_LAUNCH=0 python
tests/test_frame_sizes_gpu.py) the same cases take the 256-thread ones: the threshold is read once per process, so
test_every_case_256_thread_kernels starts one."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import frame_sizes as FS
import gpu_support as K
import realtime_urdf_filter_amd as R
from bench_support import points_check as PC
from bench_support.residuals_check import ROW

gpu = pytest.mark.gpu
F = np.float32
ERR_INVALID = -1
GUARD = 1024
SENT, SENT32, NAN_BYTE = 0x5A, 0x5A5A5A5A, 0xFF
CONFIGS = ("plain", "thresh", "two_kernel", "dilate2", "dilate16", "pad", "scene", "voxels")


def cases():
    """(frame, configuration) of every test."""
    out = []
    for frame in FS.FRAMES:
        for config in CONFIGS:
            if (config == "dilate16" and frame not in FS.MAX_DILATION_FRAMES) or (config == "voxels" and frame not in FS.VOXEL_FRAMES):
                continue
            out.append((frame, config))
    return out


def case_id(case):
    return "%s-%s" % (FS.frame_id(case[0]), case[1])


def test_the_cases_are_every_frame_in_every_configuration_it_has():
    assert len(cases()) == 13 * 6 + 9 + 5 == len(set(map(case_id, cases())))


# ---- device memory with guards ----------------------------------------------------------------------------------------------------------

class Guarded:
    """nbytes of device memory with GUARD bytes in front of them and behind them, everything filled with `fill`; payload: a host
    array the bytes start as.  ptr is 256-byte aligned."""

    def __init__(self, nbytes=None, fill=SENT, payload=None):
        torch, dev = K.torch_device()
        if payload is not None:
            payload = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
            nbytes = payload.size
        self.nbytes, self.fill = int(nbytes), fill
        host = np.full(2 * GUARD + self.nbytes, fill, np.uint8)
        if payload is not None:
            host[GUARD:GUARD + self.nbytes] = payload
        self.t = torch.from_numpy(host).to(dev)
        self.ptr = self.t.data_ptr() + GUARD
        assert self.ptr % 256 == 0

    def read(self, dtype, shape, what):
        """The bytes as a host array, once both guards are seen to hold the fill value."""
        raw = self.t.cpu().numpy()
        assert (raw[:GUARD] == self.fill).all(), "%s: written in front of the buffer" % what
        assert (raw[GUARD + self.nbytes:] == self.fill).all(), "%s: written behind the buffer" % what
        return raw[GUARD:GUARD + self.nbytes].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.t == self.fill).all())


_inputs = {}


def dev_input(w, name, u16):
    """The sensor planes ("sensor") or the frame a scene is learned from ("learn") on the device, between NaN."""
    key = (w.W, w.H, name, u16)
    if key not in _inputs:
        _inputs[key] = Guarded(payload=w.sensor(u16) if name == "sensor" else w.learn_frame(u16), fill=NAN_BYTE)
    return _inputs[key]


def launch(ctx, call, outputs, refuse, what):
    """Makes the call and retires it -> True; refuse: the call fails with RTUF_ERR_INVALID and writes nothing -> False."""
    torch, _ = K.torch_device()
    if refuse:
        with pytest.raises(R.RtufError) as e:
            call()
        assert e.value.code == ERR_INVALID, "%s: %s" % (what, e.value)
        ctx.sync()
        torch.cuda.synchronize()
        for b in outputs:
            assert b.untouched(), "%s: a refused call wrote to an output" % what
        return False
    call()
    ctx.sync()
    torch.cuda.synchronize()
    return True


def admitted(kind, u16, W):
    """include/rtuf.h: clearance tables, point lists and carves take any width in both element types; mask bits, clouds,
    scene learning and the plane form of a voxel insert need a multiple of 4 in both; filter, render and residual batches in
    16UC1 only."""
    if kind in ("clearance", "points", "carve"):
        return True
    if kind in ("bits", "cloud", "compact", "learn", "insert"):
        return W % 4 == 0
    return not u16 or W % 4 == 0


# ---- the kinds ---------------------------------------------------------------------------------------------------------------------------

def expect_mode(config):
    return "plain" if config in ("two_kernel", "voxels") else config


def run_filter(ctx, w, config, u16, labels, what):
    n, shape, px = w.n, (w.n, w.H, w.W), w.n * w.H * w.W
    d = dev_input(w, "sensor", u16)
    masked, mask, lab = Guarded(px * (2 if u16 else 4)), Guarded(px), Guarded(px * 2) if labels else None
    if labels:
        call = lambda: ctx.filter_batch_device_labels(n, d.ptr, masked.ptr, mask.ptr, lab.ptr, u16=u16)
    else:
        call = lambda: (ctx.filter_batch_device_u16 if u16 else ctx.filter_batch_device)(n, d.ptr, masked.ptr, mask.ptr)
    if not launch(ctx, call, [masked, mask] + ([lab] if labels else []), not admitted("filter", u16, w.W), what):
        return
    want_masked, want_mask = w.planes(expect_mode(config), u16)
    K.compare_planes(masked.read(np.uint16 if u16 else F, shape, what), want_masked, what, "masked")
    K.compare_labels(mask.read(np.uint8, shape, what), want_mask, what, "mask")
    if labels:
        K.compare_labels(lab.read(np.uint16, shape, what), w.labels(), what)


def run_bits(ctx, w, config, u16, what):
    words = len(K.pack_bits(np.zeros((w.H, w.W), np.uint8)))
    assert ctx.mask_bits_words() == words
    d, bits = dev_input(w, "sensor", u16), Guarded(w.n * words * 4)
    if not launch(ctx, lambda: ctx.filter_batch_device_bits(w.n, d.ptr, bits.ptr, u16=u16), [bits], not admitted("bits", u16, w.W), what):
        return
    got, want = bits.read(np.uint32, (w.n, words), what), w.bits(expect_mode(config), u16)
    assert np.array_equal(got, want), "%s: %d mask bits words differ, first %s" % (what, int((got != want).sum()), np.argwhere(got != want)[:3].tolist())


def run_render(ctx, w, u16, what):
    shape, px = (w.n, w.H, w.W), w.n * w.H * w.W
    virt, lab = Guarded(px * (2 if u16 else 4)), Guarded(px * 2)
    call = lambda: (ctx.render_batch_device_u16 if u16 else ctx.render_batch_device)(w.n, virt.ptr, lab.ptr, FS.EMPTY)
    if not launch(ctx, call, [virt, lab], not admitted("render", u16, w.W), what):
        return
    K.same_planes(virt.read(np.uint16 if u16 else F, shape, what), w.virtual(u16), what)
    K.compare_labels(lab.read(np.uint16, shape, what), w.labels(), what)


def run_residual(ctx, w, thresh, u16, what):
    d, table = dev_input(w, "sensor", u16), Guarded(w.n * FS.N_LABELS * ROW.itemsize)
    call = lambda: (ctx.link_residuals_batch_device_u16 if u16 else ctx.link_residuals_batch_device)(w.n, d.ptr, table.ptr, FS.N_LABELS)
    if not launch(ctx, call, [table], not admitted("residual", u16, w.W), what):
        return
    K.check_tables(table.read(ROW, (w.n, FS.N_LABELS), what), w.residuals(thresh, u16), what)


def run_cloud(ctx, w, config, u16, what):
    d, points = dev_input(w, "sensor", u16), Guarded(w.n * w.H * w.W * 12)
    if not launch(ctx, lambda: ctx.cloud_batch_device(w.n, d.ptr, points.ptr, u16=u16), [points], not admitted("cloud", u16, w.W), what):
        return
    got, want = points.read(np.uint32, (w.n, w.H, w.W, 3), what), w.cloud(expect_mode(config), u16)[0].view(np.uint32)
    assert np.array_equal(got, want), "%s: %d words of the organized cloud differ" % (what, int((got != want).sum()))


def run_compact(ctx, w, config, u16, what):
    cap = w.capacity(expect_mode(config), u16)
    d = dev_input(w, "sensor", u16)
    points, index, counts = Guarded(w.n * cap * 12), Guarded(w.n * cap * 4), Guarded(w.n * 4)
    call = lambda: ctx.cloud_compact_batch_device(w.n, d.ptr, points.ptr, index.ptr, counts.ptr, cap, u16=u16)
    if not launch(ctx, call, [points, index, counts], not admitted("compact", u16, w.W), what):
        return
    p, i, c = points.read(np.uint32, (w.n, cap, 3), what), index.read(np.uint32, (w.n, cap), what), counts.read(np.uint32, (w.n,), what)
    for s, (wp, wi, wc) in enumerate(w.cloud(expect_mode(config), u16)[1]):
        m = min(wc, cap)
        assert c[s] == wc, "%s stream %d: count %d instead of %d" % (what, s, c[s], wc)
        assert np.array_equal(p[s, :m], wp[:m].view(np.uint32)) and np.array_equal(i[s, :m], wi[:m]), "%s stream %d: compacted points" % (what, s)
        assert (p[s, m:] == SENT32).all() and (i[s, m:] == SENT32).all(), "%s stream %d: written at or beyond min(count, capacity)" % (what, s)


def run_clearance(ctx, w, config, u16, what):
    d, table = dev_input(w, "sensor", u16), Guarded(w.n * FS.N_LABELS * 16)
    launch(ctx, lambda: ctx.link_clearance_batch_device(w.n, d.ptr, table.ptr, FS.N_LABELS, FS.MAX_DISTANCE, u16=u16), [table], False, what)
    got = table.read(np.uint32, (w.n, FS.N_LABELS, 4), what)
    bad = np.argwhere(got != w.clearance(expect_mode(config), u16).view(np.uint32).reshape(w.n, FS.N_LABELS, 4))
    assert len(bad) == 0, "%s: clearance rows differ at %s" % (what, bad[:4].tolist())


def run_points(ctx, w, r, what):
    lists = w.point_lists()
    n, cap = len(lists), max(len(p) for p in lists)
    host = np.full((n, cap, 3), np.nan, F)
    for s, p in enumerate(lists):
        host[s, :len(p)] = p
    points, counts = Guarded(payload=host, fill=NAN_BYTE), Guarded(payload=np.array([len(p) for p in lists], np.uint32), fill=NAN_BYTE)
    verdict, pixel, summary = Guarded(n * cap), Guarded(n * cap * 4), Guarded(n * 16)
    launch(ctx, lambda: ctx.points_batch_device(n, points.ptr, counts.ptr, cap, r, verdict.ptr, pixel.ptr, summary.ptr), [], False, what)
    v, x, sm = verdict.read(np.uint8, (n, cap), what), pixel.read(np.uint32, (n, cap), what), summary.read(np.uint32, (n, 4), what)
    for s, (wv, wx) in enumerate(w.point_verdicts(r)):
        m = len(wv)
        bad = v[s, :m] != wv
        assert not bad.any(), "%s stream %d: %d verdicts differ, first at %d: %d instead of %d" % (
            what, s, int(bad.sum()), int(np.argmax(bad)), v[s, int(np.argmax(bad))], wv[int(np.argmax(bad))])
        assert np.array_equal(x[s, :m], wx), "%s stream %d: pixels" % (what, s)
        assert (v[s, m:] == SENT).all() and (x[s, m:] == SENT32).all(), "%s stream %d: written past the list's end" % (what, s)
        assert sm[s].tolist() == PC.summary(wv).tolist(), "%s stream %d: summary %s instead of %s" % (what, s, sm[s], PC.summary(wv))


def run_host_filter(ctx, w, config, what):
    """The synchronous host-plane calls: the pinned staging has size arithmetic of its own."""
    masked, mask = ctx.filter_batch(w.sensor(False))
    K.compare_planes(masked, w.planes(expect_mode(config), False)[0], what + " host planes", "masked")
    K.compare_labels(mask, w.planes(expect_mode(config), False)[1], what + " host planes", "mask")
    if admitted("filter", True, w.W):
        masked, mask = ctx.filter_batch_u16(w.sensor(True))
        K.compare_planes(masked, w.planes(expect_mode(config), True)[0], what + " 16UC1 host planes", "masked")
        K.compare_labels(mask, w.planes(expect_mode(config), True)[1], what + " 16UC1 host planes", "mask")
    else:
        with pytest.raises(R.RtufError) as e:
            ctx.filter_batch_u16(w.sensor(True))
        assert e.value.code == ERR_INVALID, e.value


# ---- the configurations ----------------------------------------------------------------------------------------------------------------------

def make_context(w, config):
    sc = w.sc
    kw = {"two_kernel": dict(flags=R.FLAG_TWO_KERNEL), "dilate2": dict(silhouette_dilation_px=2),
          "dilate16": dict(silhouette_dilation_px=FS.MAX_DILATION)}.get(config, {})
    ctx = sc.context(**kw)
    ctx.set_cloud_intrinsics(0, w.pad_intr if config == "pad" else w.intr)
    ctx.set_link_labels(sc.ids[0], np.array(FS.LINK_LABEL, np.uint16))
    ctx.set_link_spheres(sc.ids[0], [q[0] for q in w.spheres], [q[1:] for q in w.spheres])
    if config == "thresh":
        ctx.set_link_thresholds(sc.ids[0], np.array(FS.LINK_THR, F))
    if config == "pad":
        ctx.set_link_padding(sc.ids[0], np.array(FS.PADS, F))
    return ctx


def run_scene(ctx, w, what):
    """Learn from one frame in both element types (refused at a width that is no multiple of 4: the planes are then given),
    enable, filter."""
    torch, _ = K.torch_device()
    inf = np.full((w.n, w.H, w.W), np.inf, F)
    for u16 in (False, True):
        a = dev_input(w, "learn", u16)
        if admitted("learn", u16, w.W):
            ctx.clear_scene()
            ctx.learn_scene_batch_device(w.n, a.ptr, u16=u16)
            K.same_planes(ctx.get_scene_planes(), w.learned(u16), "%s learned u16=%s" % (what, u16))
        else:
            with pytest.raises(R.RtufError) as e:
                ctx.learn_scene_batch_device(w.n, a.ptr, u16=u16)
            assert e.value.code == ERR_INVALID, e.value
            K.same_planes(ctx.get_scene_planes(), inf, "%s: planes after a refused learn call" % what)
    if not admitted("learn", False, w.W):
        ctx.set_scene_planes(0, w.scene_planes())
    ctx.set_scene_margins(0, FS.MARGINS)
    for u16 in (False, True):
        run_filter(ctx, w, "scene", u16, False, "%s filter u16=%s" % (what, u16))
        run_bits(ctx, w, "scene", u16, "%s bits u16=%s" % (what, u16))


def run_voxels(ctx, w, what):
    g = FS.GRID
    ctx.set_voxel_grid(g.origin, g.voxel_size, g.dims, True)
    for s, m in enumerate(FS.VOXEL_TRANSFORMS):
        if m is not None:
            ctx.set_voxel_transforms(s, m)
    for u16 in (False, True):
        at = "%s u16=%s" % (what, u16)
        ctx.voxel_clear()
        d = dev_input(w, "sensor", u16)
        summary = Guarded(w.n * 16)
        insert = lambda: ctx.voxel_insert_batch_device(w.n, d.ptr, summary.ptr, u16=u16)
        if launch(ctx, insert, [summary], not admitted("insert", u16, w.W), at + " insert"):
            want_bits, want_counts, want_summary = w.voxel_insert(u16)
            bits, counts = ctx.voxel_grid()
            assert np.array_equal(bits, want_bits), "%s: %d occupancy words differ" % (at, int((bits != want_bits).sum()))
            assert np.array_equal(counts.reshape(-1), want_counts), "%s: voxel counts differ" % at
            got = summary.read(np.uint32, (w.n, 4), at)
            assert np.array_equal(got, want_summary), "%s: insert summary %s instead of %s" % (at, got.tolist(), want_summary.tolist())
        else:
            want_bits = np.zeros(g.n_words, np.uint32)
            assert not ctx.voxel_grid()[0].any(), "%s: a refused insert changed the grid" % at
        carved = Guarded(w.n * 16)
        launch(ctx, lambda: ctx.voxel_carve_batch_device(w.n, d.ptr, FS.CARVE_MARGIN, FS.CARVE_RADIUS, carved.ptr, u16=u16), [], False, at + " carve")
        want_free, want_carved = w.voxel_carve(u16)
        free = ctx.voxel_free()
        assert np.array_equal(free, want_free), "%s: %d free words differ" % (at, int((free != want_free).sum()))
        got = carved.read(np.uint32, (w.n, 4), at)
        assert np.array_equal(got, want_carved), "%s: carve summary %s instead of %s" % (at, got.tolist(), want_carved.tolist())
        assert np.array_equal(ctx.voxel_grid()[0], want_bits), "%s: the carve changed the occupancy words" % at


def run_case(frame, config):
    w = FS.world(frame)
    what = case_id((frame, config))
    ctx = make_context(w, config)
    for u16 in (False, True):
        at = "%s u16=%s" % (what, u16)
        if config == "plain":
            for labels in (False, True):
                run_filter(ctx, w, config, u16, labels, "%s filter labels=%s" % (at, labels))
            run_bits(ctx, w, config, u16, at + " bits")
            run_render(ctx, w, u16, at + " render")
            run_residual(ctx, w, False, u16, at + " residual")
            run_cloud(ctx, w, config, u16, at + " cloud")
            run_compact(ctx, w, config, u16, at + " compacted cloud")
            run_clearance(ctx, w, config, u16, at + " clearance")
        elif config == "thresh":
            run_filter(ctx, w, config, u16, False, at + " filter")
            run_bits(ctx, w, config, u16, at + " bits")
            run_residual(ctx, w, True, u16, at + " residual")
            run_cloud(ctx, w, config, u16, at + " cloud")
        elif config == "two_kernel":
            for labels in (False, True):
                run_filter(ctx, w, config, u16, labels, "%s filter labels=%s" % (at, labels))
        elif config == "dilate2":
            run_filter(ctx, w, config, u16, False, at + " filter")
            run_bits(ctx, w, config, u16, at + " bits")
            run_cloud(ctx, w, config, u16, at + " cloud")
            run_clearance(ctx, w, config, u16, at + " clearance")
        elif config in ("dilate16", "pad"):
            run_filter(ctx, w, config, u16, False, at + " filter")
            run_bits(ctx, w, config, u16, at + " bits")
    if config == "plain":
        for r in FS.POINT_RADII:
            run_points(ctx, w, r, "%s points r=%d" % (what, r))
        run_host_filter(ctx, w, config, what)
    elif config == "scene":
        run_scene(ctx, w, what)
    elif config == "voxels":
        run_voxels(ctx, w, what)
    # behind everything the configuration ran, refused calls included: a good call on the same context still matches
    run_filter(ctx, w, "scene" if config == "scene" else config, False, False, what + " last filter")
    assert ctx.stats()["batch_status"] == 0, what
    ctx.close()


@gpu
@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_frame(case):
    run_case(*case)


@gpu
def test_every_case_256_thread_kernels():
    """The same cases with RTUF_SMALL_LAUNCH=0: every launch takes the 256-thread tile kernels."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=600,
                       env=dict(os.environ, RTUF_SMALL_LAUNCH="0"))
    assert r.returncode == 0 and "frame sizes ok %d" % len(cases()) in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


if __name__ == "__main__":
    for frame_case in cases():
        run_case(*frame_case)
    print("frame sizes ok %d" % len(cases()))
