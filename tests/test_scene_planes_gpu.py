"""GPU: scene planes (include/rtuf.h, SCENE PLANES) -- every output form of every batch kind that honours a scene against the
numpy form of the definition on the CPU oracle's planes (tests/scene_planes_scenes.py; tests/test_scene_planes_cpu.py asserts
that its scenes hold every class of pixel), per-stream control and the way back, learning (equality: a running minimum), no
learning from provisional bits, what a clearance table measures with a scene, refusals and the Python façade."""
import os
import subprocess

import numpy as np
import pytest

import link_padding_scenes as LP
import realtime_urdf_filter_amd as R
import scene_planes_scenes as SP
import scenes as S
from bench_support import clearance_check as KC
from bench_support import cloud_check as CC
from bench_support.link_thresholds_check import expected_planes
from bench_support.link_thresholds_check import workload_draws as thr_draws
from gpu_support import (CloudBuffers, CloudExpect, bits_equal, check_comp, check_org, cloud_enqueue, compare_labels, compare_planes, example_facade,
                         filter_expected, info, intrinsics, label_planes, pack_bits, params, sensor_of, sensor_plane, torch_device, upload)
from bench_support import workloads as WL
from oracle import bindings as O
from realtime_urdf_filter_amd.filter import depth_f32_to_u16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
F = np.float32
ERR_INVALID, ERR_STATE = -1, -6
N_LABELS, SPHERE_R = 4, 0.1        # default labels 1 .. 3, one sphere per link
THRESHOLDS = (0.02, 0.3, 0.08)     # per-link depth thresholds of the cell's three links
PADS = (0.03, 0.05, 0.02)          # link padding in metres
MODES = ("plain", "two_kernel", "dilate", "thresh", "pad")


# ---- the robot filter's own outputs per mode (what the scene comes on top of) ------------------------------------------------------

def robot_expected(sc, mode, u16=False):
    """(masked, mask) [n,H,W] of the robot filter alone in `mode`."""
    if mode in ("plain", "two_kernel"):
        return filter_expected(sc, 0, u16)
    if mode == "dilate":
        return filter_expected(sc, 2, u16)
    if mode == "pad":
        ex = LP.expected(sc, PADS, u16)
        return ex.masked, ex.mask
    thr, ntris = thr_draws(sc.wl, np.array(THRESHOLDS, F))
    out = [expected_planes(sc.zwin[s], sc.prim[s], SP.sensor_metres(sc.depth[s], u16), thr, ntris, sc.wl.max_diff, sc.wl.near, sc.wl.far, sc.wl.replace_value)
           for s in range(sc.n)]
    return np.stack([depth_f32_to_u16(o[0]) if u16 else o[0] for o in out]), np.stack([o[1] for o in out])


def mode_context(sc, mode, max_streams=None, n=None, **kw):
    if mode == "two_kernel":
        kw["flags"] = R.FLAG_TWO_KERNEL
    if mode == "dilate":
        kw["silhouette_dilation_px"] = 2
    ctx = sc.context(max_streams=max_streams, n=n, **kw)
    ctx.set_cloud_intrinsics(0, [intrinsics(sc, i) for i in range(max_streams or sc.n)])
    if mode == "thresh":
        ctx.set_link_thresholds(sc.ids[0], np.array(THRESHOLDS, F))
    if mode == "pad":
        ctx.set_link_padding(sc.ids[0], np.array(PADS, F))
    return ctx


def give_scene(ctx, scene, margins, n=None):
    n = n or len(scene)
    ctx.set_scene_planes(0, scene[:n])
    ctx.set_scene_margins(0, margins[:n])


def check(want, masked, mask, what, n=None):
    n = n or len(want[1])
    if mask is not None:
        compare_labels(np.asarray(mask)[:n], want[1][:n], what, "mask")
    compare_planes(np.asarray(masked)[:n], want[0][:n], what, "masked depth")


def clearance_expected(sc, mask, u16, n, max_distance):
    links, sensor = list(range(sc.n_links)), sensor_of(sc, u16)
    want = np.zeros((n, N_LABELS), KC.DTYPE)
    for s in range(n):
        pts, idx, _ = CC.compacted(sensor[s], mask[s], intrinsics(sc, s))
        centres = KC.posed(sc.wl.link_tf[0][s], sc.wl.cam_tf[s], sc.wl.offset_inv[s], links, [(0.0, 0.0, 1.0 + 0.2 * l + 0.1 * (l == 2)) for l in links])
        want[s] = KC.table(pts, idx, centres, [SPHERE_R] * len(links), [l + 1 for l in links], links, N_LABELS, max_distance)
    return want


def give_spheres(ctx, sc):
    """One sphere per link on the link's quad (the cell's links lie at z = 1.0, 1.2 and 1.5 of their own frames)."""
    links = list(range(sc.n_links))
    ctx.set_link_spheres(sc.ids[0], links, [(0.0, 0.0, 1.0 + 0.2 * l + 0.1 * (l == 2), SPHERE_R) for l in links])


def every_output_form(ctx, sc, scene, margins, mode, what, n=None, enabled=None):
    """Every form of every kind that honours a scene, on the first n streams, against the expectation."""
    torch, dev = torch_device()
    n = n or sc.n
    rep = sc.wl.replace_value
    depth = np.ascontiguousarray(sc.depth[:n])
    depth16 = depth_f32_to_u16(depth)
    rm, rk = robot_expected(sc, mode)
    rm16, rk16 = robot_expected(sc, mode, True)
    ex = SP.expected(rm[:n], rk[:n], depth, scene, margins, rep, enabled=enabled)
    ex16 = SP.expected(rm16[:n], rk16[:n], depth, scene, margins, rep, u16=True, enabled=enabled)
    assert (ex[1] != rk[:n]).any() and (ex16[1] != rk16[:n]).any(), what + ": the scene changes nothing here"
    d, d16 = torch.from_numpy(depth).to(dev), torch.from_numpy(depth16.view(np.int16)).to(dev)
    total = ctx.max_streams
    # filter batches: host planes with and without masks, device planes with d_mask and with NULL, asynchronous, both element types
    masked, mask = ctx.filter_batch(depth)
    check(ex, masked, mask, what + " host planes")
    masked, none = ctx.filter_batch(depth, want_mask=False)
    check(ex, masked, None, what + " host planes without mask")
    for with_mask in (True, False):
        dm = torch.full((total, sc.H, sc.W), 77.0, dtype=torch.float32, device=dev)
        dk = torch.full((total, sc.H, sc.W), 7, dtype=torch.uint8, device=dev)
        ctx.filter_batch_device(n, d.data_ptr(), dm.data_ptr(), dk.data_ptr() if with_mask else None)
        ctx.sync()
        check(ex, dm.cpu().numpy(), dk.cpu().numpy() if with_mask else None, what + " device planes, mask %s" % with_mask, n)
        assert bool((dm[n:] == 77.0).all()) and bool((dk[n if with_mask else 0:] == 7).all()), what + ": planes beyond the batch"
        dm16 = torch.zeros((total, sc.H, sc.W), dtype=torch.int16, device=dev)
        ctx.filter_batch_device_u16(n, d16.data_ptr(), dm16.data_ptr(), dk.data_ptr() if with_mask else None)
        ctx.sync()
        check(ex16, dm16.cpu().numpy().view(np.uint16), dk.cpu().numpy() if with_mask else None, what + " 16UC1 device planes, mask %s" % with_mask, n)
    pin_in, pin_out, pin_k = ctx.host_alloc(depth.shape, F), ctx.host_alloc(depth.shape, F), ctx.host_alloc(depth.shape, np.uint8)
    pin_in[...] = depth
    ctx.filter_batch_async(pin_in, pin_out, pin_k)
    ctx.sync()
    check(ex, pin_out, pin_k, what + " asynchronous host planes")
    for a in (pin_in, pin_out, pin_k):
        ctx.host_free(a)
    m16, k16 = ctx.filter_batch_u16(depth16)
    check(ex16, m16, k16, what + " 16UC1 host planes")
    assert ctx.stats()["batch_status"] == 0
    # the label calls: the outputs with the scene, the label plane as without one
    if mode in ("plain", "two_kernel", "thresh"):
        masked, mask, lab = ctx.filter_batch_labels(depth)
        check(ex, masked, mask, what + " beside a label plane")
        compare_labels(lab, label_planes(sc)[:n], what + " label plane")
        masked, mask, lab = ctx.filter_batch_labels(depth16)
        check(ex16, masked, mask, what + " 16UC1 beside a label plane")
        compare_labels(lab, label_planes(sc)[:n], what + " label plane beside 16UC1")
    # mask bits (the calls refuse the two-kernel flag)
    if mode != "two_kernel":
        words = ctx.mask_bits_words()
        for u16 in (False, True):
            e = ex16 if u16 else ex
            bits = np.zeros((n, words), np.uint32)
            ctx.filter_batch_bits_async(depth16 if u16 else depth, bits)
            ctx.sync()
            db = torch.zeros((total, words), dtype=torch.int32, device=dev)
            ctx.filter_batch_device_bits(n, (d16 if u16 else d).data_ptr(), db.data_ptr(), u16=u16)
            ctx.sync()
            for s in range(n):
                want = pack_bits(e[1][s])
                assert np.array_equal(bits[s], want), "%s mask bits (u16=%s) stream %d" % (what, u16, s)
                assert np.array_equal(db[s].cpu().numpy().view(np.uint32), want), "%s device mask bits (u16=%s) stream %d" % (what, u16, s)
                xm, xk = R.expand_mask_bits(depth16[s] if u16 else depth[s], bits[s], rep)
                assert np.array_equal(xk, e[1][s]) and (np.array_equal(xm, e[0][s]) if u16 else bits_equal(xm, e[0][s])), what
            assert not db[n:].any()
    # clouds, organized and compacted, and the clearance table
    give_spheres(ctx, sc)
    for u16 in (False, True):
        e = ex16 if u16 else ex
        cx = CloudExpect(sc, e[1], u16, tuple(range(n)))
        dd = d16 if u16 else d
        org, comp = CloudBuffers(sc, n), CloudBuffers(sc, n, sc.W * sc.H)
        cloud_enqueue(ctx, dd, n, org, u16)
        cloud_enqueue(ctx, dd, n, comp, u16)
        ctx.sync()
        check_org(org.host()[0], cx, what + " organized cloud u16=%s" % u16)
        p, i, c = comp.host()
        check_comp(p, i, c, cx, sc.W * sc.H, what + " compacted cloud u16=%s" % u16)
        p, i, c = ctx.cloud_compact_batch(depth16 if u16 else depth, 3000)
        check_comp(p, i, c, cx, 3000, what + " compacted cloud, host planes u16=%s" % u16)
        check_org(ctx.cloud_batch(depth16 if u16 else depth), cx, what + " organized cloud, host planes u16=%s" % u16)
        want = clearance_expected(sc, e[1], u16, n, 1.5)
        got = ctx.link_clearance_batch(depth16 if u16 else depth, N_LABELS, 1.5)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: clearance rows u16=%s\ngot  %s\nwant %s" % (what, u16, got, want)
    assert ctx.stats()["batch_status"] == 0
    return ex, ex16


# ---- 1. every output form ---------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("mode", MODES)
def test_every_output_form_equals_the_expectation(mode):
    sc, scene, margins = SP.cell(160, 120, 4)
    ctx = mode_context(sc, mode)
    give_scene(ctx, scene, margins)
    every_output_form(ctx, sc, scene, margins, mode, "cell " + mode)
    ctx.close()


@gpu
@pytest.mark.parametrize("mode", ["plain", "dilate"])
def test_200x150_has_a_partial_bits_word_and_a_partial_chunk_per_row(mode):
    sc, scene, margins = SP.cell(200, 150, 3)
    ctx = mode_context(sc, mode)
    give_scene(ctx, scene, margins)
    every_output_form(ctx, sc, scene, margins, mode, "cell 200x150 " + mode)
    ctx.close()


@gpu
@pytest.mark.parametrize("lanes", [1, 3])
def test_launch_groups_smaller_than_the_batch(lanes):
    """Five streams in launch groups of two: group_base != 0 in both scene kernels, on one lane and on three."""
    sc, scene, margins = SP.cell(160, 120, 5)
    ctx = mode_context(sc, "plain", max_inflight_streams=2, raster_lanes=lanes)
    give_scene(ctx, scene, margins)
    every_output_form(ctx, sc, scene, margins, "plain", "groups of two, %d lanes" % lanes)
    assert ctx.stats()["groups_last_batch"] >= 3
    ctx.close()


@gpu
@pytest.mark.parametrize("mode", ["plain", "pad"])
def test_fewer_streams_than_max_streams(mode):
    sc, scene, margins = SP.cell(160, 120, 4)
    ctx = mode_context(sc, mode, max_streams=7, n=4)
    give_scene(ctx, scene, margins)
    every_output_form(ctx, sc, scene, margins, mode, "4 of 7 slots " + mode)
    every_output_form(ctx, sc, scene, margins, mode, "3 of 7 slots " + mode, n=3)
    ctx.close()


@gpu
def test_masked_plane_that_is_the_sensor_plane():
    """In place (d_masked == d_depth), where the fused filter allows it: a pixel the robot filter already replaced stays
    filtered whatever the replace value compares to, and the scene's pixels are replaced on top."""
    torch, dev = torch_device()
    sc, scene, margins = SP.cell(160, 120, 4)
    fresh = sc.context()
    d = torch.from_numpy(sc.depth).to(dev)
    fresh.filter_batch_device(sc.n, d.data_ptr(), d.data_ptr(), None)
    fresh.sync()
    legal_today = bits_equal(d.cpu().numpy(), sc.masked)
    fresh.close()
    assert legal_today                                       # (the fused kernel reads a pixel before it writes it: what stays legal)
    ctx = sc.context()
    give_scene(ctx, scene, margins)
    ex = SP.expected(sc.masked, sc.mask, sc.depth, scene, margins, sc.wl.replace_value)
    d = torch.from_numpy(sc.depth).to(dev)
    dk = torch.zeros((sc.n, sc.H, sc.W), dtype=torch.uint8, device=dev)
    ctx.filter_batch_device(sc.n, d.data_ptr(), d.data_ptr(), dk.data_ptr())
    ctx.sync()
    check(ex, d.cpu().numpy(), dk.cpu().numpy(), "in place")
    ctx.close()


# ---- 2. per-stream control ----------------------------------------------------------------------------------------------------------------

@gpu
def test_a_stream_with_filtering_disabled_equals_the_plain_result():
    sc, scene, margins = SP.cell(160, 120, 4)
    ctx = mode_context(sc, "plain")
    give_scene(ctx, scene, margins)
    ctx.set_scene_margins(1, None, n=2)                      # streams 1 and 2 off: their planes stay
    enabled = [True, False, False, True]
    ex, _ = every_output_form(ctx, sc, scene, margins, "plain", "streams 1 and 2 disabled", enabled=enabled)
    assert np.array_equal(ex[1][1], sc.mask[1]) and bits_equal(ex[0][2], sc.masked[2])
    assert bits_equal(ctx.get_scene_planes(), scene) or np.array_equal(ctx.get_scene_planes().view(np.uint32), scene.view(np.uint32))
    ctx.set_scene_margins(2, margins[2:3])                   # one of them on again, with its margins
    every_output_form(ctx, sc, scene, margins, "plain", "stream 1 disabled", enabled=[True, False, True, True])
    ctx.close()


@gpu
def test_render_and_residual_batches_are_bit_equal_with_and_without_a_scene():
    sc, scene, margins = SP.cell(160, 120, 4)
    ctx = sc.context()
    v0, l0 = ctx.render_batch(sc.n, -1.5, labels=True)
    v016, _ = ctx.render_batch(sc.n, -1.5, u16=True)
    t0 = ctx.link_residuals_batch(sc.depth, N_LABELS)
    t016 = ctx.link_residuals_batch(depth_f32_to_u16(sc.depth), N_LABELS)
    give_scene(ctx, scene, margins)
    for rep in range(2):
        v1, l1 = ctx.render_batch(sc.n, -1.5, labels=True)
        assert np.array_equal(v1.view(np.uint32), v0.view(np.uint32)) and np.array_equal(l1, l0)
        assert np.array_equal(ctx.render_batch(sc.n, -1.5, u16=True)[0], v016)
        assert np.array_equal(ctx.link_residuals_batch(sc.depth, N_LABELS), t0)
        assert np.array_equal(ctx.link_residuals_batch(depth_f32_to_u16(sc.depth), N_LABELS), t016)
        masked, mask = ctx.filter_batch(sc.depth)           # (the scene is in effect all the while)
        check(SP.expected(sc.masked, sc.mask, sc.depth, scene, margins, sc.wl.replace_value), masked, mask, "between the render batches")
    ctx.close()


def every_kind(ctx, sc):
    """One batch of every kind, as comparable host values."""
    depth, depth16 = sc.depth, depth_f32_to_u16(sc.depth)
    words = np.zeros((sc.n, ctx.mask_bits_words()), np.uint32)
    ctx.filter_batch_bits_async(depth, words)
    ctx.sync()
    out = [*ctx.filter_batch(depth), *ctx.filter_batch_u16(depth16), *ctx.filter_batch_labels(depth), words, *ctx.render_batch(sc.n, 0.0, labels=True),
           ctx.link_residuals_batch(depth, N_LABELS), ctx.cloud_batch(depth), *ctx.cloud_compact_batch(depth, sc.W * sc.H),
           ctx.link_clearance_batch(depth, N_LABELS, 1.5)]
    counts = out[-2]
    out[-4] = np.concatenate([out[-4][s][:counts[s]] for s in range(sc.n)])      # (entries beyond a stream's count are unspecified)
    out[-3] = np.concatenate([out[-3][s][:counts[s]] for s in range(sc.n)])
    return [np.ascontiguousarray(a).view(np.uint8) for a in out]


@gpu
def test_after_clear_scene_every_kind_equals_a_fresh_contexts_output():
    sc, scene, margins = SP.cell(160, 120, 4)
    fresh = mode_context(sc, "plain")
    give_spheres(fresh, sc)
    plain = every_kind(fresh, sc)
    bytes_fresh = fresh.stats()["device_bytes"]
    fresh.close()
    ctx = mode_context(sc, "plain")
    give_spheres(ctx, sc)
    give_scene(ctx, scene, margins)
    with_scene = every_kind(ctx, sc)
    assert not np.array_equal(with_scene[1], plain[1]) and ctx.stats()["device_bytes"] >= bytes_fresh + scene.nbytes      # (the planes are counted)
    ctx.clear_scene(0, 2)                                    # streams 2 and 3 keep theirs: a scene is still in effect
    masked, mask = ctx.filter_batch(sc.depth)
    check(SP.expected(sc.masked, sc.mask, sc.depth, scene, margins, sc.wl.replace_value, enabled=[False, False, True, True]), masked, mask, "two streams cleared")
    assert np.isposinf(ctx.get_scene_planes(0, 2)).all() and np.array_equal(ctx.get_scene_planes(2, 2).view(np.uint32), scene[2:].view(np.uint32))
    for step in ("cleared", "cleared twice"):
        held = ctx.stats()["device_bytes"]
        ctx.clear_scene()
        # the last touched stream is cleared: the planes and the streams' table are returned (no learn call: no scratch)
        assert ctx.stats()["device_bytes"] == held - (scene.nbytes + 16 * sc.n if step == "cleared" else 0)
        got = every_kind(ctx, sc)
        for i, (a, b) in enumerate(zip(got, plain)):
            assert np.array_equal(a, b), "%s: output %d differs from a fresh context's" % (step, i)
        assert np.isposinf(ctx.get_scene_planes()).all()
    # planes set but never enabled: nothing in effect either
    ctx.set_scene_planes(0, scene)
    for a, b in zip(every_kind(ctx, sc), plain):
        assert np.array_equal(a, b)
    ctx.close()


@gpu
@pytest.mark.parametrize("pipelines", [1, 2])
def test_alternating_scene_on_and_off_between_batches_in_the_same_slot(pipelines):
    """One-stream batches on one lane (with two pipelines they replay captured graphs): the same buffers, the scene on and off
    and other margins in turn -- a plan that did not tell the routes apart would replay the wrong kernels."""
    torch, dev = torch_device()
    sc, scene, margins = SP.cell(160, 120, 4)
    ctx = sc.context(max_streams=1, n=1, raster_lanes=1, pipelines=pipelines)
    ctx.set_scene_planes(0, scene[:1])
    d = torch.from_numpy(sc.depth[:1]).to(dev)
    dm = torch.zeros((1, sc.H, sc.W), dtype=torch.float32, device=dev)
    dk = torch.zeros((1, sc.H, sc.W), dtype=torch.uint8, device=dev)
    db = torch.zeros((1, ctx.mask_bits_words()), dtype=torch.int32, device=dev)
    wide = np.array([[0.5, 0.0]], F)
    seen = set()
    for step, m in enumerate([None, margins[:1], margins[:1], None, None, wide, margins[:1], None, wide, wide]):
        ctx.set_scene_margins(0, m, n=1)
        on = m is not None
        ex = SP.expected(sc.masked[:1], sc.mask[:1], sc.depth[:1], scene, m if on else margins, sc.wl.replace_value, enabled=[on])
        for rep in range(2):
            dm.zero_(); dk.zero_(); db.zero_()
            ctx.filter_batch_device(1, d.data_ptr(), dm.data_ptr(), dk.data_ptr())
            ctx.filter_batch_device_bits(1, d.data_ptr(), db.data_ptr())
            ctx.sync()
            check(ex, dm.cpu().numpy(), dk.cpu().numpy(), "step %d rep %d" % (step, rep))
            assert np.array_equal(db[0].cpu().numpy().view(np.uint32), pack_bits(ex[1][0])), "step %d rep %d: bits" % (step, rep)
        seen.add(ex[1].tobytes())
    assert len(seen) == 3
    ctx.close()


# ---- 3. learning --------------------------------------------------------------------------------------------------------------------------

def same_planes(got, want, what):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert got.shape == want.shape and not bad.any(), "%s: %d scene pixels differ, first %s" % (what, int(bad.sum()), np.argwhere(bad)[:3].tolist())


def pose_frames(W=160, H=120, n=4):
    return [SP.cell(W, H, n, pose)[0] for pose in range(3)]


def stage_pose(ctx, sc):
    sc.wl.stage(ctx, sc.ids, n=sc.n)


@gpu
@pytest.mark.parametrize("u16", [False, True])
def test_three_frames_in_three_poses_learn_the_running_minimum(u16):
    frames = pose_frames()
    sc0 = frames[0]
    ctx = sc0.context()
    for f in frames:
        f.ids = sc0.ids
    want = np.full((sc0.n, sc0.H, sc0.W), np.inf, F)
    same_planes(ctx.get_scene_planes(), want, "before anything")
    torch, dev = torch_device()
    for i, f in enumerate(frames):
        stage_pose(ctx, f)
        depth = depth_f32_to_u16(f.depth) if u16 else f.depth
        if i == 1:            # the device form once
            ctx.learn_scene_batch_device(f.n, upload(depth).data_ptr(), u16=u16)
        else:
            ctx.learn_scene_batch(depth)
        want = SP.learned(want, f.depth, filter_expected(f, 0, u16)[1], u16)
        same_planes(ctx.get_scene_planes(), want, "after frame %d" % i)
    assert np.isinf(want).any() and np.isfinite(want).sum() > want.size // 2      # some pixels no frame uncovered, most of the cell learned
    ctx.learn_scene_batch(depth_f32_to_u16(frames[2].depth) if u16 else frames[2].depth)      # idempotent
    same_planes(ctx.get_scene_planes(), want, "the last frame again")
    out = torch.zeros((sc0.n, sc0.H, sc0.W), dtype=torch.float32, device=dev)
    ctx.get_scene_planes_device(0, sc0.n, out.data_ptr())
    same_planes(out.cpu().numpy(), want, "device read-back")
    # learn, enable, filter: the expectation from the learned planes
    margins = SP.MARGINS[:sc0.n]
    ctx.set_scene_margins(0, margins)
    f = frames[1]
    stage_pose(ctx, f)
    rm, rk = filter_expected(f, 0, u16)
    ex = SP.expected(rm, rk, f.depth, want, margins, f.wl.replace_value, u16=u16)
    masked, mask = (ctx.filter_batch_u16 if u16 else ctx.filter_batch)(depth_f32_to_u16(f.depth) if u16 else f.depth)
    check(ex, masked, mask, "learn, enable, filter")
    assert ((ex[1] > 0) & (rk == 0)).sum() > 1000
    # and learning goes on ignoring the scene it has: the robot's bits alone
    ctx.learn_scene_batch(depth_f32_to_u16(f.depth) if u16 else f.depth)
    same_planes(ctx.get_scene_planes(), want, "learning with the scene in effect")
    ctx.close()


@gpu
def test_learning_with_padding_does_not_learn_the_halo():
    sc, _, _ = SP.cell(160, 120, 4)
    fresh = np.full((sc.n, sc.H, sc.W), np.inf, F)
    padded = SP.learned(fresh, sc.depth, LP.expected(sc, PADS).mask)
    unpadded = SP.learned(fresh, sc.depth, sc.mask)
    halo = np.isinf(padded) & np.isfinite(unpadded)
    assert halo.sum() > 200                                  # the two expectations differ: the halo is what padding keeps out
    ctx = mode_context(sc, "pad")
    ctx.learn_scene_batch(sc.depth)
    same_planes(ctx.get_scene_planes(), padded, "learned with padding")
    ctx.close()


@gpu
def test_learning_with_dilation_and_with_thresholds_uses_the_robots_bits_of_that_mode():
    sc, _, _ = SP.cell(160, 120, 4)
    fresh = np.full((sc.n, sc.H, sc.W), np.inf, F)
    for mode in ("dilate", "thresh"):
        ctx = mode_context(sc, mode)
        ctx.learn_scene_batch(sc.depth)
        want = SP.learned(fresh, sc.depth, robot_expected(sc, mode)[1])
        assert not np.array_equal(want.view(np.uint32), SP.learned(fresh, sc.depth, sc.mask).view(np.uint32)), mode
        same_planes(ctx.get_scene_planes(), want, "learned in mode " + mode)
        ctx.close()


@gpu
def test_learning_on_top_of_planes_that_were_set_and_with_fewer_streams():
    sc, scene, _ = SP.cell(160, 120, 4)
    ctx = sc.context(max_streams=6, n=4)
    given = np.concatenate([scene, scene[:2] * F(0.5)])      # six planes; NaN and +inf pixels among them
    ctx.set_scene_planes(0, given)
    ctx.learn_scene_batch(sc.depth[:3])                      # n < max_streams: streams 3 .. 5 keep theirs
    want = SP.learned(given, sc.depth[:3], sc.mask[:3])
    assert (want[:3] != given[:3]).any() and np.array_equal(want[3:].view(np.uint32), given[3:].view(np.uint32))
    same_planes(ctx.get_scene_planes(), want, "learned on top")
    assert not np.isnan(want[:3][(sc.mask[:3] == 0) & np.isfinite(sc.depth[:3]) & (sc.depth[:3] > 0)]).any()      # NaN is unknown: replaced
    ctx.close()


# ---- 4. no learning from provisional bits -------------------------------------------------------------------------------------------------------

@gpu
def test_a_learn_call_whose_first_run_overflows_learns_from_the_final_bits():
    """The pile of small triangles of the batch-status test with bins of one record: the first run of the learn call's
    mask-bits batch overflows and leaves pile pixels unmasked; learning them would carve the pile into the scene for good."""
    W, H, n = 160, 120, 3
    P = S.projection(131.25, 131.25, (W - 1) / 2, (H - 1) / 2, W, H)
    I = S.gl(np.eye(4))
    rng = np.random.default_rng(5)
    nt = 3000
    c = np.stack([rng.uniform(-0.07, -0.04, nt), rng.uniform(-0.10, -0.05, nt), rng.uniform(0.95, 1.05, nt)], axis=1)
    verts = (c[:, None, :] + rng.uniform(-0.022, 0.022, size=(nt, 3, 3)) * np.array([1.0, 0.3, 1.0])).reshape(-1, 3).astype(F)
    tris = np.arange(len(verts), dtype=np.uint32).reshape(-1, 3)
    flat = np.full((H, W), 2.0, F)
    pile = [O.filter_frame(flat, P, [(I, 0, [0.0, 0.0, 0.0], verts, tris)], I, I, replace_value=5.0)[1] > 0 for _ in range(1)][0]
    assert 50 < pile.sum() < W * H // 4
    depth = np.stack([np.where(pile, F(1.1), F(2.0 + 0.1 * s)).astype(F) for s in range(n)])       # the sensor reads the pile at pile pixels
    ctx = R.Context(W, H, n, 0, params(bin_capacity=1))
    m = ctx.add_model()
    ctx.add_draw(m, ctx.add_link(m), verts, tris, 0, [0.0, 0.0, 0.0])
    ctx.finalize_models()
    for s in range(n):
        ctx.set_camera(s, P, I, I)
        ctx.set_link_poses(s, m, np.stack([I]))
    ctx.learn_scene_batch(depth)
    st = ctx.stats()
    assert st["batch_reruns"] >= 1 and st["batch_status"] & R.STATUS_BIN_OVERFLOW, st
    mask = np.stack([O.filter_frame(depth[s], P, [(I, 0, [0.0, 0.0, 0.0], verts, tris)], I, I, replace_value=5.0)[1] for s in range(n)])
    assert all(np.array_equal(mask[s] > 0, pile) for s in range(n))
    want = SP.learned(np.full((n, H, W), np.inf, F), depth, mask)
    got = ctx.get_scene_planes()
    assert np.isposinf(got[:, pile]).all(), "%d pile pixels were learned from provisional bits" % int(np.isfinite(got[:, pile]).sum())
    same_planes(got, want, "learned from the final bits")
    ctx.close()


# ---- 5. clearance is about intruders ----------------------------------------------------------------------------------------------------------------

@gpu
def test_with_a_scene_the_clearance_row_measures_the_intruder_not_the_table():
    """The scene is the table; the sensor reads the table plus a box near the gripper (link 0).  Without the scene the gripper's
    nearest kept point lies on the table, with it on the box -- both equal to brute force over the kept points."""
    sc, _, _ = SP.cell(160, 120, 3)
    n, W, H = sc.n, sc.W, sc.H
    table = np.full((n, H, W), 1.6, F)
    table[:, 75:, :] = F(1.15)                               # the table's edge comes up close below the gripper
    depth = table.copy()
    depth[:, 20:32, 40:56] = F(1.05)                         # the box: further from the gripper's sphere than the table edge is
    on_robot = sc.prim >= 0
    virt = SP.expected_virtual(sc.zwin, sc.prim, sc.wl.near, sc.wl.far, 0.0)
    depth[on_robot] = virt[on_robot]                         # the camera reads the robot where it stands
    cell = type(sc)(sc.wl, depth, "table_and_box")
    ctx = mode_context(cell, "plain")
    give_spheres(ctx, cell)
    margins = np.tile(np.array([[0.02, 0.0]], F), (n, 1))
    without = ctx.link_clearance_batch(depth, N_LABELS, 2.0)
    want0 = clearance_expected(cell, cell.mask, False, n, 2.0)
    assert np.array_equal(without.view(np.uint32), want0.view(np.uint32))
    give_scene(ctx, table, margins)
    got = ctx.link_clearance_batch(depth, N_LABELS, 2.0)
    _, k = SP.expected(cell.masked, cell.mask, depth, table, margins, cell.wl.replace_value)
    want = clearance_expected(cell, k, False, n, 2.0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "with the scene\ngot  %s\nwant %s" % (got, want)
    for s in range(n):
        v0, u0 = divmod(int(without[s]["pixel"][1]), W)
        v1, u1 = divmod(int(got[s]["pixel"][1]), W)
        assert v0 >= 75 and depth[s, v0, u0] == F(1.15), "stream %d: without the scene the nearest point is on the table" % s
        assert 20 <= v1 < 32 and 40 <= u1 < 56, "stream %d: with the scene the nearest point is on the box" % s
        assert got[s]["clearance"][1] > without[s]["clearance"][1]
    ctx.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------

def refused(code, call, *args, **kw):
    with pytest.raises(R.RtufError) as err:
        call(*args, **kw)
    assert err.value.code == code, str(err.value)


@gpu
def test_invalid_calls_fail_with_their_code_and_change_nothing():
    sc, scene, margins = SP.cell(160, 120, 4)
    # an un-finalized context: a state error from every call
    raw = R.Context(160, 120, 2, 0, params())
    refused(ERR_STATE, raw.set_scene_planes, 0, scene[:1])
    refused(ERR_STATE, raw.get_scene_planes, 0, 1)
    refused(ERR_STATE, raw.set_scene_margins, 0, margins[:1])
    refused(ERR_STATE, raw.clear_scene)
    refused(ERR_STATE, raw.learn_scene_batch, sc.depth[:1])
    raw.close()
    ctx = sc.context()
    give_scene(ctx, scene, margins)
    ex = SP.expected(sc.masked, sc.mask, sc.depth, scene, margins, sc.wl.replace_value)
    lib, h = ctx._lib, ctx._h

    def unchanged(what):
        masked, mask = ctx.filter_batch(sc.depth)
        check(ex, masked, mask, what)
        assert np.array_equal(ctx.get_scene_planes().view(np.uint32), scene.view(np.uint32)), what

    other = (scene * F(0.5)).astype(F)
    import ctypes
    five = (ctypes.c_void_p * 5)(*[other[i % 4].ctypes.data for i in range(5)])
    refused(ERR_INVALID, ctx.set_scene_planes, 3, other[:2])
    refused(ERR_INVALID, ctx.get_scene_planes, 2, 3)
    for first, n in ((-1, 1), (0, 0), (0, -2), (4, 1), (3, 2), (0, 5), (5, 1)):
        assert lib.rtuf_set_scene_planes(h, first, n, five) == ERR_INVALID and lib.rtuf_get_scene_planes(h, first, n, five) == ERR_INVALID
        assert lib.rtuf_set_scene_planes_device(h, first, n, ctx._h) == ERR_INVALID      # (any non-NULL pointer: the range is checked first)
        assert lib.rtuf_set_scene_margins(h, first, n, margins.ctypes.data) == ERR_INVALID
        assert lib.rtuf_set_scene_margins(h, first, n, None) == ERR_INVALID
        assert lib.rtuf_clear_scene(h, first, n) == ERR_INVALID
        assert lib.rtuf_get_scene_planes_device(h, first, n, ctx._h) == ERR_INVALID
    unchanged("after bad stream ranges")
    # NULL planes and arrays
    PP = ctypes.c_void_p * 2
    assert lib.rtuf_set_scene_planes(h, 0, 2, None) == ERR_INVALID
    assert lib.rtuf_set_scene_planes(h, 0, 2, PP(other[0].ctypes.data, None)) == ERR_INVALID      # the first plane is not taken either
    assert lib.rtuf_set_scene_planes_device(h, 0, 2, None) == ERR_INVALID
    assert lib.rtuf_get_scene_planes(h, 0, 2, None) == ERR_INVALID and lib.rtuf_get_scene_planes(h, 0, 2, PP(other[0].ctypes.data, None)) == ERR_INVALID
    assert lib.rtuf_get_scene_planes_device(h, 0, 2, None) == ERR_INVALID
    assert lib.rtuf_learn_scene_batch(h, 2, None) == ERR_INVALID and lib.rtuf_learn_scene_batch(h, 2, PP(sc.depth[0].ctypes.data, None)) == ERR_INVALID
    assert lib.rtuf_learn_scene_batch_device(h, 2, None) == ERR_INVALID and lib.rtuf_learn_scene_batch_device_u16(h, 2, None) == ERR_INVALID
    assert lib.rtuf_learn_scene_batch(h, 0, PP(sc.depth[0].ctypes.data, None)) == ERR_INVALID and lib.rtuf_learn_scene_batch(h, 5, None) == ERR_INVALID
    unchanged("after NULL arguments")
    # margins: negative, NaN, infinite, rel >= 1 -- in any stream of the range, and the valid ones before it are not taken
    for a, r in ((-0.01, 0.0), (np.nan, 0.0), (np.inf, 0.0), (-np.inf, 0.0), (0.01, -0.1), (0.01, np.nan), (0.01, np.inf), (0.01, 1.0), (0.01, 1.5)):
        bad = np.array([[0.4, 0.0], [a, r]], F)
        refused(ERR_INVALID, ctx.set_scene_margins, 1, bad)
    unchanged("after bad margins")
    # the learn calls inherit the mask-bits calls' conditions: the two-kernel flag is refused
    p = params(replace=sc.wl.replace_value, max_diff=sc.wl.max_diff, flags=R.FLAG_TWO_KERNEL)
    p.near_plane, p.far_plane = sc.wl.near, sc.wl.far
    ctx.set_params(p)
    refused(ERR_INVALID, ctx.learn_scene_batch, sc.depth)
    p.flags = 0
    ctx.set_params(p)
    unchanged("after a refused learn call")
    ctx.close()
    # ... and a camera whose background quad does not cover the image is reported as the mask-bits calls report it
    from gpu_support import undrawn_scene
    und = undrawn_scene()
    uctx = und.context()
    with pytest.raises(R.RtufError) as err:
        uctx.learn_scene_batch(und.depth)
    assert err.value.code == ERR_STATE and "background quad" in str(err.value)
    assert np.isposinf(uctx.get_scene_planes()).all()        # nothing was learned
    masked, mask = uctx.filter_batch(und.depth)              # the context stays usable
    assert np.array_equal(mask, und.mask) and bits_equal(masked, und.masked)
    uctx.close()


# ---- 7. the Python façade ---------------------------------------------------------------------------------------------------------------------------

@gpu
def test_python_facade_learns_enables_and_filters():
    W, H = 640, 480
    depth = sensor_plane()
    table = np.where(np.isfinite(depth) & (depth > 0), depth, F(3.0)).astype(F)      # the empty cell as the camera reads it
    # the robot filter alone, from a façade without scene parameters
    g, _ = example_facade()
    P = g.getProjectionMatrix(info())
    g.filter(depth, P, W, H)
    rm, rk = np.array(g.masked_depth_), np.array(g.mask_)
    g.filter(table, P, W, H)
    rk_table = np.array(g.mask_)
    assert np.isposinf(g.getScene()).all()
    g.learnScene(table, P, W, H)                             # no margins in its parameters: learned, but never in effect
    g.filter(depth, P, W, H)
    assert np.array_equal(np.array(g.mask_), rk) and bits_equal(np.array(g.masked_depth_), rm)
    want_plane = SP.learned(np.full((1, H, W), np.inf, F), table[None], rk_table[None])
    same_planes(g.getScene()[None], want_plane, "façade without margins: learned plane")
    # learn, enable (the parameters), filter
    f, _ = example_facade(scene_margin=0.03, scene_margin_rel=0.01)
    assert f.getScene() is None                              # no context yet
    f.learnScene(table, f.getProjectionMatrix(info()), W, H)
    same_planes(f.getScene()[None], want_plane, "façade: learned plane")
    f.filter(depth, P, W, H)
    ex = SP.expected(rm[None], rk[None], depth[None], want_plane, np.array([[0.03, 0.01]], F), 5.0)
    check(ex, np.array(f.masked_depth_)[None], np.array(f.mask_)[None], "façade: learn, enable, filter")
    assert ((ex[1] > 0) & (rk[None] == 0)).sum() > 10000
    f.clearScene()
    assert np.isposinf(f.getScene()).all()
    f.filter(depth, P, W, H)
    assert np.array_equal(np.array(f.mask_), rk) and bits_equal(np.array(f.masked_depth_), rm)
    f.setScene(want_plane[0])
    f.filter(depth, P, W, H)
    check(ex, np.array(f.masked_depth_)[None], np.array(f.mask_)[None], "façade: setScene")


CPP = r'''
#include <cstdio>
#include <fstream>
#include <iterator>
#include "realtime_urdf_filter_amd/urdf_filter.hpp"
using namespace realtime_urdf_filter;
template <typename T> static std::vector<T> slurp(const char* path)
{
  std::ifstream f(path, std::ios::binary);
  const std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(s.size() / sizeof(T));
  memcpy(v.data(), s.data(), v.size() * sizeof(T));
  return v;
}
int main(int, char** argv)
{
  std::ifstream fx(argv[1], std::ios::binary);
  const std::string xml((std::istreambuf_iterator<char>(fx)), std::istreambuf_iterator<char>());
  const int W = 640, H = 480;
  const std::vector<float> depth = slurp<float>(argv[2]), table = slurp<float>(argv[3]);
  const std::vector<uint16_t> mm = slurp<uint16_t>(argv[4]);
  rtuf_host::StaticTransformProvider tf;
  for (const auto& kv : rtuf_host::forward_kinematics(rtuf_host::UrdfModel::from_string(xml))) tf.frames["/EXAMPLE/" + kv.first] = kv.second;
  tf.frames["/world"] = Transform();
  Transform cam;
  cam.m[0][0] = 1; cam.m[0][1] = 0; cam.m[0][2] = 0;
  cam.m[1][0] = 0; cam.m[1][1] = 0; cam.m[1][2] = 1;
  cam.m[2][0] = 0; cam.m[2][1] = -1; cam.m[2][2] = 0;
  tf.frames["/cam"] = cam;
  FilterParameters prm;
  prm.fixed_frame = "/world"; prm.camera_frame = "/cam"; prm.filter_replace_value = 5.0;
  prm.scene_margin = 0.03; prm.scene_margin_rel = 0.01;
  ModelParameter mp;
  mp.model = "d"; mp.tf_prefix = "/EXAMPLE"; mp.geometry_type = "visual";
  prm.models.push_back(mp);
  RealtimeURDFFilter f(prm, tf, {{"d", xml}});
  CameraInfo ci;
  ci.width = W; ci.height = H;
  ci.P[0] = 525.0; ci.P[5] = 520.0; ci.P[2] = 319.5; ci.P[6] = 239.5; ci.P[10] = 1;
  double P[16];
  f.getProjectionMatrix(ci, P);
  std::vector<float> masked((size_t)W * H), plane((size_t)W * H), cleared((size_t)W * H);
  std::vector<uint16_t> masked_mm((size_t)W * H);
  std::vector<uint8_t> mask((size_t)W * H), mask_mm((size_t)W * H), mask_cleared((size_t)W * H);
  if (f.getScene(plane.data())) return 1;                                  // no context yet
  if (!f.learnScene(table.data(), false, P, W, H)) return 2;               // learn ...
  if (!f.getScene(plane.data())) return 3;
  if (!f.filter_into(depth.data(), false, P, W, H, 0.0, masked.data(), mask.data())) return 4;      // ... enabled by the parameters: filter
  if (!f.filter_into(mm.data(), true, P, W, H, 0.0, masked_mm.data(), mask_mm.data())) return 5;
  f.clearScene();
  if (!f.filter_into(depth.data(), false, P, W, H, 0.0, cleared.data(), mask_cleared.data())) return 6;
  FILE* o = fopen(argv[5], "wb");
  fwrite(plane.data(), 4, plane.size(), o);
  fwrite(masked.data(), 4, masked.size(), o);
  fwrite(mask.data(), 1, mask.size(), o);
  fwrite(masked_mm.data(), 2, masked_mm.size(), o);
  fwrite(mask_mm.data(), 1, mask_mm.size(), o);
  fwrite(cleared.data(), 4, cleared.size(), o);
  fwrite(mask_cleared.data(), 1, mask_cleared.size(), o);
  fclose(o);
  return 0;
}
'''


@gpu
def test_cpp_facade_learns_enables_and_filters(tmp_path):
    W, H, px = 640, 480, 640 * 480
    depth = sensor_plane()
    table = np.where(np.isfinite(depth) & (depth > 0), depth, F(3.0)).astype(F)
    mm = np.where((depth > 0) & (depth < 65.0), depth * F(1000.0), 0).astype(np.uint16)
    g, _ = example_facade()                                  # the robot filter alone, from the Python façade
    P = g.getProjectionMatrix(info())
    g.filter(depth, P, W, H)
    rm, rk = np.array(g.masked_depth_), np.array(g.mask_)
    g.filter(table, P, W, H)
    rk_table = np.array(g.mask_)
    rm_mm, rk_mm = g.filter_callback(mm, "16UC1", info())
    rm_mm, rk_mm = np.array(rm_mm), np.array(rk_mm)
    want_plane = SP.learned(np.full((1, H, W), np.inf, F), table[None], rk_table[None])
    margins = np.array([[0.03, 0.01]], F)
    ex = SP.expected(rm[None], rk[None], depth[None], want_plane, margins, 5.0)
    ex_mm = SP.expected(rm_mm[None], rk_mm[None], CC.u16_to_metres(mm)[None], want_plane, margins, 5.0, u16=True)
    src = tmp_path / "scene_facade.cpp"
    src.write_text(CPP)
    exe = tmp_path / "scene_facade"
    lib = os.path.join(ROOT, "realtime_urdf_filter_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lrtuf",
                           "-Wl,-rpath," + lib, "-o", str(exe)])
    (tmp_path / "x.urdf").write_text(WL.EXAMPLE_URDF)
    depth.tofile(tmp_path / "d.f32")
    table.tofile(tmp_path / "t.f32")
    mm.tofile(tmp_path / "d.u16")
    r = subprocess.run([str(exe)] + [str(tmp_path / n) for n in ("x.urdf", "d.f32", "t.f32", "d.u16", "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    cut = np.cumsum([0, 4 * px, 4 * px, px, 2 * px, px, 4 * px, px])
    part = lambda i, dt: raw[cut[i]:cut[i + 1]].view(dt).reshape(H, W)
    same_planes(part(0, F)[None], want_plane, "C++ façade: learned plane")
    check(ex, part(1, F)[None], part(2, np.uint8)[None], "C++ façade: learn, enable, filter")
    check(ex_mm, part(3, np.uint16)[None], part(4, np.uint8)[None], "C++ façade: 16UC1")
    assert bits_equal(part(5, F), rm) and np.array_equal(part(6, np.uint8), rk)      # after clearScene: the robot filter alone
