"""GPU (-m gpu): link padding (include/rtuf.h, LINK PADDING; rtuf_set_link_padding, rtuf_clear_link_padding).

Every output is compared for equality with bench_support/link_padding_check.py on the CPU oracle's planes (tests/
link_padding_scenes.py: the scenes, their paddings and the expectation of a batch; tests/test_link_padding_cpu.py holds that
expectation against cases worked out by hand and shows that every scene tells padding from no padding and from a square
dilation).  Clouds and clearance tables are built from the padded mask with the expectations those features have.  In this
process the scenes' few tiles take the 1,024-thread tile kernels; run as a script (RTUF_SMALL_LAUNCH=0 python
tests/test_link_padding_gpu.py) every scene goes through the 256-thread ones: the threshold is read once per process, so
test_every_scene_256_thread_kernels starts one."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import link_padding_scenes as LP
import realtime_urdf_filter_amd as R
from bench_support import clearance_check as KC
from bench_support import cloud_check as CC
from bench_support import link_padding_check as PC
from bench_support import workloads as WL
from gpu_support import (INTR, CloudBuffers, CloudExpect, DeviceWord, bits_equal, check_comp, check_org, cloud_enqueue, compare_labels, compare_planes,
                         example_facade, filter_expected, info, intrinsics, pack_bits, params, sensor_of, sensor_plane, torch_device, upload)
from oracle import bindings as O
from realtime_urdf_filter_amd.filter import depth_f32_to_u16

gpu = pytest.mark.gpu
F = np.float32
ERR_INVALID, ERR_STATE = -1, -6
STATUS_UNCOVERED = 1 << 20


def padded_context(sc, pads, max_streams=None, n=None, intr=True, **kw):
    """A context with the scene loaded, the intrinsics of gpu_support.intrinsics in every slot and the paddings set."""
    ctx = sc.context(max_streams=max_streams, n=n, **kw)
    if intr:
        ctx.set_cloud_intrinsics(0, [intrinsics(sc, i) for i in range(max_streams or sc.n)])
    ctx.set_link_padding(sc.ids[0], np.array(pads, F))
    return ctx


def check(ex, masked, mask, what, u16=False, n=None):
    n = n or len(ex.mask)
    if mask is not None:
        compare_labels(np.asarray(mask)[:n], ex.mask[:n], what, "mask")
    compare_planes(np.asarray(masked)[:n], ex.masked[:n], what, "16UC1 masked depth" if u16 else "masked depth")


def status_word(ctx):
    """The device status word of the batch enqueued last, read after the batch was retired."""
    torch, dev = torch_device()
    return int(torch.as_tensor(DeviceWord(ctx.batch_status_device()), device=dev).cpu().numpy()[0]) & 0xffffffff


def every_output_form(ctx, sc, pads, what, bits_forms=True):
    """f32 and 16UC1 device planes with and without byte mask, host planes synchronous and asynchronous, mask bits of both
    element types on host and device buffers: all against the expectation."""
    torch, dev = torch_device()
    ex, n = LP.expected(sc, pads), sc.n
    d = torch.from_numpy(sc.depth).to(dev)
    masked, mask = ctx.filter_batch(sc.depth)
    check(ex, masked, mask, what + " host planes")
    assert ctx.stats()["batch_status"] & ~STATUS_UNCOVERED == 0 and status_word(ctx) == 0
    masked, none = ctx.filter_batch(sc.depth, want_mask=False)
    assert none is None
    check(ex, masked, None, what + " host planes without mask")
    for with_mask in (True, False):
        dm = torch.full_like(d, 77.0)
        dk = torch.full(d.shape, 7, dtype=torch.uint8, device=dev)
        ctx.filter_batch_device(n, d.data_ptr(), dm.data_ptr(), dk.data_ptr() if with_mask else None)
        ctx.sync()
        check(ex, dm.cpu().numpy(), dk.cpu().numpy() if with_mask else None, what + " device planes, mask %s" % with_mask)
        assert with_mask or bool((dk == 7).all())
    pin_in, pin_out, pin_k = ctx.host_alloc(sc.depth.shape, F), ctx.host_alloc(sc.depth.shape, F), ctx.host_alloc(sc.depth.shape, np.uint8)
    pin_in[...] = sc.depth
    ctx.filter_batch_async(pin_in, pin_out, pin_k)
    ctx.sync()
    check(ex, pin_out, pin_k, what + " asynchronous host planes")
    for a in (pin_in, pin_out, pin_k):
        ctx.host_free(a)
    if sc.W % 4:                                   # planes only: the 16UC1 kernels and the mask bits need a width that is a multiple of 4
        return
    ex16, depth16 = LP.expected(sc, pads, u16=True), depth_f32_to_u16(sc.depth)
    d16 = torch.from_numpy(depth16.view(np.int16)).to(dev)
    m16, k16 = ctx.filter_batch_u16(depth16)
    check(ex16, m16, k16, what + " 16UC1 host planes", u16=True)
    for with_mask in (True, False):
        dm = torch.zeros_like(d16)
        dk = torch.full(d16.shape, 7, dtype=torch.uint8, device=dev)
        ctx.filter_batch_device_u16(n, d16.data_ptr(), dm.data_ptr(), dk.data_ptr() if with_mask else None)
        ctx.sync()
        check(ex16, dm.cpu().numpy().view(np.uint16), dk.cpu().numpy() if with_mask else None, what + " 16UC1 device planes, mask %s" % with_mask, u16=True)
    if not bits_forms:
        return
    words = ctx.mask_bits_words()
    for u16 in (False, True):
        e = ex16 if u16 else ex
        bits = np.zeros((n, words), np.uint32)
        ctx.filter_batch_bits_async(depth16 if u16 else sc.depth, bits)
        if e.undrawn:                              # a pixel no z reaches: the call fails when the batch is retired
            with pytest.raises(R.RtufError) as err:
                ctx.sync()
            assert err.value.code == ERR_STATE and "background quad" in str(err.value)
            assert ctx.stats()["batch_status"] & STATUS_UNCOVERED
            continue
        ctx.sync()
        db = torch.zeros((n, words), dtype=torch.int32, device=dev)
        ctx.filter_batch_device_bits(n, (d16 if u16 else d).data_ptr(), db.data_ptr(), u16=u16)
        ctx.sync()
        for s in range(n):
            want = pack_bits(e.mask[s])
            assert np.array_equal(bits[s], want), "%s mask bits (u16=%s) stream %d" % (what, u16, s)
            assert np.array_equal(db[s].cpu().numpy().view(np.uint32), want), "%s device mask bits (u16=%s) stream %d" % (what, u16, s)
            xm, xk = R.expand_mask_bits(depth16[s] if u16 else sc.depth[s], bits[s], sc.wl.replace_value)
            assert np.array_equal(xk, e.mask[s]) and (np.array_equal(xm, e.masked[s]) if u16 else bits_equal(xm, e.masked[s]))


# ---- every scene, every output form ---------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("name", LP.SCENES)
def test_every_output_form_matches_the_expectation(name, lanes):
    sc, pads = LP.scene(name)
    ctx = padded_context(sc, pads, raster_lanes=lanes)
    every_output_form(ctx, sc, pads, "%s, %d lanes" % (name, lanes))
    assert ctx.stats()["raster_lanes"] == lanes
    ctx.close()


@gpu
def test_every_scene_256_thread_kernels():
    """The scenes' planes with RTUF_SMALL_LAUNCH=0: every launch takes the 256-thread tile kernels."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=600,
                       env=dict(os.environ, RTUF_SMALL_LAUNCH="0"))
    assert r.returncode == 0 and "link padding ok %d" % len(LP.SCENES) in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- the two-kernel flag does not enter -------------------------------------------------------------------------------------------

@gpu
def test_the_two_kernel_flag_changes_nothing():
    sc, pads = LP.scene("soup")
    ctx = padded_context(sc, pads, flags=R.FLAG_TWO_KERNEL)
    every_output_form(ctx, sc, pads, "two-kernel flag", bits_forms=False)
    with pytest.raises(R.RtufError):               # the rule stays: no mask bits under RTUF_FLAG_TWO_KERNEL
        ctx.filter_batch_bits_async(sc.depth, np.zeros((sc.n, ctx.mask_bits_words()), np.uint32))
    cloud_forms(ctx, sc, pads, False, "two-kernel flag")
    clearance_form(ctx, sc, pads, False, "two-kernel flag")
    ctx.close()


# ---- clouds and clearance tables follow the padded mask --------------------------------------------------------------------------------

def cloud_forms(ctx, sc, pads, u16, what):
    ex = CloudExpect(sc, LP.expected(sc, pads, u16).mask, u16, tuple(range(sc.n)))
    d = upload(depth_f32_to_u16(sc.depth) if u16 else sc.depth)
    org, comp = CloudBuffers(sc, sc.n), CloudBuffers(sc, sc.n, sc.W * sc.H)
    cloud_enqueue(ctx, d, sc.n, org, u16)
    cloud_enqueue(ctx, d, sc.n, comp, u16)
    ctx.sync()
    assert ctx.stats()["batch_status"] == 0
    check_org(org.host()[0], ex, what + " organized")
    p, i, c = comp.host()
    check_comp(p, i, c, ex, sc.W * sc.H, what + " compacted")
    p, i, c = ctx.cloud_compact_batch(depth_f32_to_u16(sc.depth) if u16 else sc.depth, 4000)
    check_comp(p, i, c, ex, 4000, what + " compacted, host planes, capacity 4000")
    return ex


SPHERE_R = 0.2      # one sphere per link, at the origin of the link's frame
N_LABELS = 7        # default labels 1 .. 6


def clearance_form(ctx, sc, pads, u16, what, max_distance=1.5):
    links = list(range(sc.n_links))
    ctx.set_link_spheres(sc.ids[0], links, [(0.0, 0.0, 0.0, SPHERE_R)] * len(links))
    mask, sensor = LP.expected(sc, pads, u16).mask, sensor_of(sc, u16)
    want = np.zeros((sc.n, N_LABELS), KC.DTYPE)
    for s in range(sc.n):
        pts, idx, _ = CC.compacted(sensor[s], mask[s], intrinsics(sc, s))
        centres = KC.posed(sc.wl.link_tf[0][s], sc.wl.cam_tf[s], sc.wl.offset_inv[s], links, [(0.0, 0.0, 0.0)] * len(links))
        want[s] = KC.table(pts, idx, centres, [SPHERE_R] * len(links), [l + 1 for l in links], links, N_LABELS, max_distance)
    assert np.isfinite(want["clearance"]).any() and (want["points_within"] > 64).any()
    got = ctx.link_clearance_batch(depth_f32_to_u16(sc.depth) if u16 else sc.depth, N_LABELS, max_distance)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: clearance rows differ\ngot  %s\nwant %s" % (what, got, want)
    torch, dev = torch_device()
    t = torch.full((sc.n, N_LABELS, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ctx.link_clearance_batch_device(sc.n, upload(depth_f32_to_u16(sc.depth) if u16 else sc.depth).data_ptr(), t.data_ptr(), N_LABELS, max_distance, u16=u16)
    ctx.sync()
    assert np.array_equal(np.ascontiguousarray(t.cpu().numpy()).view(np.uint32).reshape(sc.n, N_LABELS, 4), want.view(np.uint32).reshape(sc.n, N_LABELS, 4)), what
    return want


@gpu
@pytest.mark.parametrize("u16", [False, True])
def test_clouds_and_clearance_tables_hold_neither_the_robot_nor_its_halo(u16):
    sc, pads = LP.scene("soup")
    ctx = padded_context(sc, pads)
    padded = cloud_forms(ctx, sc, pads, u16, "cloud u16=%s" % u16)
    plain = CloudExpect(sc, filter_expected(sc, 0, u16)[1], u16, tuple(range(sc.n)))
    assert (padded.counts < plain.counts).all()     # the halo's points are gone
    clearance_form(ctx, sc, pads, u16, "clearance u16=%s" % u16)
    ctx.close()


# ---- batch and lane shapes ----------------------------------------------------------------------------------------------------------

@gpu
def test_partial_batch_of_three_in_eight_slots_with_shrunk_groups():
    """n < max_streams, three lanes, launch groups of two streams: the slot plane is per lane and per stream of the group, the
    tile kernel's label plane per stream of the batch."""
    sc, pads = LP.scene("soup")
    ctx = padded_context(sc, pads, max_streams=8, max_inflight_streams=2, raster_lanes=3)
    ex = LP.expected(sc, pads)
    torch, dev = torch_device()
    d = torch.from_numpy(sc.depth).to(dev)
    dm = torch.full((8, sc.H, sc.W), 77.0, dtype=torch.float32, device=dev)
    dk = torch.full((8, sc.H, sc.W), 7, dtype=torch.uint8, device=dev)
    for batch in range(2):
        ctx.filter_batch_device(3, d.data_ptr(), dm.data_ptr(), dk.data_ptr())
        ctx.sync()
        check(ex, dm.cpu().numpy(), dk.cpu().numpy(), "partial batch %d" % batch, n=3)
        assert status_word(ctx) == 0 and ctx.stats()["groups_last_batch"] >= 2
    assert bool((dm[3:] == 77.0).all()) and bool((dk[3:] == 7).all())       # the other streams' planes are left alone
    masked, mask = ctx.filter_batch(sc.depth)
    check(ex, masked, mask, "partial batch, host planes")
    ctx.close()


@gpu
@pytest.mark.parametrize("bits", [False, True])
def test_regrown_bins_rerun_the_batch_and_redo_both_planes(bits):
    sc, pads = LP.scene("soup")
    ctx = padded_context(sc, pads, bin_capacity=1)
    ex = LP.expected(sc, pads)
    if bits:
        out = np.zeros((sc.n, ctx.mask_bits_words()), np.uint32)
        ctx.filter_batch_bits_async(sc.depth, out)
        ctx.sync()
        for s in range(sc.n):
            assert np.array_equal(out[s], pack_bits(ex.mask[s])), s
    else:
        masked, mask = ctx.filter_batch(sc.depth)
        check(ex, masked, mask, "re-run")
    st = ctx.stats()
    assert st["regrowths"] >= 1 and st["batch_reruns"] >= 1 and st["batch_status"] != 0
    assert status_word(ctx) == 0                    # the re-run left the word at 0
    masked, mask = ctx.filter_batch(sc.depth)       # the next batch is final at once
    check(ex, masked, mask, "after the re-run")
    assert ctx.stats()["batch_status"] == 0 and status_word(ctx) == 0
    ctx.close()


@gpu
@pytest.mark.parametrize("name", ["ramp", "near_quad"])
def test_one_stream_batches_through_two_pipelines(name):
    """pipelines = 2, batches of one stream: graph replay is on, and the paddings change between batches."""
    sc, pads = LP.scene(name)
    ctx = padded_context(sc, pads, max_streams=1, n=1, raster_lanes=1, pipelines=2)
    half = tuple(0.5 * p for p in pads)
    for batch, p in enumerate((pads, pads, half, half, pads, pads)):
        ctx.set_link_padding(sc.ids[0], np.array(p, F))
        masked, mask = ctx.filter_batch(sc.depth[:1])
        check(LP.expected(sc, p, streams=[0]), masked, mask, "%s pipelines, batch %d" % (name, batch))
        assert status_word(ctx) == 0
    ctx.close()


# ---- focal lengths ------------------------------------------------------------------------------------------------------------------

@gpu
def test_every_stream_has_its_own_focal_length_and_the_larger_of_fx_and_fy_counts():
    sc, pads = LP.scene("soup")
    ctx = padded_context(sc, pads, intr=False)
    intr = [(100.0, 140.5, 80.0, 60.0), (131.25, 131.25, 79.5, 59.5), (200.0, 90.0, 70.0, 50.0)]
    ctx.set_cloud_intrinsics(0, intr)
    ex = LP.expected(sc, pads, focals=[140.5, 131.25, 200.0])
    masked, mask = ctx.filter_batch(sc.depth)
    check(ex, masked, mask, "fy > fx, fx == fy, fx > fy")
    smaller = LP.expected(sc, pads, focals=[100.0, 131.25, 90.0])
    assert (ex.mask[0] != smaller.mask[0]).any() and (ex.mask[2] != smaller.mask[2]).any()      # (min(fx, fy) would show)
    ctx.set_cloud_intrinsics(1, [(300.0, 10.0, 79.5, 59.5)])                                   # one stream's, later
    ex = LP.expected(sc, pads, focals=[140.5, 300.0, 200.0])
    masked, mask = ctx.filter_batch(sc.depth)
    check(ex, masked, mask, "stream 1 given again")
    ctx.close()


# ---- what is refused, and that clearing the padding restores everything ------------------------------------------------------------------

def refused(code, match, call, *args, **kw):
    with pytest.raises(R.RtufError) as err:
        call(*args, **kw)
    assert err.value.code == code and match in str(err.value), str(err.value)


@gpu
def test_refusals_and_the_way_back():
    sc, pads = LP.scene("soup")
    fresh = sc.context()
    plain = fresh.filter_batch(sc.depth)
    plain_labels = fresh.filter_batch_labels(sc.depth)
    plain_virtual = fresh.render_batch(sc.n)
    plain_resid = fresh.link_residuals_batch(sc.depth, N_LABELS)
    fresh.close()
    ctx = padded_context(sc, pads)
    m, nl = sc.ids[0], sc.n_links
    ex = LP.expected(sc, pads)
    words = np.zeros((sc.n, ctx.mask_bits_words()), np.uint32)

    def works():
        masked, mask = ctx.filter_batch(sc.depth)
        check(ex, masked, mask, "after a refused call")

    # the setter's own checks: nothing changes
    lib, h = ctx._lib, ctx._h
    good = np.array(pads, F)
    for bad in (-0.01, np.nan, np.inf, -np.inf):
        a = good.copy()
        a[2] = bad
        refused(ERR_INVALID, "padding must be finite", ctx.set_link_padding, m, a)
    refused(ERR_INVALID, "links", ctx.set_link_padding, m, good[:-1])
    assert lib.rtuf_set_link_padding(h, m, None, nl) == ERR_INVALID and lib.rtuf_set_link_padding(h, 5, good.ctypes.data, nl) == ERR_INVALID
    assert lib.rtuf_set_link_padding(h, -1, good.ctypes.data, nl) == ERR_INVALID and lib.rtuf_clear_link_padding(h, 5) == ERR_INVALID
    works()
    # batches that have no padded route
    refused(ERR_INVALID, "link labels", ctx.filter_batch_labels, sc.depth)
    refused(ERR_INVALID, "virtual depth", ctx.render_batch, sc.n)
    refused(ERR_INVALID, "residual", ctx.link_residuals_batch, sc.depth, N_LABELS)
    works()
    # a silhouette radius: every batch
    p = params(replace=sc.wl.replace_value, max_diff=sc.wl.max_diff, silhouette_dilation_px=2)
    p.near_plane, p.far_plane = sc.wl.near, sc.wl.far
    ctx.set_params(p)
    refused(ERR_INVALID, "silhouette dilation", ctx.filter_batch, sc.depth)
    refused(ERR_INVALID, "silhouette dilation", ctx.filter_batch_u16, depth_f32_to_u16(sc.depth))
    refused(ERR_INVALID, "silhouette dilation", ctx.filter_batch_bits_async, sc.depth, words)
    refused(ERR_INVALID, "silhouette dilation", ctx.cloud_batch, sc.depth)
    refused(ERR_INVALID, "silhouette dilation", ctx.link_clearance_batch, sc.depth, N_LABELS, 1.0)
    p.silhouette_dilation_px = 0
    ctx.set_params(p)
    works()
    # per-link thresholds in effect
    ctx.set_link_thresholds(m, np.full(nl, 0.1, F))
    refused(ERR_INVALID, "per-link depth thresholds", ctx.filter_batch, sc.depth)
    refused(ERR_INVALID, "per-link depth thresholds", ctx.filter_batch_bits_async, sc.depth, words)
    refused(ERR_INVALID, "per-link depth thresholds", ctx.cloud_batch, sc.depth)
    refused(ERR_INVALID, "per-link depth thresholds", ctx.link_clearance_batch, sc.depth, N_LABELS, 1.0)
    ctx.clear_link_thresholds(m)
    works()
    assert ctx.stats()["batch_status"] == 0
    # all-zero paddings are not "in effect", and after the clear nothing differs from a context that never used padding
    for step in ("zeros", "cleared", "cleared twice"):
        if step == "zeros":
            ctx.set_link_padding(m, np.zeros(nl, F))
        else:
            ctx.clear_link_padding(m)
        masked, mask = ctx.filter_batch(sc.depth)
        assert np.array_equal(mask, plain[1]) and bits_equal(masked, plain[0]), step
        assert np.array_equal(mask, sc.mask) and bits_equal(masked, sc.masked), step
        got = ctx.filter_batch_labels(sc.depth)
        assert all(np.array_equal(a, b) for a, b in zip(got[1:], plain_labels[1:])) and bits_equal(got[0], plain_labels[0]), step
        v = ctx.render_batch(sc.n)
        assert bits_equal(v[0], plain_virtual[0]), step
        assert np.array_equal(ctx.link_residuals_batch(sc.depth, N_LABELS), plain_resid), step
        if step == "zeros":
            ctx.set_link_padding(m, good)
            works()
    ctx.close()


@gpu
def test_a_stream_without_intrinsics_is_a_state_error():
    sc, pads = LP.scene("soup")
    ctx = padded_context(sc, pads, intr=False)
    refused(ERR_STATE, "stream 0 has no cloud intrinsics", ctx.filter_batch, sc.depth)
    ctx.set_cloud_intrinsics(0, [intrinsics(sc, i) for i in range(2)])
    refused(ERR_STATE, "stream 2 has no cloud intrinsics", ctx.filter_batch, sc.depth)
    refused(ERR_STATE, "stream 2 has no cloud intrinsics", ctx.filter_batch_bits_async, sc.depth, np.zeros((sc.n, ctx.mask_bits_words()), np.uint32))
    masked, mask = ctx.filter_batch(sc.depth[:2])                      # the batch of the two streams that have theirs
    check(LP.expected(sc, pads, streams=[0, 1]), masked, mask, "two streams")
    ctx.close()


# ---- the façades -----------------------------------------------------------------------------------------------------------------------

ENTRIES = [{"link": "wall1", "padding": 0.05}, {"link": "world", "padding": 0.08}]

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
  const std::vector<float> depth = slurp<float>(argv[2]);
  const std::vector<uint16_t> mm = slurp<uint16_t>(argv[3]);
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
  ModelParameter mp;
  mp.model = "d"; mp.tf_prefix = "/EXAMPLE"; mp.geometry_type = "visual";
  mp.link_padding.push_back({"wall1", 0.05});
  mp.link_padding.push_back({"world", 0.08});
  prm.models.push_back(mp);
  RealtimeURDFFilter f(prm, tf, {{"d", xml}});
  CameraInfo ci;
  ci.width = W; ci.height = H;
  ci.P[0] = 525.0; ci.P[5] = 520.0; ci.P[2] = 319.5; ci.P[6] = 239.5; ci.P[10] = 1;
  double P[16];
  f.getProjectionMatrix(ci, P);
  std::vector<float> masked((size_t)W * H);
  std::vector<uint16_t> masked_mm((size_t)W * H);
  std::vector<uint8_t> mask((size_t)W * H), mask_mm((size_t)W * H);
  if (!f.filter_into(depth.data(), false, P, W, H, 0.0, masked.data(), mask.data())) return 1;
  if (!f.filter_into(mm.data(), true, P, W, H, 0.0, masked_mm.data(), mask_mm.data())) return 2;
  FILE* o = fopen(argv[4], "wb");
  fwrite(masked.data(), 4, masked.size(), o);
  fwrite(mask.data(), 1, mask.size(), o);
  fwrite(masked_mm.data(), 2, masked_mm.size(), o);
  fwrite(mask_mm.data(), 1, mask_mm.size(), o);
  fclose(o);
  return 0;
}
'''


def facade_expectation(f, tf, depth, P):
    rd = f.renderers_[0]
    pad_of = {e["link"]: e["padding"] for e in ENTRIES}
    draws = [(r.gl_matrix(), d.pre_op, d.op, d.verts, d.tris) for r in rd.renderables_ for d in r.draws]
    draw_pad = [F(pad_of.get(r.urdf_link, 0.0)) for r in rd.renderables_ for d in r.draws]
    ntris = [len(d.tris) for r in rd.renderables_ for d in r.draws]
    offset_inv, cam_tf = f._camera_matrices(tf, None)
    frame = O.PreparedFrame(depth, P, draws, offset_inv, cam_tf, max_diff=0.05, replace_value=5.0, want_debug=True)
    O.run_prepared([frame], O.usable_threads())
    masked, mask, R2 = PC.expected_planes(frame.zwin, frame.prim, depth, draw_pad, ntris, F(max(INTR[0], INTR[1])), 0.1, 8.0, 0.05, 5.0)
    assert R2.max() >= 16 and (mask != frame.mask).sum() > 100            # the margins show
    return masked, mask


@gpu
def test_python_facade_with_padding_entries():
    depth = sensor_plane()
    f, tf = example_facade(model_entries={"link_depth_distance_thresholds": ENTRIES})
    P = f.getProjectionMatrix(info())
    f.filter(depth, P, 640, 480)
    masked, mask = facade_expectation(f, tf, depth, P)
    compare_labels(f.mask_, mask, "façade filter()", "mask")
    compare_planes(f.getMaskedDepth(), masked, "façade filter()")
    got = f.filter_batch(depth[None], P, [tf])
    compare_labels(got[1][0], mask, "façade filter_batch()", "mask")
    # the cloud of the same frame holds neither the robot nor its margins
    pts, idx = f.cloud(depth, P, 640, 480, compact=True)
    want = CC.compacted(depth, mask, INTR)
    assert np.array_equal(idx, want[1][:want[2]]) and np.array_equal(pts.view(np.uint32), want[0][:want[2]].view(np.uint32))


@gpu
def test_cpp_facade_with_link_padding(tmp_path):
    depth = sensor_plane()
    f, tf = example_facade(model_entries={"link_depth_distance_thresholds": ENTRIES})
    P = f.getProjectionMatrix(info())
    f.filter(depth, P, 640, 480)
    masked, mask = facade_expectation(f, tf, depth, P)
    mm = np.where((depth > 0) & (depth < 65.0), depth * F(1000.0), 0).astype(np.uint16)
    masked_mm, mask_mm = facade_expectation(f, tf, CC.u16_to_metres(mm), P)
    masked_mm = depth_f32_to_u16(masked_mm)
    src = tmp_path / "padding_facade.cpp"
    src.write_text(CPP)
    exe = tmp_path / "padding_facade"
    lib = os.path.join(ROOT, "realtime_urdf_filter_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lrtuf",
                           "-Wl,-rpath," + lib, "-o", str(exe)])
    (tmp_path / "x.urdf").write_text(WL.EXAMPLE_URDF)
    depth.tofile(tmp_path / "d.f32")
    mm.tofile(tmp_path / "d.u16")
    r = subprocess.run([str(exe)] + [str(tmp_path / n) for n in ("x.urdf", "d.f32", "d.u16", "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    px = 640 * 480
    compare_planes(raw[:4 * px].view(F).reshape(480, 640), masked, "C++ façade filter_into")
    compare_labels(raw[4 * px:5 * px].reshape(480, 640), mask, "C++ façade filter_into", "mask")
    compare_planes(raw[5 * px:7 * px].view(np.uint16).reshape(480, 640), masked_mm, "C++ façade filter_into, 16UC1", "16UC1 masked depth")
    compare_labels(raw[7 * px:].reshape(480, 640), mask_mm, "C++ façade filter_into, 16UC1", "mask")


if __name__ == "__main__":
    for scene_name in LP.SCENES:
        scene_, pads_ = LP.scene(scene_name)
        context_ = padded_context(scene_, pads_, raster_lanes=3)
        every_output_form(context_, scene_, pads_, "%s, 256-thread kernels" % scene_name)
        context_.close()
    print("link padding ok %d" % len(LP.SCENES))
