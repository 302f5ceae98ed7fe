"""GPU (-m gpu): voxel free space (include/rtuf.h, VOXEL FREE SPACE).

The expectation is bench_support/voxel_free_check.py applied to the sensor planes, the slots' intrinsics
(gpu_support.intrinsics), the streams' world_from_optical matrices and the grid -- never the library's own output.  Everything
is an integer, so free words and summaries are held for equality.  Every expectation first asserts that it is not vacuous."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bench_support import cloud_check as CC
from bench_support import voxel_check as VC
from bench_support import voxel_free_check as VF
from bench_support import workloads as WL
from gpu_support import INTR, cached, cloud_context, example_facade, filter_expected, info, intrinsics, sensor_of, sensor_plane, soup_scene, torch_device, upload

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = -1, -6
SENT32 = 0x5A5A5A5A
F = np.float32

FINE = VC.Grid((-1.5, -1.0, 0.5), 0.05, (61, 40, 64))
ODD = VC.Grid((-1.5, -1.0, -0.4), 0.05, (61, 41, 63))            # 157,563 voxels: n % 32 == 27; its first layers lie behind the cameras
COARSE = VC.Grid((-1.5, -1.0, 0.5), 0.5, (5, 4, 6))              # 120 voxels: under two waves
TRANSFORMS = (None, VC.rotation_z(0.3, (0.1, 0.0, 0.0)), VC.rotation_z(0.6, (0.0, 0.1, 0.0)))
ROLLED = tuple(VC.rotation_z(np.pi / 2, (0.05 * s, -0.02 * s, 0.0)) for s in range(3))      # a 90 degree roll about the optical axis
SINGULAR = np.array([[1.0, 2.0, 3.0, 0.1], [2.0, 4.0, 6.0, 0.2], [0.5, 0.1, 0.7, 0.3], [0, 0, 0, 1]]).T.reshape(16)
MARGIN = 0.05


@cached
def soup():
    return soup_scene(11, 160, 120)


_EXPECTED = {}


def expect(scene=None, grid=FINE, matrices=TRANSFORMS, margin=MARGIN, r=0, u16=False, streams=None):
    """(bits, summary [n,4]) of one carve of streams `streams` of the scene (in slots 0 ..) into the empty free grid: computed
    once per case and shared (nobody writes to it)."""
    sc = scene or soup()
    streams = tuple(range(sc.n)) if streams is None else tuple(streams)
    key = (sc.name, grid.origin, grid.voxel_size, grid.dims, id(matrices), margin, r, u16, streams)
    if key not in _EXPECTED:
        sensor = sensor_of(sc, u16)
        ex = VF.expected([sensor[s] for s in streams], [intrinsics(sc, i) for i in range(len(streams))], [matrices[i] for i in range(len(streams))], grid, margin, r)
        ex[0].setflags(write=False)
        ex[1].setflags(write=False)
        _EXPECTED[key] = ex
    ex = _EXPECTED[key]
    # (a vacuous pass must not hide: every stream frees voxels, leaves judged ones not free and does not see others)
    assert (ex[1][:, :3] > 0).all(), ex[1]
    return ex


def give_grid(ctx, grid, matrices, counts=True):
    ctx.set_voxel_grid(grid.origin, grid.voxel_size, grid.dims, counts)
    for s, m in enumerate(matrices or ()):
        if s < ctx.max_streams:
            ctx.set_voxel_transforms(s, m)


def context(sc, grid, matrices=TRANSFORMS, n=None, **kw):
    ctx = cloud_context(sc, n=n, **kw)
    give_grid(ctx, grid, matrices)
    return ctx


def sensor_planes(sc, u16=False):
    from realtime_urdf_filter_amd.filter import depth_f32_to_u16
    return depth_f32_to_u16(sc.depth) if u16 else sc.depth


def carve(ctx, sensor, margin=MARGIN, r=0, n=None, total=None, summary=True):
    """One device carve of the first n planes of `sensor`; -> the summary rows [total,4] (rows past n keep the sentinel)."""
    torch, dev = torch_device()
    n = n or len(sensor)
    summ = torch.full((total or n, 4), SENT32, dtype=torch.int32, device=dev)
    d = upload(np.ascontiguousarray(sensor))
    ctx.voxel_carve_batch_device(n, d.data_ptr(), margin, r, summ.data_ptr() if summary else None, u16=sensor.dtype == np.uint16)
    return np.ascontiguousarray(summ.cpu().numpy()).view(np.uint32)


def check(ctx, ex, summ, what, grid=FINE):
    free = ctx.voxel_free()
    assert free.shape == ex[0].shape and np.array_equal(free, ex[0]), "%s: %d free words differ" % (what, int((free != ex[0]).sum()))
    assert ctx.voxel_free_device()[1] == grid.n_voxels
    if summ is not None:
        assert np.array_equal(summ[:len(ex[1])], ex[1]), "%s: summary %s instead of %s" % (what, summ.tolist(), ex[1].tolist())
        assert (summ[len(ex[1]):] == SENT32).all(), "%s: summary rows beyond the batch were written" % what


# ---- 1 .. 3: grids ------------------------------------------------------------------------------------------------------------------

@gpu
def test_fine_grid_three_streams_two_of_them_transformed():
    sc = soup()
    ex = expect()
    ctx = context(sc, FINE)
    check(ctx, ex, carve(ctx, sc.depth, total=5), "fine grid")
    ctx.close()


@gpu
def test_a_grid_that_ends_inside_a_word_and_starts_behind_the_cameras():
    sc = soup()
    ex = expect(grid=ODD)
    behind = VF.centres(ODD)[:, 2] <= 0
    assert ODD.n_voxels % 32 == 27 and ODD.n_voxels % 64 != 0 and behind.sum() > 15000 and not VF.unpack(ex[0], ODD)[behind].any()
    assert (ex[1][:, 2] > behind.sum()).all()
    ctx = context(sc, ODD)
    summ = carve(ctx, sc.depth)
    check(ctx, ex, summ, "odd grid", ODD)
    free = ctx.voxel_free()
    assert len(free) == ODD.n_words and free[-1] >> 27 == 0
    ctx.close()


@gpu
def test_coarse_grid_under_two_waves():
    sc = soup()
    ex = expect(grid=COARSE)
    assert COARSE.n_voxels < 128 and (ex[1][:, 0] >= 30).all() and (ex[1][:, 1] >= 15).all()
    ctx = context(sc, COARSE)
    check(ctx, ex, carve(ctx, sc.depth), "coarse grid", COARSE)
    ctx.close()


@gpu
def test_more_streams_than_one_summary_chunk():
    """260 streams: the summary table of a workgroup holds 256 at a time.  Planes, pinholes and transforms differ per stream."""
    sc = soup()
    n = 260
    planes = np.stack([np.roll(sc.depth[s % sc.n], 3 * s, axis=1) for s in range(n)])
    intr = [intrinsics(sc, s % 7) for s in range(n)]
    matrices = [None if s % 5 == 0 else VC.rotation_z(0.002 * s, (0.001 * s, -0.0005 * s, 0.0)) for s in range(n)]
    ex = VF.expected(list(planes), intr, matrices, FINE, MARGIN, 0)
    assert (ex[1][:, :3] > 0).all() and len(ex[1]) > 256 and not np.array_equal(ex[1][256], ex[1][0])
    ctx = sc.context(max_streams=n)
    ctx.set_cloud_intrinsics(0, intr)
    give_grid(ctx, FINE, matrices)
    check(ctx, ex, carve(ctx, planes, total=n + 1), "260 streams")
    ctx.voxel_clear()
    carve(ctx, planes, summary=False)
    check(ctx, ex, None, "260 streams, no summary")
    ctx.close()


# ---- 4: radii and margins -------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("margin", [0.0, MARGIN], ids=["m0", "m5cm"])
@pytest.mark.parametrize("r", [1, 4], ids=["r1", "r4"])
def test_window_radius(r, margin):
    sc = soup()
    ex = expect(margin=margin, r=r)
    assert not np.array_equal(ex[0], expect(margin=margin, r=0)[0])
    ctx = context(sc, FINE)
    check(ctx, ex, carve(ctx, sc.depth, margin, r), "r = %d, margin %g" % (r, margin))
    ctx.close()


# ---- 5, 6: 16UC1 and no summary -------------------------------------------------------------------------------------------------------

@gpu
def test_16uc1_device_planes():
    sc = soup()
    ex = expect(u16=True)
    assert not np.array_equal(ex[0], expect()[0])           # (whole millimetres move some centres across the threshold)
    ctx = context(sc, FINE)
    check(ctx, ex, carve(ctx, sensor_planes(sc, True)), "16UC1")
    ctx.voxel_clear()
    ex4 = expect(u16=True, r=4)
    check(ctx, ex4, carve(ctx, sensor_planes(sc, True), r=4), "16UC1, r = 4")
    ctx.close()


@gpu
def test_without_a_summary_the_bits_are_the_same():
    sc = soup()
    ex = expect()
    ctx = context(sc, FINE)
    summ = carve(ctx, sc.depth, summary=False)
    assert (summ == SENT32).all()
    check(ctx, ex, None, "no summary")
    ctx.voxel_clear()
    ex2 = expect(r=2)
    carve(ctx, sc.depth, r=2, summary=False)
    check(ctx, ex2, None, "no summary, r = 2")
    ctx.close()


# ---- 7: accumulation ----------------------------------------------------------------------------------------------------------------------

@gpu
def test_carves_accumulate_until_the_grid_is_cleared_or_replaced():
    sc = soup()
    first = expect(streams=(0, 1))
    second = expect(streams=(2,))                       # stream 2's plane in slot 0: slot 0's intrinsics, no transform
    both = first[0] | second[0]
    assert (both != first[0]).any() and (both != second[0]).any()
    ctx = cloud_context(sc)
    give_grid(ctx, FINE, TRANSFORMS)
    with_grid = ctx.stats()["device_bytes"]
    assert not ctx.voxel_free().any()                    # (the first read allocates the words, zeroed)
    assert FINE.n_words % 4 == 0 and ctx.stats()["device_bytes"] == with_grid + 4 * FINE.n_words
    check(ctx, first, carve(ctx, sc.depth, n=2, total=3), "streams 0 and 1")
    check(ctx, (both, second[1]), carve(ctx, sc.depth[2:3]), "... and stream 2's plane in slot 0")
    check(ctx, (both, first[1]), carve(ctx, sc.depth, n=2), "... and the first carve again")
    bits_before = ctx.voxel_grid()[0]
    ctx.voxel_clear()
    assert not ctx.voxel_free().any() and not bits_before.any()
    check(ctx, second, carve(ctx, sc.depth[2:3]), "after voxel_clear")
    give_grid(ctx, FINE, TRANSFORMS)                     # again: freed, and zeroed when it is next read
    assert ctx.stats()["device_bytes"] == with_grid and not ctx.voxel_free().any()
    check(ctx, first, carve(ctx, sc.depth, n=2), "after the grid was set again")
    ctx.set_voxel_grid(None, 0.0, None)
    assert ctx.stats()["device_bytes"] == with_grid - 4 * FINE.n_words - 4 * FINE.n_voxels
    ctx.close()


# ---- 8: beside an insert ------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("order", ["insert_first", "carve_first"])
def test_beside_an_insert(order):
    torch, dev = torch_device()
    sc = soup()
    ex = expect()
    occ = VC.expected_planes(list(sc.depth), list(filter_expected(sc, 0)[1]), [intrinsics(sc, i) for i in range(sc.n)], TRANSFORMS, FINE)
    n_both = int((VF.unpack(occ[0], FINE) & VF.unpack(ex[0], FINE)).sum())
    assert n_both > 1000 and (occ[2][:, 0] > 0).all()
    ctx = context(sc, FINE)
    d = upload(sc.depth)
    if order == "insert_first":
        ctx.voxel_insert_batch_device(sc.n, d.data_ptr())
    summ = carve(ctx, sc.depth)
    if order == "carve_first":
        ctx.voxel_insert_batch_device(sc.n, d.data_ptr())
    check(ctx, ex, summ, order)
    bits, counts = ctx.voxel_grid()
    assert np.array_equal(bits, occ[0]) and np.array_equal(counts.reshape(-1), occ[1])
    assert int((VF.unpack(bits, FINE) & VF.unpack(ctx.voxel_free(), FINE)).sum()) == n_both
    ctx.close()


# ---- 9: widths that are no multiple of 4 ----------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("case", ["150x70", "100x75_rolled"])
def test_any_width_is_accepted(case):
    sc, matrices = (soup_scene(11, 150, 70), TRANSFORMS) if case == "150x70" else (soup_scene(3, 100, 75), ROLLED)
    assert sc.W % 4 != 0 or case != "150x70"
    for u16 in (False, True):
        ex = expect(sc, matrices=matrices, r=1, u16=u16)
        ctx = context(sc, FINE, matrices)
        check(ctx, ex, carve(ctx, sensor_planes(sc, u16), r=1), "%s%s" % (case, ", 16UC1" if u16 else ""))
        ctx.close()


# ---- 10: the batch machinery ----------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("kw", [dict(raster_lanes=3), dict(pipelines=2)], ids=["three_lanes", "two_pipelines"])
def test_a_filter_batch_in_flight_is_retired_and_correct(kw):
    torch, dev = torch_device()
    sc = soup()
    ex = expect()
    want = filter_expected(sc, 0)
    ctx = context(sc, FINE, **kw)
    d = upload(sc.depth)
    masked, mask = torch.empty_like(d), torch.zeros(d.shape, dtype=torch.uint8, device=dev)
    ctx.filter_batch_device(sc.n, d.data_ptr(), masked.data_ptr(), mask.data_ptr())
    summ = carve(ctx, sc.depth)                         # (no sync in between)
    assert np.array_equal(mask.cpu().numpy(), want[1]) and np.array_equal(masked.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    check(ctx, ex, summ, "behind a filter batch, %s" % kw)
    # ... and the filter's own output planes as the carve's input, the batch still in flight
    ctx.voxel_clear()
    ctx.filter_batch_device(sc.n, d.data_ptr(), masked.data_ptr(), mask.data_ptr())
    summ = torch.full((sc.n, 4), SENT32, dtype=torch.int32, device=dev)
    ctx.voxel_carve_batch_device(sc.n, masked.data_ptr(), MARGIN, 0, summ.data_ptr())
    ex_masked = VF.expected(list(want[0]), [intrinsics(sc, i) for i in range(sc.n)], TRANSFORMS, FINE, MARGIN, 0)
    assert (ex_masked[1][:, :3] > 0).all() and not np.array_equal(ex_masked[0], ex[0])
    check(ctx, ex_masked, np.ascontiguousarray(summ.cpu().numpy()).view(np.uint32), "the masked planes of a batch in flight")
    ctx.close()


# ---- 11: refusals -----------------------------------------------------------------------------------------------------------------------------

def refused(code, call, *args, **kw):
    import realtime_urdf_filter_amd as R
    with pytest.raises(R.RtufError) as e:
        call(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


@gpu
def test_refused_calls_write_nothing_and_leave_the_free_words_as_they_were():
    import realtime_urdf_filter_amd as R
    torch, dev = torch_device()
    sc = soup()
    ex = expect()
    d = upload(sc.depth)
    summ = torch.full((sc.n + 1, 4), SENT32, dtype=torch.int32, device=dev)
    # no grid yet
    ctx = cloud_context(sc)
    refused(STATE, ctx.voxel_carve_batch_device, sc.n, d.data_ptr(), MARGIN, 0, summ.data_ptr())
    refused(STATE, ctx.voxel_carve_batch, sc.depth, MARGIN)
    refused(STATE, ctx.voxel_free)
    refused(STATE, ctx.voxel_free_device)
    # a context that is not finalized
    raw = R.Context(sc.W, sc.H, sc.n, 0, ctx.params)
    raw.set_voxel_grid(FINE.origin, FINE.voxel_size, FINE.dims)
    raw.set_cloud_intrinsics(0, [intrinsics(sc, i) for i in range(sc.n)])
    refused(STATE, raw.voxel_carve_batch_device, sc.n, d.data_ptr(), MARGIN, 0, summ.data_ptr())
    refused(STATE, raw.voxel_carve_batch, sc.depth, MARGIN)
    assert not raw.voxel_free().any()
    raw.close()
    # bad arguments: each leaves the free words of the first carve
    give_grid(ctx, FINE, TRANSFORMS)
    first = carve(ctx, sc.depth)
    refused(INVALID, ctx.voxel_carve_batch_device, 0, d.data_ptr(), MARGIN, 0, summ.data_ptr())
    refused(INVALID, ctx.voxel_carve_batch_device, sc.n + 1, d.data_ptr(), MARGIN, 0, summ.data_ptr())
    refused(INVALID, ctx.voxel_carve_batch_device, sc.n, None, MARGIN, 0, summ.data_ptr())
    refused(INVALID, ctx.voxel_carve_batch_device, sc.n, None, MARGIN, 0, summ.data_ptr(), u16=True)
    for r in (-1, 5):
        refused(INVALID, ctx.voxel_carve_batch_device, sc.n, d.data_ptr(), MARGIN, r, summ.data_ptr())
        refused(INVALID, ctx.voxel_carve_batch, sc.depth, MARGIN, r)
    for margin in (-0.01, np.nan, np.inf, 1e39):
        refused(INVALID, ctx.voxel_carve_batch_device, sc.n, d.data_ptr(), margin, 0, summ.data_ptr())
        refused(INVALID, ctx.voxel_carve_batch, sc.depth, margin)
    PP = ctypes.c_void_p * sc.n
    host_summary = np.full((sc.n, 4), SENT32, np.uint32)
    assert ctx._lib.rtuf_voxel_carve_batch(ctx._h, sc.n, None, MARGIN, 0, host_summary.ctypes.data_as(ctypes.c_void_p)) == INVALID
    assert ctx._lib.rtuf_voxel_carve_batch(ctx._h, sc.n, PP(sc.depth[0].ctypes.data, None, sc.depth[2].ctypes.data), MARGIN, 0,
                                           host_summary.ctypes.data_as(ctypes.c_void_p)) == INVALID
    assert bool((summ == SENT32).all()) and (host_summary == SENT32).all()
    check(ctx, ex, first, "after the refused calls")
    # a singular world_from_optical on stream 1: the insert takes it, the carve names the stream
    ctx.set_voxel_transforms(1, SINGULAR)
    assert VF.inverse_transform(SINGULAR) is None
    assert "stream 1" in refused(INVALID, ctx.voxel_carve_batch_device, sc.n, d.data_ptr(), MARGIN, 0, summ.data_ptr())
    assert "stream 1" in refused(INVALID, ctx.voxel_carve_batch, sc.depth, MARGIN)
    assert bool((summ == SENT32).all())
    check(ctx, ex, None, "after the singular transform was refused")
    one = expect(streams=(0,))
    check(ctx, (ex[0] | one[0], one[1]), carve(ctx, sc.depth, n=1), "n = 1 beside a singular stream 1")
    flat = (None, SINGULAR, TRANSFORMS[2])
    occ = VC.expected_planes(list(sc.depth), list(filter_expected(sc, 0)[1]), [intrinsics(sc, i) for i in range(sc.n)], flat, FINE)
    ctx.voxel_insert_batch_device(sc.n, d.data_ptr())
    assert np.array_equal(ctx.voxel_grid()[0], occ[0]) and occ[0].any()
    ctx.set_voxel_transforms(1, TRANSFORMS[1])              # (the table is rebuilt: the stream can be carved from again)
    ctx.voxel_clear()
    check(ctx, ex, carve(ctx, sc.depth), "once stream 1 has an invertible transform again")
    ctx.close()
    # a stream without intrinsics
    ctx = cloud_context(sc, intr=False)
    give_grid(ctx, FINE, TRANSFORMS)
    refused(STATE, ctx.voxel_carve_batch_device, sc.n, d.data_ptr(), MARGIN, 0, summ.data_ptr())
    ctx.set_cloud_intrinsics(0, [intrinsics(sc, i) for i in range(2)])
    refused(STATE, ctx.voxel_carve_batch_device, sc.n, d.data_ptr(), MARGIN, 0, summ.data_ptr())
    assert bool((summ == SENT32).all()) and not ctx.voxel_free().any()
    ctx.set_cloud_intrinsics(2, [intrinsics(sc, 2)])
    check(ctx, ex, carve(ctx, sc.depth), "once every stream has intrinsics")
    ctx.close()


# ---- 12 .. 14: the host forms and the façades -------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_host_plane_forms(u16):
    sc = soup()
    ex = expect(u16=u16, r=1)
    ctx = context(sc, FINE)
    summ = ctx.voxel_carve_batch(sensor_planes(sc, u16), MARGIN, 1)
    check(ctx, ex, summ, "host planes%s" % (", 16UC1" if u16 else ""))
    ex2 = expect(u16=u16, r=1, streams=(0, 1))
    ctx.voxel_clear()
    check(ctx, ex2, ctx.voxel_carve_batch(sensor_planes(sc, u16)[:2], MARGIN, 1), "host planes, n = 2")
    ctx.close()


FACADE_GRID = VC.Grid((-1.0, -0.8, 0.3), 0.04, (50, 40, 60))
FACADE_TF = VC.rotation_z(0.2, (0.05, -0.1, 0.02))


def facade_expectation(depth, r):
    """From the sensor plane and INTR alone: the carve reads neither the mask nor the model."""
    ex = VF.expected([depth], [INTR], [FACADE_TF], FACADE_GRID, MARGIN, r)
    assert (ex[1][:, :3] > 1000).all(), ex[1]
    return ex


@gpu
def test_python_facade_carves_and_reads():
    depth = sensor_plane()
    f, tf = example_facade()
    P = f.getProjectionMatrix(info())
    f.setVoxelGrid(FACADE_GRID.origin, FACADE_GRID.voxel_size, FACADE_GRID.dims, world_from_optical=FACADE_TF)
    ex = facade_expectation(depth, 0)
    summ = f.voxelCarve(depth, P, 640, 480, MARGIN)
    assert summ.tolist() == ex[1][0].tolist() and np.array_equal(f.voxelFree(), ex[0])
    ex2 = facade_expectation(depth, 2)
    assert f.voxelCarve(depth, P, 640, 480, MARGIN, radius_px=2).tolist() == ex2[1][0].tolist()
    assert np.array_equal(f.voxelFree(), ex[0] | ex2[0])
    f.voxelClear()
    assert not f.voxelFree().any()
    mm = np.where((depth > 0) & (depth < 65.0), depth * np.float32(1000.0), 0).astype(np.uint16)
    ex_mm = facade_expectation(CC.u16_to_metres(mm), 0)
    assert f.voxelCarve(mm, P, 640, 480, MARGIN).tolist() == ex_mm[1][0].tolist() and np.array_equal(f.voxelFree(), ex_mm[0])
    # beside an insert: occupied and free stand together
    f.filter(depth, P, 640, 480)
    f.voxelInsert(depth, P, 640, 480)
    assert np.array_equal(f.voxelFree(), ex_mm[0]) and f.voxelGrid()[0].any()


CPP = r'''
#include <cstdio>
#include <fstream>
#include <iterator>
#include "realtime_urdf_filter_amd/urdf_filter.hpp"
using namespace realtime_urdf_filter;
int main(int argc, char** argv)
{
  std::ifstream fx(argv[1], std::ios::binary);
  const std::string xml((std::istreambuf_iterator<char>(fx)), std::istreambuf_iterator<char>());
  const int W = 640, H = 480;
  std::vector<float> depth((size_t)W * H);
  std::ifstream(argv[2], std::ios::binary).read(reinterpret_cast<char*>(depth.data()), (std::streamsize)depth.size() * 4);
  double cfg[4 + 3 + 1 + 16 + 1];              // intrinsics, origin, voxel size, world_from_optical, margin
  std::ifstream(argv[3], std::ios::binary).read(reinterpret_cast<char*>(cfg), sizeof cfg);
  const int dims[3] = {atoi(argv[5]), atoi(argv[6]), atoi(argv[7])};
  const size_t voxels = (size_t)dims[0] * dims[1] * dims[2], words = (voxels + 31) / 32;
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
  prm.models.push_back(mp);
  RealtimeURDFFilter f(prm, tf, {{"d", xml}});
  CameraInfo info;
  info.width = W; info.height = H;
  info.P[0] = cfg[0]; info.P[5] = cfg[1]; info.P[2] = cfg[2]; info.P[6] = cfg[3]; info.P[10] = 1;
  double P[16];
  f.getProjectionMatrix(info, P);
  std::vector<uint32_t> bits(words);
  if (f.getVoxelFree(bits.data())) return 1;              // nothing yet
  f.setVoxelGrid(cfg + 4, cfg[7], dims, true, cfg + 8);
  uint32_t summary[4] = {0, 0, 0, 0};
  if (!f.voxel_carve(depth.data(), false, P, W, H, cfg[24], 0, summary)) return 2;
  if (!f.getVoxelFree(bits.data())) return 3;
  FILE* o = fopen(argv[4], "wb");
  fwrite(summary, 4, 4, o);
  fwrite(bits.data(), 4, bits.size(), o);
  if (!f.voxel_carve(depth.data(), false, P, W, H, cfg[24], 2)) return 4;      // (no summary; ORed)
  if (!f.getVoxelFree(bits.data())) return 5;
  fwrite(bits.data(), 4, bits.size(), o);
  f.voxelClear();
  if (!f.getVoxelFree(bits.data())) return 6;
  fwrite(bits.data(), 4, bits.size(), o);
  fclose(o);
  return 0;
}
'''


@gpu
def test_cpp_facade_carves_and_reads(tmp_path):
    depth = sensor_plane()
    ex, ex2 = facade_expectation(depth, 0), facade_expectation(depth, 2)
    src = tmp_path / "voxel_free_facade.cpp"
    src.write_text(CPP)
    exe = tmp_path / "voxel_free_facade"
    lib = os.path.join(ROOT, "realtime_urdf_filter_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lrtuf",
                           "-Wl,-rpath," + lib, "-o", str(exe)])
    (tmp_path / "x.urdf").write_text(WL.EXAMPLE_URDF)
    depth.tofile(tmp_path / "d.f32")
    np.concatenate([np.asarray(INTR, np.float64), np.asarray(FACADE_GRID.origin), [FACADE_GRID.voxel_size], FACADE_TF, [MARGIN]]).tofile(tmp_path / "cfg.f64")
    r = subprocess.run([str(exe), str(tmp_path / "x.urdf"), str(tmp_path / "d.f32"), str(tmp_path / "cfg.f64"), str(tmp_path / "out.bin")] +
                       [str(q) for q in FACADE_GRID.dims], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.uint32)
    g = FACADE_GRID
    parts = np.split(raw, np.cumsum([4, g.n_words, g.n_words]))
    assert len(parts) == 4 and len(parts[3]) == g.n_words
    assert parts[0].tolist() == ex[1][0].tolist() and np.array_equal(parts[1], ex[0])
    assert np.array_equal(parts[2], ex[0] | ex2[0]) and not parts[3].any()
