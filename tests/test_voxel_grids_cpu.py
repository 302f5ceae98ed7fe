"""CPU (no GPU): voxel occupancy grids (include/rtuf.h, VOXEL OCCUPANCY GRIDS) -- the entry points' place in the ABI, the
expectation bench_support/voxel_check.py by hand on a few points, the kernel's own per-point arithmetic (rtuf_numerics.h:
voxel_of behind point_transform, compiled for the host by tests/voxel_check.cpp) against that expectation, index for index
and bit for bit, on voxel faces, the grid's outer faces, signed zeros, non-finite and huge coordinates, inexact reciprocals,
dims 1 and 2048 and random points, and the conditions on the GPU tests' inputs."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import realtime_urdf_filter_amd as R
from bench_support import points_check as PC
from bench_support import voxel_check as VC
from gpu_support import intrinsics, soup_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtuf.h")
CSRC = os.path.join(ROOT, "realtime_urdf_filter_amd", "csrc")
F = np.float32
CALLS = ("rtuf_set_voxel_grid", "rtuf_set_voxel_transforms", "rtuf_voxel_clear", "rtuf_voxel_insert_batch", "rtuf_voxel_insert_batch_u16",
         "rtuf_voxel_insert_batch_device", "rtuf_voxel_insert_batch_device_u16", "rtuf_voxel_insert_points_device", "rtuf_voxel_grid_device",
         "rtuf_get_voxel_grid")


def test_header_declares_the_calls_and_the_abi_version_is_still_6():
    text = open(HEADER).read()
    assert "VOXEL OCCUPANCY GRIDS" in text and "modulo 2^32" in text
    assert re.search(r"\bint rtuf_set_voxel_grid\(rtuf_context \*ctx, const double origin\[3\], double voxel_size, const int dims\[3\], int with_counts\);", text)
    assert re.search(r"\bint rtuf_voxel_insert_points_device\(rtuf_context \*ctx, int n_streams, const float \*d_points, const uint32_t \*d_counts, int capacity,\s*"
                     r"const uint8_t \*d_verdict, uint32_t \*d_summary\);", text)
    assert re.search(r"\bint rtuf_voxel_grid_device\(rtuf_context \*ctx, const uint32_t \*\*d_bits, const uint32_t \*\*d_counts, size_t \*n_voxels\);", text)
    lib = R.load_library()
    for name in CALLS:
        assert re.search(r"\bint %s\(rtuf_context \*ctx" % name, text), name
        assert name in R._capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define RTUF_ABI_VERSION 6\b", text) and R.ABI_VERSION == 6 and lib.rtuf_abi_version() == 6
    assert ctypes.sizeof(R._capi.Params) == 48 and ctypes.sizeof(R._capi.Stats) == 248
    for name in ("set_voxel_grid", "set_voxel_transforms", "voxel_clear", "voxel_insert_batch", "voxel_insert_batch_device", "voxel_insert_points_device",
                 "voxel_grid", "voxel_grid_device"):
        assert callable(getattr(R.Context, name)), name
    from realtime_urdf_filter_amd.filter import RealtimeURDFFilter
    assert callable(RealtimeURDFFilter.voxelInsert) and callable(RealtimeURDFFilter.setVoxelGrid)
    facade = open(os.path.join(ROOT, "include", "realtime_urdf_filter_amd", "urdf_filter.hpp")).read()
    assert re.search(r"\bbool voxel_insert\(", facade) and re.search(r"\bvoid setVoxelGrid\(", facade)


def test_struct_sizes_are_unchanged():
    src = ('#include "rtuf.h"\nstatic_assert(sizeof(rtuf_params) == 48, "params");\nstatic_assert(sizeof(rtuf_stats) == 248, "stats");\n'
           "static_assert(RTUF_ABI_VERSION == 6, \"abi\");\nint main() { return rtuf_voxel_clear(nullptr); }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_expectation_by_hand():
    """Origin 0, 0.5 m voxels (inv = 2 exactly), dims (2, 3, 4): every operation below is exact."""
    g = VC.Grid((0.0, 0.0, 0.0), 0.5, (2, 3, 4))
    assert g.n_voxels == 24 and g.n_words == 1
    tiny = np.nextafter(F(0), F(-1))
    pts = np.array([
        [0.75, 1.25, 1.75],          # g = (1.5, 2.5, 3.5): voxel (1, 2, 3) = (3 * 3 + 2) * 2 + 1 = 23
        [0.0, 0.0, 0.0],             # the low corner: voxel 0
        [-0.0, -0.0, -0.0],          # -0 >= 0: voxel 0
        [0.5, 0.0, 0.0],             # on the face between voxels 0 and 1 of x: the upper one
        [np.nextafter(F(0.5), F(0)), 0.0, 0.0],      # an ulp below the face: voxel 0
        [1.0, 0.0, 0.0],             # the high face of x is outside
        [np.nextafter(F(1.0), F(0)), 1.0, 1.5],      # an ulp inside it: (1, 2, 3)
        [0.0, 1.5, 0.0], [0.0, 0.0, 2.0],            # the high faces of y and z
        [tiny, 0.0, 0.0],            # the smallest negative number: outside
        [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [1e30, 0.0, 0.0],
    ], F)
    inside, index = VC.voxel_of(pts, g)
    assert index.tolist() == [23, 0, 0, 1, 0, -1, 23, -1, -1, -1, -1, -1, -1, -1]
    assert inside.tolist() == [i >= 0 for i in index.tolist()]
    bits, counts = VC.accumulate([index[inside]], g)
    assert bits.tolist() == [(1 << 23) | 3] and counts[0] == 3 and counts[1] == 1 and counts[23] == 2 and counts.sum() == 6
    bits2, counts2 = VC.accumulate([np.array([5])], g, bits, counts)           # continued: ORed and added
    assert bits2.tolist() == [(1 << 23) | 3 | 32] and counts2.sum() == 7
    assert VC.accumulate([np.array([1])], g, None, np.full(24, 0xFFFFFFFF, np.uint32))[1][1] == 0      # counts wrap
    # a plane by hand: 2 x 2 pixels, fx = fy = 1, cx = cy = 0: the point of pixel (u, v) with sensor s is (u s, v s, s)
    sensor = np.array([[0.25, 0.5], [np.nan, 3.0]], F)
    mask = np.array([[0, 0], [0, 0]], np.uint8)
    idx, summary = VC.plane_insert(sensor, mask, (1.0, 1.0, 0.0, 0.0), None, g)
    # (0, 0, .25) -> voxel 0; (.5, 0, .5) -> (1, 0, 1) = 7; NaN: not kept; (3, 3, 3): outside
    assert idx.tolist() == [0, 7] and summary.tolist() == [2, 1, 1, 4]
    mask[0, 1] = 255
    assert VC.plane_insert(sensor, mask, (1.0, 1.0, 0.0, 0.0), None, g)[1].tolist() == [1, 1, 2, 4]
    # ... through a shift by (0.5, 0, 0): (0, 0, .25) -> (.5, 0, .25) -> voxel 1
    M = np.eye(4)
    M[0, 3] = 0.5
    assert VC.plane_insert(sensor, mask, (1.0, 1.0, 0.0, 0.0), M.T.reshape(16), g)[0].tolist() == [1]
    # a list with verdicts: only verdict 0 is taken
    idx, summary = VC.list_insert(pts[:4], np.array([0, 1, 2, 0], np.uint8), None, None, g)
    assert idx.tolist() == [23, 1] and summary.tolist() == [2, 0, 2, 4]
    assert VC.Grid((0, 0, 0), 0.05, (1, 1, 1)).stored()[1] == F(1.0) / F(0.05)


# ---- the kernel's arithmetic on the host -------------------------------------------------------------------------------------

GRIDS = [VC.Grid((-1.5, -1.0, 0.5), 0.25, (12, 8, 16)),          # inv = 4: exact
         VC.Grid((-1.5, -1.0, 0.5), 0.05, (61, 40, 64)),         # the GPU tests' fine grid: 1 / 0.05f is inexact
         VC.Grid((0.0, 0.0, 0.0), 0.02, (2048, 1, 3)),           # dims 2048 and 1
         VC.Grid((0.1, -0.3, 0.7), 0.3, (1, 2048, 2)),
         VC.Grid((-100.0, -100.0, -100.0), 1.0 / 3.0, (600, 600, 300))]
SPECIALS = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 1e-42, -1e-42], F)


def _steps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(F(x), F(np.inf) if k > 0 else F(-np.inf))
    return F(x)


def _sweep():
    """Rows (grid number, matrix or None, point): per grid the voxel faces of every axis (every face of the small grids, a
    spread of the long axes' and always the outer two) three floats either side; every special value in every coordinate;
    signed zeros against a zero origin; 3,000 random points; and all of it again through a transform."""
    rng = np.random.default_rng(23)
    rows = []
    for gi, g in enumerate(GRIDS):
        o, inv = g.stored()
        size = F(g.voxel_size)
        mid = [F(o[r] + F(0.5) * size) for r in range(3)]
        pts = []
        for r in range(3):
            faces = sorted(set(range(0, g.dims[r] + 1)) if g.dims[r] <= 64 else {0, 1, 2, 7, 100, 1023, 1024, g.dims[r] - 1, g.dims[r]})
            for k in faces:
                with np.errstate(all="ignore"):
                    face = F(o[r] + F(F(k) * size))
                for step in range(-3, 4):
                    p = list(mid)
                    p[r] = _steps(face, step)
                    pts.append(p)
            for sp in SPECIALS:
                p = list(mid)
                p[r] = sp
                pts.append(p)
        pts.append([-0.0, -0.0, -0.0])
        pts.append([0.0, -0.0, 0.0])
        lo, hi = o - F(2) * size, o + (np.array(g.dims, F) + F(2)) * size
        pts += rng.uniform(lo, hi, (3000, 3)).astype(F).tolist()
        for matrix in (None, PC.rigid_transform(rng), VC.rotation_z(0.6, (0.3, -0.2, 0.1))):
            rows += [(gi, matrix, np.array(p, F)) for p in pts]
    return rows


def _expected(rows):
    inside, index, world = np.zeros(len(rows), bool), np.zeros(len(rows), np.int64), np.zeros((len(rows), 3), F)
    keys = [(r[0], None if r[1] is None else r[1].tobytes()) for r in rows]
    for key in set(keys):
        at = np.array([i for i, k in enumerate(keys) if k == key])
        world[at] = PC.transformed(np.stack([rows[i][2] for i in at]), rows[at[0]][1])
        inside[at], index[at] = VC.voxel_of(world[at], GRIDS[key[0]])
    return inside, index, world


@pytest.fixture(scope="module")
def sweep():
    rows = _sweep()
    return rows, _expected(rows)


def test_the_kernels_voxel_of_agrees_with_numpy_index_for_index(tmp_path, sweep):
    rows, (inside, index, world) = sweep
    exe = str(tmp_path / "voxel_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "voxel_check.cpp")])
    bits = lambda f: int(np.array(f, F).view(np.uint32))
    ident = np.eye(4).T.reshape(16)
    lines = []
    for gi, matrix, p in rows:
        g = GRIDS[gi]
        o, inv = g.stored()
        m = (ident if matrix is None else matrix).astype(F).reshape(4, 4)[:, :3].reshape(12)      # (column-major: column c, rows 0 .. 2)
        lines.append("%d %d %d %d " % ((0 if matrix is None else 1,) + g.dims) + " ".join("%x" % bits(f) for f in list(p) + list(o) + [inv] + list(m)))
    r = subprocess.run([exe], input="%d\n" % len(rows) + "\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:], r.stdout[-300:])
    got = [line.split() for line in r.stdout.splitlines()]
    assert len(got) == len(rows)
    g_inside = np.array([int(g[0]) for g in got], bool)
    g_index = np.array([int(g[1]) for g in got], np.int64)
    g_world = np.array([[int(w, 16) for w in g[2:5]] for g in got], np.uint32)
    assert np.array_equal(g_inside, inside), np.argwhere(g_inside != inside)[:5]
    assert np.array_equal(g_index, index), np.argwhere(g_index != index)[:5]
    same = (g_world == world.view(np.uint32)) | (np.isnan(g_world.view(F)) & np.isnan(world))
    assert same.all(), np.argwhere(~same)[:5]
    # (a vacuous pass must not hide: both answers occur often in every grid, with and without a transform, the first and the
    # last voxel of every axis are hit, and the largest index of the 2048-wide grids occurs)
    gis = np.array([r[0] for r in rows])
    moved = np.array([r[1] is not None for r in rows])
    for gi, g in enumerate(GRIDS):
        at = (gis == gi) & ~moved
        assert (inside & at).sum() > 100 and (~inside & at).sum() > 100, gi
        assert (~inside & (gis == gi) & moved).sum() > 100, gi        # (a grid one voxel thick keeps few points once they are rotated:
    assert (inside & moved).sum() > 2000                               # the moved points are counted over all grids)
    for gi, g in enumerate(GRIDS):
        nx, ny, nz = g.dims
        i = index[(gis == gi) & inside & ~moved]
        ix, iy, iz = i % nx, (i // nx) % ny, i // (nx * ny)
        assert ix.min() == 0 and ix.max() == nx - 1 and iy.min() == 0 and iy.max() == ny - 1 and iz.min() == 0 and iz.max() == nz - 1, gi
    assert index.max() < max(g.n_voxels for g in GRIDS) and all(g.n_voxels <= VC.MAX_VOXELS for g in GRIDS)


def test_voxel_of_does_not_exist_without_the_feature():
    """(What makes this module fail on the code before the feature: the shared header has the function and the grid struct.)"""
    text = open(os.path.join(CSRC, "rtuf_numerics.h")).read()
    assert re.search(r"RTUF_NUMERIC_HD bool voxel_of\(float x, float y, float z, const VoxelGrid& g, uint32_t& index\)", text)
    kernels = open(os.path.join(CSRC, "rtuf_kernels.hip")).read()
    for name in ("voxel_clear_kernel", "voxel_insert_kernel", "voxel_insert_points_kernel"):
        assert re.search(r"void %s\(" % name, kernels), name
    assert kernels.count("voxel_of(") >= 2 and kernels.count("point_transform(") >= 4      # (both insert kernels share the header's chain)


# ---- conditions on the GPU tests' inputs -------------------------------------------------------------------------------------

FINE = VC.Grid((-1.5, -1.0, 0.5), 0.05, (61, 40, 64))
COARSE = VC.Grid((-1.5, -1.0, 0.5), 0.5, (5, 4, 6))
TRANSFORMS = [None, VC.rotation_z(0.3, (0.1, 0.0, 0.0)), VC.rotation_z(0.6, (0.0, 0.1, 0.0))]


def test_the_scene_fills_both_grids_with_the_sensor_alone():
    """soup_scene(11, 160, 120) with an empty mask: per stream 13.3 k to 13.9 k inserted, 4.7 k to 5.2 k outside and about
    0.6 k without a point in the fine grid; the coarse grid's largest count is 721 to 917 per stream."""
    sc = soup_scene(11, 160, 120)
    empty = np.zeros((sc.H, sc.W), np.uint8)
    for s in range(sc.n):
        idx, summary = VC.plane_insert(sc.depth[s], empty, intrinsics(sc, s), TRANSFORMS[s], FINE)
        # (the figures are rounded to 0.1 k)
        assert 13250 <= summary[0] < 13950 and 4650 <= summary[1] < 5250 and 550 <= summary[2] < 750 and summary[3] == 160 * 120, summary
        idx, _ = VC.plane_insert(sc.depth[s], empty, intrinsics(sc, s), TRANSFORMS[s], COARSE)
        assert 721 <= np.bincount(idx).max() <= 917, np.bincount(idx).max()
