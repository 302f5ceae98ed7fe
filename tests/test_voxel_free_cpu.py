"""CPU (no GPU): voxel free space (include/rtuf.h, VOXEL FREE SPACE) -- the entry points' place in the ABI, the expectation
bench_support/voxel_free_check.py by hand on an exact case, the kernel's own per-voxel arithmetic (rtuf_numerics.h:
voxel_centre, voxel_inverse_transform, point_transform, point_pixel, voxel_free_test, compiled for the host by
tests/voxel_free_check.cpp) against that expectation bit for bit, and the conditions on the GPU tests' inputs."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import realtime_urdf_filter_amd as R
from bench_support import points_check as PC
from bench_support import voxel_check as VC
from bench_support import voxel_free_check as VF
from gpu_support import intrinsics, soup_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtuf.h")
CSRC = os.path.join(ROOT, "realtime_urdf_filter_amd", "csrc")
F = np.float32
CALLS = ("rtuf_voxel_carve_batch_device", "rtuf_voxel_carve_batch_device_u16", "rtuf_voxel_carve_batch", "rtuf_voxel_carve_batch_u16",
         "rtuf_voxel_free_device", "rtuf_get_voxel_free")


def test_header_declares_the_calls_and_the_abi_version_is_still_6():
    text = open(HEADER).read()
    assert "VOXEL FREE SPACE" in text and text.index("VOXEL FREE SPACE") > text.index("VOXEL OCCUPANCY GRIDS")
    assert "free-space carving along the rays" not in text and "occupied wins" in text
    assert re.search(r"\bint rtuf_voxel_carve_batch_device\(rtuf_context \*ctx, int n_streams, const float \*d_depth, double margin, int radius_px, "
                     r"uint32_t \*d_summary\);", text)
    assert re.search(r"\bint rtuf_voxel_carve_batch_u16\(rtuf_context \*ctx, int n_streams, const uint16_t \*const \*depth_mm_in, double margin, int radius_px, "
                     r"uint32_t \*summary_out\);", text)
    assert re.search(r"\bint rtuf_voxel_free_device\(rtuf_context \*ctx, const uint32_t \*\*d_free_bits, size_t \*n_voxels\);", text)
    assert re.search(r"\bint rtuf_get_voxel_free\(rtuf_context \*ctx, uint32_t \*free_out\);", text)
    lib = R.load_library()
    for name in CALLS:
        assert re.search(r"\bint %s\(rtuf_context \*ctx" % name, text), name
        assert name in R._capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define RTUF_ABI_VERSION 6\b", text) and R.ABI_VERSION == 6 and lib.rtuf_abi_version() == 6
    assert ctypes.sizeof(R._capi.Params) == 48 and ctypes.sizeof(R._capi.Stats) == 248
    for name in ("voxel_carve_batch_device", "voxel_carve_batch", "voxel_free", "voxel_free_device"):
        assert callable(getattr(R.Context, name)), name
    from realtime_urdf_filter_amd.filter import RealtimeURDFFilter
    assert callable(RealtimeURDFFilter.voxelCarve) and callable(RealtimeURDFFilter.voxelFree)
    facade = open(os.path.join(ROOT, "include", "realtime_urdf_filter_amd", "urdf_filter.hpp")).read()
    assert re.search(r"\bbool voxel_carve\(", facade) and re.search(r"\bbool getVoxelFree\(", facade)


def test_struct_sizes_are_unchanged():
    src = ('#include "rtuf.h"\nstatic_assert(sizeof(rtuf_params) == 48, "params");\nstatic_assert(sizeof(rtuf_stats) == 248, "stats");\n'
           "static_assert(RTUF_ABI_VERSION == 6, \"abi\");\nint main() { return rtuf_get_voxel_free(nullptr, nullptr); }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_the_kernel_and_the_shared_functions_exist():
    text = open(os.path.join(CSRC, "rtuf_numerics.h")).read()
    for sig in (r"RTUF_NUMERIC_HD float voxel_centre\(int i, float o, float size\)", r"RTUF_NUMERIC_HD bool voxel_free_test\(float z, float emin, float m\)",
                r"inline bool voxel_inverse_transform\(const float\* m, float\* out\)"):
        assert re.search(sig, text), sig
    kernels = open(os.path.join(CSRC, "rtuf_kernels.hip")).read()
    assert re.search(r"void voxel_carve_kernel\(VoxelCarveArgs a\)", kernels)
    body = kernels[kernels.index("void voxel_carve_kernel("):kernels.index("void launch_voxel_carve(")]
    for name in ("voxel_centre(", "point_transform(", "point_pixel(", "voxel_free_test(", "cloud_sensor_valid("):
        assert name in body, name
    assert "atomicOr" not in body and "fetch_or" not in body      # (one owner per output word)


# ---- the expectation by hand ---------------------------------------------------------------------------------------------------

HAND = VC.Grid((0.0, 0.0, 0.0), 0.5, (2, 2, 4))
UNIT = (1.0, 1.0, 0.0, 0.0)      # fx = fy = 1, cx = cy = 0: the centre (x, y, z) lands on pixel ((int)(x / z + 0.5), (int)(y / z + 0.5))


def test_expectation_by_hand():
    """Origin 0, 0.5 m voxels, dims (2, 2, 4), a 2 x 2 plane: centres at 0.25 and 0.75 in x and y and 0.25 .. 1.75 in z, every
    one of them exact.  The pixel of a centre is (int)(x / z + 0.5): voxel (0, 0, iz) lands on pixel (1, 1) for iz = 0
    (0.25 / 0.25 + 0.5 = 1.5) and on (0, 0) for iz = 1 .. 3 (1 / 3 + 0.5, 0.7, 0.25 / 1.75 + 0.5 < 1)."""
    c = VF.centres(HAND)
    assert c.shape == (16, 3) and c[0].tolist() == [0.25, 0.25, 0.25] and c[1].tolist() == [0.75, 0.25, 0.25] and c[15].tolist() == [0.75, 0.75, 1.75]
    assert c[2].tolist() == [0.25, 0.75, 0.25] and c[4].tolist() == [0.25, 0.25, 0.75]
    column = [0, 4, 8, 12]                                  # voxels (0, 0, iz): z = 0.25, 0.75, 1.25, 1.75
    state = lambda plane, m, r=0: VF.stream_state(np.array(plane, F), UNIT, None, HAND, m, r)
    # pixel (0, 0) reads 1.25: z = 0.75 is free, z = 1.25 lies exactly AT Emin - m (m = 0): not free, z = 1.75 is behind
    st = state([[1.25, 9.0], [9.0, 9.0]], 0.0)
    assert st[column].tolist() == [VF.FREE, VF.FREE, VF.NOT_FREE, VF.NOT_FREE]
    # ... one ulp above 1.25 frees z = 1.25
    st = state([[np.nextafter(F(1.25), F(2)), 9.0], [9.0, 9.0]], 0.0)
    assert st[column].tolist() == [VF.FREE, VF.FREE, VF.FREE, VF.NOT_FREE]
    # with a margin of 0.5: Emin - m = 1.75 - 0.5 = 1.25 exactly: z = 1.25 is not free, z = 0.75 is; an ulp more frees 1.25
    assert state([[1.75, 9.0], [9.0, 9.0]], 0.5)[column].tolist() == [VF.FREE, VF.FREE, VF.NOT_FREE, VF.NOT_FREE]
    assert state([[np.nextafter(F(1.75), F(2)), 9.0], [9.0, 9.0]], 0.5)[column].tolist() == [VF.FREE, VF.FREE, VF.FREE, VF.NOT_FREE]
    # NaN, 0 and +inf at the centre pixel: judged, not free -- whatever the neighbours read
    for bad in (np.nan, 0.0, np.inf, -1.0):
        for r in (0, 1):
            st = state([[bad, 9.0], [9.0, 9.0]], 0.0, r)
            assert st[[4, 8, 12]].tolist() == [VF.NOT_FREE] * 3 and st[0] == VF.FREE, (bad, r)
    # an invalid neighbour is skipped at r = 1, a valid nearer one counts: the window of (0, 0) is the whole 2 x 2 plane
    assert state([[9.0, np.nan], [0.0, np.inf]], 0.0, 1)[column].tolist() == [VF.NOT_FREE, VF.FREE, VF.FREE, VF.FREE]      # (pixel (1, 1) reads inf)
    assert state([[9.0, 1.0], [9.0, 9.0]], 0.0, 1)[column].tolist() == [VF.FREE, VF.FREE, VF.NOT_FREE, VF.NOT_FREE]
    assert state([[9.0, 1.0], [9.0, 9.0]], 0.0, 0)[column].tolist() == [VF.FREE] * 4
    # a centre at z = 0 and one behind the camera are not seen: the grid shifted down by 0.25 and by 1 in z
    at0 = VC.Grid((0.0, 0.0, -0.25), 0.5, (2, 2, 4))
    assert VF.centres(at0)[0, 2] == 0.0 and VF.centres(at0)[4, 2] == 0.5
    st = VF.stream_state(np.full((2, 2), 9.0, F), UNIT, None, at0, 0.0, 0)
    assert st[0] == VF.NOT_SEEN and st[4] == VF.FREE
    behind = VC.Grid((0.0, 0.0, -1.0), 0.5, (2, 2, 4))
    st = VF.stream_state(np.full((2, 2), 9.0, F), UNIT, None, behind, 0.0, 0)
    assert st[[0, 4]].tolist() == [VF.NOT_SEEN] * 2 and st[8] == VF.FREE
    # outside the image: voxel (1, 1, 0) has x / z = 3 -> pixel 3: not seen
    assert state([[9.0, 9.0], [9.0, 9.0]], 0.0)[3] == VF.NOT_SEEN
    # bits and summary
    bits, summary = VF.expected([np.array([[1.25, 9.0], [9.0, 9.0]], F)] * 2, [UNIT] * 2, [None, None], HAND, 0.0, 0)
    st = state([[1.25, 9.0], [9.0, 9.0]], 0.0)
    assert bits.tolist() == [sum(1 << i for i in range(16) if st[i] == VF.FREE)] and summary[0].tolist() == summary[1].tolist()
    assert summary[0].tolist() == [(st == VF.FREE).sum(), (st == VF.NOT_FREE).sum(), (st == VF.NOT_SEEN).sum(), 16] and summary[0, :3].sum() == 16
    assert np.array_equal(VF.unpack(bits, HAND), st == VF.FREE)
    # the inverse of a shift and of a quarter turn, by hand
    M = np.eye(4)
    M[:3, 3] = (0.5, -1.0, 2.0)
    assert VF.inverse_transform(M.T.reshape(16)).tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -0.5, 1.0, -2.0, 0]
    Q = np.array([[0.0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]])      # x' = -y + 1, y' = x + 2: x = y' - 2, y = -(x' - 1)
    assert VF.inverse_transform(Q.T.reshape(16)).tolist() == [0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, -2, 1, -3, 0]
    assert VF.inverse_transform(np.zeros(16)) is None and VF.inverse_transform(np.diag([1.0, 1.0, 0.0, 1.0]).reshape(16)) is None
    assert VF.inverse_transform(np.diag([1e-30, 1e-30, 1e-30, 1.0]).reshape(16))[0] == F(1e30)     # (det = 1e-90 is a fine double)
    assert VF.inverse_transform(np.diag([1e-39, 1.0, 1.0, 1.0]).reshape(16)) is None               # (1e39 is not finite as a float)


# ---- the kernel's arithmetic on the host -----------------------------------------------------------------------------------------

FINE = VC.Grid((-1.5, -1.0, 0.5), 0.05, (61, 40, 64))
ODD = VC.Grid((-1.5, -1.0, -0.4), 0.05, (61, 41, 63))
COARSE = VC.Grid((-1.5, -1.0, 0.5), 0.5, (5, 4, 6))
TRANSFORMS = (None, VC.rotation_z(0.3, (0.1, 0.0, 0.0)), VC.rotation_z(0.6, (0.0, 0.1, 0.0)))
MARGIN = 0.05
SWEEP_GRIDS = [VC.Grid((-0.4, -0.3, 0.2), 0.1, (8, 6, 10)),                # every voxel
               VC.Grid((-20.0, 0.0, 0.5), 0.02, (2048, 1, 3)),             # the first and last voxel of 2048-long axes
               VC.Grid((0.1, -30.0, 0.7), 0.03, (1, 2048, 2)),
               VC.Grid((-0.5, -0.5, -40.0), 0.05, (3, 2, 2048)),
               VC.Grid((-1.0, -1.0, 0.1), 1.0 / 3.0, (6, 6, 9)),
               VC.Grid((-0.3, -0.2, 0.4), 0.05, (12, 8, 20))]
SHEAR = np.array([[1.0, 0.2, 0.0, 0.1], [0.0, 1.1, 0.3, -0.2], [0.1, 0.0, 0.9, 0.05], [0, 0, 0, 1]]).T.reshape(16)
SINGULAR = np.array([[1.0, 2.0, 3.0, 0.1], [2.0, 4.0, 6.0, 0.2], [0.5, 0.1, 0.7, 0.3], [0, 0, 0, 1]]).T.reshape(16)
SWEEP_INTR = (131.25, 130.0, 79.5, 59.5)
SWEEP_W, SWEEP_H = 160, 120


def _steps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(F(x), F(np.inf) if k > 0 else F(-np.inf))
    return F(x)


def _emin_for(target, m):
    """A float e with (float)(e - m) == target, or None."""
    e = F(F(target) + F(m))
    for k in (0, -1, 1, -2, 2, -3, 3):
        q = _steps(e, k)
        if F(q - F(m)) == F(target):
            return q
    return None


def _sweep():
    """Rows (grid number, matrix name, (ix, iy, iz), Emin, margin): per grid and transform every voxel (small grids) or the
    ends and a spread of the long axis, each voxel against Emin values that put Emin - m exactly at the centre's optical z and
    three floats either side (margins 0 and 0.05), and against 1 m and 3 m."""
    rng = np.random.default_rng(31)
    matrices = {"none": None, "rz03": TRANSFORMS[1], "rz06": TRANSFORMS[2], "rigid": PC.rigid_transform(rng), "shear": SHEAR, "singular": SINGULAR}
    rows = []
    for gi, g in enumerate(SWEEP_GRIDS):
        nx, ny, nz = g.dims
        if g.n_voxels <= 2000:
            vox = [(x, y, z) for z in range(nz) for y in range(ny) for x in range(nx)]
        else:
            long_axis = int(np.argmax(g.dims))
            vox = []
            for k in sorted({0, 1, 2, 7, 100, 1900, 2046, 2047} | set(range(940, 1100))):      # (the ends, and the stretch the camera sees)
                for a in range(g.dims[(long_axis + 1) % 3]):
                    for b in range(g.dims[(long_axis + 2) % 3]):
                        i = [0, 0, 0]
                        i[long_axis], i[(long_axis + 1) % 3], i[(long_axis + 2) % 3] = k, a, b
                        vox.append(tuple(i))
        c = VF.centres(g)
        index = np.array([(z * ny + y) * nx + x for x, y, z in vox])
        for name, matrix in matrices.items():
            inv = None if matrix is None else VF.inverse_transform(matrix)
            if matrix is not None and inv is None:
                rows += [(gi, name, v, F(1.0), F(0.0)) for v in vox[:20]]
                continue
            opt = PC.transformed(c[index], None if inv is None else inv.astype(np.float64))
            for j, v in enumerate(vox):
                z = opt[j, 2]
                rows.append((gi, name, v, F(1.0), F(MARGIN)))
                rows.append((gi, name, v, F(3.0), F(0.0)))
                if j % 4 == 0 and np.isfinite(z) and z > 0:
                    for m in (0.0, MARGIN):
                        for step in range(-3, 4):
                            e = _emin_for(_steps(z, step), m)
                            if e is not None:
                                rows.append((gi, name, v, e, F(m)))
    return rows, matrices


def _expected(rows, matrices):
    n = len(rows)
    out = dict(ok=np.ones(n, bool), judged=np.zeros(n, bool), u=np.zeros(n, np.int64), v=np.zeros(n, np.int64), free=np.zeros(n, bool),
               centre=np.zeros((n, 3), F), optical=np.zeros((n, 3), F), inverse=np.zeros((n, 16), F))
    keys = [(r[0], r[1]) for r in rows]
    for key in sorted(set(keys)):
        at = np.array([i for i, k in enumerate(keys) if k == key])
        g, matrix = SWEEP_GRIDS[key[0]], matrices[key[1]]
        nx, ny, nz = g.dims
        c = VF.centres(g)[[(rows[i][2][2] * ny + rows[i][2][1]) * nx + rows[i][2][0] for i in at]]
        out["centre"][at] = c
        inv = None if matrix is None else VF.inverse_transform(matrix)
        if matrix is not None and inv is None:
            out["ok"][at] = False
            out["optical"][at] = c
            continue
        if inv is not None:
            out["inverse"][at] = inv
        opt = PC.transformed(c, None if inv is None else inv.astype(np.float64))
        out["optical"][at] = opt
        judged, u, v = PC.pixel_of(opt, SWEEP_INTR, SWEEP_W, SWEEP_H)
        emin, m = np.array([rows[i][3] for i in at], F), np.array([rows[i][4] for i in at], F)
        with np.errstate(all="ignore"):
            free = judged & (opt[:, 2] < (emin - m).astype(F))
        out["judged"][at], out["u"][at], out["v"][at], out["free"][at] = judged, u, v, free
    return out


@pytest.fixture(scope="module")
def sweep():
    rows, matrices = _sweep()
    return rows, matrices, _expected(rows, matrices)


def test_the_kernels_arithmetic_agrees_with_numpy_bit_for_bit(tmp_path, sweep):
    rows, matrices, ex = sweep
    exe = str(tmp_path / "voxel_free_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "voxel_free_check.cpp")])
    bits = lambda f: int(np.array(f, F).view(np.uint32))
    ident = np.eye(4).T.reshape(16)
    fixed = " ".join("%x" % bits(f) for f in PC.stored_intrinsics(*SWEEP_INTR))
    heads = {}
    for gi, g in enumerate(SWEEP_GRIDS):
        o = np.array(g.origin, np.float64).astype(F)
        for name, matrix in matrices.items():
            m = (ident if matrix is None else matrix).astype(F).reshape(4, 4)[:, :3].reshape(12)      # (column-major: column c, rows 0 .. 2)
            heads[gi, name] = (0 if matrix is None else 1, " ".join("%x" % bits(f) for f in list(o) + [F(g.voxel_size)] + list(m)) + " " + fixed)
    lines = ["%d %d %d %d %d %d %s %x %x" % ((heads[gi, name][0],) + v + (SWEEP_W, SWEEP_H, heads[gi, name][1], bits(e), bits(m))) for gi, name, v, e, m in rows]
    r = subprocess.run([exe], input="%d\n" % len(rows) + "\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:], r.stdout[-300:])
    got = [line.split() for line in r.stdout.splitlines()]
    assert len(got) == len(rows)
    flags = np.array([[int(q) for q in g[:5]] for g in got], np.int64)
    words = np.array([[int(w, 16) for w in g[5:]] for g in got], np.uint32)
    assert np.array_equal(flags[:, 0].astype(bool), ex["ok"]), np.argwhere(flags[:, 0].astype(bool) != ex["ok"])[:5]
    assert np.array_equal(words[:, :3], ex["centre"].view(np.uint32)), np.argwhere(words[:, :3] != ex["centre"].view(np.uint32))[:5]
    inv12 = ex["inverse"].reshape(-1, 4, 4)[:, :, :3].reshape(-1, 12)
    assert np.array_equal(words[:, 6:18], np.ascontiguousarray(inv12).view(np.uint32)), np.argwhere(words[:, 6:18] != np.ascontiguousarray(inv12).view(np.uint32))[:5]
    assert np.array_equal(words[:, 3:6], ex["optical"].view(np.uint32)), np.argwhere(words[:, 3:6] != ex["optical"].view(np.uint32))[:5]
    assert np.array_equal(flags[:, 1].astype(bool), ex["judged"]), np.argwhere(flags[:, 1].astype(bool) != ex["judged"])[:5]
    assert np.array_equal(flags[:, 2], ex["u"]) and np.array_equal(flags[:, 3], ex["v"])
    assert np.array_equal(flags[:, 4].astype(bool), ex["free"]), np.argwhere(flags[:, 4].astype(bool) != ex["free"])[:5]
    # (a vacuous pass must not hide: both answers occur often in every group, the singular matrix is refused and only it)
    gis, names = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    assert not ex["ok"][names == "singular"].any() and ex["ok"][names != "singular"].all() and (names == "singular").sum() >= 100
    for name in matrices:
        if name != "singular":
            at = names == name
            assert (ex["free"] & at).sum() > 100 and (ex["judged"] & ~ex["free"] & at).sum() > 100 and (~ex["judged"] & at).sum() > 100, name
    for gi in range(len(SWEEP_GRIDS)):
        at = (gis == gi) & ex["ok"]
        assert (ex["free"] & at).sum() > 100 and (ex["judged"] & ~ex["free"] & at).sum() > 100, gi
    assert (~ex["judged"] & ex["ok"]).sum() > 1000
    # ... the ties: rows whose Emin - m is the optical z itself are never free, their float neighbour above is
    with np.errstate(all="ignore"):
        thr = (np.array([r[3] for r in rows], F) - np.array([r[4] for r in rows], F)).astype(F)
    tie = ex["judged"] & (thr == ex["optical"][:, 2])
    above = ex["judged"] & (thr == np.nextafter(ex["optical"][:, 2], F(np.inf)))
    assert tie.sum() > 500 and not ex["free"][tie].any() and above.sum() > 500 and ex["free"][above].all()
    # ... and the ends of the 2048-long axes were there
    for gi in (1, 2, 3):
        axis = int(np.argmax(SWEEP_GRIDS[gi].dims))
        ks = {r[2][axis] for r in rows if r[0] == gi}
        assert 0 in ks and 2047 in ks


# ---- conditions on the GPU tests' inputs -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    return soup_scene(11, 160, 120)


def _states(sc, grid, margin=MARGIN, r=0):
    return [VF.stream_state(sc.depth[s], intrinsics(sc, s), TRANSFORMS[s], grid, margin, r) for s in range(sc.n)]


def test_the_scene_frees_blocks_and_misses_voxels_of_every_grid(scene):
    """soup_scene(11, 160, 120), margin 0.05 m.  FINE: per stream 42 k to 63 k free, 40 k to 55 k not free, 53 k to 59 k not
    seen; 6,368 voxels are occupied under an empty mask and free."""
    sc = scene
    st = _states(sc, FINE)
    for s in range(sc.n):
        n_free, n_not, n_unseen = (st[s] == VF.FREE).sum(), (st[s] == VF.NOT_FREE).sum(), (st[s] == VF.NOT_SEEN).sum()
        assert n_free > 30000 and n_not > 30000 and n_unseen > 50000, (s, n_free, n_not, n_unseen)
    seen_free_by = sum((q == VF.FREE).astype(int) for q in st)
    assert all((seen_free_by == k).sum() > 10000 for k in range(4)), np.bincount(seen_free_by)
    empty = [np.zeros((sc.H, sc.W), np.uint8)] * sc.n
    occupied = VF.unpack(VC.expected_planes(list(sc.depth), empty, [intrinsics(sc, s) for s in range(sc.n)], TRANSFORMS, FINE)[0], FINE)
    assert (occupied & (seen_free_by > 0)).sum() > 1000
    # ODD: neither a multiple of 64 nor of 32; part of it lies behind the cameras
    assert ODD.n_voxels == 157563 and ODD.n_voxels % 32 == 27 and ODD.n_voxels % 64 != 0
    st = _states(sc, ODD)
    behind = VF.centres(ODD)[:, 2] <= 0
    assert behind.sum() > 15000
    for s in range(sc.n):
        assert (st[s] == VF.NOT_SEEN).sum() > 90000 and (st[s] == VF.FREE).sum() > 30000 and (st[s][behind] == VF.NOT_SEEN).all(), s
    # COARSE: under two waves
    assert COARSE.n_voxels == 120
    for q in _states(sc, COARSE):
        assert (q == VF.FREE).sum() >= 30 and (q == VF.NOT_FREE).sum() >= 15


@pytest.mark.parametrize("margin", [0.0, MARGIN])
def test_a_radius_changes_the_free_set(scene, margin):
    sc = scene
    base = VF.expected(list(sc.depth), [intrinsics(sc, s) for s in range(sc.n)], TRANSFORMS, FINE, margin, 0)[0]
    one = VF.expected(list(sc.depth), [intrinsics(sc, s) for s in range(sc.n)], TRANSFORMS, FINE, margin, 1)[0]
    four = VF.expected(list(sc.depth), [intrinsics(sc, s) for s in range(sc.n)], TRANSFORMS, FINE, margin, 4)[0]
    assert not np.array_equal(base, one) and not np.array_equal(one, four)
    assert not (one & ~base).any() and not (four & ~one).any()      # (a wider window only takes free voxels away)


def test_every_centre_lies_in_its_own_voxel():
    for g in (FINE, ODD, COARSE, HAND):
        inside, index = VC.voxel_of(VF.centres(g), g)
        assert inside.all() and np.array_equal(index, np.arange(g.n_voxels))
