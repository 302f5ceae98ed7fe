"""CPU (no GPU): point list batches (include/rtuf.h, POINT LIST BATCHES) -- the entry points' place in the ABI, the
expectation bench_support/points_check.py by hand on ten points, the kernel's own per-point arithmetic (rtuf_numerics.h,
compiled for the host by tests/point_pixel_check.cpp, plain and under the sanitizers) against that expectation, bit for bit,
on a sweep of edge values, the new kind's kernel routes (the Points rows of tests/routes_check.cpp), and the conditions on the GPU tests'
inputs: the scenes give enough filtered points, and enough kept points on link pixels, in every stream."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import realtime_urdf_filter_amd as R
from bench_support import points_check as PC
from gpu_support import filter_expected, intrinsics, soup_scene, virtual_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtuf.h")
CSRC = os.path.join(ROOT, "realtime_urdf_filter_amd", "csrc")
F = np.float32
CALLS = ("rtuf_set_point_transforms", "rtuf_points_batch_device", "rtuf_points_batch")


def test_header_declares_the_calls_and_the_abi_version_is_still_6():
    text = open(HEADER).read()
    assert "POINT LIST BATCHES" in text
    assert re.search(r"\bint rtuf_set_point_transforms\(rtuf_context \*ctx, int first_stream, int n_streams, const double \*optical_from_points", text)
    assert re.search(r"\bint rtuf_points_batch_device\(rtuf_context \*ctx, int n_streams, const float \*d_points, const uint32_t \*d_counts, int capacity,\s*"
                     r"int radius_px, uint8_t \*d_verdict, uint32_t \*d_pixel, uint32_t \*d_summary\);", text)
    assert re.search(r"\bint rtuf_points_batch\(rtuf_context \*ctx, int n_streams, const float \*const \*points_in, const uint32_t \*counts", text)
    lib = R.load_library()
    for name in CALLS:
        assert name in R._capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define RTUF_ABI_VERSION 6\b", text) and R.ABI_VERSION == 6 and lib.rtuf_abi_version() == 6
    assert ctypes.sizeof(R._capi.Params) == 48 and ctypes.sizeof(R._capi.Stats) == 248
    for name in ("set_point_transforms", "points_batch", "points_batch_device"):
        assert callable(getattr(R.Context, name)), name
    from realtime_urdf_filter_amd.filter import RealtimeURDFFilter
    assert callable(RealtimeURDFFilter.filter_points)
    facade = open(os.path.join(ROOT, "include", "realtime_urdf_filter_amd", "urdf_filter.hpp")).read()
    assert re.search(r"\bbool points_into\(", facade)


def test_struct_sizes_are_unchanged():
    src = ('#include "rtuf.h"\nstatic_assert(sizeof(rtuf_params) == 48, "params");\nstatic_assert(sizeof(rtuf_stats) == 248, "stats");\n'
           "int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_expectation_by_hand_on_ten_points():
    """A 4 x 3 plane, fx = 2, fy = 4, cx = 1, cy = 0.5: every operation below is exact.  One link pixel (u = 2, v = 1) at 3 m,
    t = 0.5."""
    intr = (2.0, 4.0, 1.0, 0.5)
    W, H = 4, 3
    virt = np.full((H, W), np.inf, F)
    virt[1, 2] = 3.0
    below = np.nextafter(F(-1.5), F(-np.inf))
    pts = np.array([
        [1.0, 0.25, 2.0],            # uf = 0.5 * 2 + 1 + 0.5 = 2.5, vf = 0.125 * 4 + 0.5 + 0.5 = 1.5: pixel (2, 1); 2 > 2.5? no: kept
        [1.5, 0.375, 3.0],           # the same pixel; 3 > 2.5: filtered
        [1.25, 0.3125, 2.5],         # the same pixel, exactly on V - t: kept (strict)
        [0.0, 0.0, 1.0],             # uf = 1.5, vf = 1.0: pixel (1, 1), nothing drawn there: kept whatever z
        [0.0, 0.0, 0.0],             # z = 0: outside
        [0.0, 0.0, -1.0],            # negative z: outside
        [0.0, 0.0, np.inf],          # infinite z: outside
        [np.nan, 0.0, 1.0],          # NaN: the range test fails: outside
        [-1.5, 0.0, 2.0],            # a = -0.75: uf = -1.5 + 1 + 0.5 = 0 exactly: judged, pixel (0, 1)
        [below, 0.0, 2.0],           # x an ulp below: a = -0.75000006, (a * fx) + cx = -0.5000001, uf = -1.2e-7 < 0: outside
    ], F)
    judged, u, v = PC.pixel_of(pts, intr, W, H)
    assert judged.tolist() == [True, True, True, True, False, False, False, False, True, False]
    assert u[judged].tolist() == [2, 2, 2, 1, 0] and v[judged].tolist() == [1, 1, 1, 1, 1]
    assert (u[~judged] == 0).all() and (v[~judged] == 0).all()
    verdict, pixel = PC.verdicts(pts, intr, virt, 0.5)
    assert verdict.tolist() == [0, 1, 0, 0, 2, 2, 2, 2, 0, 2] and verdict.dtype == np.uint8
    assert pixel.tolist() == [6, 6, 6, 5] + [PC.NO_PIXEL] * 4 + [4, PC.NO_PIXEL] and pixel.dtype == np.uint32
    assert PC.summary(verdict).tolist() == [4, 1, 5, 10]
    # r = 1: the point on pixel (1, 1) now sees the link pixel in its window; 1 > 2.5 is still false, 2.75 is not
    assert PC.verdicts(pts[3:4], intr, virt, 0.5, r=1)[0].tolist() == [0]
    assert PC.verdicts(np.array([[0.0, 0.0, 2.75]], F), intr, virt, 0.5, r=1)[0].tolist() == [1]
    assert PC.verdicts(np.array([[0.0, 0.0, 2.75]], F), intr, virt, 0.5, r=0)[0].tolist() == [0]
    # the window is clipped to the image: pixel (0, 1) at r = 1 does not reach column 2
    assert PC.verdicts(np.array([[-3.0, 0.0, 4.0]], F), intr, virt, 0.5, r=1)[0].tolist() == [0]
    # a transform: a shift by (1, 0.25, 1) moves (0, 0, 1) onto the first point
    M = np.eye(4)
    M[:3, 3] = (1.0, 0.25, 1.0)
    moved = PC.transformed(np.array([[0.0, 0.0, 1.0]], F), M.T.reshape(16))
    assert moved.tolist() == [[1.0, 0.25, 2.0]]
    assert PC.verdicts(np.array([[0.5, 0.125, 2.0]], F), intr, virt, 0.5, matrix=M.T.reshape(16))[1].tolist() == [6]
    # without a transform an infinite x leaves y and z alone (no arithmetic): not judged because uf is infinite, nothing else
    assert PC.transformed(np.array([[np.inf, 1.0, 2.0]], F), None).tolist() == [[np.inf, 1.0, 2.0]]
    # window_min by hand
    wm = PC.window_min(virt, 1)
    assert np.isfinite(wm).sum() == 9 and wm[0, 1] == 3.0 and np.isinf(wm[0, 0])
    assert PC.stored_intrinsics(525.1, 3.3, 319.5, 0.1) == (F(525.1), F(3.3), F(319.5), F(0.1))


def _round_trip_points_land_on_their_pixels(W, H, intr, rng):
    s = rng.uniform(0.05, 12.0, (H, W)).astype(F)
    judged, u, v = PC.pixel_of(PC.grid_points(s, intr), intr, W, H)
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return bool(judged.all() and np.array_equal(u, uu.ravel()) and np.array_equal(v, vv.ravel()))


def test_a_cloud_point_lands_on_its_own_pixel_again():
    rng = np.random.default_rng(3)
    for W, H in ((100, 75), (160, 120), (640, 480)):
        for slot in range(3):
            f = 262.5 * W / 320.0
            assert _round_trip_points_land_on_their_pixels(W, H, (f + slot, f - 0.5 * slot, (W - 1) / 2.0 + 0.25 * slot, (H - 1) / 2.0 - 0.5 * slot), rng)


# ---- the kernel's arithmetic on the host ---------------------------------------------------------------------------------

PINHOLES = [(525.0, 525.0, 319.5, 239.5, 640, 480), (585.260, 585.028, 317.387, 239.264, 640, 480), (131.25, 131.25, 79.5, 59.5, 160, 120),
            (82.03125, 81.53125, 49.75, 36.5, 100, 75), (1050.3, 1049.1, 640.2, 359.4, 1280, 720)]


def _sweep():
    """Rows (W, H, moved, x, y, z, fx, fy, cx, cy, vmin, t, m[12]): every triple of the edge values; uf and vf on and either
    side of 0, W and H for every pinhole; 4,000 random points without and 4,000 with a transform."""
    rng = np.random.default_rng(17)
    ident = np.eye(4).T.reshape(16)
    rows = []

    def add(W, H, p, intr, vmin, t, matrix=None):
        m = (ident if matrix is None else matrix).reshape(4, 4)[:, :3].reshape(12)      # (column-major: column c, rows 0 .. 2)
        rows.append((W, H, 0 if matrix is None else 1) + tuple(F(q) for q in p) + PC.stored_intrinsics(*intr) + (F(vmin), F(t)) + tuple(F(q) for q in m))

    for fx, fy, cx, cy, W, H in PINHOLES:
        intr = (fx, fy, cx, cy)
        for p in PC.edge_points():
            add(W, H, p, intr, 1.0, 0.05)
        k = PC.stored_intrinsics(*intr)
        for z in (F(0.3), F(1.0), F(7.3)):
            for edge, f, c in ((0.0, k[0], k[2]), (float(W), k[0], k[2])):
                a0 = F((F(edge) - F(0.5) - c) / f)
                for step in range(-3, 4):
                    a = a0
                    for _ in range(abs(step)):
                        a = np.nextafter(a, F(np.inf) if step > 0 else F(-np.inf))
                    add(W, H, (F(a * z), F(0.0), z), intr, np.inf, 0.05)
            for edge, f, c in ((0.0, k[1], k[3]), (float(H), k[1], k[3])):
                b0 = F((F(edge) - F(0.5) - c) / f)
                for step in range(-3, 4):
                    b = b0
                    for _ in range(abs(step)):
                        b = np.nextafter(b, F(np.inf) if step > 0 else F(-np.inf))
                    add(W, H, (F(0.0), F(b * z), z), intr, np.inf, 0.05)
    for moved in (False, True):
        pts = PC.random_points(rng, 4000)
        for i, p in enumerate(pts):
            fx, fy, cx, cy, W, H = PINHOLES[i % len(PINHOLES)]
            vmin = np.inf if i % 7 == 0 else rng.uniform(0.2, 9.0)
            add(W, H, p, (fx, fy, cx, cy), vmin, rng.uniform(0.0, 0.2), PC.rigid_transform(rng) if moved else None)
    return rows


def _expected(rows):
    """(judged, u, v, verdict, points') of the rows through points_check: the transforms row by row, the pixels per pinhole."""
    n = len(rows)
    moved_pts = np.zeros((n, 3), F)
    for i, r in enumerate(rows):
        matrix = None
        if r[2]:
            M = np.zeros((4, 4))
            M[:, :3] = np.array(r[12:24], np.float64).reshape(4, 3)      # (row c of M = column c of the transform: column-major)
            M[3, 3] = 1.0
            matrix = M.reshape(16)
        moved_pts[i] = PC.transformed(np.array([r[3:6]], F), matrix)[0]
    judged, u, v = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, np.int64)
    keys = [(r[0], r[1]) + tuple(r[6:10]) for r in rows]
    for key in set(keys):
        at = np.array([i for i, k in enumerate(keys) if k == key])
        judged[at], u[at], v[at] = PC.pixel_of(moved_pts[at], key[2:], key[0], key[1])
    vmin, t = np.array([r[10] for r in rows], F), np.array([r[11] for r in rows], F)
    with np.errstate(all="ignore"):
        filtered = moved_pts[:, 2] > (vmin - t).astype(F)
    verdict = np.where(judged, np.where(filtered, PC.FILTERED, PC.KEPT), PC.OUTSIDE).astype(np.uint8)
    return judged, u, v, verdict, moved_pts


@pytest.fixture(scope="module")
def sweep():
    rows = _sweep()
    return rows, _expected(rows)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_the_kernels_helper_agrees_with_numpy_bit_for_bit(tmp_path, sweep, sanitize):
    rows, (judged, u, v, verdict, moved) = sweep
    exe = str(tmp_path / "point_pixel_check")
    flags = ["-O2", "-ffp-contract=off"] + (["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"] if sanitize else [])
    subprocess.check_call(["g++"] + flags + ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "point_pixel_check.cpp")])
    bits = lambda f: int(np.array(f, F).view(np.uint32))
    text = "%d\n" % len(rows) + "\n".join("%d %d %d " % r[:3] + " ".join("%x" % bits(f) for f in r[3:]) for r in rows) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stderr[-3000:], r.stdout[-300:])
    got = [line.split() for line in r.stdout.splitlines()]
    assert len(got) == len(rows)
    g_judged = np.array([int(g[0]) for g in got], bool)
    g_u, g_v = np.array([int(g[1]) for g in got]), np.array([int(g[2]) for g in got])
    g_verdict = np.array([int(g[3]) for g in got], np.uint8)
    g_pts = np.array([[int(w, 16) for w in g[4:7]] for g in got], np.uint32)
    assert np.array_equal(g_judged, judged), np.argwhere(g_judged != judged)[:5]
    assert np.array_equal(g_u, u) and np.array_equal(g_v, v), np.argwhere((g_u != u) | (g_v != v))[:5]
    assert np.array_equal(g_verdict, verdict), np.argwhere(g_verdict != verdict)[:5]
    same = (g_pts == moved.view(np.uint32)) | (np.isnan(g_pts.view(F)) & np.isnan(moved))
    assert same.all(), np.argwhere(~same)[:5]
    # (a vacuous pass must not hide: every verdict occurs often, and points land on the first and last column and row)
    assert (verdict == 0).sum() > 500 and (verdict == 1).sum() > 500 and (verdict == 2).sum() > 2000
    Ws, Hs = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    assert (judged & (u == 0)).sum() > 10 and (judged & (u == Ws - 1)).sum() > 10 and (judged & (v == 0)).sum() > 10 and (judged & (v == Hs - 1)).sum() > 10


def test_points_routes(tmp_path):
    exe = str(tmp_path / "routes_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "routes_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok", r.stdout + r.stderr
    # (the walk's 1,792 combinations hold the 256 of a points batch this asserted before; field 7: the points routes, 2 as before)
    ok = r.stdout.splitlines()[0].split()
    assert ok[1] == "1792" and ok[7] == "2", r.stdout
    assert {p for p in r.stdout.splitlines()[1].split() if p.startswith("Points:")} == {"Points:NoLabelPlane", "Points:PointsDilation", "Points:PointsPadding",
                                                                                        "Points:PointsThresh"}


# ---- conditions on the GPU tests' inputs -------------------------------------------------------------------------------------

def _grid_counts(sc):
    """Per stream: filtered pixel-grid points, and kept ones that land on a link pixel (oracle only)."""
    virt = virtual_planes(sc, empty=np.inf)
    filtered, kept_on_link = [], []
    for s in range(sc.n):
        intr = intrinsics(sc, s)
        verdict, pixel = PC.verdicts(PC.grid_points(sc.depth[s], intr), intr, virt[s], sc.wl.max_diff)
        on_link = np.isfinite(virt[s]).ravel()[np.where(verdict != PC.OUTSIDE, pixel, 0)] & (verdict != PC.OUTSIDE)
        filtered.append(int((verdict == PC.FILTERED).sum()))
        kept_on_link.append(int(((verdict == PC.KEPT) & on_link).sum()))
    return filtered, kept_on_link


def test_the_scenes_give_filtered_points_and_kept_points_on_links():
    sc = soup_scene(3, 100, 75)
    filtered, kept_on_link = _grid_counts(sc)
    assert filtered == [2210, 2480, 2508] and all(f >= 2000 for f in filtered), filtered
    assert kept_on_link == [139, 211, 75] and all(k >= 75 for k in kept_on_link), kept_on_link
    big = soup_scene(1, 160, 120)
    filtered, _ = _grid_counts(big)
    assert filtered == [8593, 18452, 10805], filtered
    # ... and the pixel-grid verdict is the filter's mask bit wherever a link holds the pixel
    virt = virtual_planes(sc, empty=np.inf)
    mask = filter_expected(sc, 0)[1]
    for s in range(sc.n):
        intr = intrinsics(sc, s)
        verdict, _ = PC.verdicts(PC.grid_points(sc.depth[s], intr), intr, virt[s], sc.wl.max_diff)
        link = np.isfinite(virt[s]).ravel() & (verdict != PC.OUTSIDE)
        assert np.array_equal(verdict[link] == PC.FILTERED, mask[s].ravel()[link] != 0)
