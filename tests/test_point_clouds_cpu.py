"""CPU (no GPU): filtered point clouds (include/rtuf.h, FILTERED POINT CLOUDS) -- the entry points' place in the ABI, the
expectation bench_support/cloud_check.py by hand on nine pixels, and the kernels' own per-pixel arithmetic (rtuf_numerics.h,
compiled for the host by tests/cloud_point_check.cpp) against that expectation, bit for bit, on a sweep of edge values."""
import os
import re
import subprocess

import numpy as np

import realtime_urdf_filter_amd as R
from bench_support import cloud_check as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtuf.h")
CSRC = os.path.join(ROOT, "realtime_urdf_filter_amd", "csrc")
F = np.float32
CALLS = ("rtuf_cloud_batch_device", "rtuf_cloud_batch_device_u16", "rtuf_cloud_compact_batch_device", "rtuf_cloud_compact_batch_device_u16",
         "rtuf_cloud_batch", "rtuf_cloud_batch_u16", "rtuf_cloud_compact_batch", "rtuf_cloud_compact_batch_u16")
EDGE = [F(np.nan), F(0.0), F(-0.0), F(-1.0), F(np.inf), F(1e-30), F(65.535)]


def test_header_declares_the_calls_and_the_abi_version_is_still_6():
    text = open(HEADER).read()
    assert "FILTERED POINT CLOUDS" in text
    assert re.search(r"\bint rtuf_set_cloud_intrinsics\(rtuf_context \*ctx, int first_stream, int n_streams, const double \*fx_fy_cx_cy", text)
    assert "rtuf_set_cloud_intrinsics" in R._capi.SYMBOLS
    for name in CALLS:
        assert re.search(r"\bint %s\(rtuf_context \*ctx, int n_streams," % name, text), name
        assert name in R._capi.SYMBOLS, name
    assert re.search(r"#define RTUF_ABI_VERSION 6\b", text) and R.ABI_VERSION == 6
    for name in ("set_cloud_intrinsics", "cloud_batch", "cloud_batch_u16", "cloud_compact_batch", "cloud_compact_batch_u16", "cloud_batch_device",
                 "cloud_batch_device_u16", "cloud_compact_batch_device", "cloud_compact_batch_device_u16"):
        assert callable(getattr(R.Context, name)), name
    from realtime_urdf_filter_amd.filter import RealtimeURDFFilter
    assert callable(RealtimeURDFFilter.cloud)
    facade = open(os.path.join(ROOT, "include", "realtime_urdf_filter_amd", "urdf_filter.hpp")).read()
    assert re.search(r"\bbool cloud_into\(", facade)


def test_struct_sizes_are_unchanged():
    src = ('#include "rtuf.h"\nstatic_assert(sizeof(rtuf_params) == 48, "params");\nstatic_assert(sizeof(rtuf_link_residuals) == 64, "row");\n'
           "int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_expectation_by_hand_on_nine_pixels():
    """3 x 3: the seven edge values, one masked valid value and one kept value."""
    intr = (2.0, 4.0, 1.0, 0.5)                    # kx = 0.5, ky = 0.25: every product below is exact
    s = np.array(EDGE + [F(3.0), F(2.0)], F).reshape(3, 3)
    mask = np.zeros((3, 3), np.uint8)
    mask[2, 1] = 255
    k = CC.kept(s, mask)
    #                        NaN    0      -0     -1     +inf   1e-30 65.535 masked kept
    assert k.ravel().tolist() == [False, False, False, False, False, True, True, False, True]
    assert CC.classes(s, mask) == (3, 1, 5)          # (the masked pixel holds a valid value)
    org = CC.organized(s, mask, intr)
    assert org.shape == (3, 3, 3) and (org.view(np.uint32)[~k] == 0x7FC00000).all()
    # pixel (u = 2, v = 2), s = 2: x = ((2 - 1) * 2) * 0.5 = 1, y = ((2 - 0.5) * 2) * 0.25 = 0.75
    assert org[2, 2].tolist() == [1.0, 0.75, 2.0]
    # pixel (u = 0, v = 2), s = 65.535: x = ((0 - 1) * s) * 0.5, y = ((2 - 0.5) * s) * 0.25, single float32 operations
    s6 = F(65.535)
    assert org[2, 0].tolist() == [F(F(F(-1.0) * s6) * F(0.5)), F(F(F(1.5) * s6) * F(0.25)), s6]
    # pixel (u = 2, v = 1), s = 1e-30: products may go subnormal, the point is still kept
    assert org[1, 2, 2] == F(1e-30) and np.isfinite(org[1, 2]).all()
    pts, idx, count = CC.compacted(s, mask, intr)
    assert count == 3 and idx.tolist() == [5, 6, 8] and idx.dtype == np.uint32
    assert np.array_equal(pts.view(np.uint32), org.reshape(-1, 3)[[5, 6, 8]].view(np.uint32))
    assert np.array_equal(CC.u16_to_metres(np.array([0, 1, 65535], np.uint16)), F([0.0, 0.001, 65.535]))
    kx, ky, cx, cy = CC.stored_intrinsics(525.0, 3.0, 319.5, 0.1)
    assert (kx, ky, cx, cy) == (F(1.0 / 525.0), F(1.0 / 3.0), F(319.5), F(0.1))


def _sweep():
    """(u, v, s, kx, ky, cx, cy): the edge values x u in {0, 1, 63, 64, 99, 516} x several intrinsics, plus 4,000 random
    triples (u, v, s) with random intrinsics."""
    intrinsics = [(525.0, 525.0, 319.5, 239.5), (585.260, 585.028, 317.387, 239.264), (131.25, 131.25, 79.5, 59.5), (1e-3, 1e6, -4.25, 1000.0),
                  (262.5 * 517 / 320.0, 300.0, 258.0, 194.0)]
    rows = []
    for fx, fy, cx, cy in intrinsics:
        k = CC.stored_intrinsics(fx, fy, cx, cy)
        for s in EDGE + [F(0.5), F(7.99), np.nextafter(F(0.0), F(1.0)), np.nextafter(F(np.inf), F(0.0))]:
            for u in (0, 1, 63, 64, 99, 516):
                for v in (0, 74, 388):
                    rows.append((u, v, s) + k)
    rng = np.random.default_rng(7)
    for u, v, s, fx, fy, cx, cy in zip(rng.integers(0, 1920, 4000), rng.integers(0, 1080, 4000), rng.uniform(-0.5, 12.0, 4000),
                                      rng.uniform(50, 2000, 4000), rng.uniform(50, 2000, 4000), rng.uniform(0, 1920, 4000), rng.uniform(0, 1080, 4000)):
        rows.append((int(u), int(v), F(s)) + CC.stored_intrinsics(fx, fy, cx, cy))
    return rows


def test_the_kernels_helper_agrees_with_numpy_bit_for_bit(tmp_path):
    exe = str(tmp_path / "cloud_point_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cloud_point_check.cpp")])
    rows = _sweep()
    bits = lambda f: int(np.array(f, F).view(np.uint32))
    text = "%d\n" % len(rows) + "\n".join("%d %d %x %x %x %x %x" % ((r[0], r[1]) + tuple(bits(f) for f in r[2:])) for r in rows) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.array([[int(w, 16) for w in line.split()] for line in r.stdout.splitlines()], np.uint32)
    assert got.shape == (len(rows), 4)
    u, v = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    s = np.array([r[2] for r in rows], F)
    kx, ky, cx, cy = (np.array([r[i] for r in rows], F) for i in (3, 4, 5, 6))
    with np.errstate(all="ignore"):
        x = (((u.astype(F) - cx).astype(F) * s).astype(F) * kx).astype(F)
        y = (((v.astype(F) - cy).astype(F) * s).astype(F) * ky).astype(F)
        valid = (s > 0) & (s < F(np.inf))
    assert np.array_equal(got[:, 0], valid.astype(np.uint32))
    for name, want, col in (("x", x, 1), ("y", y, 2), ("z", s, 3)):
        assert np.array_equal(got[:, col], want.view(np.uint32)), (name, np.argwhere(got[:, col] != want.view(np.uint32))[:5])
    assert np.array_equal(got[:, 1:][valid], np.stack([x, y, s], axis=1).view(np.uint32)[valid])      # every kept point, bit for bit
    assert valid.sum() > 3000 and (~valid).sum() > 100
    # ... and cloud_check.points is that same arithmetic
    p = CC.points(np.array([[F(2.5)]], F), (525.0, 500.0, 319.5, 239.5), u=np.array([[99]]), v=np.array([[7]]))
    k = CC.stored_intrinsics(525.0, 500.0, 319.5, 239.5)
    assert p[0, 0].tolist() == [F(F(F(F(99) - k[2]) * F(2.5)) * k[0]), F(F(F(F(7) - k[3]) * F(2.5)) * k[1]), F(2.5)]
