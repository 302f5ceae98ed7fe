"""CPU (no GPU): link clearance tables (include/rtuf.h, LINK CLEARANCE TABLES) -- the entry points' place in the ABI, the
expectation bench_support/clearance_check.py by hand on nine pixels and three spheres, the kernels' own arithmetic
(rtuf_numerics.h, compiled for the host by tests/clearance_check.cpp) against that expectation bit for bit on a sweep of edge
values, and geometry.bounding_spheres against its C++ twin in host.hpp."""
import os
import re
import subprocess

import numpy as np

import realtime_urdf_filter_amd as R
from bench_support import clearance_check as KC
from realtime_urdf_filter_amd.geometry import bounding_spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtuf.h")
CSRC = os.path.join(ROOT, "realtime_urdf_filter_amd", "csrc")
F = np.float32
CALLS = ("rtuf_link_clearance_batch_device", "rtuf_link_clearance_batch_device_u16", "rtuf_link_clearance_batch", "rtuf_link_clearance_batch_u16")
INF, NONE = F(np.inf), 0xFFFFFFFF


def test_header_declares_the_calls_and_the_abi_version_is_still_6():
    text = open(HEADER).read()
    assert "LINK CLEARANCE TABLES" in text
    assert re.search(r"\bint rtuf_set_link_spheres\(rtuf_context \*ctx, int model, const int32_t \*link[^,]*, const float \*xyzr[^,]*, int n_spheres\)", text)
    assert "rtuf_set_link_spheres" in R._capi.SYMBOLS
    for name in CALLS:
        assert re.search(r"\bint %s\(rtuf_context \*ctx, int n_streams," % name, text), name
        assert name in R._capi.SYMBOLS, name
    assert re.search(r"\}\s*rtuf_link_clearance;", text)
    assert re.search(r"#define RTUF_ABI_VERSION 6\b", text) and R.ABI_VERSION == 6
    for name in ("set_link_spheres", "link_clearance_batch", "link_clearance_batch_u16", "link_clearance_batch_device", "link_clearance_batch_device_u16"):
        assert callable(getattr(R.Context, name)), name
    from realtime_urdf_filter_amd.filter import RealtimeURDFFilter
    assert callable(RealtimeURDFFilter.clearance)
    facade = open(os.path.join(ROOT, "include", "realtime_urdf_filter_amd", "urdf_filter.hpp")).read()
    assert re.search(r"\bbool clearance_into\(", facade)
    assert R.LINK_CLEARANCE_DTYPE.itemsize == 16 and KC.DTYPE == R.LINK_CLEARANCE_DTYPE


def test_struct_sizes():
    src = ('#include "rtuf.h"\nstatic_assert(sizeof(rtuf_link_clearance) == 16, "row");\nstatic_assert(sizeof(rtuf_params) == 48, "params");\n'
           'static_assert(RTUF_ABI_VERSION == 6, "abi");\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_expectation_by_hand_on_nine_pixels_and_three_spheres():
    """A 3 x 3 image whose nine kept points lie in the plane z = 0 at x, y in {-1, 0, 1} (pixel index v * 3 + u):
    label 1: sphere id 0 at (0, 0, 0) r = 1.5 -- the centre pixel is inside it (clearance -1.5), the edge pixels at -0.5;
    label 2: spheres id 1 at (-3, 0, 0) and id 2 at (3, 0, 0), r = 1: pixels 3 (x = -1) and 5 (x = 1) both have clearance
             1 to their sphere: a tie between two pixels and two spheres, won by pixel 3, and at pixel 3 only sphere 1 gives it;
    label 3: a sphere far away: no point in range."""
    xs = np.array([-1.0, 0.0, 1.0], F)
    pts = np.array([[x, y, 0.0] for y in xs for x in xs], F)
    idx = np.arange(9, dtype=np.uint32)
    centres = np.array([[0, 0, 0], [-3, 0, 0], [3, 0, 0], [0, 0, 50]], F)
    radii, labels, ids = F([1.5, 1.0, 1.0, 0.5]), [1, 2, 2, 3], [0, 1, 2, 3]
    t = KC.table(pts, idx, centres, radii, labels, ids, 4, 1.25)
    assert t.dtype == KC.DTYPE
    assert t[1].tolist() == (-1.5, 4, 0, 9)                       # every point within 1.25 of sphere 0; the nearest is inside it
    # label 2: x = -1 column (pixels 0, 3, 6) to sphere 1: sqrt(4 + y^2) - 1 = 1 at y = 0, 1.236.. at |y| = 1: all < 1.25; same at x = 1
    assert t[2].tolist() == (1.0, 3, 1, 6)
    assert t[3].tolist() == (np.inf, NONE, NONE, 0)
    assert t[0].tolist() == (-1.5, 4, 0, 9)                       # the whole robot: 9 points, not 9 + 6
    # a tie between two spheres at ONE pixel: the smaller id wins
    t2 = KC.table(pts[4:5], idx[4:5], centres[1:3], radii[1:3], [2, 2], [7, 5], 3, 5.0)
    assert t2[2].tolist() == (2.0, 4, 5, 1) and t2[0].tolist() == (2.0, 4, 5, 1) and t2[1].tolist() == (np.inf, NONE, NONE, 0)
    # exactly at max_distance: not counted; one ulp above it: counted
    one = F(1.0)
    t3 = KC.table(pts, idx, centres[1:3], radii[1:3], [2, 2], [1, 2], 3, one)
    assert t3[2].tolist() == (np.inf, NONE, NONE, 0)
    t4 = KC.table(pts, idx, centres[1:3], radii[1:3], [2, 2], [1, 2], 3, np.nextafter(one, F(2.0)))
    assert t4[2].tolist() == (1.0, 3, 1, 2)
    # labels 0 and >= n_labels take no part, in row 0 either
    t5 = KC.table(pts, idx, centres, radii, [0, 2, 2, 1], ids, 2, np.inf)
    assert t5[0].tolist() == t5[1].tolist() and t5[1]["sphere"] == 3 and t5[1]["points_within"] == 9
    # +inf as max_distance counts every finite clearance
    t6 = KC.table(pts, idx, centres, radii, labels, ids, 4, np.inf)
    assert t6["points_within"].tolist() == [9, 9, 9, 9] and t6[3]["clearance"] == F(F(50.0) - F(0.5))


def test_centres_are_three_elementwise_products_in_double():
    m = np.arange(1.0, 17.0) / 7.0
    p = np.array([0.1, -0.2, 0.3], F)
    got = KC.transform(m, p.astype(np.float64))
    x, y, z = (float(v) for v in p)
    want = [((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] for r in range(3)]
    assert got.tolist() == want
    eye = np.eye(4).T.reshape(16)
    assert KC.centre(eye, eye, eye, p).tolist() == p.tolist()


def _bits32(f):
    return int(np.array(f, F).view(np.uint32))


def _sweep():
    rng = np.random.default_rng(11)
    tiny, huge, sub = F(1e-30), F(3e38), np.nextafter(F(0.0), F(1.0))
    pairs = []
    edge = [F(0.0), tiny, sub, F(1e-20), F(1.0), F(-2.5), F(1e19), huge]
    for a in edge:
        for r in (F(0.0), sub, tiny, F(0.25), F(1e30), huge):
            pairs.append((a, F(0.5), F(-1.0), a, F(0.5), F(-1.0), r))          # d = 0
            pairs.append((a, F(0.0), F(0.0), F(0.0), F(0.0), F(0.0), r))        # one component
            pairs.append((a, a, a, -a, tiny, F(0.0), r))                         # products that underflow or overflow
    for _ in range(4000):
        p = rng.uniform(-4, 4, 3)
        c = p + rng.normal(0, 1, 3) * rng.choice([1e-4, 0.05, 1.0])
        pairs.append(tuple(F(v) for v in p) + tuple(F(v) for v in c) + (F(rng.uniform(0, 0.5)),))
    mats = []
    for i in range(4000):
        scale = 10.0 ** rng.integers(-3, 4) if i % 5 == 0 else 1.0
        m = [rng.normal(0, 1, 16) * scale for _ in range(3)]
        c = rng.uniform(-2, 2, 3) * (1e-30 if i % 50 == 0 else 1.0)
        mats.append((np.concatenate(m), F(c)))
    return pairs, mats


def test_the_kernels_helpers_agree_with_numpy_bit_for_bit(tmp_path):
    exe = str(tmp_path / "clearance_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "clearance_check.cpp")])
    pairs, mats = _sweep()
    lines = ["%d" % (len(pairs) + len(mats))]
    lines += ["p " + " ".join("%x" % _bits32(f) for f in row) for row in pairs]
    lines += ["c " + " ".join("%x" % int(b) for b in m.view(np.uint64)) + " " + " ".join("%x" % _bits32(f) for f in c) for m, c in mats]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(pairs) + len(mats)
    a = np.array(pairs, F)
    want = np.array([KC.point_sphere(a[i, :3], a[i, 3:6], a[i, 6]) for i in range(len(a))], F).view(np.uint32)
    got = np.array([int(line, 16) for line in out[:len(pairs)]], np.uint32)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    neg = want.view(F) < 0
    assert neg.sum() > 100 and (want.view(F)[:144] == 0).sum() >= 1 and np.isinf(want.view(F)).sum() >= 1
    gotc = np.array([[int(w, 16) for w in line.split()] for line in out[len(pairs):]], np.uint32)
    wantc = np.array([KC.centre(m[:16], m[16:32], m[32:], c) for m, c in mats], F).view(np.uint32)
    assert np.array_equal(gotc, wantc), np.argwhere(gotc != wantc)[:5]


def test_bounding_spheres_python_against_cpp(tmp_path):
    rng = np.random.default_rng(3)
    clouds = [rng.normal(0, 1, (200, 3)) * [0.05, 0.4, 0.05], rng.uniform(-1, 1, (57, 3)), np.array([[0.1, 0.2, 0.3]]), np.array([[0, 0, 0], [0, 0, 1.0]]),
              np.repeat([[1.0, 2.0, 3.0]], 5, axis=0)]
    src = tmp_path / "spheres.cpp"
    src.write_text('#include "realtime_urdf_filter_amd/host.hpp"\n#include <cstdio>\n#include <cstring>\n'
                   "int main() { int n, seg; while (scanf(\"%d %d\", &n, &seg) == 2) { std::vector<float> v(3 * (size_t)n);\n"
                   "  for (float& f : v) { unsigned u; if (scanf(\"%x\", &u) != 1) return 2; memcpy(&f, &u, 4); }\n"
                   "  const std::vector<float> s = rtuf_host::bounding_spheres(v, seg); printf(\"%zu\", s.size() / 4);\n"
                   "  for (float f : s) { unsigned u; memcpy(&u, &f, 4); printf(\" %x\", u); } printf(\"\\n\"); } return 0; }\n")
    exe = str(tmp_path / "spheres")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    cases = [(c.astype(F), seg) for c in clouds for seg in (1, 4, 7)]
    text = "".join("%d %d %s\n" % (len(v), seg, " ".join("%x" % _bits32(f) for f in v.ravel())) for v, seg in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(cases)
    several = 0
    for (v, seg), line in zip(cases, out):
        sp = bounding_spheres(v, seg)
        words = line.split()
        assert int(words[0]) == len(sp) and 1 <= len(sp) <= seg
        assert [int(w, 16) for w in words[1:]] == sp.view(np.uint32).ravel().tolist(), (seg, sp)
        several += len(sp) > 1
        # every vertex lies inside a sphere (in double, against the float radius)
        d = np.sqrt(((v.astype(np.float64)[:, None, :] - sp[None, :, :3].astype(np.float64)) ** 2).sum(axis=2))
        assert (d <= sp[None, :, 3].astype(np.float64) * (1 + 1e-12)).any(axis=1).all()
    assert several >= 4
    assert bounding_spheres(np.zeros((0, 3)), 3).shape == (0, 4)
    one = bounding_spheres([[0, 0, 0], [2, 0, 0]], 1)
    assert one.tolist() == [[1.0, 0.0, 0.0, 1.0]]
