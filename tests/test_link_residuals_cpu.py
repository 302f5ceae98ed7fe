"""CPU (no GPU): link residual tables (include/rtuf.h, LINK RESIDUAL TABLES) -- the entry points' place in the ABI, the numpy
row dtype, the expectation bench_support/residuals_check.py on a committed golden scene, and the kernels' own per-pixel
arithmetic (rtuf_numerics.h, compiled for the host by tests/link_residual_check.cpp) against that expectation on a sweep of
edge values."""
import os
import re
import subprocess

import numpy as np

import golden_io
import realtime_urdf_filter_amd as R
from bench_support.labels_check import expected_labels
from bench_support.link_thresholds_check import expected_planes
from bench_support.residuals_check import ROW, classify, expected_table, quantise, table_from_planes, tables_equal, virtual_depth
from oracle import bindings as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtuf.h")
CSRC = os.path.join(ROOT, "realtime_urdf_filter_amd", "csrc")
F = np.float32
CALLS = ("rtuf_link_residuals_batch_device", "rtuf_link_residuals_batch_device_u16", "rtuf_link_residuals_batch", "rtuf_link_residuals_batch_u16")


def test_header_declares_the_calls_and_the_64_byte_row():
    text = open(HEADER).read()
    assert "LINK RESIDUAL TABLES" in text
    for name in CALLS:
        assert re.search(r"\bint %s\(rtuf_context \*ctx, int n_streams," % name, text), name
        assert name in R._capi.SYMBOLS, name
    body = re.search(r"typedef struct \{([^}]*)\} rtuf_link_residuals;", text).group(1)
    fields = re.findall(r"^\s*(u?int64_t)\s+(\w+);", body, re.M)
    assert [f[1] for f in fields] == list(ROW.names) and len(fields) * 8 == 64
    assert [f[0] for f in fields] == ["uint64_t"] * 6 + ["int64_t", "uint64_t"]
    src = '#include "rtuf.h"\nstatic_assert(sizeof(rtuf_link_residuals) == 64, "row");\nint main() { return 0; }\n'
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_abi_version_is_still_6():
    assert re.search(r"#define RTUF_ABI_VERSION 6\b", open(HEADER).read()) and R.ABI_VERSION == 6


def test_numpy_dtype_is_the_headers_row():
    assert R.LINK_RESIDUALS_DTYPE.itemsize == 64 and R.LINK_RESIDUALS_DTYPE == ROW
    assert [R.LINK_RESIDUALS_DTYPE.fields[n][1] for n in ROW.names] == list(range(0, 64, 8))
    for name in ("link_residuals_batch", "link_residuals_batch_u16", "link_residuals_batch_device", "link_residuals_batch_device_u16"):
        assert callable(getattr(R.Context, name)), name
    from realtime_urdf_filter_amd.filter import RealtimeURDFFilter
    assert callable(RealtimeURDFFilter.link_residuals)


def test_expectation_by_hand():
    v = virtual_depth(F(0.99), 0.1, 8.0)
    t = F(0.05)
    lo, hi = F(v - t), F(v + t)
    #            agree      in front           behind             invalid+filtered  invalid           undrawn valid  undrawn invalid
    s = F([v + F(0.01), np.nextafter(lo, F(-9)), np.nextafter(hi, F(9)), 0.0, np.nan, 1.0, -1.0, lo, hi])
    drawn = np.array([1, 1, 1, 1, 1, 0, 0, 1, 1], bool)
    lab = np.array([2, 2, 2, 2, 2, 0, 0, 1, 1])
    tab = table_from_planes(lab, drawn, s, np.full(9, v, F), np.full(9, t, F), 4)
    assert tuple(tab[2])[:6] == (5, 2, 2, 1, 1, 1) and tab[2]["sum_residual"] == quantise(F(F(s[0] - v) * F(1048576.0)))
    assert tuple(tab[0])[:6] == (2, 1, 0, 0, 0, 0) and tab[0]["sum_residual"] == 0
    assert tuple(tab[1])[:6] == (2, 0, 1, 1, 0, 1)                 # s == lo is not filtered: in front; s == hi is not beyond: agrees
    assert not tab[3:4].view(np.uint64).any()
    assert quantise(F([2.5, 3.5, -2.5, np.nan, 3e9, -3e9, np.inf])).tolist() == [2, 4, -2, 0, 2147483647, -2147483648, 2147483647]


def test_expectation_on_a_golden_scene():
    fx = golden_io.Fixture("mesh_links_seed21_160x120")
    _, _, zwin, prim, _ = O.filter_frame(fx.depth, fx.projection, fx.draws, fx.offset_inv, fx.cam_tf, z_near=fx.z_near, z_far=fx.z_far,
                                         max_diff=fx.max_diff, replace_value=fx.replace_value, want_debug=True)
    nd = len(fx.draws)
    dlab, dn = np.arange(1, nd + 1), [len(d[4]) for d in fx.draws]
    dthr = np.linspace(-0.05, 0.4, nd).astype(F)
    sensor = fx.depth.copy()
    sensor[::7, ::5] = np.nan
    sensor[3::11, 1::3] = 0.0
    n_labels = nd + 2
    tab = expected_table(zwin, prim, sensor, dlab, dn, dthr, fx.max_diff, fx.z_near, fx.z_far, n_labels)
    labels = expected_labels(prim, dlab, dn)
    assert np.array_equal(tab["pixels"], np.bincount(labels.ravel(), minlength=n_labels)) and (tab["pixels"][1:nd + 1] > 0).any()
    _, mask = expected_planes(zwin, prim, sensor, dthr, dn, fx.max_diff, fx.z_near, fx.z_far, fx.replace_value)
    assert np.array_equal(tab["filtered"], np.bincount(labels[mask == 255], minlength=n_labels)) and tab["filtered"].sum() > 0
    undrawn = np.bincount(labels[prim == -1], minlength=n_labels)
    rows = undrawn == 0
    assert rows.any()
    assert np.array_equal((tab["invalid"] + tab["in_front"] + tab["behind"] + tab["agree"])[rows], tab["pixels"][rows])
    assert tab["invalid"].sum() > 0 and tab["agree"].sum() > 0
    assert (tab["sum_abs_residual"].astype(np.int64) >= np.abs(tab["sum_residual"])).all()
    ok, _ = tables_equal(tab, tab.copy())
    assert ok


def _sweep():
    """(s, v, t) triples: for every v and t the values the issue names for s, among them lo, hi and their neighbours."""
    inf, nan = F(np.inf), F(np.nan)
    vs = F([0.43, 1.0, 2.7182817, 7.99, 0.1])
    ts = F([0.0, 0.05, -0.05, 0.3, nan, inf, -inf, 1e-8, 4000.0])
    out = []
    with np.errstate(all="ignore"):
        for v in vs:
            for t in ts:
                lo, hi = F(v - t), F(v + t)
                ss = [nan, F(0.0), F(-0.0), F(-1.0), inf, -inf, lo, np.nextafter(lo, -inf), np.nextafter(lo, inf), hi, np.nextafter(hi, -inf),
                      np.nextafter(hi, inf), v, np.nextafter(v, inf), F(v + F(0.0123)), F(v - F(0.0123)), F(v + F(4.76837158203125e-07) * F(2.5)),
                      F(3000.0), F(65.535), F(1e-30)]
                out += [(F(s), v, t) for s in ss]
    rng = np.random.default_rng(5)
    out += [(F(a), F(b), F(c)) for a, b, c in zip(rng.uniform(-1, 9, 4000), rng.uniform(0.1, 8, 4000), rng.uniform(-0.1, 0.5, 4000))]
    return np.array(out, F)


def test_the_kernels_helper_agrees_with_numpy_on_the_edge_sweep(tmp_path):
    exe = str(tmp_path / "link_residual_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "link_residual_check.cpp")])
    tr = _sweep()
    text = "%d\n" % len(tr) + "\n".join("%x %x %x" % tuple(int(w) for w in row.view(np.uint32)) for row in tr) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.array([[int(w) for w in line.split()] for line in r.stdout.splitlines()], np.int64)
    assert got.shape == (len(tr), 3)
    invalid, filtered, in_front, behind, agree, q = classify(tr[:, 0], tr[:, 1], tr[:, 2])
    want = 1 + 2 * invalid + 4 * filtered + 8 * in_front + 16 * behind + 32 * agree
    assert np.array_equal(got[:, 0], want), np.argwhere(got[:, 0] != want)[:5]
    assert np.array_equal(got[:, 1], q), np.argwhere(got[:, 1] != q)[:5]
    assert np.array_equal(got[:, 2], 1 + 2 * invalid)
    # the sweep reaches every class, saturation and the NaN residual
    assert all(c.any() for c in (invalid, filtered, in_front, behind, agree)) and (invalid & filtered).any()
    assert (q[agree] == 2147483647).any() and (np.isnan(tr[:, 0]) & (q == 0)).any()
