"""CPU (no GPU): link padding (include/rtuf.h, LINK PADDING) -- the kernel's own arithmetic (rtuf_numerics.h's
link_padding_reach2, compiled for the host by tests/link_padding_check.cpp) against the numpy mirror bit for bit, the
expectation bench_support/link_padding_check.py on cases worked out by hand, the scenes of tests/test_link_padding_gpu.py
(each must tell padding from no padding AND from the square dilation of its largest reach, or it proves nothing), the
calls' place in the ABI and the bindings, and the kernel routes with padding in effect (the padded rows of tests/routes_check.cpp)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import link_padding_scenes as LP
import realtime_urdf_filter_amd as R
from bench_support import link_padding_check as PC
from bench_support.dilation_check import drawn_z, shade, window_min
from realtime_urdf_filter_amd.filter import FilterParameters, RealtimeURDFFilter
from bench_support import workloads as WL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtuf.h")
CSRC = os.path.join(ROOT, "realtime_urdf_filter_amd", "csrc")
F = np.float32


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------

def test_reach2_of_the_kernels_header_equals_the_numpy_mirror_bit_for_bit(tmp_path):
    exe = str(tmp_path / "link_padding_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "link_padding_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    head, body, tail = lines[0].split(), lines[1:-2], lines[-2].split()
    assert head[0] == "consts" and tail == ["done", str(len(body))] and len(body) > 50000
    num, off = (np.array([int(w, 16)], np.uint32).view(F)[0] for w in head[1:])
    assert (num, off) == PC.shade_consts(0.1, 8.0)
    rows = np.array([[int(w, 16) for w in line.split()[:3]] + [int(line.split()[3])] for line in body], np.uint32)
    z, pad, f = (np.ascontiguousarray(rows[:, i]).view(F) for i in range(3))
    got = rows[:, 3]
    want = PC.reach2_values(z, pad, f, num, off)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # the sweep shows what it is for: every value 0 .. 256, the clamp, rho just below 1, rho^2 next to an integer on both sides
    assert set(got.tolist()) == set(range(257))
    with np.errstate(all="ignore"):
        rho = ((pad * f) / (num / (z - off))).astype(F)
        sq = (rho * rho).astype(F)
    assert ((rho > 16) & (got == 256)).sum() > 100 and ((rho < 1) & (rho > F(0.999999)) & (got == 0)).sum() >= 3
    with np.errstate(all="ignore"):
        frac = sq - np.floor(sq)
    near = (pad > 0) & ~np.isnan(z) & (sq > 1) & (sq < 256)
    assert (near & (frac < 1e-4)).sum() > 1000 and (near & (frac > 1 - 1e-4)).sum() > 1000
    assert (got[np.isnan(z)] == 0).all() and (got[pad == 0] == 0).all()


def test_reach2_by_hand():
    # f = 525, pad 0.02 m: rho = 10.5 / d pixels.  d = 1 m: R2 = 110; d = 0.5 m: clamped, 256; d = 4 m: rho 2.625, R2 6; d = 12 m: 0
    num, off = PC.shade_consts(0.1, 8.0)
    for d, want in ((1.0, 110), (0.5, 256), (4.0, 6), (7.9, 1)):
        z = F(F(num) / F(d) + off)                     # d = num / (z - off)
        assert abs(float(num / (z - off)) - d) < 1e-3
        assert int(PC.reach2_values(z, F(0.02), F(525.0), num, off)) == want, d
    assert int(PC.reach2_values(F(np.nan), F(0.02), F(525.0), num, off)) == 0
    assert int(PC.reach2_values(F(0.9), F(0.0), F(525.0), num, off)) == 0
    # the header's sentence: a 2 cm margin reaches 16 pixels at d = f / 800
    z = F(F(num) / F(525.0 / 800.0) + off)
    assert int(PC.reach2_values(z, F(0.02), F(525.0), num, off)) in (255, 256)


def test_reach2_maps_primitives_to_draws_to_links():
    prim = np.array([[-1, -2, 0, 1, 2, 4]], np.int32)
    zwin = np.full(prim.shape, 0.95, F)
    R2 = PC.reach2(zwin, prim, [0.0, 0.02, 0.05], [2, 2, 2], 525.0, 0.1, 8.0)
    assert R2[0, :4].tolist() == [0, 0, 0, 0] and R2[0, 4] > 0 and R2[0, 5] > R2[0, 4]


# ---- the expectation's own sanity -----------------------------------------------------------------------------------------------

def test_all_pads_zero_is_the_identity():
    rng = np.random.default_rng(1)
    z = rng.uniform(0.5, 1.0, (40, 50)).astype(F)
    z[rng.random(z.shape) < 0.3] = np.nan
    out = PC.padded_z(z, np.zeros(z.shape, np.uint32))
    assert np.isnan(z).sum() > 100 and np.array_equal(np.isnan(out), np.isnan(z)) and np.array_equal(out[~np.isnan(z)], z[~np.isnan(z)])


def test_one_flat_quad_with_one_pad_is_the_disc_dilation_of_radius_floor_rho():
    H, W = 48, 64
    num, off = PC.shade_consts(0.1, 8.0)
    z_quad = F(F(num) / F(2.0) + off)                   # a quad at 2 m: rho = 0.02 * 525 / 2 = 5.25
    z = np.full((H, W), np.nan, F)
    z[20:28, 5:30] = z_quad                             # undrawn around it, and it touches nothing
    z[0:3, 60:64] = z_quad                              # ... and a piece in the corner: the disc is clipped by the image
    prim = np.where(np.isnan(z), -1, 0).astype(np.int32)
    R2 = PC.reach2(np.nan_to_num(z), prim, [0.02], [2], 525.0, 0.1, 8.0)
    rho = float((F(0.02) * F(525.0)) / (num / (z_quad - off)))
    assert 5.2 < rho < 5.3 and set(R2[~np.isnan(z)].tolist()) == {int(rho * rho)} == {27}
    out = PC.padded_z(z, R2)
    drawn = ~np.isnan(z)
    yy, xx = np.mgrid[0:H, 0:W]
    want = np.zeros((H, W), bool)
    for y, x in np.argwhere(drawn):                     # the disc of radius floor(rho) = 5 in the integer metric dx^2 + dy^2 <= 27
        want |= (yy - y) ** 2 + (xx - x) ** 2 <= 27
    assert np.array_equal(~np.isnan(out), want) and (out[want] == z_quad).all()
    assert want[15, 17] and not want[14, 17] and want[17, 1] and not want[16, 1]      # 5 rows above, (4, 3) diagonally, not (4, 4)


def test_a_nearer_source_wins_where_two_discs_overlap_and_a_farther_one_does_not_hide_it():
    z = np.full((9, 30), np.nan, F)
    z[4, 5], z[4, 12] = 0.9, 0.8                        # two sources 7 apart, the right one nearer
    R2 = np.zeros(z.shape, np.uint32)
    R2[4, 5], R2[4, 12] = 25, 9
    out = PC.padded_z(z, R2)
    assert out[4, 9] == F(0.8) and out[4, 10] == F(0.8) and out[4, 8] == F(0.9) and out[4, 5] == F(0.9) and out[4, 12] == F(0.8)
    assert np.isnan(out[4, 16]) and out[4, 15] == F(0.8) and out[4, 0] == F(0.9)


# ---- the GPU scenes: padding must show, and must not be a square dilation ----------------------------------------------------------

@pytest.mark.parametrize("name", LP.SCENES)
def test_scene_tells_padding_from_no_padding_and_from_the_square_dilation(name):
    sc, pads = LP.scene(name)
    ex = LP.expected(sc, pads)
    differs_plain = differs_square = 0
    for s in range(sc.n):
        z = drawn_z(sc.zwin[s], sc.prim[s])
        plain = shade(z, sc.depth[s], sc.wl.near, sc.wl.far, sc.wl.max_diff, sc.wl.replace_value)[1]
        m = int(np.floor(np.sqrt(float(ex.R2[s].max()))))
        square = shade(window_min(z, m), sc.depth[s], sc.wl.near, sc.wl.far, sc.wl.max_diff, sc.wl.replace_value)[1]
        differs_plain += int((ex.mask[s] != plain).sum())
        differs_square += int((ex.mask[s] != square).sum())
    if name == "undrawn":
        # gpu_support's scene has no link in view (its shifted projection moves them out of the image): with padding in effect
        # it shows the uncovered flag and nothing else; "undrawn_links" is the scene whose padding meets the clear colour
        assert ex.R2.max() == 0 and (sc.prim[0] >= 0).sum() == 0 and np.isnan(ex.zp).any()
        return
    assert ex.R2.max() > 0 and differs_plain > 20 and differs_square > 20, (name, differs_plain, differs_square)
    if name == "near_quad":
        assert ex.R2.max() == 256                       # the clamp
    if name == "ramp":
        r2 = ex.R2[0][sc.prim[0] >= 0]
        assert r2.max() == 256 and r2.min() == 0 and len(np.unique(r2)) > 40      # from the clamp down to 0 along the quad
    if name == "undrawn_links":
        z = drawn_z(sc.zwin[0], sc.prim[0])
        assert (np.isnan(z) & ~np.isnan(ex.zp[0])).sum() > 100 and np.isnan(ex.zp).any()      # clear colour became drawn, and some is left: the bits call fails on retire


# ---- ABI, bindings, façades ---------------------------------------------------------------------------------------------------------

def test_header_declares_the_two_calls_and_the_abi_version_is_still_6():
    text = open(HEADER).read()
    assert "LINK PADDING" in text and "d = f / 800" in text
    assert re.search(r"#define RTUF_MAX_LINK_PADDING_PX 16\b", text)
    assert re.search(r"\bint rtuf_set_link_padding\(rtuf_context \*ctx, int model, const float \*padding_m, int n_links\);", text)
    assert re.search(r"\bint rtuf_clear_link_padding\(rtuf_context \*ctx, int model\);", text)
    assert re.search(r"#define RTUF_ABI_VERSION 6\b", text) and R.ABI_VERSION == 6
    src = ('#include "rtuf.h"\nstatic_assert(sizeof(rtuf_params) == 48, "params");\nstatic_assert(RTUF_ABI_VERSION == 6, "abi");\n'
           'static_assert(RTUF_MAX_LINK_PADDING_PX == 16, "clamp");\n'
           'int (*a)(rtuf_context*, int, const float*, int) = rtuf_set_link_padding;\nint (*b)(rtuf_context*, int) = rtuf_clear_link_padding;\n'
           'int main() { return a && b ? 0 : 1; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    numerics = open(os.path.join(CSRC, "rtuf_numerics.h")).read()
    assert "link_padding_reach2" in numerics and "d = f / 800" in numerics and "kMaxLinkPaddingPx = 16" in numerics


def test_capi_signatures():
    for name in ("rtuf_set_link_padding", "rtuf_clear_link_padding"):
        assert name in R._capi.SYMBOLS
    assert callable(R.Context.set_link_padding) and callable(R.Context.clear_link_padding)
    lib = R.load_library()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert list(lib.rtuf_set_link_padding.argtypes) == [vp, ci, vp, ci]
    assert list(lib.rtuf_clear_link_padding.argtypes) == [vp, ci]


def _facade(entries, ignore=()):
    model = {"model": "d", "tf_prefix": "/EXAMPLE", "geometry_type": "visual", "ignore": list(ignore),
             "link_depth_distance_thresholds": entries}
    return RealtimeURDFFilter(FilterParameters("/world", "/cam", [model], 0.05), None, {"d": WL.EXAMPLE_URDF})


def test_facade_takes_a_padding_beside_or_instead_of_a_threshold():
    f = _facade([{"link": "wall1", "padding": 0.02}, {"link": "world", "threshold": 0.2, "padding": 0.05}, {"link": "wall2", "threshold": 0.1}])
    f.loadModels()                                 # (loading the models needs no GPU: the context comes after)
    rd = f.renderers_[0]
    assert rd.link_padding_ == {"wall1": 0.02, "world": 0.05} and rd.link_thresholds_ == {"world": 0.2, "wall2": 0.1}
    with pytest.raises(ValueError, match="no_such_link"):
        _facade([{"link": "no_such_link", "padding": 0.1}]).loadModels()
    with pytest.raises(KeyError):
        _facade([{"link": "wall1"}]).loadModels()      # neither value


def test_cpp_facade_header_has_the_model_field():
    src = ('#include "realtime_urdf_filter_amd/urdf_filter.hpp"\n'
           'int main() { realtime_urdf_filter::ModelParameter mp; mp.link_padding.push_back({"wall1", 0.02});\n'
           '  return (int)mp.link_padding.size() - 1; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-"],
                       input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- routes ---------------------------------------------------------------------------------------------------------------------------

def test_routes_with_padding_in_effect_are_the_table(tmp_path):
    exe = str(tmp_path / "routes_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "routes_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    # (the walk's 1,792 combinations hold the 384 with padding in effect this asserted before; field 6: the padded routes, 6 as before)
    ok = r.stdout.splitlines()[0].split()
    assert r.returncode == 0 and ok[:2] == ["ok", "1792"] and ok[6] == "6", r.stdout
    refused = set(r.stdout.splitlines()[1].split()[1:])
    assert {"Filter:LabelsPadding", "Filter:DilationPadding", "Filter:ThreshPadding", "Bits:DilationPadding", "Bits:ThreshPadding", "Render:LabelsPadding",
            "Render:RenderPadding", "Residual:ResidualPadding", "Cloud:DilationPadding", "Cloud:ThreshPadding", "Clearance:DilationPadding",
            "Clearance:ThreshPadding", "Points:PointsPadding"} == {p for p in refused if "Padding" in p}
    routes = open(os.path.join(CSRC, "rtuf_routes.h")).read()
    assert re.search(r"bool padded;[^\n]*\n\};", routes)                 # the last member: older brace lists leave it false
    assert re.search(r"enum class Post \{ None, Compare, Dilate, Pad \};", routes)
    # padding brought no new output and no new variant of the tile kernel
    assert "enum class TileOut { Planes, ZSurface, Bits, Render, Residual };" in routes
