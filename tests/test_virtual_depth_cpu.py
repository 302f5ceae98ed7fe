"""CPU: the virtual depth entry points' place in the ABI, and the expectation the GPU tests use (bench_support/
virtual_check.py) against the CPU oracle: thresholding the expected virtual depth reproduces the oracle's mask, so its
arithmetic is the oracle's; its metres_to_u16 reproduces the 16UC1 outputs of the fixtures."""
import ctypes
import os

import numpy as np
import pytest

import golden_io
import realtime_urdf_filter_amd as R
from bench_support.virtual_check import bits_equal_f32, expected_virtual, expected_virtual_u16, metres_to_u16
from oracle import bindings as O
from realtime_urdf_filter_amd.filter import RealtimeURDFFilter, depth_f32_to_u16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtuf.h")
RENDER_CALLS = ("rtuf_render_batch_device", "rtuf_render_batch_device_u16", "rtuf_render_batch", "rtuf_render_batch_u16")
FIXTURES = [n for n in golden_io.fixture_names() if n.endswith("_160x120")]


def test_render_entry_points_are_declared_exported_and_bound():
    text = open(HEADER).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "realtime_urdf_filter_amd", "lib", "librtuf.so"))
    for name in RENDER_CALLS:
        assert name + "(" in text and name in R._capi.SYMBOLS, name
        assert getattr(lib, name) is not None
    assert "VIRTUAL DEPTH" in text
    for name in ("render_batch", "render_batch_device", "render_batch_device_u16"):
        assert callable(getattr(R.Context, name)), name
    for name in ("render", "getVirtualDepth"):
        assert callable(getattr(RealtimeURDFFilter, name)), name
    # no struct change
    assert "#define RTUF_ABI_VERSION 6" in text
    assert ctypes.sizeof(R._capi.Params) == 48 and ctypes.sizeof(R._capi.Stats) == 248


@pytest.mark.parametrize("name", FIXTURES)
def test_thresholding_the_expected_virtual_depth_gives_the_oracles_mask(name):
    fx = golden_io.Fixture(name)
    masked, mask, zwin, prim, _ = O.filter_frame(fx.depth, fx.projection, fx.draws, fx.offset_inv, fx.cam_tf, z_near=fx.z_near, z_far=fx.z_far,
                                                 max_diff=fx.max_diff, replace_value=fx.replace_value, want_debug=True)
    drawn = prim >= 0
    virt = expected_virtual(zwin, prim, fx.z_near, fx.z_far, np.nan)
    assert np.isnan(virt[~drawn]).all()
    with np.errstate(invalid="ignore"):
        filt = fx.depth > (virt - np.float32(fx.max_diff)).astype(np.float32)
    assert np.array_equal(filt[drawn], mask[drawn] == 255)
    # the 16UC1 conversion: the fixture's masked plane (replace value where filtered) as the 16UC1 calls deliver it
    assert np.array_equal(metres_to_u16(masked)[drawn], depth_f32_to_u16(fx.expected_masked())[drawn])
    assert np.array_equal(metres_to_u16(np.float32(fx.replace_value)), depth_f32_to_u16(np.float32(fx.replace_value)))


def test_expectation_forms_and_edge_values():
    zwin = np.array([[0.75, 0.9, 0.5]], np.float32)
    prim = np.array([[3, -2, -1]], np.int32)
    v = expected_virtual(zwin, prim, 0.1, 8.0, -1.5)
    f = np.float32
    num, off = (f(0.1) * f(8.0)) / (f(0.1) - f(8.0)), f(8.0) / (f(8.0) - f(0.1))
    assert v.dtype == np.float32 and v[0, 0] == f(num) / (f(0.75) - f(off)) and v[0, 1] == v[0, 2] == f(-1.5)
    assert expected_virtual_u16(zwin, prim, 0.1, 8.0, -1.5).tolist() == [[int(metres_to_u16(v[0, 0])), 0, 0]]
    edge = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0004, 1.2344, 65.0, 70.0, 3e9], np.float32)
    assert metres_to_u16(edge).tolist() == [0, 0, 0, 0, 0, 1234, 65000, 65535, 0]
    assert bits_equal_f32(np.array([np.nan, 1.0], np.float32), np.array([-np.nan, 1.0], np.float32))
    assert not bits_equal_f32(np.array([0.0], np.float32), np.array([-0.0], np.float32))
