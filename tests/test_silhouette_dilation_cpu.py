"""CPU: the silhouette dilation parameter (rtuf_params.silhouette_dilation_px) through every layer that needs no GPU: the C ABI's
layout, the header, the Python parameters and the C++ facade."""
import ctypes
import os
import re
import subprocess

from realtime_urdf_filter_amd import _capi
from realtime_urdf_filter_amd.filter import FilterParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_params_field_takes_the_place_of_reserved0():
    assert _capi.Params.silhouette_dilation_px.offset == 40
    assert _capi.Params.silhouette_dilation_px.size == 4
    assert _capi.Params.reserved.offset == 44
    assert ctypes.sizeof(_capi.Params) == 48


def test_default_params_leave_dilation_off():
    assert _capi.default_params().silhouette_dilation_px == 0


def test_header_declares_the_field_before_the_last_reserved_word():
    with open(os.path.join(ROOT, "include", "rtuf.h")) as f:
        h = f.read()
    body = h[h.index("typedef struct {\n  float near_plane;"):h.index("} rtuf_params;")]
    fields = re.findall(r"^\s+(?:uint32_t|float)\s+(\w+(?:\[\d+\])?);", body, re.M)
    assert fields[-2:] == ["silhouette_dilation_px", "reserved[1]"]


def test_filter_parameters_read_it_from_the_rosparams():
    base = {"fixed_frame": "/world", "camera_frame": "/cam", "depth_distance_threshold": 0.05}
    assert FilterParameters.from_dict(base).silhouette_dilation_px == 0
    assert FilterParameters.from_dict(dict(base, silhouette_dilation_px=3)).silhouette_dilation_px == 3


def test_ros_launch_parameters_name_it():
    with open(os.path.join(ROOT, "ros", "launch", "rtuf_filter_parameters.yaml")) as f:
        assert re.search(r"^silhouette_dilation_px: 0\b", f.read(), re.M)
    with open(os.path.join(ROOT, "ros", "include", "realtime_urdf_filter_amd_ros", "ros_filter.hpp")) as f:
        assert '{"silhouette_dilation_px", false,' in f.read()


def test_cpp_facade_compiles_with_it_set(tmp_path):
    src = tmp_path / "dilation_facade.cpp"
    src.write_text('#include "realtime_urdf_filter_amd/urdf_filter.hpp"\n'
                   "int main() {\n"
                   "  realtime_urdf_filter::FilterParameters p;\n"
                   "  p.silhouette_dilation_px = 4;\n"
                   "  rtuf_params q;\n"
                   "  rtuf_default_params(&q);\n"
                   "  q.silhouette_dilation_px = p.silhouette_dilation_px;\n"
                   "  return (int)q.reserved[0];\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
