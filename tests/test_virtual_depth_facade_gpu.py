"""GPU (-m gpu): virtual depth through the Python and the C++ façades (RealtimeURDFFilter) on the example URDF: render() /
getVirtualDepth() against the oracle's winners over the façade's own draw list, render_into / getVirtualDepth() of the C++
façade against the Python result, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import golden_io
from bench_support import workloads as WL
from bench_support.labels_check import expected_labels
from bench_support.virtual_check import bits_equal_f32, expected_virtual, metres_to_u16
from gpu_support import example_facade, info
from oracle import bindings as O
from realtime_urdf_filter_amd.filter import RealtimeURDFFilter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX, FY, CX, CY = 525.0, 525.0, 319.5, 239.5
EMPTY = -2.5

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
  rtuf_host::StaticTransformProvider tf;
  for (const auto& kv : rtuf_host::forward_kinematics(rtuf_host::UrdfModel::from_string(xml))) tf.frames["/EXAMPLE/" + kv.first] = kv.second;
  tf.frames["/world"] = Transform();
  Transform cam;
  cam.m[0][0] = 1; cam.m[0][1] = 0; cam.m[0][2] = 0;
  cam.m[1][0] = 0; cam.m[1][1] = 0; cam.m[1][2] = 1;
  cam.m[2][0] = 0; cam.m[2][1] = -1; cam.m[2][2] = 0;
  tf.frames["/cam"] = cam;
  FilterParameters prm;
  prm.fixed_frame = "/world"; prm.camera_frame = "/cam"; prm.filter_replace_value = 5.0; prm.link_labels = true;
  ModelParameter mp;
  mp.model = "d"; mp.tf_prefix = "/EXAMPLE"; mp.geometry_type = "visual";
  prm.models.push_back(mp);
  RealtimeURDFFilter f(prm, tf, {{"d", xml}});
  CameraInfo info;
  info.width = W; info.height = H;
  info.P[0] = FX_; info.P[5] = FY_; info.P[2] = CX_; info.P[6] = CY_; info.P[10] = 1;
  double P[16];
  f.getProjectionMatrix(info, P);
  std::vector<float> virt((size_t)W * H, 77.0f);
  std::vector<uint16_t> mm((size_t)W * H, 0xffff), labels((size_t)W * H, 0xffff);
  if (!f.getVirtualDepth().empty()) return 2;
  if (!f.render_into(P, W, H, 0.0, virt.data(), false, EMPTY_, labels.data())) return 1;
  if (f.getVirtualDepth().size() != virt.size() || std::memcmp(f.getVirtualDepth().data(), virt.data(), virt.size() * 4) != 0) return 3;
  if (f.getLabels() != labels) return 4;
  if (!f.render_into(P, W, H, 0.0, mm.data(), true, EMPTY_)) return 5;
  std::ofstream(argv[2], std::ios::binary).write(reinterpret_cast<const char*>(virt.data()), (std::streamsize)virt.size() * 4);
  std::ofstream(argv[3], std::ios::binary).write(reinterpret_cast<const char*>(mm.data()), (std::streamsize)mm.size() * 2);
  std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char*>(labels.data()), (std::streamsize)labels.size() * 2);
  return 0;
}
'''.replace("FX_", repr(FX)).replace("FY_", repr(FY)).replace("CX_", repr(CX)).replace("CY_", repr(CY)).replace("EMPTY_", "%rf" % EMPTY)


def python_facade():
    f, tf = example_facade(labels=True)
    P = f.getProjectionMatrix(info(intr=(FX, FY, CX, CY)))
    assert f.getVirtualDepth() is None
    f.render(P, 640, 480, empty_value=EMPTY)
    return f, P, tf


def test_python_facade_renders_the_oracles_virtual_depth():
    fx = golden_io.Fixture("example_urdf_640x480")
    f, P, tf = python_facade()
    rd = f.renderers_[0]
    draws = [(r.gl_matrix(), d.pre_op, d.op, d.verts, d.tris) for r in rd.renderables_ for d in r.draws]
    links = f.getLinkLabels()
    dlab = [links[(0, r.urdf_link)] for r in rd.renderables_ for d in r.draws]
    offset_inv, cam_tf = f._camera_matrices(tf, None)
    _, _, zwin, prim, _ = O.filter_frame(fx.depth, P, draws, offset_inv, cam_tf, max_diff=0.05, replace_value=5.0, want_debug=True)
    assert (prim >= 0).any()
    assert bits_equal_f32(f.getVirtualDepth(), expected_virtual(zwin, prim, f.near_plane_, f.far_plane_, EMPTY))
    assert np.array_equal(f.getLabels(), expected_labels(prim, dlab, [len(d[4]) for d in draws]))
    # the same render through a façade without labels
    g = RealtimeURDFFilter(f.params, tf, {"d": WL.EXAMPLE_URDF})
    g.render(P, 640, 480, empty_value=EMPTY)
    assert bits_equal_f32(g.getVirtualDepth(), f.getVirtualDepth()) and g.getLabels() is None


def test_cpp_facade_render_into_matches_the_python_facade(tmp_path):
    f, _, _ = python_facade()
    src = tmp_path / "virtual_facade.cpp"
    src.write_text("#include <cstring>\n" + CPP)
    exe = tmp_path / "virtual_facade"
    lib = os.path.join(ROOT, "realtime_urdf_filter_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lrtuf",
                           "-Wl,-rpath," + lib, "-o", str(exe)])
    (tmp_path / "x.urdf").write_text(WL.EXAMPLE_URDF)
    r = subprocess.run([str(exe), str(tmp_path / "x.urdf"), str(tmp_path / "v.f32"), str(tmp_path / "v.u16"), str(tmp_path / "l.u16")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    virt = np.fromfile(tmp_path / "v.f32", np.float32).reshape(480, 640)
    assert bits_equal_f32(virt, f.getVirtualDepth())
    assert np.array_equal(np.fromfile(tmp_path / "v.u16", np.uint16).reshape(480, 640), metres_to_u16(f.getVirtualDepth()))
    assert np.array_equal(np.fromfile(tmp_path / "l.u16", np.uint16).reshape(480, 640), f.getLabels())
