"""GPU (-m gpu): per-link depth thresholds through the Python and the C++ façades and the ROS adapter, keyed by URDF link name
(a model entry's link_depth_distance_thresholds), on the example URDF: the outputs agree with the oracle's winners mapped
through URDF link -> threshold and with each other; an unknown link name is an error at load."""
import os
import subprocess

import numpy as np
import pytest

import golden_io
from bench_support import workloads as WL
from bench_support.link_thresholds_check import expected_planes
from gpu_support import example_facade, example_transforms, info
from oracle import bindings as O
from realtime_urdf_filter_amd.filter import CameraInfo, FilterParameters, RealtimeURDFFilter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX, FY, CX, CY = 525.0, 525.0, 319.5, 239.5
WALL1 = 0.75                                  # a wide margin for wall1; wall2 keeps the global 0.05

CPP = r'''
#include <cstdio>
#include <fstream>
#include <iterator>
#include "realtime_urdf_filter_amd/urdf_filter.hpp"
using namespace realtime_urdf_filter;
int main(int argc, char** argv)
{
  std::ifstream fx(argv[1], std::ios::binary), fd(argv[2], std::ios::binary);
  const std::string xml((std::istreambuf_iterator<char>(fx)), std::istreambuf_iterator<char>());
  std::string depth((std::istreambuf_iterator<char>(fd)), std::istreambuf_iterator<char>());
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
  prm.fixed_frame = "/world"; prm.camera_frame = "/cam"; prm.filter_replace_value = 5.0;
  ModelParameter mp;
  mp.model = "d"; mp.tf_prefix = "/EXAMPLE"; mp.geometry_type = "visual";
  mp.link_depth_distance_thresholds = {{"wall1", WALL1_}, {"world", 3.0}};        // (world: no geometry, no effect)
  if (argc > 4) mp.link_depth_distance_thresholds.push_back({argv[4], 0.1});
  prm.models.push_back(mp);
  try {
    RealtimeURDFFilter f(prm, tf, {{"d", xml}});
    CameraInfo info;
    info.width = W; info.height = H;
    info.P[0] = FX_; info.P[5] = FY_; info.P[2] = CX_; info.P[6] = CY_; info.P[10] = 1;
    double P[16];
    f.getProjectionMatrix(info, P);
    std::vector<float> masked((size_t)W * H);
    std::vector<uint8_t> mask((size_t)W * H);
    if (!f.filter_into(depth.data(), false, P, W, H, 0.0, masked.data(), mask.data())) return 1;
    std::ofstream(argv[3], std::ios::binary).write(reinterpret_cast<const char*>(mask.data()), (std::streamsize)mask.size());
  } catch (const std::exception& e) {
    std::printf("error %s\n", e.what());
    return 3;
  }
  return 0;
}
'''.replace("FX_", repr(FX)).replace("FY_", repr(FY)).replace("CX_", repr(CX)).replace("CY_", repr(CY)).replace("WALL1_", repr(WALL1))


def python_facade(depth, entries):
    f, tf = example_facade(model_entries={"link_depth_distance_thresholds": entries})
    ci = info(intr=(FX, FY, CX, CY))
    out, mask = f.filter_callback(depth, "32FC1", ci)
    return f, out, mask, f.getProjectionMatrix(ci), tf


def _depth():
    """The example fixture's sensor plane, pulled 0.3 m towards the camera on its upper half: there wall1's wide margin
    filters what the global one keeps."""
    d = golden_io.Fixture("example_urdf_640x480").depth.copy()
    d[:240] -= np.float32(0.3)
    return d


def expected(f, depth, P, tf, thr_of_link):
    rd = f.renderers_[0]
    draws = [(r.gl_matrix(), d.pre_op, d.op, d.verts, d.tris) for r in rd.renderables_ for d in r.draws]
    dthr = [thr_of_link.get(r.urdf_link, 0.05) for r in rd.renderables_ for d in r.draws]
    offset_inv, cam_tf = f._camera_matrices(tf, None)
    _, _, zwin, prim, _ = O.filter_frame(depth, P, draws, offset_inv, cam_tf, max_diff=0.05, replace_value=5.0, want_debug=True)
    return expected_planes(zwin, prim, depth, dthr, [len(d[4]) for d in draws], 0.05, 0.1, 8.0, 5.0)


def test_python_facade_per_link_thresholds():
    depth = _depth()
    f, out, mask, P, tf = python_facade(depth, [{"link": "wall1", "threshold": WALL1}, {"link": "world", "threshold": 3.0}])
    wm, wk = expected(f, depth, P, tf, {"wall1": WALL1})
    assert np.array_equal(mask, wk), int((mask != wk).sum())
    assert np.array_equal(out.view(np.uint32), wm.view(np.uint32))
    _, k0 = expected(f, depth, P, tf, {})
    assert (wk != k0).sum() > 1000                            # (the wide margin shows)
    # an entry for a link on the ignore list is accepted and has no effect
    tf2 = example_transforms()
    model = {"model": "d", "tf_prefix": "/EXAMPLE", "geometry_type": "visual", "ignore": ["wall2"],
             "link_depth_distance_thresholds": [{"link": "wall2", "threshold": 9.0}]}
    g = RealtimeURDFFilter(FilterParameters("/world", "/cam", [model], 0.05, filter_replace_value=5.0), tf2, {"d": WL.EXAMPLE_URDF})
    g.filter_callback(depth, "32FC1", CameraInfo(640, 480, [FX, 0, CX, 0, 0, FY, CY, 0, 0, 0, 1, 0]))
    # an unknown link name is an error at load
    with pytest.raises(ValueError):
        python_facade(depth, [{"link": "no_such_link", "threshold": 0.1}])


def test_cpp_facade_matches_the_python_facade(tmp_path):
    depth = _depth()
    _, _, mask, _, _ = python_facade(depth, [{"link": "wall1", "threshold": WALL1}])
    src = tmp_path / "thr_facade.cpp"
    src.write_text(CPP)
    exe = tmp_path / "thr_facade"
    lib = os.path.join(ROOT, "realtime_urdf_filter_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lrtuf",
                           "-Wl,-rpath," + lib, "-o", str(exe)])
    (tmp_path / "x.urdf").write_text(WL.EXAMPLE_URDF)
    np.ascontiguousarray(depth, np.float32).tofile(tmp_path / "d.f32")
    r = subprocess.run([str(exe), str(tmp_path / "x.urdf"), str(tmp_path / "d.f32"), str(tmp_path / "m.u8")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "m.u8", np.uint8).reshape(480, 640)
    assert np.array_equal(got, mask), int((got != mask).sum())
    r = subprocess.run([str(exe), str(tmp_path / "x.urdf"), str(tmp_path / "d.f32"), str(tmp_path / "m2.u8"), "no_such_link"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 3 and "no_such_link" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_ros_adapter_on_frame_with_a_per_link_entry(tmp_path):
    exe = os.path.join(ROOT, "examples", "bin", "ros_link_thresholds_harness")
    if not os.path.exists(exe):
        subprocess.check_call([os.path.join(ROOT, "realtime_urdf_filter_amd", "csrc", "build_facade.sh")])
    depth = _depth()
    (tmp_path / "m.urdf").write_text(WL.EXAMPLE_URDF)
    np.ascontiguousarray(depth, np.float32).tofile(tmp_path / "d.bin")
    cmd = [exe, str(tmp_path / "m.urdf"), str(tmp_path / "d.bin"), "640", "480", "525", "525", "319.5", "239.5", "5.0",
           str(tmp_path / "o.depth"), str(tmp_path / "o.mask"), "wall1", repr(WALL1)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    _, out, mask, _, _ = python_facade(depth, [{"link": "wall1", "threshold": WALL1}])
    got_k = np.fromfile(tmp_path / "o.mask", np.uint8).reshape(480, 640)
    got_m = np.fromfile(tmp_path / "o.depth", np.float32).reshape(480, 640)
    assert np.array_equal(got_k, mask), int((got_k != mask).sum())
    assert np.array_equal(got_m.view(np.uint32), out.view(np.uint32))
