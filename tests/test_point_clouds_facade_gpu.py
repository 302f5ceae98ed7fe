"""GPU (-m gpu): filtered point clouds through the Python and the C++ façades (RealtimeURDFFilter) on the example scene:
cloud() and cloud_into against bench_support/cloud_check.py on the mask the dilation tests expect (the CPU oracle's), organized
planes as uint32 bit patterns, compacted output for equality together with count and index."""
import os
import subprocess

import numpy as np
import pytest

from bench_support import cloud_check as CC
from bench_support import workloads as WL
from gpu_support import INTR, info, example_facade, sensor_plane

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CPP = r'''
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include "realtime_urdf_filter_amd/urdf_filter.hpp"
using namespace realtime_urdf_filter;
static std::vector<float> plane(const std::vector<float>& d, int W, int step)      // every step-th pixel of every step-th row
{
  std::vector<float> o;
  for (int y = 0; y < 480; y += step) for (int x = 0; x < W; x += step) o.push_back(d[(size_t)y * W + x]);
  return o;
}
int main(int argc, char** argv)
{
  std::ifstream fx(argv[1], std::ios::binary);
  const std::string xml((std::istreambuf_iterator<char>(fx)), std::istreambuf_iterator<char>());
  const int W = 640, H = 480;
  std::vector<float> depth((size_t)W * H);
  std::ifstream(argv[2], std::ios::binary).read(reinterpret_cast<char*>(depth.data()), (std::streamsize)depth.size() * 4);
  double intr[4];
  std::ifstream(argv[3], std::ios::binary).read(reinterpret_cast<char*>(intr), sizeof intr);
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
  prm.models.push_back(mp);
  FILE* o = fopen(argv[5], "wb");
  {
    RealtimeURDFFilter f(prm, tf, {{"d", xml}});
    CameraInfo info;
    info.width = W; info.height = H;
    info.P[0] = intr[0]; info.P[5] = intr[1]; info.P[2] = intr[2]; info.P[6] = intr[3]; info.P[10] = 1;
    double P[16];
    f.getProjectionMatrix(info, P);
    std::vector<float> org((size_t)W * H * 3), comp((size_t)1000 * 3);
    std::vector<uint32_t> index(1000);
    uint32_t count = 0;
    if (!f.cloud_into(depth.data(), false, P, W, H, 0.0, org.data())) return 1;
    if (!f.cloud_into(depth.data(), false, P, W, H, 0.0, comp.data(), index.data(), &count, 1000)) return 2;
    std::vector<uint16_t> mm(depth.size());
    std::ifstream(argv[4], std::ios::binary).read(reinterpret_cast<char*>(mm.data()), (std::streamsize)mm.size() * 2);
    std::vector<float> org_mm((size_t)W * H * 3);
    if (!f.cloud_into(mm.data(), true, P, W, H, 0.0, org_mm.data())) return 3;
    // a second image size with the same intrinsics: the façade makes a new context, which must be given them again
    info.width = W / 2; info.height = H / 2;
    double P2[16];
    f.getProjectionMatrix(info, P2);
    const std::vector<float> half = plane(depth, W, 2);
    std::vector<float> org_half(half.size() * 3);
    if (!f.cloud_into(half.data(), false, P2, W / 2, H / 2, 0.0, org_half.data())) return 4;
    if (!f.cloud_into(depth.data(), false, P, W, H, 0.0, org.data())) return 5;      // ... and back
    fwrite(&count, sizeof count, 1, o);
    fwrite(org.data(), 4, org.size(), o);
    fwrite(comp.data(), 4, comp.size(), o);
    fwrite(index.data(), 4, index.size(), o);
    fwrite(org_mm.data(), 4, org_mm.size(), o);
    fwrite(org_half.data(), 4, org_half.size(), o);
  }
  {
    // use_own_calibration: the CameraInfo's P is ignored, the intrinsics are own_calibration rounded to float
    prm.use_own_calibration = true;
    RealtimeURDFFilter f(prm, tf, {{"d", xml}});
    CameraInfo info;
    info.width = W; info.height = H;
    info.P[0] = 100; info.P[5] = 100; info.P[2] = 1; info.P[6] = 1; info.P[10] = 1;
    double P[16];
    f.getProjectionMatrix(info, P);
    std::vector<float> org((size_t)W * H * 3);
    if (!f.cloud_into(depth.data(), false, P, W, H, 0.0, org.data())) return 6;
    fwrite(org.data(), 4, org.size(), o);
  }
  fclose(o);
  return 0;
}
'''


def facade_expectation(f, tf, depth, P, intr):
    """The oracle's mask over the façade's own draw list and camera, and cloud_check on it."""
    from oracle import bindings as O
    rd = f.renderers_[0]
    draws = [(r.gl_matrix(), d.pre_op, d.op, d.verts, d.tris) for r in rd.renderables_ for d in r.draws]
    offset_inv, cam_tf = f._camera_matrices(tf, None)
    _, mask = O.filter_frame(depth, P, draws, offset_inv, cam_tf, max_diff=0.05, replace_value=5.0)
    k, fl, inv = CC.classes(depth, mask)
    assert k > 0 and fl > 0 and inv > 0, (k, fl, inv)
    return CC.organized(depth, mask, intr), CC.compacted(depth, mask, intr)


def test_python_facade_cloud_matches_the_expectation():
    depth = sensor_plane()
    f, tf = example_facade()
    P = f.getProjectionMatrix(info())
    first = f.cloud(depth, P, 640, 480)          # (loads the models and poses the links: the expectation reads the façade's draw list)
    org, (pts, idx, count) = facade_expectation(f, tf, depth, P, INTR)
    got = f.cloud(depth, P, 640, 480)
    assert np.array_equal(got.view(np.uint32), first.view(np.uint32))
    assert got.shape == (480, 640, 3) and np.array_equal(got.view(np.uint32), org.view(np.uint32))
    gp, gi = f.cloud(depth, P, 640, 480, compact=True)
    assert len(gp) == count and np.array_equal(gp.view(np.uint32), pts.view(np.uint32)) and np.array_equal(gi, idx)
    mm = np.where((depth > 0) & (depth < 65.0), depth * np.float32(1000.0), 0).astype(np.uint16)
    org_mm, _ = facade_expectation(f, tf, CC.u16_to_metres(mm), P, INTR)
    assert np.array_equal(f.cloud(mm, P, 640, 480).view(np.uint32), org_mm.view(np.uint32))


OWN = (585.260, 585.028, 317.387, 239.264)      # (none of them a float)
OWN_F = tuple(float(np.float32(v)) for v in OWN)


def test_python_facade_cloud_at_a_second_image_size():
    """The same intrinsics at 320 x 240: the façade makes a new context, which must be given the intrinsics again."""
    depth = sensor_plane()
    half = np.ascontiguousarray(depth[::2, ::2])
    f, tf = example_facade()
    P = f.getProjectionMatrix(info())
    first = f.cloud(depth, P, 640, 480)
    P2 = f.getProjectionMatrix(info(320, 240))
    got = f.cloud(half, P2, 320, 240)
    org, _ = facade_expectation(f, tf, half, P2, INTR)
    assert got.shape == (240, 320, 3) and np.array_equal(got.view(np.uint32), org.view(np.uint32))
    again = f.cloud(depth, P, 640, 480)
    assert np.array_equal(again.view(np.uint32), first.view(np.uint32))


def test_python_facade_own_calibration_counts_as_floats():
    depth = sensor_plane()
    f, tf = example_facade(use_own_calibration=True, own_calibration=OWN)
    P = f.getProjectionMatrix(info(intr=(100.0, 100.0, 1.0, 1.0)))          # (the camera info's intrinsics are ignored)
    got = f.cloud(depth, P, 640, 480)
    assert OWN_F != OWN and f.cloud_intrinsics_ == OWN_F
    org, _ = facade_expectation(f, tf, depth, P, OWN_F)
    assert np.array_equal(got.view(np.uint32), org.view(np.uint32))


def test_cpp_facade_cloud_into_matches_the_expectation(tmp_path):
    depth = sensor_plane()
    f, tf = example_facade()
    P = f.getProjectionMatrix(info())
    first = f.cloud(depth, P, 640, 480)          # (loads the models and poses the links: the expectation reads the façade's draw list)
    org, (pts, idx, count) = facade_expectation(f, tf, depth, P, INTR)
    mm = np.where((depth > 0) & (depth < 65.0), depth * np.float32(1000.0), 0).astype(np.uint16)
    org_mm, _ = facade_expectation(f, tf, CC.u16_to_metres(mm), P, INTR)
    half = np.ascontiguousarray(depth[::2, ::2])
    P2 = f.getProjectionMatrix(info(320, 240))
    f.cloud(half, P2, 320, 240)
    org_half, _ = facade_expectation(f, tf, half, P2, INTR)
    g, tfg = example_facade(use_own_calibration=True, own_calibration=OWN)
    Pg = g.getProjectionMatrix(info())
    g.cloud(depth, Pg, 640, 480)
    org_own, _ = facade_expectation(g, tfg, depth, Pg, OWN_F)
    src = tmp_path / "cloud_facade.cpp"
    src.write_text(CPP)
    exe = tmp_path / "cloud_facade"
    lib = os.path.join(ROOT, "realtime_urdf_filter_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lrtuf",
                           "-Wl,-rpath," + lib, "-o", str(exe)])
    (tmp_path / "x.urdf").write_text(WL.EXAMPLE_URDF)
    depth.tofile(tmp_path / "d.f32")
    mm.tofile(tmp_path / "d.u16")
    np.asarray(INTR, np.float64).tofile(tmp_path / "p.f64")
    r = subprocess.run([str(exe), str(tmp_path / "x.urdf"), str(tmp_path / "d.f32"), str(tmp_path / "p.f64"), str(tmp_path / "d.u16"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.uint32)
    px = 640 * 480 * 3
    assert int(raw[0]) == count and count > 1000
    parts = np.split(raw[1:], np.cumsum([px, 3000, 1000, px, px // 4]))
    assert len(parts) == 6 and len(parts[5]) == px
    assert np.array_equal(parts[0], org.view(np.uint32).ravel()) and np.array_equal(parts[0], first.view(np.uint32).ravel())
    assert np.array_equal(parts[1], pts[:1000].view(np.uint32).ravel())
    assert np.array_equal(parts[2], idx[:1000])
    assert np.array_equal(parts[3], org_mm.view(np.uint32).ravel())
    assert np.array_equal(parts[4], org_half.view(np.uint32).ravel()), "second image size"
    assert np.array_equal(parts[5], org_own.view(np.uint32).ravel()), "own calibration"
