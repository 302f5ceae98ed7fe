"""GPU (-m gpu): point list batches through the Python and the C++ façades (RealtimeURDFFilter) on the example scene:
filter_points() and points_into against bench_support/points_check.py on the virtual depth plane of the CPU oracle, for
equality: verdicts, pixels and summary."""
import os
import subprocess

import numpy as np
import pytest

from bench_support import cloud_check as CC
from bench_support import points_check as PC
from bench_support import workloads as WL
from bench_support.virtual_check import expected_virtual
from gpu_support import INTR, example_facade, info, oracle_frames, sensor_plane

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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
  const uint32_t count = (uint32_t)atoi(argv[4]);
  std::vector<float> points((size_t)count * 3);
  std::ifstream(argv[2], std::ios::binary).read(reinterpret_cast<char*>(points.data()), (std::streamsize)points.size() * 4);
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
  RealtimeURDFFilter f(prm, tf, {{"d", xml}});
  CameraInfo info;
  info.width = W; info.height = H;
  info.P[0] = intr[0]; info.P[5] = intr[1]; info.P[2] = intr[2]; info.P[6] = intr[3]; info.P[10] = 1;
  double P[16];
  f.getProjectionMatrix(info, P);
  FILE* o = fopen(argv[5], "wb");
  for (int r = 0; r <= 2; r += 2) {
    std::vector<uint8_t> verdict(count, 0x5a);
    std::vector<uint32_t> pixel(count, 0x5a5a5a5au);
    uint32_t summary[4] = {0, 0, 0, 0};
    if (!f.points_into(points.data(), count, P, W, H, 0.0, verdict.data(), pixel.data(), summary, r)) return 1 + r;
    fwrite(verdict.data(), 1, verdict.size(), o);
    fwrite(pixel.data(), 4, pixel.size(), o);
    fwrite(summary, 4, 4, o);
  }
  std::vector<uint8_t> only(count, 0x5a);
  if (!f.points_into(points.data(), count, P, W, H, 0.0, only.data())) return 5;      // (no pixels, no summary, radius 0)
  fwrite(only.data(), 1, only.size(), o);
  fclose(o);
  return 0;
}
'''


def facade_virtual(f, tf, P):
    """The oracle's virtual depth plane (+inf where no link drew) over the façade's own draw list and camera."""
    rd = f.renderers_[0]
    draws = [(r.gl_matrix(), d.pre_op, d.op, d.verts, d.tris) for r in rd.renderables_ for d in r.draws]
    offset_inv, cam_tf = f._camera_matrices(tf, None)
    zwin, prim = oracle_frames([(P, draws, offset_inv, cam_tf, f.near_plane_, f.far_plane_)], np.zeros((1, 480, 640), np.float32))
    return expected_virtual(zwin[0], prim[0], f.near_plane_, f.far_plane_, np.inf)


def example_points():
    """The sensor plane's own points, every third pixel, then the edge values and a box of random points."""
    depth = sensor_plane()
    grid = CC.points(depth, INTR).reshape(-1, 3)[::3]
    return np.ascontiguousarray(np.concatenate([grid, PC.edge_points(), PC.random_points(np.random.default_rng(5), 5000)]), np.float32)


def expectation(f, tf, P, pts):
    f.filter_points(pts[:16], P, 640, 480)       # (loads the models and poses the links: the expectation reads the façade's draw list)
    virt = facade_virtual(f, tf, P)
    ex = {r: PC.verdicts(pts, INTR, virt, 0.05, r) for r in (0, 2)}
    for r in ex:
        assert all(c > 200 for c in PC.summary(ex[r][0])[:3]), PC.summary(ex[r][0])
    assert not np.array_equal(ex[0][0], ex[2][0])
    return ex


def test_python_facade_filter_points_matches_the_expectation():
    pts = example_points()
    f, tf = example_facade()
    P = f.getProjectionMatrix(info())
    ex = expectation(f, tf, P, pts)
    for r in (0, 2):
        verdict, pixel, summary = f.filter_points(pts, P, 640, 480, radius_px=r)
        assert np.array_equal(verdict, ex[r][0]) and np.array_equal(pixel, ex[r][1]), "r=%d" % r
        assert summary.tolist() == PC.summary(ex[r][0]).tolist()
    # filter() on the same façade still works, and a cloud's points fed back are all kept
    depth = sensor_plane()
    cloud, index = f.cloud(depth, P, 640, 480, compact=True)
    verdict, pixel, summary = f.filter_points(cloud, P, 640, 480)
    assert len(cloud) > 1000 and (verdict == PC.KEPT).all() and np.array_equal(pixel, index)


def test_cpp_facade_points_into_matches_the_expectation(tmp_path):
    pts = example_points()
    f, tf = example_facade()
    P = f.getProjectionMatrix(info())
    ex = expectation(f, tf, P, pts)
    src = tmp_path / "points_facade.cpp"
    src.write_text(CPP)
    exe = tmp_path / "points_facade"
    lib = os.path.join(ROOT, "realtime_urdf_filter_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lrtuf",
                           "-Wl,-rpath," + lib, "-o", str(exe)])
    (tmp_path / "x.urdf").write_text(WL.EXAMPLE_URDF)
    pts.tofile(tmp_path / "p.f32")
    np.asarray(INTR, np.float64).tofile(tmp_path / "k.f64")
    r = subprocess.run([str(exe), str(tmp_path / "x.urdf"), str(tmp_path / "p.f32"), str(tmp_path / "k.f64"), str(len(pts)), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    n = len(pts)
    per = n + 4 * n + 16
    assert raw.size == 2 * per + n
    for i, rad in enumerate((0, 2)):
        part = raw[i * per:(i + 1) * per]
        assert np.array_equal(part[:n], ex[rad][0]), "r=%d verdicts" % rad
        assert np.array_equal(part[n:5 * n].copy().view(np.uint32), ex[rad][1]), "r=%d pixels" % rad
        assert part[5 * n:].copy().view(np.uint32).tolist() == PC.summary(ex[rad][0]).tolist()
    assert np.array_equal(raw[2 * per:], ex[0][0])
