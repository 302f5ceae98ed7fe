"""GPU (-m gpu): link clearance tables through the Python and the C++ façades (RealtimeURDFFilter) on the example scene:
clearance() and clearance_into give the rows of the C calls, which are the rows of bench_support/clearance_check.py on the
oracle's mask over the façade's own draw list, link matrices and camera."""
import os
import subprocess

import numpy as np
import pytest

from bench_support import clearance_check as KC
from bench_support import cloud_check as CC
from bench_support import workloads as WL
from gpu_support import INTR, info, example_facade, sensor_plane
from oracle import bindings as O
from realtime_urdf_filter_amd import OP_SCALE, OP_TRANSLATE
from realtime_urdf_filter_amd.geometry import bounding_spheres

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DISTANCE = 3.0

CPP = r'''
#include <cstdio>
#include <fstream>
#include <iterator>
#include "realtime_urdf_filter_amd/urdf_filter.hpp"
using namespace realtime_urdf_filter;
template <typename T> static std::vector<T> slurp(const char* path)
{
  std::ifstream f(path, std::ios::binary);
  const std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(s.size() / sizeof(T));
  memcpy(v.data(), s.data(), v.size() * sizeof(T));
  return v;
}
int main(int, char** argv)
{
  std::ifstream fx(argv[1], std::ios::binary);
  const std::string xml((std::istreambuf_iterator<char>(fx)), std::istreambuf_iterator<char>());
  const int W = 640, H = 480;
  const std::vector<float> depth = slurp<float>(argv[2]);
  const std::vector<uint16_t> mm = slurp<uint16_t>(argv[3]);
  const std::vector<int32_t> link = slurp<int32_t>(argv[4]);
  const std::vector<float> xyzr = slurp<float>(argv[5]);
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
  CameraInfo ci;
  ci.width = W; ci.height = H;
  ci.P[0] = 525.0; ci.P[5] = 520.0; ci.P[2] = 319.5; ci.P[6] = 239.5; ci.P[10] = 1;
  double P[16];
  f.getProjectionMatrix(ci, P);
  f.setLinkSpheres(0, link, xyzr);
  std::vector<rtuf_link_clearance> a(3), b(3), c(3);
  if (!f.clearance_into(depth.data(), false, P, W, H, 0.0, a.data(), 3, 3.0f)) return 1;
  if (!f.clearance_into(mm.data(), true, P, W, H, 0.0, b.data(), 3, 3.0f)) return 2;
  // a second image size and back: the new context must be given the spheres again
  ci.width = W / 2; ci.height = H / 2;
  double P2[16];
  f.getProjectionMatrix(ci, P2);
  std::vector<float> half;
  for (int y = 0; y < H; y += 2) for (int x = 0; x < W; x += 2) half.push_back(depth[(size_t)y * W + x]);
  if (!f.clearance_into(half.data(), false, P2, W / 2, H / 2, 0.0, c.data(), 3, 3.0f)) return 3;
  if (!f.clearance_into(depth.data(), false, P, W, H, 0.0, c.data(), 3, 3.0f)) return 4;
  FILE* o = fopen(argv[6], "wb");
  fwrite(a.data(), sizeof(rtuf_link_clearance), 3, o);
  fwrite(b.data(), sizeof(rtuf_link_clearance), 3, o);
  fwrite(c.data(), sizeof(rtuf_link_clearance), 3, o);
  fclose(o);
  return 0;
}
'''


def spheres_of(f):
    link, xyzr = [], []
    for li, r in enumerate(f.renderers_[0].renderables_):
        for d in r.draws:
            # (spheres live in the link's frame: the draw's glScalef / glTranslatef applied to its vertices first)
            v = np.asarray(d.verts, np.float64)
            v = v * np.asarray(d.op) if d.pre_op == OP_SCALE else (v + np.asarray(d.op) if d.pre_op == OP_TRANSLATE else v)
            for q in bounding_spheres(v, 3):
                link.append(li)
                xyzr.append(q)
    return np.array(link, np.int32), np.array(xyzr, np.float32)


def expectation(f, tf, depth, P, link, xyzr, n_labels):
    rd = f.renderers_[0]
    draws = [(r.gl_matrix(), d.pre_op, d.op, d.verts, d.tris) for r in rd.renderables_ for d in r.draws]
    offset_inv, cam_tf = f._camera_matrices(tf, None)
    _, mask = O.filter_frame(depth, P, draws, offset_inv, cam_tf, max_diff=0.05, replace_value=5.0)
    pts, idx, count = CC.compacted(depth, mask, INTR)
    assert count > 1000
    link_tf = np.stack([np.asarray(r.gl_matrix(), np.float64).reshape(16) for r in rd.renderables_])
    centres = KC.posed(link_tf, cam_tf, offset_inv, link, xyzr[:, :3])
    return KC.table(pts, idx, centres, xyzr[:, 3], [l + 1 for l in link], np.arange(len(link)), n_labels, MAX_DISTANCE)


def loaded():
    depth = sensor_plane()
    f, tf = example_facade()
    P = f.getProjectionMatrix(info())
    f.cloud(depth, P, 640, 480)                  # (loads the models and poses the links: the spheres come from the façade's draw list)
    link, xyzr = spheres_of(f)
    f.setLinkSpheres(0, link, xyzr)
    return f, tf, P, depth, link, xyzr


def test_python_facade_clearance_matches_the_c_call_and_the_expectation():
    f, tf, P, depth, link, xyzr = loaded()
    rows = f.numLinkResidualRows()
    assert rows == 3 and len(link) >= 2
    got = f.clearance(depth, P, 640, 480, MAX_DISTANCE)
    want = expectation(f, tf, depth, P, link, xyzr, rows)
    assert np.isfinite(want["clearance"]).any() and (want["points_within"] > 64).any()
    assert got.dtype == KC.DTYPE and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    direct = f._ctx.link_clearance_batch(depth[None], rows, MAX_DISTANCE)[0]
    assert np.array_equal(direct.view(np.uint32), got.view(np.uint32))
    # a second image size and back: the new context gets the spheres again
    half = np.ascontiguousarray(depth[::2, ::2])
    P2 = f.getProjectionMatrix(info(320, 240))
    # (loadModels appends the models again with every new context, as the reference's does: the table grows by their rows,
    # which stay empty -- the spheres belong to model 0 -- and rows 0 .. 2 are what they were)
    def same_rows(got, want3):
        assert len(got) == f.numLinkResidualRows() >= 3
        assert np.array_equal(got[:3].view(np.uint32), want3.view(np.uint32)), (got, want3)
        assert np.isinf(got["clearance"][3:]).all() and (got["points_within"][3:] == 0).all() and (got["sphere"][3:] == KC.NONE).all()
    same_rows(f.clearance(half, P2, 320, 240, MAX_DISTANCE), expectation(f, tf, half, P2, link, xyzr, 3))
    same_rows(f.clearance(depth, P, 640, 480, MAX_DISTANCE), want)


def test_cpp_facade_clearance_into_matches(tmp_path):
    f, tf, P, depth, link, xyzr = loaded()
    want = f.clearance(depth, P, 640, 480, MAX_DISTANCE)          # (gives the context its spheres; the C call below then agrees)
    assert np.array_equal(want.view(np.uint32), f._ctx.link_clearance_batch(depth[None], 3, MAX_DISTANCE)[0].view(np.uint32))
    assert np.array_equal(want.view(np.uint32), expectation(f, tf, depth, P, link, xyzr, 3).view(np.uint32))
    mm = np.where((depth > 0) & (depth < 65.0), depth * np.float32(1000.0), 0).astype(np.uint16)
    want_mm = f._ctx.link_clearance_batch(mm[None], 3, MAX_DISTANCE)[0]
    assert np.array_equal(want_mm.view(np.uint32), expectation(f, tf, CC.u16_to_metres(mm), P, link, xyzr, 3).view(np.uint32))
    src = tmp_path / "clearance_facade.cpp"
    src.write_text(CPP)
    exe = tmp_path / "clearance_facade"
    lib = os.path.join(ROOT, "realtime_urdf_filter_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lrtuf",
                           "-Wl,-rpath," + lib, "-o", str(exe)])
    (tmp_path / "x.urdf").write_text(WL.EXAMPLE_URDF)
    depth.tofile(tmp_path / "d.f32")
    mm.tofile(tmp_path / "d.u16")
    link.tofile(tmp_path / "link.i32")
    xyzr.tofile(tmp_path / "xyzr.f32")
    r = subprocess.run([str(exe)] + [str(tmp_path / n) for n in ("x.urdf", "d.f32", "d.u16", "link.i32", "xyzr.f32", "out.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", KC.DTYPE).reshape(3, 3)
    assert np.array_equal(raw[0].view(np.uint32), want.view(np.uint32)), (raw[0], want)
    assert np.array_equal(raw[1].view(np.uint32), want_mm.view(np.uint32))
    assert np.array_equal(raw[2].view(np.uint32), want.view(np.uint32)), "after a second image size"
