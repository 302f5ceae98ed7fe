"""GPU (-m gpu): link residual tables through the Python and the C++ façades (RealtimeURDFFilter) on the example URDF:
link_residuals() against the oracle's winners over the façade's own draw list and against the device call on the façade's
context, link_residuals_into of the C++ façade against the Python result.  Tables are compared for equality."""
import os
import subprocess

import numpy as np
import pytest

import golden_io
from bench_support import workloads as WL
from bench_support.residuals_check import ROW, expected_table
from gpu_support import check_tables, example_facade, info
from oracle import bindings as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX, FY, CX, CY = 525.0, 525.0, 319.5, 239.5

CPP = r'''
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include "realtime_urdf_filter_amd/urdf_filter.hpp"
using namespace realtime_urdf_filter;
int main(int argc, char** argv)
{
  std::ifstream fx(argv[1], std::ios::binary);
  const std::string xml((std::istreambuf_iterator<char>(fx)), std::istreambuf_iterator<char>());
  const int W = 640, H = 480;
  std::vector<float> depth((size_t)W * H);
  std::ifstream(argv[2], std::ios::binary).read(reinterpret_cast<char*>(depth.data()), (std::streamsize)depth.size() * 4);
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
  std::vector<rtuf_link_residuals> table(64);
  std::memset(table.data(), 0x5a, table.size() * sizeof(rtuf_link_residuals));
  if (!f.link_residuals_into(depth.data(), false, P, W, H, 0.0, table.data(), 64)) return 1;
  const int rows = f.numLinkResidualRows();
  if (rows < 2 || rows > 64) return 2;
  std::vector<uint16_t> mm(depth.size());
  for (size_t i = 0; i < mm.size(); i++) mm[i] = (uint16_t)(depth[i] > 0 && depth[i] < 65.0f ? depth[i] * 1000.0f : 0.0f);
  std::vector<rtuf_link_residuals> table_mm((size_t)rows);
  if (!f.link_residuals_into(mm.data(), true, P, W, H, 0.0, table_mm.data(), rows)) return 3;
  FILE* o = fopen(argv[3], "wb");
  fwrite(&rows, sizeof rows, 1, o);
  fwrite(table.data(), sizeof(rtuf_link_residuals), 64, o);
  fwrite(table_mm.data(), sizeof(rtuf_link_residuals), (size_t)rows, o);
  fclose(o);
  return 0;
}
'''.replace("FX_", repr(FX)).replace("FY_", repr(FY)).replace("CX_", repr(CX)).replace("CY_", repr(CY))


def python_facade(labels=True):
    f, tf = example_facade(labels=labels)
    return f, f.getProjectionMatrix(info(intr=(FX, FY, CX, CY))), tf


def sensor_plane():
    fx = golden_io.Fixture("example_urdf_640x480")
    d = np.ascontiguousarray(fx.depth, np.float32).copy()
    d[::9, ::4] = np.nan
    d[5::13, 2::7] = 0.0
    return d


def test_python_facade_against_the_oracle_and_the_device_call():
    import torch
    depth = sensor_plane()
    f, P, tf = python_facade()
    tab = f.link_residuals(depth, P, 640, 480)
    rows = f.numLinkResidualRows()
    assert tab.shape == (rows,) and tab.dtype == ROW and rows == len(f.getLinkLabels()) + 1
    rd = f.renderers_[0]
    draws = [(r.gl_matrix(), d.pre_op, d.op, d.verts, d.tris) for r in rd.renderables_ for d in r.draws]
    links = f.getLinkLabels()
    dlab = [links[(0, r.urdf_link)] for r in rd.renderables_ for d in r.draws]
    offset_inv, cam_tf = f._camera_matrices(tf, None)
    _, _, zwin, prim, _ = O.filter_frame(depth, P, draws, offset_inv, cam_tf, max_diff=0.05, replace_value=5.0, want_debug=True)
    want = expected_table(zwin, prim, depth, dlab, [len(d[4]) for d in draws], None, 0.05, f.near_plane_, f.far_plane_, rows)
    check_tables(tab, want, "python facade")
    assert tab["pixels"].sum() == 640 * 480 and (tab["pixels"][1:] > 0).any() and tab["agree"].sum() > 0 and tab["invalid"].sum() > 0
    # the device call on the facade's own context, staged by the facade
    dev = torch.device("cuda:0")
    d = torch.from_numpy(depth[None]).to(dev)
    table = torch.full((1, rows, 8), -1, dtype=torch.int64, device=dev)
    f._ctx.link_residuals_batch_device(1, d.data_ptr(), table.data_ptr(), rows)
    f._ctx.sync()
    check_tables(np.ascontiguousarray(table.cpu().numpy()).view(ROW).reshape(rows), want, "device call")
    # 16UC1 input
    mm = np.where((depth > 0) & (depth < 65.0), depth * np.float32(1000.0), 0).astype(np.uint16)
    want_mm = expected_table(zwin, prim, mm.astype(np.float32) * np.float32(0.001), dlab, [len(d[4]) for d in draws], None, 0.05, f.near_plane_,
                             f.far_plane_, rows)
    check_tables(f.link_residuals(mm, P, 640, 480), want_mm, "python facade 16UC1")
    # a facade without labels: default labels, one row per renderable
    g, _, _ = python_facade(labels=False)
    tab_g = g.link_residuals(depth, P, 640, 480)
    assert tab_g.shape == (sum(len(r.renderables_) for r in g.renderers_) + 1,)
    assert tab_g["pixels"].sum() == 640 * 480 and tab_g[0] == tab[0]


def test_cpp_facade_link_residuals_into_matches_the_python_facade(tmp_path):
    depth = sensor_plane()
    f, P, _ = python_facade()
    tab = f.link_residuals(depth, P, 640, 480)
    mm = np.where((depth > 0) & (depth < 65.0), depth * np.float32(1000.0), 0).astype(np.uint16)
    tab_mm = f.link_residuals(mm, P, 640, 480)
    src = tmp_path / "residuals_facade.cpp"
    src.write_text(CPP)
    exe = tmp_path / "residuals_facade"
    lib = os.path.join(ROOT, "realtime_urdf_filter_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lrtuf",
                           "-Wl,-rpath," + lib, "-o", str(exe)])
    (tmp_path / "x.urdf").write_text(WL.EXAMPLE_URDF)
    depth.tofile(tmp_path / "d.f32")
    r = subprocess.run([str(exe), str(tmp_path / "x.urdf"), str(tmp_path / "d.f32"), str(tmp_path / "t.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(tmp_path / "t.bin", "rb").read()
    rows = int(np.frombuffer(raw[:4], np.int32)[0])
    assert rows == len(tab)
    big = np.frombuffer(raw[4:4 + 64 * 64], ROW)
    check_tables(big[:rows], tab, "C++ facade f32")
    assert not np.ascontiguousarray(big[rows:]).view(np.uint64).any()          # spare rows are zeroed
    check_tables(np.frombuffer(raw[4 + 64 * 64:], ROW), tab_mm, "C++ facade 16UC1")
