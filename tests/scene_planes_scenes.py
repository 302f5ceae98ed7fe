"""Scenes and expectations of the scene-plane tests (include/rtuf.h, SCENE PLANES): a small cell -- three links in front of a
static scene -- whose sensor planes are built FROM the scene planes, so that every stream holds every class of pixel the
definition tells apart.  The numpy form of the definition on the CPU oracle's planes is bench_support/scene_check.py's.
Imported by tests/test_scene_planes_cpu.py (which asserts the class counts) and tests/test_scene_planes_gpu.py."""
import functools

import numpy as np

import scenes as S
from bench_support.virtual_check import expected_virtual
from bench_support.scene_check import expected, learned, scene_filtered, sensor_metres, threshold      # noqa: F401 (the tests reach them through here)
from gpu_support import OracleScene, centred_projection, quad, workload_of

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
# {abs_m, rel} of stream slot i: rel = 0, abs_m = 0, a rel close to 1 and both at once are all there
MARGINS = np.array([(0.02, 0.01), (0.03, 0.0), (0.0, 0.02), (0.01, 0.9), (0.05, 0.005)], F)
CLASSES = ("robot_only", "scene_only", "both", "neither", "sensor_nan", "sensor_zero", "sensor_inf", "scene_inf", "scene_nan", "tie_kept",
           "tie_next_filtered")


def cell_geometry():
    """The "gripper" (link 0, 1 m), an upper arm (1.2 m) and a forearm (1.5 m)."""
    return [quad(-0.15, 0.15, -0.15, 0.15, 1.0), quad(-0.5, -0.3, -0.3, 0.3, 1.2), quad(0.25, 0.5, -0.1, 0.35, 1.5)]


def cell_poses(n, pose):
    """Link matrices [n, 3, 16] of robot pose `pose`: every pose moves the links by 6 cm, every stream by 1 cm more."""
    geo = cell_geometry()
    tfs = np.empty((n, len(geo), 16))
    for s in range(n):
        for l in range(len(geo)):
            T = np.eye(4)
            T[0, 3] = 0.06 * pose * (1 if l != 1 else -1) + 0.01 * s
            T[1, 3] = 0.04 * pose * (l - 1)
            tfs[s, l] = S.gl(T)
    return tfs


def scene_planes(W, H, n):
    """The empty cell: a wavy back wall around 2 m, a table edge at 1.7 m in the lower rows, one block never seen (+inf), one block
    of NaN, and single unknown pixels scattered over the rest."""
    y, x = np.mgrid[0:H, 0:W].astype(F)
    out = np.empty((n, H, W), F)
    for s in range(n):
        t = (2.0 + 0.25 * np.sin(x / 17.0 + s) + 0.1 * np.cos(y / 11.0)).astype(F)
        t[H - 25:, :] = F(1.7) + (0.001 * x[H - 25:, :]).astype(F)
        t[0:6, 0:21] = INF
        t[10:14, W - 9:] = NAN
        t[3 + s::19, 7::23] = INF
        t[5::17, 2 + s::29] = NAN
        out[s] = t
    return out


@functools.lru_cache(maxsize=None)
def cell(W=160, H=120, n=4, pose=0):
    """(OracleScene with sensor planes, scene planes [n,H,W], margins [n,2]).  The sensor reads the scene where nothing is in
    front of it; on the left half of every link it reads the link, on the right half it still reads the scene (a stale or
    see-through reading: robot AND scene filter it); a box at 60 cm in front of the scene stands half over the forearm; and
    scattered pixels hold no reading, or sit exactly on the scene threshold, or one float above it."""
    geo = cell_geometry()
    wl = workload_of("cell_%dx%d_pose%d" % (W, H, pose), W, H, geo, cell_poses(n, pose), np.tile(centred_projection(W, H), (n, 1)))
    bare = OracleScene(wl)
    scene = scene_planes(W, H, n)
    margins = MARGINS[:n].copy()
    virt = expected_virtual(bare.zwin, bare.prim, wl.near, wl.far, 0.0)
    x = np.mgrid[0:H, 0:W][1]
    depth = np.empty((n, H, W), F)
    for s in range(n):
        d = np.where(np.isfinite(scene[s]), scene[s], F(2.0)).astype(F)
        robot = bare.prim[s] >= 0
        for l in range(len(geo)):
            cols = x[robot & (np.abs(virt[s] - F(geo[l][2][0, 2])) < 0.01)]
            if len(cols):
                mid = (int(cols.min()) + int(cols.max())) // 2
                on = robot & (np.abs(virt[s] - F(geo[l][2][0, 2])) < 0.01) & (x <= mid)
                d[on] = virt[s][on]
        d[40:75, W - 60:W - 25] = (d[40:75, W - 60:W - 25] - F(0.6)).astype(F)          # the box: in front of the scene, half over the forearm
        thr = threshold(scene[s], *margins[s])
        d[3::7, 5::9] = thr[3::7, 5::9]
        d[4::7, 6::9] = np.nextafter(thr[4::7, 6::9], INF)
        d[1::9, 0::4] = NAN
        d[5::13, 2::7] = F(0.0)
        d[7::31, 3::11] = INF
        depth[s] = d
    return OracleScene(wl, depth), scene, margins


def class_counts(mask, sensor, scene, margins):
    """[n, len(CLASSES)] pixels of every class of CLASSES per stream, from the robot's mask (the oracle's), the sensor planes in
    metres, the scene planes and the margins."""
    out = np.zeros((len(mask), len(CLASSES)), np.int64)
    for s in range(len(mask)):
        robot = np.asarray(mask[s]) > 0
        sf = scene_filtered(sensor[s], scene[s], *margins[s])
        thr = threshold(scene[s], *margins[s])
        valid = np.isfinite(sensor[s]) & (sensor[s] > 0)
        with np.errstate(all="ignore"):
            nxt = np.nextafter(thr, INF)
        out[s] = [(robot & ~sf).sum(), (~robot & sf).sum(), (robot & sf).sum(), (~robot & ~sf & valid & np.isfinite(scene[s])).sum(),
                  np.isnan(sensor[s]).sum(), (sensor[s] == 0).sum(), np.isposinf(sensor[s]).sum(), np.isposinf(scene[s]).sum(),
                  np.isnan(scene[s]).sum(), (~robot & ~sf & np.isfinite(thr) & (sensor[s] == thr)).sum(),
                  (sf & np.isfinite(thr) & (sensor[s] == nxt)).sum()]
    return out
