"""Scene planes (include/rtuf.h, SCENE PLANES): the numpy form of the definition, on planes the CPU oracle (or anything else)
gives for the robot filter alone:
    mask'   = mask | (sensor > thr),  thr = scene - (abs_m + rel * scene)   (float32, every operation rounded on its own)
    masked' = where(mask', replace, sensor)
and of learning: the running minimum over the pixels the robot filter keeps and that hold a reading.  Used by the tests
(tests/scene_planes_scenes.py) and by scripts/scene_rate.py, which checks every stream of a timed batch with it."""
import numpy as np

from realtime_urdf_filter_amd.filter import depth_f32_to_u16, depth_u16_to_f32

F = np.float32


def threshold(scene, abs_m, rel):
    """thr of the definition, float32 throughout (numpy rounds every float32 operation on its own)."""
    scene = np.asarray(scene, F)
    with np.errstate(all="ignore"):
        return (scene - (F(abs_m) + (F(rel) * scene).astype(F)).astype(F)).astype(F)


def scene_filtered(sensor, scene, abs_m, rel):
    with np.errstate(all="ignore"):
        return np.asarray(sensor, F) > threshold(scene, abs_m, rel)


def sensor_metres(depth, u16):
    """The sensor planes as the kernels see them: 16UC1 goes through millimetres and back."""
    return depth_u16_to_f32(depth_f32_to_u16(depth)) if u16 else np.asarray(depth, F)


def expected(robot_masked, robot_mask, depth, scene, margins, replace, u16=False, enabled=None):
    """(masked, mask) with the scene on top of the robot filter's outputs (robot_masked in the batch's element type, robot_mask
    0 / 255, each [n,H,W]); enabled[i] False: stream i has scene filtering off."""
    sensor = sensor_metres(depth, u16)
    n = len(robot_mask)
    sf = np.stack([scene_filtered(sensor[s], scene[s], *margins[s]) & (enabled is None or bool(enabled[s])) for s in range(n)])
    rep = depth_f32_to_u16(np.full((1,), replace, F))[0] if u16 else F(replace)
    masked = np.where(sf, rep, np.asarray(robot_masked)[:n]).astype(np.uint16 if u16 else F)
    mask = np.where(sf, np.uint8(255), np.asarray(robot_mask)[:n]).astype(np.uint8)
    return masked, mask


def learned(scene, depth, robot_mask, u16=False):
    """The planes after one learn call: the running minimum over the pixels the robot filter keeps and that hold a reading (a
    NaN plane value is unknown: the reading replaces it)."""
    sensor = sensor_metres(depth, u16)
    scene = np.array(scene, F)
    take = (np.asarray(robot_mask) == 0) & np.isfinite(sensor) & (sensor > 0)
    with np.errstate(all="ignore"):
        take &= ~(scene[:len(sensor)] <= sensor)
    scene[:len(sensor)][take] = sensor[take]
    return scene
