"""CPU (no GPU): scene planes (include/rtuf.h, SCENE PLANES) -- the kernels' own arithmetic (rtuf_numerics.h's scene_threshold,
scene_filtered and scene_learned, compiled for the host by tests/scene_check.cpp) against the numpy form of
tests/scene_planes_scenes.py bit for bit, the kernel routes with a scene in effect (tests/routes_check.cpp: the scene changes nothing
but the scene stage), the scenes of tests/test_scene_planes_gpu.py (every stream must hold every class of
pixel the definition tells apart, or a GPU test on it proves nothing), and the calls' place in the ABI and the bindings."""
import os
import re
import subprocess

import numpy as np
import pytest

import realtime_urdf_filter_amd as R
import scene_planes_scenes as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realtime_urdf_filter_amd", "csrc")
F = np.float32


def build_and_run(tmp_path, name, flags=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", *flags, "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", name + ".cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_threshold_predicate_and_learning_of_the_kernels_header_equal_numpy_bit_for_bit(tmp_path):
    lines = build_and_run(tmp_path, "scene_check", ("-ffp-contract=off",)).split("\n")
    body, tail = lines[:-2], lines[-2].split()
    assert tail == ["done", str(len(body))] and len(body) > 100000
    rows = np.array([[int(w, 16) for w in line.split()[:5]] + [int(line.split()[5])] + [int(w, 16) for w in line.split()[6:]] for line in body], np.uint32)
    scene, abs_m, rel, sensor, thr = (np.ascontiguousarray(rows[:, i]).view(F) for i in range(5))
    filt, keep_l, filt_l = rows[:, 5], np.ascontiguousarray(rows[:, 6]).view(F), np.ascontiguousarray(rows[:, 7]).view(F)
    with np.errstate(all="ignore"):
        want_thr = (scene - (abs_m + (rel * scene).astype(F)).astype(F)).astype(F)
        want_f = sensor > want_thr
    same = lambda a, b: (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    assert same(thr, want_thr).all(), np.argwhere(~same(thr, want_thr))[:5]
    assert np.array_equal(filt != 0, want_f), np.argwhere((filt != 0) != want_f)[:5]
    # the margins the issue names are in the grid, and the grid holds 0, denormals, +inf and NaN scene values
    assert (rel == 0).any() and (abs_m == 0).any() and (rel > F(0.99999)).any() and (rel < 1).all()
    den = (scene != 0) & (np.abs(scene) < F(1.1754944e-38))
    assert (scene == 0).any() and den.any() and np.isposinf(scene).any() and np.isnan(scene).any()
    # an unknown scene pixel never filters anything, whatever the sensor holds: nothing is special-cased, thr is +inf or NaN
    unknown = np.isposinf(scene) | np.isnan(scene)
    assert (np.isposinf(thr[unknown]) | np.isnan(thr[unknown])).all() and not filt[unknown].any()
    assert np.isnan(thr[np.isposinf(scene)]).all()         # (rel * inf is inf or, for rel = 0, NaN: inf - inf or a NaN either way)
    # a NaN sensor is never filtered; the tie is kept and the next float above it filtered
    assert not filt[np.isnan(sensor)].any()
    fin = np.isfinite(thr)
    assert not filt[fin & (sensor.view(np.uint32) == thr.view(np.uint32))].any()
    with np.errstate(all="ignore"):
        assert filt[fin & (sensor == np.nextafter(thr, F(np.inf))) & (thr < F(3.4e38))].all()
    # learning: the running minimum over readings that carry a point, and nothing where the robot filters
    valid = np.isfinite(sensor) & (sensor > 0)
    with np.errstate(all="ignore"):
        want_l = np.where(valid & ~(scene <= sensor), sensor, scene).astype(F)
    assert same(keep_l, want_l).all() and same(filt_l, scene).all()
    assert (valid & np.isnan(scene) & (keep_l == sensor)).any() and (same(keep_l, scene) & valid).any()


def test_scene_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    out = build_and_run(tmp_path, "scene_check", ("-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert out.split("\n")[-2].startswith("done ")


def test_routes_with_a_scene_differ_by_the_scene_stage_only_and_the_older_route_checks_still_pass(tmp_path):
    # One program now: its 1,792 combinations hold the 768 pairs with and without a scene this asserted, and the 384 + 384 of
    # the two older checks; fields 5, 6 and 8 are their figures: 66 plain and 6 padded routes as before, and 56 > 0 scene routes.
    out = build_and_run(tmp_path, "routes_check", ("-Wall", "-Werror")).splitlines()[0].split()
    assert out[:4] == ["ok", "1792", "44", "88"] and int(out[8]) == 56 > 0 and out[5:7] == ["66", "6"], out


@pytest.mark.parametrize("W,H,n,pose", [(160, 120, 4, 0), (160, 120, 4, 1), (160, 120, 4, 2), (200, 150, 3, 0), (160, 120, 5, 0)])
def test_every_stream_of_every_scene_holds_every_class_of_pixel(W, H, n, pose):
    sc, scene, margins = SP.cell(W, H, n, pose)
    for u16 in (False, True):
        if u16:           # the mask of the 16UC1 form: the oracle on the sensor as the kernels see it
            from gpu_support import filter_expected
            mask = filter_expected(sc, 0, True)[1]
        else:
            mask = sc.mask
        counts = SP.class_counts(mask, SP.sensor_metres(sc.depth, u16), scene, margins)
        need = [c for c in SP.CLASSES if not (u16 and c in ("sensor_nan", "sensor_inf", "tie_kept", "tie_next_filtered"))]      # (millimetres hold neither)
        for s in range(n):
            missing = [c for c in need if counts[s][SP.CLASSES.index(c)] == 0]
            assert not missing, "%s u16=%s stream %d lacks %s: %s" % (sc.name, u16, s, missing, dict(zip(SP.CLASSES, counts[s].tolist())))
    # the scene changes something, and leaves something: neither all nor nothing of the kept pixels is scene-filtered
    _, k = SP.expected(sc.masked, sc.mask, sc.depth, scene, margins, sc.wl.replace_value)
    assert ((k > 0) & (sc.mask == 0)).sum() > 1000 and (k == 0).sum() > 500


def test_learning_three_poses_differs_from_learning_one_and_padding_matters():
    """The expectation's own sanity: the robot hides part of the scene in every pose, three poses uncover more than one."""
    sc0, scene, _ = SP.cell(160, 120, 4, 0)
    fresh = np.full(scene.shape, np.inf, F)
    one = SP.learned(fresh, sc0.depth, sc0.mask)
    three = one
    for pose in (1, 2):
        sc = SP.cell(160, 120, 4, pose)[0]
        three = SP.learned(three, sc.depth, sc.mask)
    assert np.isinf(one).sum() > np.isinf(three).sum() > 0
    assert np.array_equal(SP.learned(three, sc0.depth, sc0.mask).view(np.uint32), three.view(np.uint32))      # idempotent


def test_the_calls_are_in_the_header_the_symbol_list_and_the_bindings():
    text = open(os.path.join(ROOT, "include", "rtuf.h")).read()
    assert "SCENE PLANES" in text
    names = ["rtuf_set_scene_planes", "rtuf_set_scene_planes_device", "rtuf_get_scene_planes", "rtuf_get_scene_planes_device", "rtuf_set_scene_margins",
             "rtuf_clear_scene", "rtuf_learn_scene_batch", "rtuf_learn_scene_batch_u16", "rtuf_learn_scene_batch_device", "rtuf_learn_scene_batch_device_u16"]
    for nm in names:
        assert re.search(r"\bint %s\(rtuf_context \*ctx" % nm, text), nm
        assert nm in R._capi.SYMBOLS
    for m in ("set_scene_planes", "get_scene_planes", "set_scene_margins", "clear_scene", "learn_scene_batch", "learn_scene_batch_u16", "learn_scene_batch_device"):
        assert callable(getattr(R.Context, m))
    assert "#define RTUF_ABI_VERSION 6" in text
