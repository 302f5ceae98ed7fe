"""The scenes of the link padding tests (tests/test_link_padding_gpu.py; tests/test_link_padding_cpu.py checks on the oracle
alone that each of them tells padding from no padding and from a square dilation) with the paddings of their links, and the
expectation of a batch: bench_support/link_padding_check.py on the CPU oracle's planes, stream by stream, with the focal
length of the slot the stream sits in (gpu_support.intrinsics: different for every slot, fx != fy from slot 1 on)."""
import functools

import numpy as np

import scenes as S
from bench_support import link_padding_check as PC
from bench_support.dilation_check import drawn_z, shade
from gpu_support import (OracleScene, border_scene, centred_projection, intrinsics, near_quad_scene, neighbour_scene, quad, small_links_scene,
                         soup_scene, undrawn_scene, workload_of)
from realtime_urdf_filter_amd.filter import depth_f32_to_u16, depth_u16_to_f32

F = np.float32
SCENES = ("small_links", "neighbour", "border", "near_quad", "undrawn", "undrawn_links", "soup", "ramp")


def ramp_scene(W=150, H=70):
    """150 x 70: neither dimension is a multiple of the 64 x 32 tile and the width is no multiple of 4 (planes only).  Link 0 is
    a quad slanted from 0.4 m at the left to 4 m at the right; with its padding of 6 cm and f = 123 its reach runs from the
    clamp (18 pixels asked for at 0.4 m) down to 1.8 pixels at 4 m -- a factor of ten in depth cannot span the factor of sixteen
    between the clamp and a reach below one pixel, so link 1, a quad behind it slanted from 4.5 m to 7.5 m with 5 cm, takes the
    reach from 1.4 pixels down to 0 (below one pixel from 6.2 m on).  Link 0's discs lie over link 1's pixels and its own
    padding.  The sensor is at 7 m: behind both links, in front of the background plane."""
    def slanted(x0, z0, x1, z1, y0, y1):
        v = np.array([[x0, y0, z0], [x1, y0, z1], [x1, y1, z1], [x0, y1, z0]], np.float32)
        return (0, [0.0, 0.0, 0.0], v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
    geo = [slanted(-0.21, 0.4, 2.1, 4.0, -0.1, 0.1), slanted(-1.6, 4.5, 2.6, 7.5, -0.9, 0.5)]
    wl = workload_of("ramp_%dx%d" % (W, H), W, H, geo, np.tile(S.gl(np.eye(4)), (1, len(geo), 1)), centred_projection(W, H)[None])
    depth = np.where(np.isfinite(S.sensor_depth(W, H, 0.4)) & (S.sensor_depth(W, H, 0.4) > 0), F(7.0), S.sensor_depth(W, H, 0.4)).astype(F)
    return OracleScene(wl, depth[None])


def undrawn_links_scene(W=160, H=120):
    """gpu_support.undrawn_scene's projection (clip-space x shifted by 160: the background quad leaves columns 0 .. 37 at the
    clear colour) shows none of that scene's links: the shift moves anything near the optical axis far out of the image.  Here
    three quads sit where that projection looks, 97.56 m to the side: link 0 across the edge of the background quad, link 1
    in front of the quad, link 2 where nothing else is drawn -- so padding turns clear-colour pixels into drawn ones, and
    some stay."""
    P = centred_projection(W, H)
    P[12] = 160.0
    x0 = -97.56
    geo = [quad(x0 - 0.62, x0 - 0.30, -0.25, 0.1, 1.0), quad(x0 + 0.1, x0 + 0.3, 0.0, 0.3, 1.5), quad(x0 - 0.5, x0 - 0.45, 0.25, 0.3, 0.8)]
    wl = workload_of("undrawn_links_%dx%d" % (W, H), W, H, geo, np.tile(S.gl(np.eye(4)), (1, len(geo), 1)), P[None])
    return OracleScene(wl, S.sensor_depth(W, H, 0.9)[None])


def _with_sensor(sc, phase, scale=1.0):
    """A cached scene of gpu_support that has no sensor planes, with some (the cached scene itself is left alone)."""
    depth = np.stack([S.sensor_depth(sc.W, sc.H, phase + 0.3 * s) for s in range(sc.n)]) * F(scale)
    return OracleScene(sc.wl, depth.astype(F), sc.name)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(OracleScene with sensor planes, padding in metres of every link).  One model each."""
    if name == "small_links":
        sc = _with_sensor(small_links_scene(), 0.2)
        return sc, tuple(0.005 * (l % 7) for l in range(sc.n_links))          # reaches of 0 .. 3.9 pixels, neighbours differ
    if name == "neighbour":
        return neighbour_scene(), (0.04, 0.06)
    if name == "border":
        return border_scene(), (0.03, 0.05, 0.02, 0.04)
    if name == "near_quad":
        return _with_sensor(near_quad_scene(), 0.7), (0.03, 0.02)             # the quad at the near plane asks for 26 pixels: clamped
    if name == "undrawn":                  # (no link of it is in view: what it shows is the uncovered flag while padding is in effect)
        return undrawn_scene(), (0.03, 0.05, 0.0, 0.08)
    if name == "undrawn_links":
        return undrawn_links_scene(), (0.04, 0.03, 0.05)
    if name == "soup":
        return soup_scene(1, 160, 120), (0.02, 0.05, 0.0, 0.03, 0.08, 0.01)      # (the soup of the route tests: stream 1 has cover tiles)
    if name == "ramp":
        return ramp_scene(), (0.06, 0.05)
    raise KeyError(name)


def focal(sc, slot):
    """(float)max(fx, fy) of the intrinsics the tests give slot `slot`."""
    fx, fy = intrinsics(sc, slot)[:2]
    return F(max(fx, fy))


@functools.lru_cache(maxsize=None)
def _padded_z(name_key, sc_id, s, pads, f):
    sc = _scenes_by_id[sc_id]
    draw_pad, ntris = PC.workload_draws(sc.wl, pads)
    R2 = PC.reach2(sc.zwin[s], sc.prim[s], draw_pad, ntris, f, sc.wl.near, sc.wl.far)
    return R2, PC.padded_z(drawn_z(sc.zwin[s], sc.prim[s]), R2)


_scenes_by_id = {}


class Expected:
    """masked, mask, R2, zp [len(streams), H, W] of a batch that holds stream streams[i] of the scene in slot i, with the
    paddings `pads` (per link) and focal lengths `focals` (per slot; default: those of gpu_support.intrinsics)."""

    def __init__(self, sc, pads, u16=False, streams=None, focals=None):
        streams = list(range(sc.n)) if streams is None else list(streams)
        _scenes_by_id[id(sc)] = sc
        out = []
        for i, s in enumerate(streams):
            f = focal(sc, i) if focals is None else F(focals[i])
            R2, zp = _padded_z(sc.name, id(sc), s, tuple(float(p) for p in pads), float(f))
            sensor = depth_u16_to_f32(depth_f32_to_u16(sc.depth[s])) if u16 else sc.depth[s]
            m, k = shade(zp, sensor, sc.wl.near, sc.wl.far, sc.wl.max_diff, sc.wl.replace_value)
            out.append((depth_f32_to_u16(m) if u16 else m, k, R2, zp))
        self.masked, self.mask, self.R2, self.zp = (np.stack([o[j] for o in out]) for j in range(4))
        self.undrawn = bool(np.isnan(self.zp).any())


def expected(sc, pads, u16=False, streams=None, focals=None):
    return Expected(sc, pads, u16, streams, focals)
