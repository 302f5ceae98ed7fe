"""GPU (-m gpu): the frustum clipper on every plane, corner and tie in every route, on the scenes of tests/clip_scenes.py.

Every scene crosses the frustum somewhere on purpose (tests/test_clip_scenes_cpu.py shows where, from a census of the
classification and the clipper, and that the CPU oracle renders the scenes as Mesa llvmpipe does).  One robot link per
colour, so the label plane and the virtual depth plane show which triangle got every pixel.  The expectation is the
oracle's, compared bit for bit on every kind of batch (gpu_support.filter_routes), each batch twice, in a context of one
stream, in two-kernel mode (there a labelled filter batch takes the z-surface + labels route: all kinds but the mask bits),
with three raster lanes, in launch groups of two streams (group_base 2 and 4) and, where triangles share edges, in the
other draw order.  Stream s looks from its own camera pose (the tie scenes apart), so a clip item that is worked on with
another stream's matrix shows.  The sensor lies 7 m away in whole millimetres: one oracle run serves float and 16UC1.

ctx.stats() pins the path: the number of triangles the set-up kernel hands to the clipper is the census's, stream by
stream; `many` overflows a fresh context's clip lists and runs again after they, and the spill area, have grown; `walls`
goes through the cover pass; the tie cases that lie on a plane without crossing it are not clipped at all.

Run as a script (RTUF_SMALL_LAUNCH=0 python tests/test_clipper_gpu.py) the walls, around and levers scenes go through the
256-thread tile kernels: the threshold is read once per process, so test_large_scenes_256_thread_kernels starts one."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import clip_scenes as C
import realtime_urdf_filter_amd as R
from gpu_support import OracleScene, bits_equal, filter_routes, label_planes, same_planes
from realtime_urdf_filter_amd.filter import depth_f32_to_u16, depth_u16_to_f32

pytestmark = pytest.mark.gpu
REPLACE, MAX_DIFF, STREAMS = 5.0, 0.05, 5
BOTH_ORDERS = ("plane", "corner", "ties", "walls")
LARGE = ("walls", "around", "levers")


def build(name, reverse):
    """A clip scene as a batch of five streams, each under its own camera pose and sensor plane, with the oracle's planes."""
    sc = C.scene(name)
    wl, _ = C.workload(name, STREAMS, reverse)
    assert (wl.near, wl.far, wl.max_diff, wl.replace_value) == (C.NEAR, C.FAR, MAX_DIFF, REPLACE)
    mm = C.sensor_mm(name, STREAMS)
    g = OracleScene(wl, depth_u16_to_f32(mm), name + ("_reversed" if reverse else ""))          # whole millimetres: one oracle run serves f32 and 16UC1
    g.sc, g.mm, g.reverse = sc, mm, reverse
    assert np.array_equal(depth_f32_to_u16(g.depth), mm)
    g.labels = label_planes(g)
    g.n_labels = len(wl.models[0]) + 1
    g.zsurface = np.where(g.prim == -1, np.float32(np.nan), g.zwin).astype(np.float32)
    for c in sorted(set(sc.colour)):          # what the CPU tests show of stream 0 holds for the batch: every link is seen in some stream
        assert bool((g.labels == sc.link_of_colour(c, reverse)).any()) != (c in sc.nothing), (g.name, c)
    return g


_scenes = {}


def gscene(name, reverse=False):
    if (name, reverse) not in _scenes:
        _scenes[(name, reverse)] = build(name, reverse)
    return _scenes[(name, reverse)]


def clipped(sc, n):
    """The triangles of the first n streams that the set-up kernel hands to the clipper, by the census."""
    return sum(int(sc.census(s).needs_clip.sum()) + C.background_clipped(sc.mvp(s, n)[1]) for s in range(n))


def nothing_drawn(g):
    """check_labels for filter_routes: the links that draw nothing on purpose (the wholly-outside twins of the grazing scenes,
    the misses, the edges in a plane) are in no label plane."""
    def check(lab, what):
        for c in g.sc.nothing:
            assert not (lab == g.sc.link_of_colour(c, g.reverse)).any(), "%s: the link of colour %d is drawn" % (what, c)
    return check


def path_checks(name, g, st, n):
    """What ctx.stats() must show after the scene's second plain filter batch of n streams."""
    assert st["batch_status"] == 0, (name, st)
    want = clipped(g.sc, n)
    assert st["triangles_clipped"] == want and (want > 0) == (name != "ties_unclipped"), (name, n, want, st)
    if name == "walls":
        assert st["cover_pass"] == 1 and st["cover_tiles"] > 0, (name, st)


def run_scene(name):
    g = gscene(name)
    # a batch of one stream
    ctx = g.context(1, 1)
    if name == "many":          # a fresh context: a shard's clip list overflows, the lists and the spill area grow, the batch runs again
        masked, mask = ctx.filter_batch(g.depth[:1])
        first = ctx.stats()
        assert first["regrowths"] >= 1, first
        same_planes(mask, g.mask[:1], "many, first batch: mask")
        assert bits_equal(masked, g.masked[:1]), "many, first batch: masked depth"
    st = filter_routes(g, ctx, 1, "one stream", check_labels=nothing_drawn(g))
    path_checks(name, g, st, 1)
    if name == "many":
        assert ctx.stats()["regrowths"] == first["regrowths"], (first, ctx.stats())
    ctx.close()
    # two-kernel mode, all streams
    ctx = g.context(g.n, g.n, flags=R.FLAG_TWO_KERNEL)
    st = filter_routes(g, ctx, g.n, "two-kernel", two_kernel=True, check_labels=nothing_drawn(g))
    path_checks(name, g, st, g.n)
    ctx.close()
    # a batch of 3 in a context of 4 with three raster lanes
    ctx = g.context(4, 3, raster_lanes=3)
    st = filter_routes(g, ctx, 3, "3 of 4 streams, 3 lanes", check_labels=nothing_drawn(g))
    path_checks(name, g, st, 3)
    ctx.close()
    # launch groups of two streams: group_base 0, 2 and 4
    ctx = g.context(g.n, g.n, max_inflight_streams=2)
    st = filter_routes(g, ctx, g.n, "groups of 2 streams", check_labels=nothing_drawn(g))
    path_checks(name, g, st, g.n)
    assert st["groups_last_batch"] == 3, (name, st)
    ctx.close()
    # the other draw order
    if C.kind_of(name) in BOTH_ORDERS:
        g = gscene(name, reverse=True)
        ctx = g.context(4, 3, raster_lanes=3)
        st = filter_routes(g, ctx, 3, "3 of 4 streams, 3 lanes", check_labels=nothing_drawn(g))
        path_checks(name, g, st, 3)
        ctx.close()


@pytest.mark.parametrize("name", C.NAMES)
def test_every_route_clips_as_the_oracle_does(name):
    run_scene(name)


def test_large_scenes_256_thread_kernels():
    """The same checks with RTUF_SMALL_LAUNCH=0 on the scenes whose clipped records fill the frame: every launch takes the
    256-thread tile kernels."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=300,
                       env=dict(os.environ, RTUF_SMALL_LAUNCH="0"))
    assert r.returncode == 0 and "scenes ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


if __name__ == "__main__":
    for scene_name in LARGE:
        run_scene(scene_name)
    print("scenes ok")
