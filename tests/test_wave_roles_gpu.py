"""GPU (-m gpu): which wave of a workgroup gets which share of the work, at the sizes where that share falls on a wave's edge.

The set-up kernel and the tile kernel hand out all their work as base + thread index: the first wave of a workgroup is busy in
every loop, the last in few (docs/experiments.md R8).  Whatever changes who does what -- the record pass that runs from the top
wave downwards, the near box that a tail pass behind the record pass bins -- must leave every output what it was.  The scenes are
one draw = one chunk each at 128 x 96 (2 x 3 tiles of 64 x 32), on the 1/256 px lattice of tests/lattice_scenes.py with every
vertex a quarter pixel off a pixel centre, and every output is the CPU oracle's bit for bit, in two batches (the first batch of
a context sweeps its work list with the strided variant of the set-up kernel).

In this process the six tiles of a stream take the 1,024-thread tile kernels; run as a script
(RTUF_SMALL_LAUNCH=0 python tests/test_wave_roles_gpu.py) the same cases take the 256-thread ones: the threshold is read once
per process, so test_every_case_256_thread_kernels starts one."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import lattice_scenes as LS
import scenes as S
from gpu_support import OracleScene, cached, compare_labels, compare_planes, workload_of

pytestmark = pytest.mark.gpu

W, H = 128, 96
Q = 64                          # every vertex lies a quarter pixel right of and below a pixel centre


def px(x, y):
    return (int(x) * LS.PX + Q, int(y) * LS.PX + Q)


def sheet(n, size, x0, y0, per_row, slots=None):
    """n triangles: squares of `size` px with a corner at pixel (x0, y0) + a quarter, per_row to a row, each cut along one
    diagonal.  A triangle's box of pixel centres is size x size from (x + 1, y + 1) on; both halves own at least one of them.
    With `slots`, triangle t takes the place of triangle t % slots (the scene then stacks layers)."""
    out = []
    for t in range(n):
        u = t % slots if slots else t
        col, row = (u // 2) % per_row, (u // 2) // per_row
        x, y = x0 + col * size, y0 + row * size
        a, b, c, d = px(x, y), px(x + size, y), px(x + size, y + size), px(x, y + size)
        out.append((a, b, c) if u % 2 == 0 else (a, c, d))
    return out


def strip(V):
    """V vertices in a zigzag, 0.45 px apart, and the V - 2 triangles between each three in a row (V = 1: one triangle of that
    vertex three times).  The zigzag's height changes every 16 vertices: boxes of all three classes."""
    amp = (0.8, 1.7, 4.5)
    xy = [(int(round((3 + 0.45 * i) * LS.PX)) + Q, int(round((40 + (1 if i & 1 else -1) * amp[(i // 16) % 3]) * LS.PX)) + Q) for i in range(V)]
    tris = [(i, i + 1, i + 2) for i in range(V - 2)] if V >= 3 else [(0, 0, 0)]
    return xy, tris


def draw_of(tris, z=LS.Z_MAIN):
    """Triangles of snapped window coordinates (each with a depth, or all at z) as one draw: three vertices per triangle; the
    library makes vertices with the same coordinates one."""
    zs = z if isinstance(z, (list, tuple)) else [z] * len(tris)
    verts = np.concatenate([LS.unproject(np.asarray(t, np.int64), zt, W, H) for t, zt in zip(tris, zs)])
    return (0, [0.0, 0.0, 0.0], np.ascontiguousarray(verts, np.float32), np.arange(3 * len(tris), dtype=np.uint32).reshape(-1, 3))


def indexed_draw(xy, tris, z=LS.Z_MAIN):
    return (0, [0.0, 0.0, 0.0], LS.unproject(np.asarray(xy, np.int64), z, W, H), np.asarray(tris, np.uint32))


def shifted(dx_px=0.0, dy_px=0.0):
    """A link pose that moves geometry at 1 m by (dx, dy) pixels."""
    T = np.eye(4)
    T[0, 3], T[1, 3] = dx_px / (W / 2.0) * LS.Z_MAIN, dy_px / (H / 2.0) * LS.Z_MAIN
    return S.gl(T)


def scene_of(name, draw, poses):
    """One link with one draw, a stream per pose, sensor planes of their own."""
    n = len(poses)
    wl = workload_of(name, W, H, [draw], np.stack(poses)[:, None, :], np.tile(LS.projection(W, H), (n, 1)))
    wl.near, wl.far = LS.NEAR, LS.FAR
    return OracleScene(wl, np.stack([S.sensor_depth(W, H, 0.21 * s + 0.4) for s in range(n)]))


def winners(sc, s):
    """How many of the scene's triangles win at least one pixel of stream s."""
    p = sc.prim[s]
    return len(np.unique(p[p >= 0]))


def run(sc, batches=2, **param_overrides):
    ctx = sc.context(**param_overrides)
    try:
        for b in range(batches):
            masked, mask = ctx.filter_batch(sc.depth)
            compare_labels(mask, sc.mask, "%s batch %d" % (sc.name, b), "mask")
            compare_planes(masked, sc.masked, "%s batch %d" % (sc.name, b))
        st = ctx.stats()
        assert st["batch_status"] == 0, st
        return st
    finally:
        ctx.close()


# ---- chunk sizes: every role boundary on and next to a wave's edge -----------------------------------------------------------

TRIANGLES = [1, 64, 65, 255, 256]
VERTICES = [1, 64, 65, 256]


@cached
def triangles_scene(T):
    """One chunk of T triangles with boxes of 3 x 3: fragments where the box lies in one tile, records where it straddles."""
    return scene_of("triangles_%d" % T, draw_of(sheet(T, 3, 2, 2, 30)), [shifted(0, 0)])


@cached
def vertices_scene(V):
    xy, tris = strip(V)
    return scene_of("vertices_%d" % V, indexed_draw(xy, tris), [shifted(0, 0)])


@pytest.mark.parametrize("T", TRIANGLES)
def test_one_chunk_of_t_triangles(T):
    sc = triangles_scene(T)
    assert winners(sc, 0) == T
    st = run(sc)
    assert st["work_items"] == 1 and st["triangles_binned"] == T, st


@pytest.mark.parametrize("V", VERTICES)
def test_one_chunk_of_v_distinct_vertices(V):
    sc = vertices_scene(V)
    if V >= 64:
        assert winners(sc, 0) > V // 4, winners(sc, 0)
    st = run(sc)
    assert st["work_items"] == 1, st


# ---- streams per work item, with one and with three raster lanes ----------------------------------------------------------------

POSES = [shifted(0, 0), shifted(1.04, 1.6), shifted(-0.56, 3.3), shifted(2.1, -2.2)]
STREAMS_LANES = [(n, lanes) for n in (1, 2, 3, 4) for lanes in (1, 3)]


@cached
def streams_scene(n):
    xy, tris = strip(171)
    return scene_of("streams_%d" % n, indexed_draw(xy, tris), POSES[:n])


@pytest.mark.parametrize("n,lanes", STREAMS_LANES)
def test_items_of_one_two_and_three_live_streams(n, lanes):
    """Batches of 1, 2, 3 and 4 streams that all see the chunk: items of 1, 2 and 3 live streams, and of 3 + 1 (with three
    lanes a lane's launch group may hold fewer streams: never more than three to an item either way)."""
    sc = streams_scene(n)
    assert all(winners(sc, s) > 40 for s in range(n))
    st = run(sc, raster_lanes=lanes)
    assert 1 <= st["work_items"] <= n, st


# ---- a list that needs a second trip of 256 ------------------------------------------------------------------------------------

SECOND_TRIP = ["tiny", "small", "records"]


@cached
def second_trip_scene(kind):
    """256 triangles that each cover a pixel, seen by three streams: 768 survivors in ONE list, three trips of 256.
    tiny: boxes of 2 x 2.  small: boxes of 4 x 4 from pixel (4, 4) on, 15 squares to a row, moved by whole boxes from stream to
    stream: none straddles a tile.  records: boxes of 6 x 6."""
    if kind == "tiny":
        return scene_of("trip_tiny", draw_of(sheet(256, 2, 4, 4, 30)), [shifted(0, 0), shifted(3, 7), shifted(-2, 11)])
    if kind == "small":
        return scene_of("trip_small", draw_of(sheet(256, 4, 3, 3, 15)), [shifted(0, 0), shifted(0, 4), shifted(0, 8)])
    return scene_of("trip_records", draw_of(sheet(256, 6, 4, 4, 16)), [shifted(0, 0), shifted(0, 10), shifted(0, 20)])


@pytest.mark.parametrize("kind", SECOND_TRIP)
def test_a_list_that_needs_a_second_trip(kind):
    sc = second_trip_scene(kind)
    assert [winners(sc, s) for s in range(3)] == [256, 256, 256]
    st = run(sc)
    assert st["work_items"] == 1 and st["triangles_binned"] == 768, st
    if kind == "records":
        assert st["fragments_binned"] == 0 and st["bin_entries"] >= 768, st
    else:
        assert st["bin_entries"] == 0 and st["fragments_binned"] >= 768, st


# ---- the near box: handed to the record list behind phase 2's entries, binned by the tail pass ----------------------------------

def near_box():
    """A 4 x 4 box inside one tile, 3 um behind the near plane: its z plane reaches below window z 0.51."""
    return sheet(1, 4, 99, 67, 1), [LS.Z_NEAR]


@cached
def near_scene(with_near, with_records):
    tris, zs = [], []
    if with_records:          # 100 ordinary records (boxes of 6 x 6) in the same item
        tris, zs = sheet(100, 6, 4, 4, 10), [LS.Z_MAIN] * 100
    if with_near:
        nt, nz = near_box()
        tris, zs = tris + nt, zs + nz
    return scene_of("near_%d_%d" % (with_near, with_records), draw_of(tris, zs), [shifted(0, 0)])


def test_near_box_alone():
    sc = near_scene(True, False)
    near = sc.zwin[0] < 0.5
    assert winners(sc, 0) == 1 and near.any() and near.sum() <= 16
    st = run(sc)
    assert st["work_items"] == 1 and st["triangles_binned"] == 1 and st["bin_entries"] == 1 and st["fragments_binned"] == 0, st


def test_near_box_among_ordinary_records():
    without, with_it = near_scene(False, True), near_scene(True, True)
    assert (winners(without, 0), winners(with_it, 0)) == (100, 101)
    a, b = run(without), run(with_it)
    assert a["fragments_binned"] == 0 and b["fragments_binned"] == 0, (a, b)
    # one record more, in the one bin its box lies in
    assert b["triangles_binned"] == a["triangles_binned"] + 1 == 101 and b["bin_entries"] == a["bin_entries"] + 1, (a, b)


# ---- a bin of 257 records: the tile kernel's last window is one lane -------------------------------------------------------------

@cached
def bin_of_257_scene():
    """257 triangles with boxes of 5 x 5, all inside the first tile: 144 places (12 x 6 squares), the second layer behind the
    first.  Two chunks; every triangle is one record of the same bin."""
    n = 257
    return scene_of("bin_257", draw_of(sheet(n, 5, 1, 1, 12, slots=144), [LS.Z_MAIN if t < 144 else LS.Z_FAR_LAYER for t in range(n)]), [shifted(0, 0)])


def test_a_bin_of_257_records():
    sc = bin_of_257_scene()
    assert winners(sc, 0) == 144
    st = run(sc)
    assert st["triangles_binned"] == 257 and st["bin_entries"] == 257 and st["fragments_binned"] == 0, st


# ---- the same cases through the 256-thread tile kernels ---------------------------------------------------------------------------

def all_cases():
    for T in TRIANGLES:
        test_one_chunk_of_t_triangles(T)
    for V in VERTICES:
        test_one_chunk_of_v_distinct_vertices(V)
    for n, lanes in STREAMS_LANES:
        test_items_of_one_two_and_three_live_streams(n, lanes)
    for kind in SECOND_TRIP:
        test_a_list_that_needs_a_second_trip(kind)
    test_near_box_alone()
    test_near_box_among_ordinary_records()
    test_a_bin_of_257_records()
    return len(TRIANGLES) + len(VERTICES) + len(STREAMS_LANES) + len(SECOND_TRIP) + 3


def test_every_case_256_thread_kernels():
    """The same cases with RTUF_SMALL_LAUNCH=0: every launch takes the 256-thread tile kernels."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=600,
                       env=dict(os.environ, RTUF_SMALL_LAUNCH="0"))
    assert r.returncode == 0 and "cases ok 23" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


if __name__ == "__main__":
    print("cases ok %d" % all_cases())
