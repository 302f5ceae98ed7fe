"""GPU (-m gpu): the set-up kernel's work item at the sizes where its loops and list counters turn over.

A work item is one chunk (<= 256 triangles with <= 256 vertices of their own) and up to three streams that see it.  Its
survivors go to three LDS lists -- records, boxes of at most 2 x 2 pixel centres ("tiny") and of at most 4 x 4 inside one
tile ("small") -- whose fill is one packed word (list_counts, rtuf_numerics.h; tests/test_setup_lists_cpu.py): one addition per
wave and stream reserves in all three, the box lists are walked in trips of 256 entries, and a box that may reach window z 0.5
is handed over to the record list.  The scenes here are one draw = one chunk each, at 160 x 120, built on the 1/256 px
lattice of tests/lattice_scenes.py with every vertex a quarter pixel off a pixel centre (so its box is what the size says,
whatever the last bit of the projection does), and every output is the CPU oracle's bit for bit, in two batches: a context's
first batch sizes its set-up grid without a previous work list and sweeps the rest with the strided variant of the kernel.

What a scene claims about its lists -- so many triangles that each win a pixel, per stream -- is read back from the oracle's
primitive plane before the GPU is asked anything."""
import numpy as np
import pytest

import lattice_scenes as LS
import scenes as S
from gpu_support import OracleScene, cached, compare_labels, compare_planes, workload_of

pytestmark = pytest.mark.gpu

W, H = 160, 120
Q = 64                          # every vertex lies a quarter pixel right of and below a pixel centre


def px(x, y):
    return (int(x) * LS.PX + Q, int(y) * LS.PX + Q)


def sheet(n, size, x0, y0, per_row):
    """n triangles: squares of `size` px with a corner at pixel (x0, y0) + a quarter, per_row to a row, each cut along one
    diagonal (an odd n ends in half a square).  A triangle's box of pixel centres is size x size from (x + 1, y + 1) on; both
    halves own at least one of them."""
    out = []
    for t in range(n):
        col, row = (t // 2) % per_row, (t // 2) // per_row
        x, y = x0 + col * size, y0 + row * size
        a, b, c, d = px(x, y), px(x + size, y), px(x + size, y + size), px(x, y + size)
        out.append((a, b, c) if t % 2 == 0 else (a, c, d))
    return out


def strip(V):
    """V vertices in a zigzag along the image's middle, 0.6 px apart, and the V - 2 triangles between each three in a row (V = 1:
    one triangle of that vertex three times).  The zigzag's height changes every 16 vertices: boxes of all three classes."""
    amp = (0.8, 1.7, 4.5)
    xy = [(int(round((3 + 0.6 * i) * LS.PX)) + Q, int(round((40 + (1 if i & 1 else -1) * amp[(i // 16) % 3]) * LS.PX)) + Q) for i in range(V)]
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


def shifted(dx_px=0.0, dy_px=0.0, away=False):
    """A link pose that moves geometry at 1 m by (dx, dy) pixels -- or behind the camera."""
    T = np.eye(4)
    T[0, 3], T[1, 3] = dx_px / (W / 2.0) * LS.Z_MAIN, dy_px / (H / 2.0) * LS.Z_MAIN
    if away:
        T[2, 3] = -5.0
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


def run(sc, batches=2):
    ctx = sc.context()
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


# ---- one chunk of V vertices seen by three streams: 2 V and 3 V lie on both sides of 256, 512 and 768 ----------------------

@cached
def strip_scene(V, poses_key):
    poses = {"three": [shifted(0, 0), shifted(1.04, 1.6), shifted(-0.56, 3.3)],
             "one": [shifted(0, 0)],
             "two": [shifted(0, 0), shifted(1.04, 1.6)],
             "middle_away_of_3": [shifted(0, 0), shifted(away=True), shifted(-0.56, 3.3)],
             "middle_away_of_4": [shifted(0, 0), shifted(away=True), shifted(-0.56, 3.3), shifted(2.1, -2.2)],
             "four": [shifted(0, 0), shifted(1.04, 1.6), shifted(-0.56, 3.3), shifted(2.1, -2.2)]}[poses_key]
    xy, tris = strip(V)
    return scene_of("strip_%d_%s" % (V, poses_key), indexed_draw(xy, tris), poses)


@pytest.mark.parametrize("V", [1, 85, 86, 128, 171, 255, 256])
def test_one_chunk_of_v_vertices_in_three_streams(V):
    sc = strip_scene(V, "three")
    if V >= 85:
        assert min(winners(sc, s) for s in range(3)) > V // 4, [winners(sc, s) for s in range(3)]
    run(sc)


@pytest.mark.parametrize("poses,live", [("one", 1), ("two", 2), ("middle_away_of_3", 2), ("middle_away_of_4", 3), ("four", 4)])
def test_items_of_one_two_and_three_live_streams(poses, live):
    """Batches of 1, 2, 3 and 4 streams; a middle stream that looks away is not in the chunk's item (2 and 3 live streams);
    four streams that all look make an item of three and one of one."""
    sc = strip_scene(171, poses)
    seeing = [s for s in range(sc.n) if winners(sc, s) > 0]
    assert len(seeing) == live and (live == sc.n or 1 not in seeing), seeing
    st = run(sc)
    assert st["work_items"] == (2 if live == 4 else 1), st


# ---- the two box lists on both sides of a wave, and of a trip of 256 ----------------------------------------------------------

def boxes_draw(ntiny, nsmall, small_x0=3):
    """ntiny boxes of 2 x 2 from pixel (4, 4) on, 30 squares to a row; nsmall of 4 x 4, each inside one tile, from (small_x0, 35) on."""
    return draw_of(sheet(ntiny, 2, 4, 4, 30) + sheet(nsmall, 4, small_x0, 35, 15 if small_x0 == 3 else 1))


@cached
def wave_scene(ntiny, nsmall):
    return scene_of("boxes_%d_%d" % (ntiny, nsmall), boxes_draw(ntiny, nsmall), [shifted(0, 0)])


@pytest.mark.parametrize("ntiny,nsmall", [(63, 1), (64, 1), (65, 1), (1, 63), (1, 64), (1, 65)])
def test_box_lists_around_one_wave(ntiny, nsmall):
    sc = wave_scene(ntiny, nsmall)
    assert winners(sc, 0) == ntiny + nsmall
    st = run(sc)
    # every triangle left the kernel, as fragments: none as a record
    assert st["triangles_binned"] == ntiny + nsmall and st["bin_entries"] == 0 and st["fragments_binned"] >= ntiny + nsmall, st


@cached
def trip_scene(ntiny, nsmall):
    """Two streams; the second sees everything 20 px further right, where the small boxes (from x = 151 on) have left the
    frame: the item holds 2 ntiny + nsmall boxes."""
    return scene_of("trip_%d_%d" % (ntiny, nsmall), boxes_draw(ntiny, nsmall, small_x0=151), [shifted(0, 0), shifted(20.0, 0)])


@pytest.mark.parametrize("ntiny,nsmall,total", [(127, 1, 255), (127, 2, 256), (128, 1, 257)])
def test_box_lists_around_one_trip(ntiny, nsmall, total):
    sc = trip_scene(ntiny, nsmall)
    assert (winners(sc, 0), winners(sc, 1)) == (ntiny + nsmall, ntiny) and 2 * ntiny + nsmall == total
    st = run(sc)
    assert st["work_items"] == 1 and st["triangles_binned"] == total and st["bin_entries"] == 0, st


# ---- the hand-over of a near box to a record list that is full to the trip ------------------------------------------------------

@cached
def hand_over_scene():
    """128 triangles with boxes of 6 x 6 (records) in two streams that see the same: 256 entries, one trip of the record pass.
    One 4 x 4 box 3 um behind the near plane is handed over by both streams: entries 257 and 258."""
    tris = sheet(128, 6, 4, 4, 16) + sheet(1, 4, 131, 67, 1)
    return scene_of("hand_over", draw_of(tris, [LS.Z_MAIN] * 128 + [LS.Z_NEAR]), [shifted(0, 0), shifted(0, 0)])


def test_near_box_is_handed_over_to_a_full_record_list():
    sc = hand_over_scene()
    assert (winners(sc, 0), winners(sc, 1)) == (129, 129)
    near = sc.zwin[0] < 0.5
    assert near.any() and near.sum() <= 16          # the near box's pixels, and nothing else, lie below window z 0.5
    st = run(sc)
    # 256 records and the near box twice, which did not leave as fragments
    assert st["work_items"] == 1 and st["triangles_binned"] == 258 and st["fragments_binned"] == 0, st
