"""The inputs of tests/test_frame_sizes_gpu.py (tests/frame_sizes.py) on the CPU: at every frame the oracle's planes of
gpu_support.edge_scene(SEED, W, H) tell a right kernel from a wrong one.  A GPU case whose expectation is all-kept, all-filtered
or nothing-drawn proves nothing, so each condition is asserted at every frame where it can hold, and the frames where it
cannot are named here with the reason."""
import numpy as np
import pytest

import frame_sizes as FS
import gpu_support as K
from bench_support import points_check as PC
from bench_support import voxel_free_check as VF

FRAME_IDS = [FS.frame_id(f) for f in FS.FRAMES]
# one pixel per stream: no window, disc or per-link threshold reaches another pixel or changes the one there
ONE_PIXEL = (1, 1)


def test_the_frames_are_the_thirteen_and_the_subsets_are_among_them():
    assert len(FS.FRAMES) == 13 == len(set(FS.FRAMES)) and all(1 <= W <= 2048 and 1 <= H <= 2048 for W, H in FS.FRAMES)
    assert set(FS.MAX_DILATION_FRAMES) <= set(FS.FRAMES) and len(FS.MAX_DILATION_FRAMES) == 9
    assert set(FS.VOXEL_FRAMES) <= set(FS.FRAMES) and len(FS.VOXEL_FRAMES) == 5
    assert sorted(f for f in FS.FRAMES if f[0] % 4) == [(1, 1), (1, 2048), (3, 5), (65, 33), (2047, 3)]
    assert all(W * H <= 74000 for W, H in FS.FRAMES)


def test_edge_scene_is_soup_scene_where_the_frame_is_at_least_4_to_3():
    """The same draws in the same order, and the same focal length where W >= 4 H / 3."""
    a, b = K.edge_scene(1, 160, 120), K.soup_scene(1, 160, 120)
    assert np.array_equal(a.wl.projection, b.wl.projection) and np.array_equal(a.depth.view(np.uint32), b.depth.view(np.uint32))
    assert np.array_equal(a.wl.link_tf[0], b.wl.link_tf[0]) and np.array_equal(a.wl.cam_tf, b.wl.cam_tf) and np.array_equal(a.wl.offset_inv, b.wl.offset_inv)
    assert np.array_equal(a.mask, b.mask) and np.array_equal(a.prim, b.prim)
    assert K.edge_focal(1, 1536) == K.edge_focal(2048, 1536) == 262.5 * 2048 / 320 and K.edge_intrinsics(a, 2) == K.intrinsics(b, 2)
    tall = K.edge_scene(1, 1, 2048)
    assert (tall.prim >= 0).sum() > 1000 > 9 >= (K.soup_scene(1, 1, 2048).prim >= 0).sum()


@pytest.mark.parametrize("frame", FS.FRAMES, ids=FRAME_IDS)
def test_kept_and_filtered_pixels_and_links_on_the_last_column_and_row(frame):
    w = FS.world(frame)
    mask, link = w.sc.mask, w.sc.prim >= 0
    kept, filtered = int((mask == 0).sum()), int((mask != 0).sum())
    assert kept >= 1 and filtered >= 1
    if frame == (1, 1):
        assert (kept, filtered) == (2, 1)
    last_column, last_row = int(link[:, :, -1].sum()), int(link[:, -1, :].sum())
    assert last_column >= 1 and last_row >= 1
    if frame in ((4, 1), (2048, 1)):
        assert last_column == {(4, 1): 1, (2048, 1): 2}[frame]
    for u16 in (False, True):                      # (the 16UC1 sensor planes keep the property)
        k = w.planes("plain", u16)[1]
        assert (k == 0).any() and (k != 0).any()


@pytest.mark.parametrize("frame", FS.FRAMES, ids=FRAME_IDS)
def test_dilation_changes_the_mask(frame):
    w = FS.world(frame)
    changed = int((w.planes("dilate2", False)[1] != w.sc.mask).sum())
    if frame == ONE_PIXEL:
        assert changed == 0                        # the dilated batches still run there; they do not discriminate
    else:
        assert changed >= 3
    if frame in FS.MAX_DILATION_FRAMES:
        more = int((w.planes("dilate16", False)[1] != w.planes("dilate2", False)[1]).sum())
        # at the four smallest frames a window of radius 2 already holds every pixel: radius 16 gives the same mask, from a
        # window that is larger than the image on every side
        assert more == 0 if frame in FS.SMALL_FRAMES else more >= 300


@pytest.mark.parametrize("frame", FS.FRAMES, ids=FRAME_IDS)
def test_per_link_thresholds_change_the_mask_from_60x31_up(frame):
    w = FS.world(frame)
    changed = int((w.planes("thresh", False)[1] != w.sc.mask).sum())
    if frame in FS.SMALL_FRAMES:
        assert changed == 0                        # the threshold variants still run there; they do not discriminate
    else:
        assert changed >= 13


@pytest.mark.parametrize("frame", FS.FRAMES, ids=FRAME_IDS)
def test_padding_reaches_the_clamp_and_changes_the_mask(frame):
    w = FS.world(frame)
    for u16 in (False, True):
        ex = w.padded(u16)
        assert int(ex.R2.max()) == 16 * 16         # some source asks for the clamp or more
        changed = int((ex.mask != w.planes("plain", u16)[1]).sum())
        assert changed == 0 if frame == ONE_PIXEL else changed >= 3


@pytest.mark.parametrize("frame", FS.FRAMES, ids=FRAME_IDS)
def test_the_scene_filters_some_of_what_the_robot_filter_keeps_and_keeps_some(frame):
    w = FS.world(frame)
    for u16 in (False, True):
        robot, scene = w.planes("plain", u16)[1], w.planes("scene", u16)[1]
        assert ((scene != 0) & (robot == 0)).sum() >= 1 and (scene == 0).sum() >= 1
        learned = w.learned(u16)
        assert np.isfinite(learned).any() and (np.isinf(learned).any() or frame == ONE_PIXEL)


@pytest.mark.parametrize("frame", FS.FRAMES, ids=FRAME_IDS)
def test_point_lists_hold_kept_filtered_and_outside_points(frame):
    w = FS.world(frame)
    lists = w.point_lists()
    assert len({len(p) for p in lists}) == len(lists)          # the lists end at different places
    for r in FS.POINT_RADII:
        total = np.array([PC.summary(v[0]) for v in w.point_verdicts(r)]).sum(axis=0)
        assert (total[:3] >= 10).all(), total


@pytest.mark.parametrize("frame", FS.FRAMES, ids=FRAME_IDS)
def test_the_compacted_capacity_cuts_one_stream_and_not_another(frame):
    w = FS.world(frame)
    for mode in ("plain",):                        # (the compacted form runs in the plain contexts)
        for u16 in (False, True):
            counts = [c[2] for c in w.cloud(mode, u16)[1]]
            cap = w.capacity(mode, u16)
            assert 1 <= cap <= frame[0] * frame[1]
            if max(counts) - min(counts) >= 2:     # (1 x 1 and 4 x 1 keep too few pixels for a capacity in between)
                assert min(counts) < cap < max(counts)
            else:
                assert frame in ((1, 1), (4, 1))


@pytest.mark.parametrize("frame", FS.VOXEL_FRAMES, ids=[FS.frame_id(f) for f in FS.VOXEL_FRAMES])
def test_voxels_are_occupied_free_and_unseen(frame):
    w = FS.world(frame)
    assert 2000 <= FS.GRID.n_voxels <= 5000 and FS.GRID.n_voxels % 32 != 0
    for u16 in (False, True):
        bits, counts, summary = w.voxel_insert(u16)
        free, carved = w.voxel_carve(u16)
        occupied, free = VF.unpack(bits, FS.GRID), VF.unpack(free, FS.GRID)
        assert occupied.sum() >= 10 and free.sum() >= 40 and (~occupied & ~free).sum() >= 1000
        assert summary[:, 0].sum() >= 10 and summary[:, 2].sum() >= 10 and int(counts.sum()) == int(summary[:, 0].sum())
        assert (carved[:, :3].sum(axis=0) > 0).all(), carved
