"""The lattice scenes of tests/lattice_scenes.py on the CPU: the oracle against the independent integer rasteriser of
tests/fill_rule.py, and the conditions on the scenes themselves that keep tests/test_fill_rule_gpu.py from passing vacuously.

What the tie conditions ask.  An edge's direction class fixes whether it owns its boundary (a top edge always does, a bottom
edge never), so "owned and not owned" cannot both occur within one class: they are asked of the two classes of every line
family (the two sides of the same lines), and within every owning class the ties must show both outcomes for the pixel -- the
triangle got it, and the triangle did not get it because another of its edges gave it away (a vertex on a pixel centre).  On
an edge that does not own its boundary no tie pixel may be covered at all."""
import numpy as np
import pytest

import fill_rule as F
import lattice_scenes as L
from oracle import bindings as O

OWNING = ("horizontal_top", "vertical_left", "diagonal_left_upper", "diagonal_left_lower")


def oracle_prim(name):
    sc = L.scene(name)
    wl, _ = L.workload(name)
    depth = np.full((sc.H, sc.W), 3.0, np.float32)
    _, _, _, prim, _ = O.filter_frame(depth, wl.projection[0], wl.oracle_draws(0), wl.offset_inv[0], wl.cam_tf[0], z_near=L.NEAR, z_far=L.FAR,
                                      want_debug=True)
    return prim


@pytest.mark.parametrize("name", L.NAMES)
def test_oracle_gives_every_pixel_to_the_triangle_the_rule_names(name):
    want, got = L.expected_prim(name), oracle_prim(name)
    bad = want != got
    assert not bad.any(), "%s: %d pixels differ, first (y, x) %s: oracle %d, rule %d" % (
        name, int(bad.sum()), tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


@pytest.mark.parametrize("name", L.NAMES)
def test_partitions_cover_every_pixel_exactly_once(name):
    sc = L.scene(name)
    _, count, _ = L.reference(name)
    want = sc.expected_count()
    assert want.any()
    assert np.array_equal(count[want > 0], want[want > 0]), "%s: %d pixels of its partitions" % (name, int((count != want)[want > 0].sum()))
    zs = np.asarray(sc.zs)
    for z in np.unique(zs):                        # no two triangles of one depth overlap anywhere
        layer = [t for t, tz in zip(sc.tris, zs) if tz == z]
        assert F.rasterise(layer, sc.W, sc.H)[1].max() <= 1, (name, z)
    for t in sc.degenerate:
        assert F.oriented(sc.tris[t]) is None and F.triangle_coverage(sc.tris[t], sc.W, sc.H) is None
    assert len(sc.degenerate) == (4 if name.startswith("tiny") else 0)


@pytest.mark.parametrize("name", L.NAMES)
def test_scenes_hold_the_ties_they_are_built_for(name):
    tally = L.reference(name)[2]
    for cls in F.CLASS_NAMES:
        if cls not in OWNING:
            assert tally.owned(cls) == 0 and tally.covered(cls) == 0, (name, cls)
        else:
            assert tally.not_owned(cls) == 0, (name, cls)
    if name.startswith("limit"):
        for family, (a, b) in F.FAMILIES.items():          # rows, columns and both diagonals of 2048 pixels
            assert tally.total(a) >= 2048 and tally.total(b) >= 2048, (name, family, tally.ties)
        return
    for cls in F.CLASS_NAMES:
        assert tally.total(cls) >= 8, (name, cls, tally.ties[cls])
    for family, pair in F.FAMILIES.items():
        assert sum(tally.owned(c) for c in pair) >= 8 and sum(tally.not_owned(c) for c in pair) >= 8, (name, family)
    for cls in OWNING:
        assert tally.covered(cls) >= 1 and tally.not_covered(cls) >= 1, (name, cls, tally.ties[cls])


@pytest.mark.parametrize("name", L.NAMES)
def test_scenes_reach_the_paths_they_are_built_for(name):
    """The size classes as rtuf_kernels.hip has them at this commit (quoted in tests/lattice_scenes.py)."""
    sc = L.scene(name)
    kind = name.split("_")[0]
    frag = sc.fragment_sized()
    boxes = sc.boxes()
    live = (boxes[:, 2] >= boxes[:, 0]) & (boxes[:, 3] >= boxes[:, 1])
    areas, ntiles = sc.tile_clipped_areas()
    if kind == "tiny":
        assert frag[live].all()
        w, h = (boxes[:, 2] - boxes[:, 0] + 1)[live], (boxes[:, 3] - boxes[:, 1] + 1)[live]
        assert w.max() == 2 and h.max() == 2
        assert (ntiles == 2).sum() >= 16 and (ntiles == 4).sum() >= 4          # across a tile border; across four tiles
        assert sc.filled == 3 * 16 * len(L.OFFSETS)                             # every shape, variant and offset found a place
    elif kind == "small":
        assert frag.sum() >= 200 and (live & ~frag).sum() >= 50               # inside one tile; across a border: records
        assert areas[areas > 0].max() <= L.FRONT_AREA
        assert sc.filled >= 5 * 16 * 3                                          # every shape and variant at three offsets or more
    elif kind == "records":
        for limit in (L.FRONT_AREA, L.SMALL_AREA, L.QUARTER_AREA, L.WALL_AREA):
            below, above = areas[areas <= limit].max(), areas[areas > limit].min()
            assert below == limit and above - limit <= 2, (name, limit, below, above)
        assert (ntiles == L.COOP_TILES).any() and ((ntiles > L.COOP_TILES).any() or name.startswith("records_160x120"))
        # the 48 x 32 and the 53 x 29 rectangle's tiles hold more than kParkBelow records
        for tx in (0, 1):
            in_tile = (boxes[:, 0] // L.TILE_W <= tx) & (boxes[:, 2] // L.TILE_W >= tx) & (boxes[:, 1] // L.TILE_H == 0) & live
            assert in_tile.sum() > L.PARK_BELOW, (name, tx, int(in_tile.sum()))
    elif kind == "tiles":
        assert (ntiles > L.COOP_TILES).any()          # big records: the cover pass and the drop test see them
    else:
        assert kind == "limit" and sc.W == 2048 and len(sc.tris) == 10
    b = sc.boxes()
    x = np.asarray(sc.tris)
    if sc.W in (160, 200) and kind in ("tiny", "small", "records"):           # the last, partial tile column and row
        assert (b[live, 2] == sc.W - 1).any() and (b[live, 3] == sc.H - 1).any()
        assert (x[..., 0] == 256 * sc.W - 128).any() and (x[..., 1] == 256 * sc.H - 128).any()      # vertices on the frame's border
