"""CPU: the clip scenes of tests/clip_scenes.py are what their names say, and the oracle renders them as Mesa llvmpipe does.

The census (a float32 restatement of the kernels' classification and clipper) shows per kind that no scene is vacuous: the
planes that cut are the ones the name says, the polygons and vertex pools have the sizes the scene is built for, the ties
are exact.  The oracle's prim plane shows that every link is seen and that the drawn pixels reach the border or the plane's
trace.  tests/golden/llvmpipe/clip_scenes_WxH.npz (tests/golden/generate_llvmpipe_clip.py) holds what the REAL reference
shaders render on llvmpipe for every scene; the oracle must give the same mask and masked depth, and must stop doing so
when its clipper interpolates from the other end point or takes the shaded vertices' viewport form."""
import hashlib

import numpy as np
import pytest

import clip_scenes as C
import scenes as S
from oracle import bindings as O

_stored, _oracle = {}, {}


def stored(W, H):
    if (W, H) not in _stored:
        z = np.load(C.llvmpipe_path(W, H))
        keys = bytes(z["keys"]).decode().split("\n")
        _stored[(W, H)] = (z, {k: i for i, k in enumerate(keys)})
    return _stored[(W, H)]


def oracle(name):
    """(zwin, prim, prim_of_tri) of stream 0 under the whole-millimetre sensor, once."""
    if name not in _oracle:
        wl, prim_of_tri = C.workload(name)
        depth = C.sensor_mm(name)[0].astype(np.float32) * np.float32(0.001)
        r = O.filter_frame(depth, wl.projection[0], wl.oracle_draws(0), wl.offset_inv[0], wl.cam_tf[0], z_near=C.NEAR, z_far=C.FAR,
                           replace_value=5.0, want_debug=True)
        _oracle[name] = (r[2], r[3], prim_of_tri)
    return _oracle[name]


def popcount(a):
    return np.array([bin(int(x)).count("1") for x in a])


def test_the_matrix_stack_is_restated_bit_for_bit():
    for name in ("plane_px", "ties", "levers"):
        sc = C.scene(name)
        off, cam = sc.cameras(3)
        for s in range(3):
            out, op = np.zeros(16, np.float32), np.zeros(3, np.float32)
            a = [np.ascontiguousarray(m, np.float64) for m in (sc.P, off[s], cam[s], C.IDENTITY)]
            O.lib().rtuf_oracle_compose_mvp(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, 0, op.ctypes.data, out.ctypes.data)
            assert np.array_equal(out, C.compose_mvp(sc.P, off[s], cam[s], C.IDENTITY)[0]), (name, s)


def test_the_census_agrees_with_the_oracle_on_what_is_set_up():
    """The oracle takes in every triangle and sets up the fan triangles with snapped area of every clipped polygon, and
    every triangle with area that lies inside all planes: the census counts the same."""
    for name in C.NAMES:
        sc, cs = C.scene(name), C.scene(name).census()
        wl, _ = C.workload(name)
        depth = np.zeros((sc.H, sc.W), np.float32)
        dbg = O.filter_frame(depth, wl.projection[0], wl.oracle_draws(0), wl.offset_inv[0], wl.cam_tf[0], want_debug=True)[4]
        bg = O.filter_frame(depth, wl.projection[0], [], wl.offset_inv[0], wl.cam_tf[0], want_debug=True)[4]
        x, y = C.window_vs(sc.clip(), sc.W, sc.H)
        with np.errstate(invalid="ignore"):          # (a vertex with w == 0 has no window position; its triangle is clipped)
            whole = (cs.ormask == 0) & ((x[:, 0] - x[:, 1]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 0] - y[:, 1]) != 0)
        assert dbg[0] - bg[0] == len(sc.eye) and not cs.bad.any(), name
        assert dbg[1] - bg[1] == np.where(cs.needs_clip, cs.fan, whole).sum(), (name, dbg, bg)


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.kind_of(n) == "plane"])
def test_plane_scenes_cross_their_plane_only(name):
    sc, cs = C.scene(name), C.scene(name).census()
    assert cs.needs_clip.all() and (cs.cut == C.planes_of(name)).all() and (cs.pool == 5).all(), name
    for case in ("ccw", "cw"):          # one vertex outside: a quad; two: a triangle
        assert set(cs.poly[sc.cases(case)].tolist()) == {3, 4}, (name, case)
    assert (cs.area2[sc.cases("ccw")] > 0).all() != (cs.area2[sc.cases("cw")] > 0).all() and (cs.area2 != 0).all(), name
    # every crossing edge that two triangles share is cut by both, from different ends, to the same vertex
    clip = sc.clip()
    made = {}
    for t in range(len(sc.eye)):
        for k in np.flatnonzero(cs.made[t]):
            made.setdefault((cs.sx[t, k], cs.sy[t, k]), set()).add(t)
    edges = {}
    for t in range(len(sc.eye)):
        for i in range(3):
            a, b = clip[t, i].tobytes(), clip[t, (i + 1) % 3].tobytes()
            if (C.clipmask_of(clip[t, i]) != 0) != (C.clipmask_of(clip[t, (i + 1) % 3]) != 0):
                edges.setdefault(frozenset((a, b)), []).append((a, b))
    shared = [e for e in edges.values() if len(e) == 2]
    assert len(shared) == 18 and all(e[0] == e[1][::-1] for e in shared), (name, len(shared))          # 9 per strip, walked both ways
    assert sum(len(ts) == 2 for ts in made.values()) == len(shared) and sum(len(ts) == 1 for ts in made.values()) == 4, name
    assert len(set(sc.colour)) == 3


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.kind_of(n) == "corner"])
def test_corner_scenes_cover_their_corner(name):
    sc, cs = C.scene(name), C.scene(name).census()
    want = C.planes_of(name)
    planes = popcount([want])[0]
    assert planes in (2, 3) and cs.needs_clip.all(), name
    corner, side = sc.cases("corner"), sc.cases("side")
    assert (cs.cut[corner] == want).all() and (cs.pool[corner] == 3 + 2 * planes).all(), (name, cs.cut, cs.pool)
    assert (cs.cut[side] & ~want == 0).all() and (popcount(cs.cut[side]) == planes - 1).all() and (cs.pool[side] == 1 + 2 * planes).all(), name
    assert np.bitwise_or.reduce(cs.cut) == want and cs.pool.max() >= 7 and cs.pool.max() > C.CLIP_LDS_V - (planes == 2) * 2, name
    # the corner triangles are drawn along both borders; without a depth plane up to the frame's corner pixel (beyond the
    # near or far plane the frustum's corner edge is cut away, and the background shows)
    _, prim, pot = oracle(name)
    x = sc.W - 1 if "px" in name else 0
    y = sc.H - 1 if "py" in name else 0
    assert np.isin(prim[:, x], pot[corner]).any() and np.isin(prim[y, :], pot[corner]).any(), name
    if planes == 2:
        assert prim[y, x] in pot[corner], (name, prim[y, x])


def test_around_scene():
    sc, cs = C.scene("around"), C.scene("around").census()
    assert (C.clipmask_of(sc.clip()) != 0).all(), "a vertex lies inside the frustum"
    m = sc.cases("contains")
    assert (cs.cut[m] == 15).all() and (cs.poly[m] == 4).all()
    m = sc.cases("six")
    assert m.sum() == 4 and (cs.cut[m] == 63).all() and (cs.poly[m] == 9).all() and (cs.pool[m] == 15).all()
    assert (cs.area2[m] > 0).sum() == 2 and (cs.area2[m] < 0).sum() == 2
    m = sc.cases("miss")
    assert cs.needs_clip[m].all() and (cs.poly[m] == 0).all() and (cs.andmask[m] == 0).all() and (cs.ormask[m] != 0).all()
    m = sc.cases("thin")
    assert (cs.poly[m] == 4).all() and (cs.area2[m] == 0).all() and (cs.fan[m] == 0).all() and set(cs.cut[m].tolist()) == {3, 12}


def test_tie_scenes_are_exact():
    sc, cs = C.scene("ties"), C.scene("ties").census()
    planes = set()
    for t, case in enumerate(sc.case):
        kind, p = case.rsplit("_", 1)
        planes.add(p)
        d = cs.dist[t, :, C.PLANES.index(p)]
        assert (d == 0).sum() == (1 if kind.startswith("on") else 2), (case, d)          # exactly on the plane
        assert bool(cs.needs_clip[t]) == kind.endswith("out") and (d < 0).sum() == int(kind.endswith("out")), (case, d)
        if kind == "edge_out":
            assert cs.area2[t] == 0, case
        if kind == "on_out":
            assert cs.area2[t] != 0 and cs.cut[t] == 1 << C.PLANES.index(p) and cs.pool[t] == 5, case
    for p in ("near", "far"):
        assert (p in planes) != ("skipped_" + p in sc.notes), sc.notes
    assert planes >= {"px", "nx", "py", "ny"}
    un = C.scene("ties_unclipped")
    assert not un.census().needs_clip.any() and len(un.eye) == len(sc.eye) // 2


def test_behind_scene():
    sc, cs = C.scene("behind"), C.scene("behind").census()
    w = sc.clip()[..., 3]
    assert cs.needs_clip.all() and (cs.poly >= 3).all()
    assert (w[sc.cases("w_negative")].min(1) < 0).all()
    for s in range(5):          # stream s looks from s/64 m to the side: w is as exact as in stream 0, x is not the same
        assert ((sc.clip(s)[..., 3][sc.cases("w_zero")] == 0).sum(1) == 1).all() and np.array_equal(sc.clip(s)[..., 3], w)
        assert (s == 0) == np.array_equal(sc.clip(s)[..., 0], sc.clip()[..., 0])
    assert ((sc.clip()[sc.cases("eye")][..., [0, 1, 3]] == 0).all(2).sum(1) == 1).all()
    m = sc.cases("needle")
    assert m.sum() == 24 and (w[m].min(1) < -0.4).all() and (w[m].max(1) > 0.3).all()


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.kind_of(n) == "grazing"])
def test_grazing_chunks_reach_in_by_less_than_the_slack(name):
    sc = C.scene(name)
    p = C.PLANES.index(name.split("_")[1])
    mv, col = sc.model_verts(), np.asarray(sc.colour)
    assert (col == 0).sum() == 40 and (col == 1).sum() == 40
    for s in range(5):          # (stream s looks from s/64 m along the plane: the same margins)
        M = sc.mvp(s)[0]
        reach_in, reach, slack = C.chunk_margin(M, mv[col == 0].reshape(-1, 3), p)
        assert 0 < reach_in < 0.001 * reach and reach_in < slack - reach, (name, s, reach_in, reach, slack)
        reach_in, reach, slack = C.chunk_margin(M, mv[col == 1].reshape(-1, 3), p)
        assert reach_in < -0.01 * reach and reach_in - reach < -slack, (name, s, reach_in, reach, slack)
        assert not np.array_equal(M, sc.mvp(0)[0]) or s == 0
    _, prim, pot = oracle(name)
    assert np.isin(prim, pot[sc.cases("reach") & (col == 0)]).sum() >= 5, name
    assert not np.isin(prim, pot[col == 1]).any(), name


def test_walls_scene():
    sc, cs = C.scene("walls"), C.scene("walls").census()
    wall = sc.cases("wall")
    assert (cs.cut[wall] & 16 != 0).any() and (cs.cut[wall] & 15 != 0).all() and cs.pool[wall].max() > C.CLIP_LDS_V
    _, prim, pot = oracle("walls")
    won = np.isin(prim, pot[wall])
    whole = [(tx, ty) for ty in range(0, sc.H, 32) for tx in range(0, sc.W, 64) if won[ty:ty + 32, tx:tx + 64].all()]
    assert whole, "no tile is covered completely"
    inside = np.arange(C.CLIP_MAX_P)[None] < cs.poly[wall][:, None]
    x, y = cs.sx[wall] / 256 + 0.5, cs.sy[wall] / 256 + 0.5
    tiles = (np.where(inside, x, -1).max(1) // 64 - np.maximum(np.where(inside, x, 1e9).min(1), 0) // 64 + 1) * \
            (np.where(inside, y, -1).max(1) // 32 - np.maximum(np.where(inside, y, 1e9).min(1), 0) // 32 + 1)
    assert (tiles > C.COOP_TILES).all(), tiles          # (the fans' triangles: at least one of each polygon spans as much)


def test_levers_scene():
    sc, cs = C.scene("levers"), C.scene("levers").census()
    assert len(sc.eye) == 64 and C.levers_ok(sc) and not cs.bad.any()
    lo, hi = C._outside(sc, cs)
    assert lo.any() and hi.any() and (cs.pool == 15).any()
    # ... and never by more than one unit of 1/256 px
    m = cs.made
    assert cs.sx[m].min() >= -129 and cs.sy[m].min() >= -129 and cs.sx[m].max() <= 256 * sc.W - 127 and cs.sy[m].max() <= 256 * sc.H - 127


@pytest.mark.parametrize("name", C.NAMES)
def test_clipper_made_vertices_snap_at_most_one_unit_outside_the_frame(name):
    """Measured on the census, every stream of a batch of five: what the records' packed coordinates must hold."""
    sc = C.scene(name)
    for s in range(5):
        cs = sc.census(s)
        m = cs.made
        if m.any():
            assert cs.sx[m].min() >= -129 and cs.sy[m].min() >= -129 and cs.sx[m].max() <= 256 * sc.W - 127 and cs.sy[m].max() <= 256 * sc.H - 127, (name, s)


def test_many_scene_overflows_a_fresh_clip_list():
    sc, cs = C.scene("many"), C.scene("many").census()
    assert len(sc.eye) > C.COUNTER_SHARDS * C.CLIP_CAPACITY and len(sc.eye) % C.CHUNK_TRIS == 0
    assert cs.needs_clip.all() and (popcount(cs.cut) >= 3).all() and (cs.pool >= 9).all() and not cs.bad.any()
    wl, _ = C.workload("many")
    assert all(len(d.tris) == C.CHUNK_TRIS and len(np.unique(d.verts, axis=0)) <= 258 for link in wl.models[0] for d in link)


@pytest.mark.parametrize("name", C.NAMES)
def test_every_link_is_seen(name):
    sc = C.scene(name)
    _, prim, pot = oracle(name)
    col = np.asarray(sc.colour)
    for c in sorted(set(sc.colour)):
        n = int(np.isin(prim, pot[col == c]).sum())
        assert (n == 0) == (c in sc.nothing), (name, c, n)


def trace_segments(sc, cs):
    """Window-space segments between consecutive polygon vertices that both lie on a frustum plane (the clipper made them,
    or their plane distance is exactly 0): the frame's border or the trace of the near or far plane."""
    clip = sc.clip()
    segs = []
    for t in range(len(sc.eye)):
        if cs.needs_clip[t]:
            n = int(cs.poly[t])
            pts = [(cs.sx[t, k] / 256 + 0.5, cs.sy[t, k] / 256 + 0.5, bool(cs.made[t, k])) for k in range(n)]
        else:
            x, y = C.window_vs(clip[t], sc.W, sc.H)
            pts = [(x[k] / 256 + 0.5, y[k] / 256 + 0.5, bool((cs.dist[t, k] == 0).any())) for k in range(3)]
        segs += [(a[:2], b[:2]) for a, b in zip(pts, pts[1:] + pts[:1]) if a[2] and b[2]]
    return segs


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.kind_of(n) in ("plane", "corner", "ties")])
def test_drawn_pixels_reach_the_border_or_the_trace(name):
    sc, cs = C.scene(name), C.scene(name).census()
    _, prim, _ = oracle(name)
    yy, xx = np.mgrid[0:sc.H, 0:sc.W]
    px, py = xx + 0.5, yy + 0.5
    close = np.zeros((sc.H, sc.W), bool)
    segs = trace_segments(sc, cs)
    for (ax, ay), (bx, by) in segs:
        dx, dy = bx - ax, by - ay
        t = np.clip(((px - ax) * dx + (py - ay) * dy) / max(dx * dx + dy * dy, 1e-12), 0, 1)
        close |= np.hypot(px - ax - t * dx, py - ay - t * dy) <= 2.0
    n = int((close & (prim >= 0)).sum())
    assert len(segs) >= 4 and n >= 30, (name, len(segs), n)


# ---- the oracle against llvmpipe ---------------------------------------------------------------------------------------------

def test_every_scene_is_stored():
    for W, H in C.FRAMES:
        z, index = stored(W, H)
        keys = [k for n in C.llvmpipe_names(W, H) for k, *_ in C.llvmpipe_frames(n)]
        assert sorted(keys) == sorted(index) and len(z["mask_bits"]) == len(keys)
        assert b"llvmpipe" in bytes(z["renderer"])
    assert sorted(n for W, H in C.FRAMES for n in C.llvmpipe_names(W, H)) == sorted(C.NAMES)


def compare_with_stored(name):
    """The keys of the scene's frames whose mask or masked depth the oracle, as it is set now, does not reproduce."""
    sc = C.scene(name)
    z, index = stored(sc.W, sc.H)
    bad = []
    for key, P, depth, offinv, camtf, rend, draws in C.llvmpipe_frames(name):
        i = index[key]
        assert S.scene_digest(P, depth, offinv, camtf, draws) == bytes(z["inputs_sha256"][i]), \
            "%s: tests/clip_scenes.py no longer builds the scene the stored result was rendered from (tests/golden/generate_llvmpipe_clip.py)" % key
        g_mask = np.unpackbits(z["mask_bits"][i])[: sc.W * sc.H].reshape(sc.H, sc.W) * np.uint8(255)
        o_masked, o_mask = O.filter_frame(depth, P, draws, offinv, camtf, z_near=C.NEAR, z_far=C.FAR, replace_value=C.LLVMPIPE_REPLACE)
        if (g_mask != o_mask).any() or hashlib.sha256(np.ascontiguousarray(o_masked).tobytes()).digest() != bytes(z["masked_sha256"][i]):
            bad.append(key)
    return bad


@pytest.mark.parametrize("name", C.NAMES)
def test_clip_scene_matches_llvmpipe(name):
    assert compare_with_stored(name) == []


DEFAULT = {"vs_fma": 0, "vp_fma": 1, "clip_vp_fma": 0, "interp_fma": 1, "frag_div_rcp": 0, "cw_swap_12": 0, "edge_rule_flip": 0, "clip_old_t": 0}


@pytest.mark.parametrize("variant", ["clip_old_t", "clip_vp_fma"])
def test_the_stored_frames_see_the_clipper_s_numerical_choices(variant):
    """With the interpolation from the fixed end point, or with the fused viewport form for the clipper's vertices, the oracle
    no longer reproduces the stored frames: the scenes see both choices."""
    for name in C.NAMES:          # the frames' threshold sensors come from the oracle as it is by default: built before the switch
        C.llvmpipe_frames(name)
    try:
        O.set_variants(**{variant: 1 - DEFAULT[variant]})
        bad = [k for name in C.NAMES if name != "many" for k in compare_with_stored(name)]
    finally:
        O.set_variants(**DEFAULT)
    assert bad, "variant %s changes no stored frame" % variant
    print("%s: %d frames differ, of %s" % (variant, len(bad), sorted({k.split("/")[0] for k in bad})))
