"""Scenes that cross the frustum's planes, corners and ties (test helper for the clipper tests), and a census of what
the classification and the clipper do with every triangle of them.

A scene is a list of triangles given in EYE coordinates (what the camera matrices make of a model vertex: clip x grows
with x, clip y with y, and z is clip w, the distance along the view axis), each with a colour, a case name and a draw
number.  One robot link per colour, so the label and virtual depth planes show which triangle won a pixel; a link holds
one draw per draw number.  Two projections:

  exact    lattice_scenes.projection() with the identity camera: clip = (x, y, A z + B, z) with no rounding in x, y and w,
           so a vertex with |x| == z or |y| == z lies ON a side plane and the census is exact.  The tie scenes use it, and
           their streams are identical.  So do `behind` (w == 0 needs it) and the grazing scenes (a rotated camera
           inflates a chunk's box): there stream s looks from s/64 m to the side, a translation that leaves w exact and,
           in the grazing scenes, runs along the grazed plane.
  generic  scenes.projection() with an off-centre principal point and scenes.random_camera(): the model coordinates are
           the eye coordinates taken back through stream 0's camera in float64 and cast to float32.  Stream s looks from a
           pose a few millimetres and milliradians away, so every stream clips differently.

The census restates in float32 what realtime_urdf_filter_amd/csrc/rtuf_kernels.hip computes (the matrix stack of
pose_kernel, vs_position, clipmask_of, the reject / clip / keep decision of the set-up kernel's phase 2 and clip_one's plane
loop with its interpolation from the end point nearer the plane; viewport_clip and snap for the vertices the clipper
makes) and returns per triangle the clip masks, the planes that made a vertex, the vertex pool's size, the polygon's size and
the snapped position of every clipper-made vertex of the final polygon.  Only viewport_vs (a fused multiply-add) is
evaluated in float64 and rounded once more: the census uses it for nothing but the zero-area case of `around`.

Constants the scenes are sized against (quoted, not imported): kClipLdsV = 8 (pool indices 0 .. 7 live in LDS, 8 .. 15 in
the per-thread global spill area), kClipMaxV = 16, kClipMaxP = 12, kClipBlock = 128, RTUF_COUNTER_SHARDS = 64, the
initial clip_capacity of a context of up to 8 streams = 1024 items per shard (it grows fourfold on overflow),
kCoopTiles = 4, a set-up chunk = at most 256 triangles of one draw, chunk_outside_plane's slack = 0.1 % of the box's
reach along the plane normal (+ 1e-5 (|w| + |coordinate|) of its centre)."""
import os

import numpy as np

import lattice_scenes as L
import scenes as S
from bench_support import workloads as WL

CLIP_LDS_V, CLIP_MAX_V, CLIP_MAX_P, CLIP_BLOCK, COUNTER_SHARDS, CLIP_CAPACITY, COOP_TILES, CHUNK_TRIS = 8, 16, 12, 128, 64, 1024, 4, 256
NEAR, FAR = 0.1, 8.0
PLANES = ("px", "nx", "py", "ny", "near", "far")          # bit i of a clip mask, in the clipper's order
F32 = np.float32
IDENTITY = L.IDENTITY


# ---- float32 restatements ---------------------------------------------------------------------------------------------

def matmul4(a, b):
    """out = a x b on column-major 16-vectors, every sum in float32 in the kernels' order."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    out = np.zeros(16, F32)
    for i in range(4):
        for j in range(4):
            s = a[i] * b[4 * j]
            for k in range(1, 4):
                s = F32(s + a[i + 4 * k] * b[4 * j + k])
            out[4 * j + i] = s
    return out


def compose_mvp(P, offset_inv, cam_tf, link_tf):
    """The float32 model-view-projection matrix of a draw without a scale or translate operation, and the background
    quad's (projection x look-at only)."""
    eye = np.eye(4, dtype=F32).reshape(16)
    proj = matmul4(eye, np.asarray(P, np.float64).astype(F32))
    mv = matmul4(eye, np.array([-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1], F32))
    bg = matmul4(proj, mv)
    for m in (offset_inv, cam_tf, link_tf):
        mv = matmul4(mv, np.asarray(m, np.float64).astype(F32))
    return matmul4(proj, mv), bg


def vs_position(M, v):
    """[n, 3] float32 vertices -> [n, 4] clip coordinates."""
    v = np.asarray(v, F32)
    c = np.empty((len(v), 4), F32)
    for r in range(4):
        s = M[r] * v[:, 0]
        s = s + M[4 + r] * v[:, 1]
        s = s + M[8 + r] * v[:, 2]
        c[:, r] = s + M[12 + r]
    return c


def clipmask_of(c):
    z = F32(0)
    return ((c[..., 0] > c[..., 3]) * 1 | (z > c[..., 0] + c[..., 3]) * 2 | (c[..., 1] > c[..., 3]) * 4 | (z > c[..., 1] + c[..., 3]) * 8
            | (z > c[..., 2] + c[..., 3]) * 16 | (c[..., 2] > c[..., 3]) * 32).astype(np.int64)


def clipdist(c, plane):
    """dot4(clip, plane) as the kernel sums it (the products with 0 and +-1 are exact)."""
    k, sign = plane >> 1, (-1 if plane & 1 == 0 else 1)
    if plane == 4:
        k, sign = 2, 1
    elif plane == 5:
        k, sign = 2, -1
    return (F32(sign) * c[..., k] + c[..., 3]).astype(F32)


def snap(v):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.rint(((v - F32(0.5)) * F32(256)).astype(F32)).astype(np.float64)


def window_clip(c, W, H):
    """viewport_clip + snap of [..., 4] clip coordinates: (snapped x, snapped y)."""
    with np.errstate(all="ignore"):
        oow = F32(1) / c[..., 3]
        sx, sy = F32(0.5 * W), F32(0.5 * H)
        return snap(c[..., 0] * oow * sx + sx), snap(c[..., 1] * oow * sy + sy)


def window_vs(c, W, H):
    """viewport_vs + snap (the fused multiply-add in float64, rounded once more)."""
    with np.errstate(all="ignore"):
        rhw = F32(1) / c[..., 3]
        sx, sy = 0.5 * W, 0.5 * H
        f = lambda t, s: (np.float64(t) * s + s).astype(F32)
        return snap(f(c[..., 0] * rhw, sx)), snap(f(c[..., 1] * rhw, sy))


class Census:
    """Per triangle: ormask, andmask, needs_clip, cut (bit p: plane p made a vertex), pool (vertices in the pool at the
    end), poly (vertices of the final polygon, 0 if it is dropped), made [n, 12] bool (the polygon's vertex is the clipper's),
    sx, sy [n, 12] (snapped window position of the polygon's vertices), area2 (twice the snapped polygon's signed area), fan (its
    fan triangles with snapped area), dist [n, 3, 6] (the vertices' plane distances)."""


def clip_census(clip, W, H):
    """clip: [n, 3, 4] float32 clip coordinates of n triangles.  Restates clip_one, all triangles at once."""
    n = len(clip)
    cs = Census()
    masks = clipmask_of(clip)
    cs.ormask, cs.andmask = masks[:, 0] | masks[:, 1] | masks[:, 2], masks[:, 0] & masks[:, 1] & masks[:, 2]
    cs.needs_clip = (cs.andmask == 0) & (cs.ormask != 0)
    cs.dist = np.stack([clipdist(clip, p) for p in range(6)], -1)
    pool = np.zeros((n, CLIP_MAX_V, 4), F32)
    pool[:, :3] = clip
    npool = np.full(n, 3)
    inl = np.zeros((n, CLIP_MAX_P + 1), np.int64)
    inl[:, :3] = [0, 1, 2]
    nv = np.where(cs.needs_clip, 3, 0)
    bad = np.zeros(n, bool)
    cut = np.zeros(n, np.int64)
    rows = np.arange(n)
    for plane in range(6):
        act = (cs.ormask >> plane & 1 == 1) & (nv >= 3) & ~bad
        bad |= act & (nv >= CLIP_MAX_P)
        act &= ~bad
        if not act.any():
            continue
        outl = np.zeros_like(inl)
        outc = np.zeros(n, np.int64)
        prev = inl[:, 0].copy()
        cprev = pool[rows, prev]
        dprev = clipdist(cprev, plane)
        for i in range(1, CLIP_MAX_P + 1):
            live = act & (i <= nv) & ~bad
            if not live.any():
                break
            cur = np.where(i == nv, inl[:, 0], inl[:, min(i, CLIP_MAX_P)])
            ccur = pool[rows, cur]
            dp = clipdist(ccur, plane)
            keep = live & (dprev >= 0)
            over = keep & (outc >= CLIP_MAX_P)
            bad |= over
            keep &= ~over
            outl[rows[keep], outc[keep]] = prev[keep]
            outc[keep] += 1
            diff = live & ~bad & np.where(dprev >= 0, dp < 0, ~(dp < 0))
            over = diff & ((npool >= CLIP_MAX_V) | (outc >= CLIP_MAX_P))
            bad |= over
            diff &= ~over
            if diff.any():
                d, dq = dp[diff], dprev[diff]
                with np.errstate(all="ignore"):
                    denom = (d - dq).astype(F32)
                    from_cur = np.where(d < 0, dq > -d, ~(d > -dq))
                    tt = np.where(from_cur, d / denom, -dq / denom).astype(F32)
                    o = np.where(from_cur[:, None], ccur[diff], cprev[diff])
                    q = np.where(from_cur[:, None], cprev[diff], ccur[diff])
                    nc = (((q - o).astype(F32) * tt[:, None]).astype(F32) + o).astype(F32)
                pool[rows[diff], npool[diff]] = nc
                outl[rows[diff], outc[diff]] = npool[diff]
                outc[diff] += 1
                npool[diff] += 1
                cut[diff] |= 1 << plane
            upd = live
            prev, cprev, dprev = np.where(upd, cur, prev), np.where(upd[:, None], ccur, cprev), np.where(upd, dp, dprev)
        inl = np.where(act[:, None], outl, inl)
        nv = np.where(act, outc, nv)
    nv = np.where(bad | (nv < 3), 0, nv)
    cs.cut, cs.pool, cs.poly, cs.bad = cut, np.where(cs.needs_clip, npool, 0), nv, bad
    idx = inl[:, :CLIP_MAX_P]
    inside = np.arange(CLIP_MAX_P)[None] < nv[:, None]
    cs.made = inside & (idx >= 3)
    pc = pool[rows[:, None], idx]
    cx, cy = window_clip(pc, W, H)
    vx, vy = window_vs(pc, W, H)
    cs.sx, cs.sy = np.where(idx >= 3, cx, vx), np.where(idx >= 3, cy, vy)
    cs.sx[~inside], cs.sy[~inside] = 0, 0
    x, y = cs.sx, cs.sy          # twice the snapped polygon's signed area (shoelace over its vertices)
    x1, y1 = np.roll(x, -1, 1), np.roll(y, -1, 1)
    last = np.arange(CLIP_MAX_P)[None] == nv[:, None] - 1
    x1, y1 = np.where(last, x[:, :1], x1), np.where(last, y[:, :1], y1)
    cs.area2 = np.where(inside, x * y1 - x1 * y, 0).sum(1)
    # fan triangles (v[i-1], v[i], v[0]) with snapped area: what is set up of the polygon
    fan = np.zeros(n, np.int64)
    for i in range(2, CLIP_MAX_P):
        a = (x[:, i - 1] - x[:, i]) * (y[:, 0] - y[:, i - 1]) - (x[:, 0] - x[:, i - 1]) * (y[:, i - 1] - y[:, i])
        fan += (i < nv) & (a != 0)
    cs.fan = fan
    return cs


def background_clipped(bg_mvp, far=FAR):
    """How many of the background quad's two triangles go through the clipper: none where pose_kernel finds that the quad
    is a constant plane around the whole view (its mode 1: the tile kernel then starts from its depth), else both."""
    zq = F32(np.float64(F32(far)) * 0.99)
    c = vs_position(bg_mvp, np.array([[-100, -100, zq], [100, -100, zq], [100, 100, zq], [-100, 100, zq]], F32))
    m = clipmask_of(c)
    ok = (c[:, 2] == c[0, 2]).all() and (c[:, 3] == c[0, 3]).all() and not (m & 48).any() and (c[:, 3] > 0).all()
    ok = ok and (np.abs(c[:, 0]) > 2 * c[:, 3]).all() and (np.abs(c[:, 1]) > 2 * c[:, 3]).all() and np.bitwise_and.reduce(m) == 0
    neg = c[:, :2] < 0
    ok = ok and neg[0, 0] != neg[1, 0] and neg[1, 1] != neg[2, 1] and neg[2, 0] != neg[3, 0] and neg[3, 1] != neg[0, 1]
    return 0 if ok else 2


def chunk_margin(M, verts, plane):
    """chunk_outside_plane in float64 for the box of `verts`: (d + reach, reach, slack): the box counts as outside where
    d + reach < reach - slack, i.e. d < -slack.  d + reach > 0: a corner of the box lies inside the plane."""
    v = np.asarray(verts, np.float64)
    lo, hi = v.min(0), v.max(0)
    cen, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    M = np.asarray(M, np.float64)
    k, sg = (plane >> 1, 1.0 if plane & 1 else -1.0) if plane < 4 else (2, 1.0 if plane == 4 else -1.0)
    row = lambda r: np.array([M[r], M[4 + r], M[8 + r]])
    cw, ck = row(3) @ cen + M[15], row(k) @ cen + M[12 + k]
    nrm = row(3) + sg * row(k)
    d = cw + sg * ck
    reach = np.abs(nrm) @ half
    return d + reach, reach, reach * 1.001 + 1e-5 * (abs(cw) + abs(ck)) + 1e-30


# ---- scenes -------------------------------------------------------------------------------------------------------------

def generic_projection(W, H):
    f = 262.5 * W / 320.0
    return S.projection(f, 0.97 * f, 0.46 * W, 0.53 * H, W, H, NEAR, FAR)


def _mat(gl16):
    return np.asarray(gl16, np.float64).reshape(4, 4).T


class ClipScene:
    def __init__(self, name, W, H, exact=False, seed=0, shift=None):
        self.name, self.W, self.H, self.exact = name, W, H, exact
        self.shift = shift            # exact scenes: the axis (0: x, 1: y) along which stream s looks from s/64 m off stream 0
        self.eye, self.colour, self.case, self.draw = [], [], [], []
        self.nothing = set()          # colours (links) that draw nothing, on purpose
        self.notes = {}
        if exact:
            self.P = L.projection(W, H)
            self.offset_inv, self.cam_tf = IDENTITY.copy(), IDENTITY.copy()
        else:
            self.P = generic_projection(W, H)
            self.offset_inv, self.cam_tf = S.random_camera(np.random.default_rng(1000 + seed), small=True)

    # -- building -----------------------------------------------------------------------------------------------------
    def ndc(self, u, v, w):
        """The eye coordinates of the point that projects to normalised device (u, v) -- u = +1: the +x plane -- at clip w."""
        P = self.P
        return ((u * w + P[8] * w) / -P[0], (v * w + P[9] * w) / P[5], w)

    def clipc(self, cx, cy, w):
        """The eye coordinates of the point with clip coordinates (cx, cy, ., w)."""
        P = self.P
        return ((cx + P[8] * w) / -P[0], (cy + P[9] * w) / P[5], w)

    def add(self, tri, colour, case, draw=0, flip=False):
        tri = [tuple(float(x) for x in p) for p in tri]
        self.eye.append(tri[::-1] if flip else tri)
        self.colour.append(colour)
        self.case.append(case)
        self.draw.append(draw)

    def add_ndc(self, tri, colour, case, draw=0, flip=False, canon=0):
        """(u, v, w) vertices; canon maps the canonical +x plane onto plane `canon` (0 .. 3) by mirroring and swapping u, v."""
        m = lambda u, v: [(u, v), (-u, v), (v, u), (v, -u)][canon]
        self.add([self.ndc(*m(u, v), w) for u, v, w in tri], colour, case, draw, flip)

    # -- derived --------------------------------------------------------------------------------------------------------
    def cases(self, *names):
        c = np.asarray(self.case)
        return np.isin(c, names) if names else np.ones(len(c), bool)

    def model_verts(self):
        """[n, 3, 3] float32 model coordinates: the eye coordinates (what the camera matrices make of a model vertex, before the
        filter's fixed look-at diag(-1, 1, -1), whose signs the projection's take back) back through stream 0's camera."""
        e = np.asarray(self.eye, np.float64).reshape(-1, 3)
        inv = np.linalg.inv(_mat(self.offset_inv) @ _mat(self.cam_tf))
        m = e @ inv[:3, :3].T + inv[:3, 3]
        return m.astype(F32).reshape(-1, 3, 3)

    def cameras(self, n):
        """(offset_inv [n,16], cam_tf [n,16]): stream s a few millimetres and milliradians off stream 0; in exact scenes not at
        all, or s/64 m along the axis `shift` (a dyadic translation across the view axis: clip w stays exactly z)."""
        off, cam = np.tile(self.offset_inv, (n, 1)), np.tile(self.cam_tf, (n, 1))
        if self.exact and self.shift is not None:
            cam[:, 12 + self.shift] = np.arange(n) / 64.0
        elif not self.exact:
            for s in range(1, n):
                a = 0.002 * s
                T = np.array([[np.cos(a), 0, np.sin(a), 0.003 * s], [0, 1, 0, -0.002 * s], [-np.sin(a), 0, np.cos(a), 0.001 * s], [0, 0, 0, 1.0]])
                cam[s] = S.gl(_mat(self.cam_tf) @ T)
        return off, cam

    def workload(self, n=1, reverse=False):
        """(Workload of n streams, prim_of_tri): links in colour order (reverse: from the last colour), in a link its draws by
        number, in a draw the scene's triangles in order; prim_of_tri[t] is scene triangle t's number in the oracle's prim plane."""
        col, drw = np.asarray(self.colour), np.asarray(self.draw)
        mv = self.model_verts()
        colours = sorted(set(col.tolist()), reverse=reverse)
        prim_of_tri = np.empty(len(col), np.int64)
        links, k = [], 0
        for c in colours:
            draws = []
            for d in sorted(set(drw[col == c].tolist())):
                idx = np.flatnonzero((col == c) & (drw == d))
                prim_of_tri[idx] = k + np.arange(len(idx))
                k += len(idx)
                draws.append(L._Draw(np.ascontiguousarray(mv[idx].reshape(-1, 3)), np.arange(3 * len(idx), dtype=np.uint32).reshape(-1, 3)))
            links.append(draws)
        wl = WL.Workload(self.name + ("_reversed" if reverse else ""), self.W, self.H, n)
        wl.models = [links]
        wl.link_tf = [np.tile(IDENTITY, (n, len(links), 1))]
        wl.projection = np.tile(self.P, (n, 1))
        wl.offset_inv, wl.cam_tf = self.cameras(n)
        wl.near, wl.far = NEAR, FAR
        return wl, prim_of_tri

    def mvp(self, stream=0, n=None):
        off, cam = self.cameras(max(n or 0, stream + 1))
        return compose_mvp(self.P, off[stream], cam[stream], IDENTITY)

    def clip(self, stream=0):
        return vs_position(self.mvp(stream)[0], self.model_verts().reshape(-1, 3)).reshape(-1, 3, 4)

    def census(self, stream=0):
        key = ("census", stream)
        if key not in self.notes:
            self.notes[key] = clip_census(self.clip(stream), self.W, self.H)
        return self.notes[key]

    def link_of_colour(self, colour, reverse=False):
        """The label of a colour's link (labels start at 1; 0 is the background)."""
        return sorted(set(self.colour), reverse=reverse).index(colour) + 1


# the canonical plane +x mapped onto the four side planes, and the corner (+x, +y) onto the four corners
SIDE = {"px": 0, "nx": 1, "py": 2, "ny": 3}


def _strip(sc, canon, inner, outer, v0, v1, K, flip, case, wz=(1.0, 1.7, 2.6)):
    """A zig-zag strip between an inner row (u = inner) and an outer row (u = outer) from v0 to v1: triangles with one vertex
    on the outer side (quad result) alternate with triangles with two (triangle result); neighbours share their edges, and
    consistently wound neighbours walk a shared edge in opposite directions.  The vertex order starts at another vertex in
    every triangle."""
    vs = np.linspace(v0, v1, K + 1)
    I = [(inner(k), vs[k], wz[k % 3]) for k in range(K + 1)]
    O = [(outer(k), 0.5 * (vs[k] + vs[min(k + 1, K)]), wz[(k + 1) % 3]) for k in range(K + 1)]
    t = 0
    for k in range(K):
        for tri in ((I[k], O[k], I[k + 1]), (O[k], O[k + 1], I[k + 1])):
            r = t % 3
            sc.add_ndc(list(tri[r:] + tri[:r]), t % 3, case, flip=flip, canon=canon)
            t += 1


def plane_scene(p):
    """A strip in three colours across plane p only, in both windings, with one and with two vertices outside."""
    sc = ClipScene("plane_" + p, 160, 120, seed=PLANES.index(p))
    if p in SIDE:
        c = SIDE[p]
        _strip(sc, c, lambda k: 0.55 + 0.05 * (k % 2), lambda k: 1.2 + 0.1 * (k % 3), -0.85, -0.05, 5, False, "ccw")
        _strip(sc, c, lambda k: 0.6 - 0.05 * (k % 2), lambda k: 1.3 - 0.1 * (k % 3), 0.05, 0.85, 5, True, "cw")
    else:
        wi, wo = ((0.25, 0.31, 0.4), (0.03, 0.05, 0.07)) if p == "near" else ((3.0, 4.0, 5.0), (10.0, 12.0, 15.0))
        for flip, (u0, u1) in ((False, (-0.8, -0.05)), (True, (0.05, 0.8))):
            us = np.linspace(u0, u1, 6)
            I = [(us[k], -0.45 + 0.05 * (k % 2), wi[k % 3]) for k in range(6)]
            O = [(0.5 * (us[k] + us[min(k + 1, 5)]), 0.4 - 0.05 * (k % 3), wo[k % 3]) for k in range(6)]
            t = 0
            for k in range(5):
                for tri in ((I[k], O[k], I[k + 1]), (O[k], O[k + 1], I[k + 1])):
                    r = t % 3
                    sc.add_ndc(list(tri[r:] + tri[:r]), t % 3, "cw" if flip else "ccw", flip=flip)
                    t += 1
    return sc


def corner_scene(sx, sy, depth=None):
    """Fans around a vertex within the view's sides whose rim goes round the frustum's corner edge (sx, sy): the middle
    triangle covers the corner and both side planes cut it; with `depth` the fan's centre lies beyond the near or the far
    plane, which cuts off a third corner of every triangle."""
    name = "corner_" + ("px" if sx > 0 else "nx") + ("py" if sy > 0 else "ny") + ("_" + depth if depth else "")
    sc = ClipScene(name, 160, 120, seed=17 + (sx > 0) + 2 * (sy > 0) + 4 * (PLANES.index(depth) if depth else 0))
    wa, wr = {None: (1.0, 1.6), "near": (0.08, 0.5), "far": (12.0, 5.0)}[depth]
    for f, (a, scale) in enumerate((((0.1, 0.15), 1.0), ((0.3, 0.25), 0.93))):
        A = (sx * a[0], sy * a[1], wa * scale)
        rim = [(0.35, -0.4), (1.6, 0.75), (0.7, 1.7), (-0.4, 0.4)]          # the first and the last within the view
        R = [(sx * u, sy * v, wr * (1.0 + 0.1 * i) * scale) for i, (u, v) in enumerate(rim)]
        for i in range(3):
            tri = (A, R[i], R[i + 1])
            sc.add_ndc(list(tri[i:] + tri[:i]), (i + f) % 3, "side" if i != 1 else "corner", flip=bool(f))
    return sc


def _six_plane_triangles(sc, count=2):
    """Seeded search (the draws are the same every time) for triangles with no vertex inside that all six planes cut and that
    end as 9-gons: the first `count` found, each in both windings."""
    # In (clip x, clip y, w) space the frustum is |x| <= w, |y| <= w, near <= w <= far.  A plane that meets all six faces cuts
    # it in a hexagon; three lines that each cut off one of the hexagon's corners 0, 2 and 4 bound a triangle whose
    # intersection with the frustum has 6 - 3 + 6 = 9 corners.
    rng = np.random.default_rng(6)
    half = np.array([[-1, 0, 1, 0], [1, 0, 1, 0], [0, -1, 1, 0], [0, 1, 1, 0], [0, 0, 1, -NEAR], [0, 0, -1, FAR]], np.float64)
    found = []
    for _ in range(4000):
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        p0 = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.1, 0.6)])
        e1 = np.cross(nrm, [0.3, 0.5, 0.8])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(nrm, e1)
        poly = [p0 + 1e3 * (a * e1 + b * e2) for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        for h in half:          # Sutherland-Hodgman in float64
            d = [h[:3] @ q + h[3] for q in poly]
            nxt = []
            for i in range(len(poly)):
                j = (i + 1) % len(poly)
                if d[i] >= 0:
                    nxt.append(poly[i])
                if (d[i] >= 0) != (d[j] >= 0):
                    nxt.append(poly[i] + (poly[j] - poly[i]) * (d[i] / (d[i] - d[j])))
            poly = nxt
            if len(poly) < 3:
                break
        if len(poly) != 6:
            continue
        to2 = lambda q: np.array([(q - p0) @ e1, (q - p0) @ e2])
        h2 = [to2(q) for q in poly]
        lines = []          # through the points 40 % along the two edges that leave corner k: (point, direction)
        for k in (0, 2, 4):
            a, b = h2[k] + 0.4 * (h2[k - 1] - h2[k]), h2[k] + 0.4 * (h2[(k + 1) % 6] - h2[k])
            lines.append((a, b - a))
        tri = []
        for (a, da), (b, db) in ((lines[0], lines[1]), (lines[1], lines[2]), (lines[2], lines[0])):
            s = np.linalg.solve(np.stack([da, -db], 1), b - a)
            q = a + s[0] * da
            tri.append(p0 + q[0] * e1 + q[1] * e2)
        tri = np.array(tri)
        if np.abs(tri).max() > 1e3:
            continue
        eye = np.stack([(tri[:, 0] + sc.P[8] * tri[:, 2]) / -sc.P[0], (tri[:, 1] + sc.P[9] * tri[:, 2]) / sc.P[5], tri[:, 2]], 1)
        cs = _census_of_eye(sc, eye[None])
        if cs.cut[0] == 63 and cs.poly[0] == 9 and cs.andmask[0] == 0 and abs(cs.area2[0]) > 2 * 256 * 256 * 300:
            found.append(eye)
            if len(found) == count:
                return found
    raise AssertionError("no six-plane triangle found")


def around_scene():
    sc = ClipScene("around", 256, 128, seed=40)
    n = sc.ndc
    sc.add([n(-4, -3, 2.0), n(4, -3.5, 2.5), n(0.3, 5, 3.0)], 0, "contains")          # the whole view lies inside it
    for i, eye in enumerate(_six_plane_triangles(sc)):
        sc.add(eye, 1 + i % 2, "six")
        sc.add(eye[::-1] + np.array([0.0, 0.0, 0.004]), 2 - i % 2, "six")          # the other winding, 4 mm behind
    for i, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))):          # past a corner: OR-mask set, AND-mask clear, nothing left
        sc.add_ndc([(sx * 1.8, sy * 0.4, 1.0), (sx * 0.4, sy * 1.8, 1.2), (sx * 1.9, sy * 1.9, 1.1)], 3, "miss", flip=bool(i & 1))
    for i in range(4):          # slivers 2e-7 of the half frame wide from side to side of the view: every snapped vertex on one row or column
        v = (0.1, -0.3, 0.45, -0.6)[i]
        sc.add_ndc([(-1.5, v, 1.0), (1.5, v + 1e-7, 1.5), (1.5, v - 1e-7, 1.5)], 3, "thin", canon=i)
    sc.nothing.add(3)
    return sc


def _exact_plane_z(far):
    """A float32 z near the plane whose clip z, as the kernel rounds it, equals -w (near) or +w (far) exactly; None if the
    4000 float32 values around the plane hold none."""
    P = L.projection(160, 120).astype(F32)
    A, B = F32(-P[10]), F32(P[14])          # clip z = A z + B after the look-at's z -> -z
    z = F32(FAR if far else NEAR)
    cand = [z]
    lo = hi = z
    for _ in range(2000):
        lo, hi = np.nextafter(lo, F32(0)), np.nextafter(hi, F32(100))
        cand += [lo, hi]
    for c in cand:
        cz = F32(F32(A * c) + B)
        if (cz == c) if far else (F32(cz + c) == 0 and cz == -c):
            return float(c)
    return None


def ties_scene(only_unclipped=False):
    """Exact projection.  Per plane four cases in bands along it: `on_in` one vertex ON the plane, the rest inside (not
    clipped: > and >= 0 agree that it is inside); `on_out` one on the plane, one outside, one inside; `edge_in` an edge IN the
    plane, the third vertex inside (not clipped); `edge_out` an edge in the plane, the third outside (clipped to two vertices:
    draws nothing)."""
    sc = ClipScene("ties_unclipped" if only_unclipped else "ties", 160, 120, exact=True)
    q = 1.0 / 64
    for p, canon in SIDE.items():
        for j, case in enumerate(("on_in", "on_out", "edge_in", "edge_out")):
            v, h = (-18 + 12 * j) * q, 4 * q
            tri = {"on_in": [(1, v, 1.0), (0.5, v - h, 1.0), (0.5, v + h, 2.0)],
                   "on_out": [(1, v - h, 2.0), (1.5, v + h, 1.0), (0.4375, v, 1.0)],
                   "edge_in": [(1, v - h, 1.0), (1, v + h, 2.0), (0.5, v, 1.0)],
                   "edge_out": [(1, v - h, 2.0), (1, v + h, 1.0), (1.5, v, 1.0)]}[case]
            if only_unclipped and case in ("on_out", "edge_out"):
                continue
            sc.add_ndc(tri, j, case + "_" + p, flip=bool(canon & 1), canon=canon)
    for far in (False, True):
        p = "far" if far else "near"
        z = _exact_plane_z(far)
        if z is None:
            sc.notes["skipped_" + p] = "no float32 z within 2000 ulps of the plane has clip z == %sw exactly" % ("" if far else "-")
            continue
        zin, zout = (4.0, 12.0) if far else (0.5, 0.05)
        for j, case in enumerate(("on_in", "on_out", "edge_in", "edge_out")):
            u, v, h = (6 if far else -22) * q, (-18 + 12 * j) * q, 4 * q
            tri = {"on_in": [(u, v, z), (u + 16 * q, v - h, zin), (u + 16 * q, v + h, zin)],
                   "on_out": [(u, v - h, z), (u, v + h, zout), (u + 16 * q, v, zin)],
                   "edge_in": [(u, v - h, z), (u, v + h, z), (u + 16 * q, v, zin)],
                   "edge_out": [(u, v - h, z), (u, v + h, z), (u + 16 * q, v, zout)]}[case]
            if only_unclipped and case in ("on_out", "edge_out"):
                continue
            sc.add_ndc(tri, j, case + "_" + p, flip=far)
    if not only_unclipped:
        sc.nothing.add(3)
    return sc


def behind_scene():
    """Exact projection (w == 0 needs it): vertices behind the eye, in the eye's plane, at the eye, and needles from in front
    of the lens to behind it."""
    sc = ClipScene("behind", 160, 120, exact=True, shift=0)
    sc.add([(-0.5, -0.4, 1.0), (-0.1, -0.5, 1.5), (-0.4, 0.3, -0.5)], 0, "w_negative")
    sc.add([(0.1, -0.4, 1.0), (0.5, -0.5, 1.5), (2.0, 1.0, -3.0)], 1, "w_negative", flip=True)
    sc.add([(-0.6, 0.1, 1.0), (-0.2, 0.2, 1.25), (-0.25, 0.125, 0.0)], 2, "w_zero")
    sc.add([(0.2, 0.1, 1.0), (0.6, 0.3, 2.0), (0.5, -0.5, 0.0)], 0, "w_zero", flip=True)
    sc.add([(-0.1, 0.5, 1.0), (0.2, 0.6, 1.0), (0.0, 0.0, 0.0)], 1, "eye")
    sc.add([(0.0, 0.0, 0.0), (-0.3, -0.1, 0.5), (-0.25, -0.2, 0.5)], 2, "eye")
    rng = np.random.default_rng(5)
    for i in range(24):
        a = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), rng.uniform(0.4, 2.0)])
        b = a + np.array([rng.normal(scale=0.05), rng.normal(scale=0.05), -rng.uniform(2.5, 4.0)])
        c = a + rng.normal(scale=0.02, size=3)
        sc.add([a, b, c], i % 3, "needle", flip=bool(i & 1))
    return sc


def grazing_scene(p):
    """Colour 0: one draw of 40 triangles (one chunk) whose box lies outside plane p except that its first triangle reaches in
    by less than the chunk test's slack.  Colour 1: the same 40 moved out until the box is outside by more than 1 % of its
    reach.  Exact projection: the chunk's box is aligned with the eye's axes, so what reaches in is the triangle and not a
    corner of a box that a rotated camera inflates; stream s looks from s/64 m along the plane.
    What this catches: a chunk test that drops the chunk although a triangle of it is seen -- a slack of the wrong sign, a
    reach computed too small, another stream's matrix.  What it cannot: the size of the slack itself, since a corner of the box
    lies inside the plane (d + reach > 0) and a test without any slack keeps the chunk as well."""
    sc = ClipScene("grazing_" + p, 160, 120, exact=True, shift=1 if p in ("px", "nx") else 0)
    rng = np.random.default_rng(60)
    for colour, out in ((0, 0.0), (1, 1.0)):
        if p in SIDE:
            shift = out * (0.013 + 0.25)          # reach about 20 in u: 1 % = 0.2
            tris = [[(1 - 0.0125 + shift, 0.1, 1.0), (1.3 + shift, -2.9, 1.0), (1.3 + shift, 3.1, 1.0)]]
            for i in range(39):
                u, v = 38 + rng.uniform(0, 2), rng.uniform(-0.5, 0.5)
                tris.append([(u + shift, v, 1.0), (u + 0.1 + shift, v, 1.0), (u + shift, v + 0.1, 1.0)])
            for t in tris:
                sc.add_ndc(t, colour, "reach" if t is tris[0] else "out", canon=SIDE[p])
        elif p == "near":
            dz = -out * 0.05
            tris = [[(0.0, 0.0, 0.1002 + dz), (-5.0, -3.0, 0.05 + dz), (5.0, -3.0, 0.05 + dz)]]          # (eye coordinates)
            for i in range(39):
                x, y = rng.uniform(-0.3, 0.3, 2)
                tris.append([(x, y, -1.0 + dz), (x + 0.01, y, -1.0 + dz), (x, y + 0.01, -1.1 + dz)])
            for t in tris:
                sc.add(t, colour, "reach" if t is tris[0] else "out")
        else:
            dz = out * 12.0
            tris = [[(0.0, 0.0, 7.85 + dz), (-11000.0, -6000.0, 500.0 + dz), (11000.0, -6000.0, 500.0 + dz)]]
            for i in range(39):
                x, y = rng.uniform(-30, 30, 2)
                tris.append([(x, y, 900.0 + dz), (x + 1, y, 900.0 + dz), (x, y + 1, 910.0 + dz)])
            for t in tris:
                sc.add(t, colour, "reach" if t is tris[0] else "out")
    sc.nothing.add(1)
    return sc


def walls_scene():
    """A 10 m wall that passes 5 cm beside the lens, from 2 m behind the camera obliquely across the view to 7.5 m (it crosses
    the near plane and three side planes, its clipped records touch more than kCoopTiles tiles and cover whole tiles), a small
    link in front of it and one behind it (hidden)."""
    sc = ClipScene("walls", 256, 128, seed=70)
    a, b, c, d = (-0.25, -5.0, -2.0), (-0.25, 5.0, -2.0), (0.7, 5.0, 7.5), (0.7, -5.0, 7.5)          # x = -0.05 + 0.1 z
    sc.add([a, b, c], 0, "wall")
    sc.add([a, c, d], 0, "wall")
    sc.add([(0.15, -0.1, 1.0), (0.4, -0.1, 1.0), (0.3, 0.1, 1.0)], 1, "front")
    sc.add([(-0.2, -0.1, 1.0), (0.0, -0.1, 1.0), (-0.1, 0.1, 1.0)], 2, "hidden")          # (every ray to it meets the wall first)
    sc.nothing.add(2)
    return sc


LEVER_BLOCK = 4096
LEVER_PICKS = ((528, 754, True), (7, 1288, True), (1, 1285, False))          # (block seed, index in the block, mirrored): what levers_search() found


def _lever_block(sc, seed):
    """[LEVER_BLOCK, 3, 3] eye coordinates: one vertex inside the frustum, two at 3, 300 or 30,000 m from it in random
    directions; in every fourth triangle one of them lies back past the eye (such triangles meet the near face too)."""
    rng = np.random.default_rng(seed)
    n = LEVER_BLOCK
    w = np.exp(rng.uniform(np.log(0.12), np.log(6.0), n))
    a = np.stack(sc.ndc(rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n), w), 1)
    scale = np.array([3.0, 300.0, 30000.0])[np.arange(n) % 3][:, None]
    b, c = a + rng.normal(size=(n, 3)) * scale, a + rng.normal(size=(n, 3)) * scale
    d = -a / np.linalg.norm(a, axis=1, keepdims=True) + rng.normal(scale=0.3, size=(n, 3))
    back = a + scale * d / np.linalg.norm(d, axis=1, keepdims=True)
    b = np.where((np.arange(n) % 4 == 0)[:, None], back, b)
    return np.stack([a, b, c], 1)


def _mirrored(sc, eye):
    """The triangles with clip x negated."""
    e = np.array(eye, np.float64)
    cx = -sc.P[0] * e[..., 0] - sc.P[8] * e[..., 2]
    e[..., 0] = (-cx + sc.P[8] * e[..., 2]) / -sc.P[0]
    return e


def _census_of_eye(sc, eye):
    one = ClipScene("search", sc.W, sc.H)
    one.P, one.offset_inv, one.cam_tf = sc.P, sc.offset_inv, sc.cam_tf
    one.eye = np.asarray(eye)
    return clip_census(vs_position(sc.mvp()[0], one.model_verts().reshape(-1, 3)).reshape(-1, 3, 4), sc.W, sc.H)


def _outside(sc, cs):
    """([n] a clipper-made vertex snapped below the frame, [n] one above it), in x or y."""
    lo = (cs.made & ((cs.sx < -128) | (cs.sy < -128))).any(1)
    hi = (cs.made & ((cs.sx > 256 * sc.W - 128) | (cs.sy > 256 * sc.H - 128))).any(1)
    return lo, hi


def levers_search(blocks=2000):
    """How LEVER_PICKS was found: the first triangle of the seeded blocks (or of their mirror images) with a clipper-made vertex
    snapped below the frame, the first with one above it, and the first whose pool reaches 15."""
    sc = ClipScene("levers", 256, 128, seed=80)
    want = {"lo": None, "hi": None, "pool": None}
    for seed in range(blocks):
        for mirror in (False, True):
            eye = _lever_block(sc, seed)
            cs = _census_of_eye(sc, _mirrored(sc, eye) if mirror else eye)
            lo, hi = _outside(sc, cs)
            for key, hit in (("lo", lo), ("hi", hi), ("pool", cs.pool >= 15)):
                if want[key] is None and hit.any():
                    want[key] = (seed, int(np.flatnonzero(hit)[0]), mirror)
        if all(v is not None for v in want.values()):
            break
    return tuple(want.values())


def levers_scene():
    """64 triangles with one vertex inside the frustum and two at 3, 300 and 30,000 m from it: the interpolation parameter
    is tiny or close to one, and the clipper's vertices land up to one unit of 1/256 px outside the frame.  The picks of
    levers_search() first, the rest from the start of block 0."""
    sc = ClipScene("levers", 256, 128, seed=80)
    tris = [(_mirrored(sc, _lever_block(sc, seed)) if mirror else _lever_block(sc, seed))[i] for seed, i, mirror in LEVER_PICKS]
    tris += list(_lever_block(sc, 0)[:64 - len(tris)])
    for i, t in enumerate(tris):
        sc.add(t, i % 3, "lever", flip=bool(i & 1))
    return sc


def levers_ok(sc):
    """The census conditions the picks are chosen for."""
    cs = sc.census()
    lo, hi = _outside(sc, cs)
    return bool(lo.any() and hi.any() and (cs.pool >= 15).any())


MANY_FANS = 264          # x 256 slivers = 67,584 > 64 shards x 1024 items


def many_scene():
    """Fans of 256 thin slivers (one draw = one chunk each; a fan shares its apex and the neighbours share rim vertices) from
    beyond the +y plane through the view to behind the near plane and past the +x plane next to the eye: each cuts at least
    three planes and its pool grows to 9 .. 13, so every lane of every clip workgroup uses the spill area (its slots 8 .. 12:
    13 and 14 are reached by single triangles of `around` and `levers` only)."""
    sc = ClipScene("many", 160, 120, seed=90)
    rng = np.random.default_rng(90)
    fans = []
    for f in range(2 * MANY_FANS):          # (seeded: the same candidates every time; the fans whose every sliver qualifies are kept)
        apex = sc.clipc(rng.uniform(0.04, 0.1), rng.uniform(-0.6, -0.4), -rng.uniform(0.2, 0.3))          # behind the lens
        u0, du = rng.uniform(-0.6, -0.25), 1.2 / 80 / 256
        rim = [sc.ndc(u0 + du * i, 1.3, 1.0 + 0.002 * f) for i in range(257)]
        fans.append([[apex, rim[i], rim[i + 1]] for i in range(256)])
    cs = _census_of_eye(sc, np.array(fans).reshape(-1, 3, 3))
    bits = sum((cs.cut >> p) & 1 for p in range(6))
    good = ((bits >= 3) & (cs.pool >= 9) & (cs.poly >= 3)).reshape(-1, 256).all(1)
    keep = np.flatnonzero(good)[:MANY_FANS]
    assert len(keep) == MANY_FANS, good.sum()
    for k, f in enumerate(keep):
        for tri in fans[f]:
            sc.add(tri, k % 3, "sliver", draw=k // 3, flip=bool(k & 1))
    return sc


# ---- the list ---------------------------------------------------------------------------------------------------------

BUILDERS = {}
for _p in PLANES:
    BUILDERS["plane_" + _p] = (lambda p=_p: plane_scene(p))
for _sx, _sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
    for _d in (None, "near", "far"):
        _n = "corner_" + ("px" if _sx > 0 else "nx") + ("py" if _sy > 0 else "ny") + ("_" + _d if _d else "")
        BUILDERS[_n] = (lambda sx=_sx, sy=_sy, d=_d: corner_scene(sx, sy, d))
BUILDERS["around"] = around_scene
BUILDERS["ties"] = ties_scene
BUILDERS["ties_unclipped"] = lambda: ties_scene(True)
BUILDERS["behind"] = behind_scene
for _p in PLANES:
    BUILDERS["grazing_" + _p] = (lambda p=_p: grazing_scene(p))
BUILDERS["walls"] = walls_scene
BUILDERS["levers"] = levers_scene
BUILDERS["many"] = many_scene
NAMES = tuple(BUILDERS)
FRAMES = [(160, 120), (256, 128)]
_built, _workloads = {}, {}


def scene(name):
    if name not in _built:
        _built[name] = BUILDERS[name]()
    return _built[name]


def kind_of(name):
    return name.split("_")[0]


def planes_of(name):
    """The planes a plane_ or corner_ scene's name says its triangles cut, as a mask."""
    rest = name.split("_", 1)[1]
    return sum(1 << i for i, p in enumerate(PLANES) if p in rest)


def workload(name, n=1, reverse=False):
    """(Workload, prim_of_tri) of ClipScene.workload(), built once: a pair, as lattice_scenes.workload() returns one."""
    if (name, n, reverse) not in _workloads:
        _workloads[(name, n, reverse)] = scene(name).workload(n, reverse)
    return _workloads[(name, n, reverse)]


def sensor_mm(name, n=1):
    """[n, H, W] uint16 sensor planes in whole millimetres, 7 m away and a few millimetres apart per stream and pixel: in
    front of the background, behind everything the scenes draw nearer than 6.9 m, so the mask is that coverage."""
    sc = scene(name)
    yy, xx = np.mgrid[0:sc.H, 0:sc.W]
    return np.stack([(7000 + 7 * s + (xx + yy) % 3).astype(np.uint16) for s in range(n)])


# ---- what Mesa llvmpipe renders for the scenes: tests/golden/llvmpipe/clip_scenes_WxH.npz --------------------------------

LLVMPIPE_REPLACE = 5.0


def llvmpipe_path(W, H):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "llvmpipe", "clip_scenes_%dx%d.npz" % (W, H))


def llvmpipe_names(W, H):
    return [n for n in NAMES if (scene(n).W, scene(n).H) == (W, H)]


_frames = {}


def llvmpipe_frames(name):
    """[(key, projection, sensor depth, offset_inv, cam_tf, harness renderables, oracle draws)] of a scene as stream 0 sees
    it: all links, then each link alone (`many`: all links only), then all links under a sensor plane that lies on the
    threshold of the oracle's own z (key .../thr: gpu_support.threshold_sensor; the oracle is imported here, not with the
    module).  The oracle must be at its default variants when a scene's frames are first asked for."""
    if name in _frames:
        return _frames[name]
    from gpu_support import threshold_sensor
    from oracle import bindings as O
    wl, _ = workload(name)
    depth = (sensor_mm(name)[0].astype(np.float32) * np.float32(0.001)).astype(np.float32)
    draws = wl.oracle_draws(0)
    first, k = [], 0          # the first draw of every link
    for link in wl.models[0]:
        first.append(k)
        k += len(link)
    first.append(k)
    P, off, cam = wl.projection[0], wl.offset_inv[0], wl.cam_tf[0]
    rend = lambda part: [(tf, [("mesh", pre, op, v, t)]) for tf, pre, op, v, t in part]
    out = [("%s/all" % name, P, depth, off, cam, rend(draws), draws)]
    for which in ([] if name == "many" else range(len(first) - 1)):
        part = draws[first[which]:first[which + 1]]
        out.append(("%s/link%d" % (name, which), P, depth, off, cam, rend(part), part))
    zwin = O.filter_frame(depth, P, draws, off, cam, z_near=NEAR, z_far=FAR, replace_value=LLVMPIPE_REPLACE, want_debug=True)[2]
    out.append(("%s/thr" % name, P, threshold_sensor(zwin, NEAR, FAR, 0.05, seed=NAMES.index(name)), off, cam, rend(draws), draws))
    _frames[name] = out
    return out
