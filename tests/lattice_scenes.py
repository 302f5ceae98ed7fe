"""Scenes whose vertices lie exactly on the rasteriser's 1/256 px lattice (test helper for the fill-rule tests).

A scene is a list of triangles in snapped integer window coordinates (the centre of pixel (px, py) is (256 px, 256 py); the
frame spans -128 .. 256 W - 128), all at one of a few depths, that never overlap within a depth.  The vertices are unprojected
in float64 through a plain pinhole camera -- focal lengths W/2 and H/2, principal point in the middle of the frame, near 0.1,
far 8, identity camera, so the projection matrix holds only 0, +-1 and the two depth terms -- and cast to float32.  The depths
are powers of two (1, 2 and 4 m), so 1/w is exact and the only roundings are the vertex's own cast and the viewport's fused
multiply-add: a few 1e-5 px at these frame sizes, against the 1/512 px that would move a snapped coordinate (at 2048 x 2048
every step is exact).  The near scenes lie at a float32 just behind the near plane: 1/w rounds as well, another 1e-5 px.  tests/test_fill_rule_cpu.py proves the snap by comparing the oracle with tests/fill_rule.py.

`regions` lists pixel rectangles [x0, x1) x [y0, y1) that the scene's triangles partition: every pixel centre in one belongs to
exactly one triangle per listed rectangle (rectangles of two depth layers may lie on top of each other).

Triangles are coloured greedily so that two whose bounding boxes touch never share a colour; one robot link per colour, so
the label plane shows which triangle won every pixel.

Constants of realtime_urdf_filter_amd/csrc/rtuf_kernels.hip that the scenes are sized against (quoted, not imported):
kTileW x kTileH = 64 x 32; a box of at most 2 x 2 pixel centres, or of at most 4 x 4 inside one tile, is resolved to fragments
by the set-up kernel unless it may reach window z < 0.51; kFrontArea = 24, kSmallArea = 96, kQuarterArea = 256,
kWallArea = 1536 (tile-clipped box areas; the last one in bins of more than kParkBelow = 128 records), kCoopTiles = 4."""
import numpy as np

from bench_support import workloads as WL

TILE_W, TILE_H = 64, 32
FRONT_AREA, SMALL_AREA, QUARTER_AREA, WALL_AREA, PARK_BELOW, COOP_TILES = 24, 96, 256, 1536, 128, 4
NEAR, FAR = 0.1, 8.0
Z_FAR_LAYER, Z_MAIN = 2.0, 1.0          # metres; window z 0.962 and 0.911
# 3 um behind the near plane: window z 3e-5, 24-bit depth about 500 -- below 2^10, the most that exact_z_floor() of rtuf_numerics.h
# ever is, so the winners go through the exact-z pass whatever the scene's triangle count (at 0.15 m the keys' low bits
# carry the float z and no tile runs that pass)
Z_NEAR = float(np.float32(0.100003))
PX = 256
IDENTITY = np.eye(4).T.reshape(16).copy()


def projection(W, H):
    """fx = W/2, fy = H/2, cx = W/2, cy = H/2 in the layout of tests/scenes.py's projection()."""
    P = np.zeros(16)
    P[0], P[5], P[11] = -1.0, 1.0, -1.0
    P[10] = -(FAR + NEAR) / (FAR - NEAR)
    P[14] = -2.0 * FAR * NEAR / (FAR - NEAR)
    return P


def unproject(snapped, z, W, H):
    """[..., 2] snapped window coordinates at depth z -> [..., 3] float32 model coordinates (the oracle's fixed model-view
    matrix diag(-1, 1, -1) and the projection above give clip = (x, y, ., z))."""
    s = np.asarray(snapped, np.float64)
    wx, wy = s[..., 0] / 256.0 + 0.5, s[..., 1] / 256.0 + 0.5
    out = np.stack([(wx - W / 2.0) / (W / 2.0) * z, (wy - H / 2.0) / (H / 2.0) * z, np.broadcast_to(np.float64(z), wx.shape)], -1)
    return out.astype(np.float32)


class _Draw:
    def __init__(self, verts, tris):
        self.pre_op, self.op, self.verts, self.tris = 0, [0.0, 0.0, 0.0], verts, tris


# ---- local shapes: partitions of the square [0, S]^2 (S in 1/256 px) ----------------------------------------------------

def diag(S):
    return [((0, 0), (S, 0), (S, S)), ((0, 0), (S, S), (0, S))]


def cross4(S):
    c = (S // 2, S // 2)
    k = [(0, 0), (S, 0), (S, S), (0, S)]
    return [(c, k[i], k[(i + 1) % 4]) for i in range(4)]


def fan8(S):
    c, h = (S // 2, S // 2), S // 2
    rim = [(0, 0), (h, 0), (S, 0), (S, h), (S, S), (h, S), (0, S), (0, h)]
    return [(c, rim[i], rim[(i + 1) % 8]) for i in range(8)]


def variant(shape, S, k):
    """Symmetry k & 7 of the square (bit 0: flip x, bit 1: flip y, bit 2: transpose) and, with bit 3, the other winding."""
    out = []
    for tri in shape:
        t = []
        for x, y in tri:
            if k & 4:
                x, y = y, x
            if k & 1:
                x = S - x
            if k & 2:
                y = S - y
            t.append((x, y))
        out.append(tuple(t[::-1]) if k & 8 else tuple(t))
    return out


class Lattice:
    def __init__(self, name, W, H, z=Z_MAIN):
        self.name, self.W, self.H, self.z = name, W, H, z
        self.tris, self.zs, self.regions = [], [], []
        self.busy = np.zeros((H, W), bool)          # pixels whose neighbourhood a placed shape's geometry lies in

    # -- building ---------------------------------------------------------------------------------------------------------
    def add(self, tri, z=None):
        for x, y in tri:          # in-frustum: the frame's borders included
            assert -128 <= x <= 256 * self.W - 128 and -128 <= y <= 256 * self.H - 128, (self.name, tri)
        self.tris.append(tuple((int(x), int(y)) for x, y in tri))
        self.zs.append(self.z if z is None else z)

    def square(self, shape, S, k, ox, oy, partition=True):
        """Variant k of a square's partition with its corner at snapped (ox, oy)."""
        for tri in variant(shape, S, k):
            self.add(tuple((x + ox, y + oy) for x, y in tri))
        if partition:
            self.region_snapped(ox, oy, ox + S, oy + S)

    def place(self, shape, S, k, gx, gy, off=(0, 0)):
        """Variant k of a square's partition with its corner `off` (1/256 px, each within -128 .. 129) from the centre of pixel
        (gx, gy), if the pixels gx - 1 .. gx + n + 1 (n = the side in px; the same in y) are still free: two placed shapes then
        never touch.  Returns whether it was placed."""
        n = S // PX
        x0, y0, x1, y1 = max(gx - 1, 0), max(gy - 1, 0), min(gx + n + 1, self.W - 1), min(gy + n + 1, self.H - 1)
        if gx < 0 or gy < 0 or gx + n > self.W - 1 or gy + n > self.H - 1 or self.busy[y0:y1 + 1, x0:x1 + 1].any():
            return False
        self.busy[y0:y1 + 1, x0:x1 + 1] = True
        self.square(shape, S, k, gx * PX + off[0], gy * PX + off[1])
        return True

    def reserve(self, x, y, w, h):
        assert not self.busy[y:y + h, x:x + w].any(), (self.name, x, y, w, h)
        self.busy[max(y - 1, 0):y + h + 1, max(x - 1, 0):x + w + 1] = True

    def rect(self, x, y, w, h, k=0, z=None, region=True):
        """A w x h px rectangle with its corner at pixel coordinates (x, y) -- whole numbers: on a pixel centre; halves: on a
        pixel corner -- split along one diagonal (bit 0 of k picks it), wound one way or the other (bit 1)."""
        x0, y0, x1, y1 = (int(round(v * PX)) for v in (x, y, x + w, y + h))
        if k & 1:
            tris = [((x0, y0), (x1, y0), (x0, y1)), ((x1, y0), (x1, y1), (x0, y1))]
        else:
            tris = [((x0, y0), (x1, y0), (x1, y1)), ((x0, y0), (x1, y1), (x0, y1))]
        for t in tris:
            self.add(t[::-1] if k & 2 else t, z)
        if region:
            self.region_snapped(x0, y0, x1, y1)

    def region_snapped(self, x0, y0, x1, y1):
        """The pixel centres p with x0 <= p_x < x1 and y0 <= p_y < y1: what the top-left rule gives the closed rectangle."""
        c = lambda v: -((-v) // PX)
        r = (max(c(x0), 0), max(c(y0), 0), min(c(x1), self.W), min(c(y1), self.H))
        if r[2] > r[0] and r[3] > r[1]:
            self.regions.append(r)

    # -- derived ----------------------------------------------------------------------------------------------------------
    def expected_count(self):
        e = np.zeros((self.H, self.W), np.int32)
        for x0, y0, x1, y1 in self.regions:
            e[y0:y1, x0:x1] += 1
        return e

    def boxes(self):
        """[n, 4] pixel-centre boxes (bx0, by0, bx1, by1) as the rasteriser bounds them: the low side inclusive, a centre on
        the high side excluded, clipped to the frame."""
        t = np.asarray(self.tris, np.int64)
        lo, hi = t.min(1), t.max(1)
        bx0, by0 = np.maximum(-((-lo[:, 0]) // PX), 0), np.maximum(-((-lo[:, 1]) // PX), 0)
        bx1, by1 = np.minimum((hi[:, 0] - 1) // PX, self.W - 1), np.minimum((hi[:, 1] - 1) // PX, self.H - 1)
        return np.stack([bx0, by0, bx1, by1], 1)

    def fragment_sized(self):
        """[n] bool: triangles the set-up kernel resolves to fragments when they are not near."""
        b = self.boxes()
        w, h = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
        live = (w > 0) & (h > 0)
        one_tile = (b[:, 0] // TILE_W == b[:, 2] // TILE_W) & (b[:, 1] // TILE_H == b[:, 3] // TILE_H)
        return live & (((w <= 2) & (h <= 2)) | ((w <= 4) & (h <= 4) & one_tile))

    def tile_clipped_areas(self):
        """Every (triangle, tile) pair's box area inside the tile, and the number of tiles each box touches."""
        areas, ntiles = [], []
        for bx0, by0, bx1, by1 in self.boxes():
            if bx1 < bx0 or by1 < by0:
                ntiles.append(0)
                continue
            n = 0
            for ty in range(by0 // TILE_H, by1 // TILE_H + 1):
                for tx in range(bx0 // TILE_W, bx1 // TILE_W + 1):
                    w = min(bx1, tx * TILE_W + TILE_W - 1) - max(bx0, tx * TILE_W) + 1
                    h = min(by1, ty * TILE_H + TILE_H - 1) - max(by0, ty * TILE_H) + 1
                    areas.append(int(w * h))
                    n += 1
            ntiles.append(n)
        return np.asarray(areas), np.asarray(ntiles)

    def colours(self):
        """Greedy colouring: triangles whose snapped bounding boxes touch get different colours."""
        if getattr(self, "_colours", None) is not None and len(self._colours) == len(self.tris):
            return self._colours
        t = np.asarray(self.tris, np.int64)
        lo, hi = t.min(1), t.max(1)
        col = np.full(len(t), -1, np.int64)
        for i in range(len(t)):
            near = np.flatnonzero((lo[:i, 0] <= hi[i, 0]) & (hi[:i, 0] >= lo[i, 0]) & (lo[:i, 1] <= hi[i, 1]) & (hi[:i, 1] >= lo[i, 1]))
            used = set(col[near].tolist())
            c = 0
            while c in used:
                c += 1
            col[i] = c
        self._colours = col
        return col

    def workload(self, n=1, reverse=False):
        """(Workload of n identical streams with one link per colour, prim_of_tri): the oracle numbers the triangles over the
        draw list, colour by colour (with `reverse` from the last colour to the first: of two triangles that both claim a pixel
        at one depth the earlier draw wins, so a pixel covered twice shows in one of the two orders whoever claims it wrongly);
        prim_of_tri[t] is scene triangle t's number there."""
        col = self.colours()
        if reverse:
            col = col.max() - col
        order = np.argsort(col, kind="stable")
        prim_of_tri = np.empty(len(col), np.int64)
        prim_of_tri[order] = np.arange(len(col))
        t = np.asarray(self.tris, np.int64)
        zs = np.asarray(self.zs, np.float64)
        links = []
        for c in range(int(col.max()) + 1):
            idx = order[col[order] == c]
            verts = np.concatenate([unproject(t[i], zs[i], self.W, self.H) for i in idx])
            links.append([_Draw(np.ascontiguousarray(verts, np.float32), np.arange(3 * len(idx), dtype=np.uint32).reshape(-1, 3))])
        wl = WL.Workload(self.name + ("_reversed" if reverse else ""), self.W, self.H, n)
        wl.models = [links]
        wl.link_tf = [np.tile(IDENTITY, (n, len(links), 1))]
        wl.projection = np.tile(projection(self.W, self.H), (n, 1))
        wl.offset_inv = np.tile(IDENTITY, (n, 1))
        wl.cam_tf = np.tile(IDENTITY, (n, 1))
        wl.near, wl.far = NEAR, FAR
        return wl, prim_of_tri


# ---- tiny and small: squares that the set-up kernel resolves to fragments ------------------------------------------------

# a square's corner against a pixel centre: on it, on the pixel's corner, and 1/256 px off either
OFFSETS = [(0, 0), (128, 128), (1, 0), (0, -1), (-1, 1), (129, 128), (128, 127), (127, 129), (0, 128), (128, 0)]


def _across_borders(sc, shapes, n):
    """Squares of n px laid across the tile borders x = 64 and y = 32, across every point where four tiles meet, into the
    frame's last columns and rows (partial tiles at 160 x 120 and 200 x 150) and into its first and last corner; on pixel
    corners the squares at the frame's end lie on the frame's border itself.  All 16 variants at every kind of place."""
    W, H, pitch, back = sc.W, sc.H, n + 3, max(n // 2, 1)
    i = 0
    for ty in range(TILE_H, H - n, TILE_H):          # four tiles meet: the first of them gets the last shape (the fan of eight)
        for tx in range(TILE_W, W - n, TILE_W):
            shape, S = shapes[-1] if i == 0 else shapes[i % len(shapes)]
            off = (128, 128) if i % 3 == 2 else (0, 0)
            assert sc.place(shape, S, (5 * i) % 16, tx - back, ty - back, off)
            i += 1
    placed = {"x": 0, "y": 0, "last_col": 0, "last_row": 0}
    for k in range(16):
        shape, S = shapes[k % len(shapes)]
        off = OFFSETS[k % 4]
        placed["x"] += sc.place(shape, S, k, TILE_W - back, 2 + k * pitch, off)              # across x = 64 (where no junction is)
        placed["y"] += sc.place(shape, S, (k + 3) % 16, 2 + k * pitch, TILE_H - back, off)   # across y = 32
        edge = (128, 128) if k & 1 else (0, 0)          # (128: the square ends on the frame's border)
        placed["last_col"] += sc.place(shape, S, (k + 6) % 16, W - 1 - n, 2 + k * pitch, edge)
        placed["last_row"] += sc.place(shape, S, (k + 9) % 16, 2 + k * pitch, H - 1 - n, edge)
    assert min(placed.values()) >= 8, (sc.name, placed)
    shape, S = shapes[0]
    sc.square(shape, S, 3, -128, -128)          # the frame's first corner: two sides on the frame's border
    sc.busy[:n + 1, :n + 1] = True


def _fill(sc, shapes, n, offsets):
    """Every shape under all 16 variants and the given offsets into the cells that are still free, row by row: the grid runs
    over the whole frame.  Returns how many of the combinations found a place."""
    pitch = n + 3
    cells = ((gx, gy) for gy in range(1, sc.H - n - 1, pitch) for gx in range(1, sc.W - n - 1, pitch))
    done = 0
    for off in offsets:
        for shape, S in shapes:
            for k in range(16):
                for gx, gy in cells:
                    if sc.place(shape, S, k, gx, gy, off):
                        done += 1
                        break
                else:
                    return done
    return done


def _slivers(sc, x, y):
    """At pixel (x, y), in free space.  Zero-area triangles through pixel centres -- collinear along a diagonal, a row and a
    column, and two vertices in one place -- cover nothing.  Slivers 1/256 px thick with their long edge along a row, a column
    and a diagonal of pixel centres cover what the rule gives them (no partition: they are compared, not counted)."""
    sc.reserve(x, y, 44, 3)
    p = lambda ax, ay: ((x + ax) * PX, (y + ay) * PX)
    sc.add((p(0, 0), p(1, 1), p(2, 2)))
    sc.add((p(4, 0), p(6, 0), p(5, 0)))
    sc.add((p(8, 0), p(8, 2), p(8, 1)))
    sc.add((p(10, 0), p(10, 0), p(12, 2)))
    first_degenerate = len(sc.tris) - 4
    thin = [((0, 1), (2, 1), (0, 1)), ((0, 1), (2, 1), (0, -1)), ((1, 0), (1, 2), (1, 0)), ((1, 0), (1, 2), (-1, 0)),
            ((0, 0), (2, 2), (1, 0)), ((0, 0), (2, 2), (0, 1)), ((2, 0), (0, 2), (1, 0)), ((2, 0), (0, 2), (0, -1))]
    for i, (a, b, d) in enumerate(thin):
        a, b = p(14 + 4 * i + a[0], a[1]), p(14 + 4 * i + b[0], b[1])
        mid = ((a[0] + b[0]) // 2 + d[0], (a[1] + b[1]) // 2 + d[1])
        sc.add((a, b, mid) if i & 1 else (b, a, mid))
    return list(range(first_degenerate, first_degenerate + 4))


def tiny_scene(W, H, z=Z_MAIN):
    """Right triangles with legs of 1 and 2 px and fans of eight around a pixel centre: boxes of at most 2 x 2 pixel centres,
    which the set-up kernel resolves with small_box_coverage<2> and emits with MAY_STRADDLE."""
    sc = Lattice("tiny_%dx%d%s" % (W, H, "_near" if z == Z_NEAR else ""), W, H, z)
    shapes = [(diag(PX), PX), (diag(2 * PX), 2 * PX), (fan8(2 * PX), 2 * PX)]
    sc.degenerate = _slivers(sc, 70, 40)
    _across_borders(sc, shapes, 2)
    sc.filled = _fill(sc, shapes, 2, OFFSETS)
    return sc


def small_scene(W, H, z=Z_MAIN):
    """Squares of 3 and 4 px split along a diagonal or along both: boxes of 3 x 3, 4 x 2 and 4 x 4 pixel centres -- inside one
    tile small_box_coverage<4>, across a tile border records that are binned from the front of their bins."""
    sc = Lattice("small_%dx%d%s" % (W, H, "_near" if z == Z_NEAR else ""), W, H, z)
    shapes = [(diag(3 * PX), 3 * PX), (diag(4 * PX), 4 * PX), (cross4(3 * PX), 3 * PX), (cross4(4 * PX), 4 * PX), (fan8(4 * PX), 4 * PX)]
    sc.degenerate = []
    _across_borders(sc, shapes, 4)
    sc.filled = _fill(sc, shapes, 4, OFFSETS[:4])
    return sc


# ---- records: rectangles on both sides of every size class ---------------------------------------------------------------

def _pack(sc, x, y, w, h, rw, rh, k0=0):
    """Fills the w x h px area at (x, y) with rw x rh rectangles, as many as fit."""
    n = 0
    for ry in range(y, y + h - rh + 1, rh):
        for rx in range(x, x + w - rw + 1, rw):
            sc.rect(rx, ry, rw, rh, k0 + n)
            n += 1
    return n


def records_scene(W, H, z=Z_MAIN):
    """Rectangles with their corners on pixel centres, split along either diagonal and wound either way.  A w x h rectangle's
    triangles have boxes of w x h pixel centres, so the tile-clipped box areas lie on both sides of every class limit:
    24 | 25 (4 x 6, 6 x 4 | 5 x 5), 96 | 98 (8 x 12, 12 x 8, 16 x 6 | 14 x 7, 49 x 2; 97 is prime, so inside a 64 x 32 tile it
    does not exist; the 97 x 1 rectangle lies across two tiles, as 56 x 1 and 41 x 1), 256 | 258 (16 x 16, 32 x 8, 8 x 32 | 43 x 6; 257 is prime and a
    257 x 1 rectangle is wider than these frames) and 1536 | 1537 (48 x 32 | 53 x 29), the last pair once in bins of more than
    128 records (the rest of their tiles is packed with 5 x 1 rectangles) and once in bins of a few.  Boxes touch 1, 2, 3,
    exactly 4 and more than 4 tiles."""
    sc = Lattice("records_%dx%d%s" % (W, H, "_near" if z == Z_NEAR else ""), W, H, z)
    sc.degenerate = []
    # tile (0, 0): 48 x 32 and 192 slivers; tile (1, 0): 53 x 29 and 188 slivers
    sc.rect(0, 0, 48, 32, 0)
    _pack(sc, 48, 0, 16, 32, 5, 1, 1)
    sc.rect(64, 0, 53, 29, 1)
    _pack(sc, 117, 0, 11, 32, 5, 1, 2)
    _pack(sc, 64, 29, 53, 3, 5, 1, 3)
    # tile (0, 1): a few records of every class
    for i, (x, y, w, h) in enumerate([(1, 33, 4, 6), (7, 33, 6, 4), (15, 33, 5, 5), (22, 33, 8, 12), (32, 33, 12, 8), (46, 33, 14, 7),
                                      (46, 41, 16, 6), (1, 47, 16, 16), (19, 47, 43, 6), (19, 54, 32, 8), (5, 63, 49, 2)]):
        sc.rect(x, y, w, h, i)
    # tiles (1, 1) and (2, 1): the largest classes in bins of a few records
    sc.rect(64, 32, 48, 32, 3)
    sc.rect(113, 33, 8, 31, 2)          # crosses y = 64: 8 x 31 and 8 x 0
    sc.rect(136, 32, 8, 32, 1)
    sc.rect(118, 66, 20, 20, 2)         # crosses x = 128 only
    # from y = 66: boxes over several tiles
    sc.rect(8, 66, 97, 1, 0)            # 97 x 1: two tiles
    sc.rect(60, 64, 80, 2, 1)           # three tiles: x = 64 and x = 128
    sc.rect(2, 72, 50, 38, 1)           # two tiles: y = 96
    sc.rect(54, 86, 20, 20, 3)          # exactly 4 tiles: across the point (64, 96)
    sc.rect(76, 88, 66, 22, 2)          # exactly 4 tiles: x = 128 and y = 96
    sc.rect(146, 3, 1, H - 11, 0)       # 1 px wide: 4 tiles at 120 and 128 rows, 5 at 150
    sc.rect(148, 3, 2, 61, 3)
    # the frame's last columns and rows (partial tiles at 160 x 120 and 200 x 150): the far sides lie on the frame's border
    sc.rect(W - 8.5, 2, 8, 70, 2)
    sc.rect(W - 30.5, H - 6.5, 30, 6, 1)
    sc.rect(4, H - 5.5, 110, 5, 0)                          # two tiles in the last row
    if W > 192:
        sc.rect(154, 76, W - 0.5 - 154, 30, 1)              # 4 tiles: into the last (partial) tile column
        sc.rect(2, 114, 140, 4 + (H - 128) // 4, 3)         # 3 tiles in a row
    if W >= 256:
        sc.rect(152, 3, 48, 70, 0)                          # 2 x 3 tiles: more than kCoopTiles (at 200 x 150 the 1 px rectangle's 5)
    return sc


# ---- tiles: edges through the corner pixels of tiles ---------------------------------------------------------------------

def _fan(sc, poly, apex, k=0, z=None):
    """The convex polygon (snapped vertices in order) as a fan from its vertex number `apex`."""
    n = len(poly)
    for i in range(1, n - 1):
        t = (poly[apex], poly[(apex + i) % n], poly[(apex + i + 1) % n])
        sc.add(t[::-1] if (k + i) & 1 else t, z)


TILES_KINDS = ("first", "last", "top_right", "bottom_left", "row_first", "row_last", "column_first", "column_last", "cover")


def tiles_scene(W, H, kind):
    """Triangles over the 3 x 3 tiles [0, 192] x [0, 96] px (big records: their boxes touch more than 4 tiles).

    first, last, top_right, bottom_left: the region is cut by one line of slope -1/2 or +1/2 through that corner pixel's centre
    of the middle tile (pixels 64 .. 127 x 32 .. 63), which lies on one side of the line and touches it in that one pixel; the
    same line passes through corner pixels of other tiles.  The triangle on the tile's side covers the tile completely exactly
    if its edge owns the boundary; the triangle on the other side touches the tile, in that single pixel, exactly if its edge
    does.  The tests "covers the tile completely", "does not touch the tile" and classify_box decide on E == 0 here.
    row_first, row_last, column_first, column_last: an edge that lies exactly on the middle tile's first or last pixel row
    (y = 32, 63) or column (x = 64, 127), of a triangle that contains the rest of the tile: E == 0 along a whole side of the tile.
    cover: two triangles along the diagonal through the tiles' first pixels cover six tiles completely, three of them twice
    behind each other (a second pair at 2 m: records behind a cover) and with small rectangles at 4 m behind them."""
    sc = Lattice("tiles_%s_%dx%d" % (kind, W, H), W, H)
    sc.degenerate = []
    X, Y = 192 * PX, 96 * PX
    p = lambda x, y: (int(round(x * PX)), int(round(y * PX)))
    if kind == "first":            # x + 2 y = 128 through (64, 32): the tile lies below and right of it
        _fan(sc, [p(0, 0), p(128, 0), p(0, 64)], 0)
        _fan(sc, [p(192, 96), p(0, 96), p(0, 64), p(128, 0), p(192, 0)], 0, 1)
    elif kind == "last":           # x + 2 y = 253 through (127, 63): the tile lies above and left of it
        _fan(sc, [p(0, 0), p(192, 0), p(192, 30.5), p(61, 96), p(0, 96)], 0)
        _fan(sc, [p(192, 96), p(61, 96), p(192, 30.5)], 0, 1)
    elif kind == "top_right":      # x - 2 y = 63 through (127, 32): the tile lies below and left of it
        _fan(sc, [p(63, 0), p(192, 0), p(192, 64.5)], 0)
        _fan(sc, [p(0, 96), p(0, 0), p(63, 0), p(192, 64.5), p(192, 96)], 0, 1)
    elif kind == "bottom_left":    # x - 2 y = -62 through (64, 63): the tile lies above and right of it
        _fan(sc, [p(192, 0), p(192, 96), p(130, 96), p(0, 31), p(0, 0)], 0)
        _fan(sc, [p(0, 96), p(0, 31), p(130, 96)], 0, 1)
    elif kind == "row_first":      # y = 32, the middle tile's first row: the triangle below owns it and covers the tile completely
        sc.rect(0, 0, 192, 32, 0, region=False)
        _fan(sc, [p(96, 96), p(0, 32), p(192, 32)], 0)
        _fan(sc, [p(0, 96), p(0, 32), p(96, 96)], 0, 1)
        _fan(sc, [p(192, 96), p(96, 96), p(192, 32)], 0)
    elif kind == "row_last":       # y = 63, its last row: the triangle above covers all of the tile but that row
        _fan(sc, [p(96, 0), p(192, 63), p(0, 63)], 0)
        _fan(sc, [p(0, 0), p(96, 0), p(0, 63)], 0, 1)
        _fan(sc, [p(192, 0), p(192, 63), p(96, 0)], 0)
        sc.rect(0, 63, 192, 33, 1, region=False)
    elif kind == "column_first":   # x = 64, its first column
        sc.rect(0, 0, 64, 96, 1, region=False)
        _fan(sc, [p(192, 48), p(64, 96), p(64, 0)], 0)
        _fan(sc, [p(192, 0), p(192, 48), p(64, 0)], 0, 1)
        _fan(sc, [p(192, 96), p(64, 96), p(192, 48)], 0)
    elif kind == "column_last":    # x = 127, its last column
        _fan(sc, [p(0, 48), p(127, 0), p(127, 96)], 0)
        _fan(sc, [p(0, 0), p(127, 0), p(0, 48)], 0, 1)
        _fan(sc, [p(0, 96), p(0, 48), p(127, 96)], 0)
        sc.rect(127, 0, 65, 96, 0, region=False)
    elif kind == "cover":
        sc.rect(0, 0, 192, 96, 0, region=False)
        sc.rect(0, 0, 192, 96, 2, z=Z_FAR_LAYER)                       # the same cut, behind
        for i, (x, y) in enumerate([(130, 2), (150, 6), (2, 66), (30, 70), (70, 4), (140, 40)]):
            sc.rect(x, y, 12, 9, i, z=2 * Z_FAR_LAYER)                 # ... and more behind both: these add to the count
    sc.regions.append((0, 0, 192, 96))
    # beside the region: a square of 48 px cut along both diagonals, so that every scene has ties of all eight classes
    gx, gy = (4, 100) if H >= 150 else (200, 4)
    sc.square(cross4(48 * PX), 48 * PX, TILES_KINDS.index(kind), gx * PX, gy * PX)
    return sc


# ---- limit: the largest frame ----------------------------------------------------------------------------------------------

def limit_scene(N=2048):
    """The N x N frame cut by the rows and columns through the centre of pixel N/2 and by both of its diagonals (x = y and
    x + y = N - 1 pass through pixel centres and through the frame's corners).  Vertices lie on the frame's corners and borders
    (in-frustum); the edge values A px + B py + C reach N/2 * 256 * N = 2^29 in magnitude at N = 2048, the top of the 32-bit
    range that the 24-bit multiplies' sums and the stepped edge values are exact in."""
    sc = Lattice("limit_%dx%d" % (N, N), N, N)
    sc.degenerate = []
    lo, hi, m = -128, N * PX - 128, (N // 2) * PX
    # upper left and lower right squares: along x = y
    _fan(sc, [(lo, lo), (m, lo), (m, m), (lo, m)], 0)
    _fan(sc, [(m, m), (hi, m), (hi, hi), (m, hi)], 0, 1)
    # upper right: x + y = (N - 1) * 256 from the frame's corner (hi, lo) meets the column x = m at y = m - 256
    _fan(sc, [(hi, lo), (m, m - PX), (m, lo)], 0)
    _fan(sc, [(hi, lo), (hi, m), (m, m), (m, m - PX)], 0, 1)
    # lower left: ... and the row y = m at x = m - 256
    _fan(sc, [(lo, hi), (lo, m), (m - PX, m)], 0)
    _fan(sc, [(lo, hi), (m - PX, m), (m, m), (m, hi)], 0, 1)
    sc.regions.append((0, 0, N, N))
    return sc


# ---- the list -----------------------------------------------------------------------------------------------------------

FRAMES = [(160, 120), (200, 150), (256, 128)]
BUILDERS = {}
for _W, _H in FRAMES:
    BUILDERS["tiny_%dx%d" % (_W, _H)] = (lambda W=_W, H=_H: tiny_scene(W, H))
    BUILDERS["small_%dx%d" % (_W, _H)] = (lambda W=_W, H=_H: small_scene(W, H))
    BUILDERS["records_%dx%d" % (_W, _H)] = (lambda W=_W, H=_H: records_scene(W, H))
for _W, _H in FRAMES[1:]:
    for _kind in TILES_KINDS:
        BUILDERS["tiles_%s_%dx%d" % (_kind, _W, _H)] = (lambda W=_W, H=_H, kind=_kind: tiles_scene(W, H, kind))
BUILDERS["tiny_160x120_near"] = lambda: tiny_scene(160, 120, Z_NEAR)
BUILDERS["small_160x120_near"] = lambda: small_scene(160, 120, Z_NEAR)
BUILDERS["records_200x150_near"] = lambda: records_scene(200, 150, Z_NEAR)
BUILDERS["limit_2048x2048"] = limit_scene
NAMES = tuple(BUILDERS)
_built = {}


def scene(name):
    if name not in _built:
        _built[name] = BUILDERS[name]()
    return _built[name]


def kind_of(name):
    return "near" if name.endswith("_near") else name.split("_")[0]


_reference = {}


def reference(name):
    """(winner, count, tally) of tests/fill_rule.py for a scene, computed once."""
    if name not in _reference:
        import fill_rule
        sc = scene(name)
        _reference[name] = fill_rule.rasterise(sc.tris, sc.W, sc.H, sc.zs)
    return _reference[name]


def expected_prim(name, n=1, reverse=False):
    """The oracle's prim plane as the integer reference predicts it: the winner's number in the draw list, -2 (the background
    quad, which covers these frames) where no triangle won."""
    winner = reference(name)[0]
    _, prim_of_tri = workload(name, n, reverse)
    return np.where(winner >= 0, prim_of_tri[np.maximum(winner, 0)], -2).astype(np.int32)


_workloads = {}


def workload(name, n=1, reverse=False):
    if (name, n, reverse) not in _workloads:
        _workloads[(name, n, reverse)] = scene(name).workload(n, reverse)
    return _workloads[(name, n, reverse)]


def covered_tiles(name):
    """The (tx, ty) of the tiles, as far as they lie in the frame, that one triangle whose box touches more than kCoopTiles tiles
    covers completely: whole-tile covers."""
    import fill_rule
    sc = scene(name)
    _, ntiles = sc.tile_clipped_areas()
    out = []
    for t in np.flatnonzero(ntiles > COOP_TILES):
        got = fill_rule.triangle_coverage(sc.tris[t], sc.W, sc.H)
        if got is None:
            continue
        full = np.zeros((sc.H, sc.W), bool)
        full[got[1]:got[1] + got[2].shape[0], got[0]:got[0] + got[2].shape[1]] = got[2]
        for ty in range(0, sc.H, TILE_H):
            for tx in range(0, sc.W, TILE_W):
                if full[ty:ty + TILE_H, tx:tx + TILE_W].all():
                    out.append((tx // TILE_W, ty // TILE_H))
    return out


# ---- what Mesa llvmpipe renders for the scenes: tests/golden/llvmpipe/lattice_scenes_WxH.npz ------------------------------

LLVMPIPE_REPLACE = 5.0


def llvmpipe_path(W, H):
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "llvmpipe", "lattice_scenes_%dx%d.npz" % (W, H))


def llvmpipe_names(W, H):
    """The scenes of one frame size that are stored: the tiny, small, records and tiles scenes at 1 m."""
    return [n for n in NAMES if n.endswith("_%dx%d" % (W, H)) and kind_of(n) in ("tiny", "small", "records", "tiles")]


def llvmpipe_frames(name):
    """(key, projection, sensor depth, harness renderables, oracle draws) of a scene: all links, then each link alone.  The
    sensor plane lies half a metre behind the front layer, so the mask is the coverage."""
    sc = scene(name)
    wl, _ = workload(name)
    depth = np.full((sc.H, sc.W), min(sc.zs) + 0.5, np.float32)
    draws = wl.oracle_draws(0)
    for which in [None] + list(range(len(draws))):
        part = draws if which is None else draws[which:which + 1]
        rend = [(tf, [("mesh", pre, op, v, t)]) for tf, pre, op, v, t in part]
        yield "%s/%s" % (name, "all" if which is None else "link%d" % which), wl.projection[0], depth, rend, part
