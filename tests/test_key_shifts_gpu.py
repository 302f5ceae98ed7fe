"""GPU (-m gpu): near geometry at every depth-key shift the library can choose.

The tile kernel's depth key is {z24, draw order << shift | low `shift` bits of the float z}, with shift = key_shift_for(n_tris)
(rtuf_numerics.h) for the triangles of EVERY model in the context.  In tiles with near geometry (window z <= 0.5) the shift
decides the low-bit mask, the exact-z floor exact_z_floor(shift) below which a winner takes the exact-z pass, the decoding
near_z_from_key and where the order lands in records and fragments.  tests/near_key_check.cpp proves those functions on the CPU
for every shift; these tests run the kernel's wiring of them at shifts 16 .. 7 against the CPU oracle, bit for bit: mask, masked
depth, the two-kernel z-surface (against the oracle's winning float z) and the bit-packed output.

The shift is set by padding the context with one model that no stream renders: many triangles over four vertices behind the
camera, placed BETWEEN the two models that are rendered, so the first model keeps draw orders from 1 and the second one ends at
n_tris -- the last triangle's order sets the top bit of the order field (n = 2^(31 - s), the smallest count with shift s) or
every bit of it (n = 2^(32 - s) - 1).  The oracle draws the two rendered models only: the relative draw order is the same.

The scene (window coordinates, unprojected through the projection): tilted quads whose z runs from behind the near plane
(clipped) through 1.5x a level L, for L = 2^-15 .. 0.3, so that every shift's floor exact_z_floor(s) * 2^-24 = 2^(2-s) has drawn
pixels below and above it; a near triangle over a whole tile; a far wall over whole tiles; small far triangles (fragments) all
over; fronto-parallel layers at the same eye depth (z ties decided by draw order) in both models and in records and fragments;
and pairs of layers with equal 24-bit depth but different float z, the later one (up to the context's very last triangle)
with the smaller float: GL_LESS keeps the first, whose float must come back from the key's low bits.  The sensor sits on the
compare threshold of the oracle's winners (and one ulp either side), so a winner's z that is off by a few ulps of the threshold
flips the mask.

Shift 7 needs 2^24 padding triangles (200 MB of indices); finalize takes about 1 s and the context about 200 MB of device
memory (printed with pytest -s), so every shift down to 7 is run.

The exact-z floor has a margin: near_z_from_key also decodes every float with z24 in [floor / 2, floor), so a kernel that used
exact_z_floor(shift + 1) would give the same results and no test can tell.  A floor 8x too low decodes some floats wrong at
the lower shifts, and these tests fail then."""
import time

import numpy as np
import pytest

import realtime_urdf_filter_amd as R
import scenes as S
from gpu_support import params
from gpu_support import run_modes, threshold_sensor
from oracle import bindings as O

pytestmark = pytest.mark.gpu

W, H = 384, 256
FX = 200.0
CX, CY = (W - 1) / 2.0, (H - 1) / 2.0
NEAR, FAR = 0.1, 8.0
P = S.projection(FX, FX, CX, CY, W, H, NEAR, FAR)
MAX_DIFF, REPLACE = 0.05, 5.0
IDENT = S.gl(np.eye(4))


def key_shift_for(n_tris):
    """rtuf_numerics.h key_shift_for: draw orders 1 .. n_tris take the key word's top bits, at most 16 bits remain for the
    float z's low bits (tests/near_key_check.cpp checks the rule and its users on the CPU)."""
    return min(16, 32 - int(n_tris).bit_length())


def exact_z_floor(shift):
    """rtuf_numerics.h exact_z_floor: winners with z24 below it take the exact-z pass in tiles with near geometry."""
    return 1 << (26 - shift)


def z24_of(z):
    """rtuf_numerics.h z24_of: round(clamp(z, 0, 1) * (2^24 - 1)), half to even, in float32."""
    zc = np.clip(np.asarray(z, np.float32), np.float32(0), np.float32(1))
    return np.rint((zc * np.float32(16777215.0)).astype(np.float32)).astype(np.int64)


def eye_depth(zw, near=NEAR, far=FAR):
    """Eye distance of window z zw (float64): the inverse of the projection's depth row and the viewport."""
    m22, m23 = -(far + near) / (far - near), -2.0 * far * near / (far - near)
    return m23 / ((2.0 * zw - 1.0) + m22)


def win_to_obj(xw, yw, zw, near=NEAR, far=FAR, fx=FX, cx=CX, cy=CY, h=H):
    d = eye_depth(zw, near, far)
    return [(xw - cx) / fx * d, (yw - (h - cy)) / fx * d, d]


def plane_tri(pts, zfun):
    """A triangle through window points pts [(x, y)] with window z zfun(x, y) (affine: a plane in eye space)."""
    return [win_to_obj(x, y, zfun(x, y)) for x, y in pts]


def front_rect(x0, y0, x1, y1, d):
    """Two fronto-parallel triangles at eye distance d (float32): every pixel's z is the same float."""
    d = float(np.float32(d))
    c = [[(x - CX) / FX * d, (y - (H - CY)) / FX * d, d] for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
    return [[c[0], c[1], c[3]], [c[1], c[2], c[3]]]


def oracle_z(draws):
    """The oracle's winning float z (NaN where only the background quad won) and primitive ids, for a dummy sensor."""
    _, _, zwin, prim, _ = O.filter_frame(np.full((H, W), 3.0, np.float32), P, draws, want_debug=True)
    z = zwin.copy()
    z[prim < 0] = np.nan
    return z, prim


def tie_depths(zw, count):
    """`count` pairs of float32 eye distances near window z zw whose fronto-parallel layers have EQUAL 24-bit depth but
    different float z: (d_first, d_later, z_first, z_later) with z_later < z_first -- probed through the oracle."""
    d0 = np.float32(eye_depth(zw))
    cand = [d0]
    for _ in range(47):
        cand.append(np.nextafter(cand[-1], np.float32(0)))
    draws, cells = [], []
    for i, d in enumerate(cand):
        x0, y0 = 8 + 20 * (i % 12), 8 + 20 * (i // 12)
        v = np.asarray(front_rect(x0, y0, x0 + 10, y0 + 10, d), np.float32).reshape(-1, 3)
        draws.append((IDENT, 0, [0.0, 0.0, 0.0], v, np.arange(6, dtype=np.uint32).reshape(2, 3)))
        cells.append((y0 + 5, x0 + 5))
    z, _ = oracle_z(draws)
    zs = [np.float32(z[c]) for c in cells]
    out = []
    for i in range(len(cand)):
        for j in range(i + 1, len(cand)):
            if zs[j] < zs[i] and z24_of(zs[i]) == z24_of(zs[j]) and all(cand[i] != o[0] for o in out):
                out.append((float(cand[i]), float(cand[j]), zs[i], zs[j]))
                break
        if len(out) == count:
            return out
    raise AssertionError("no equal-z24 layer pairs near window z %g" % zw)


LEVELS = [2.0 ** -15, 2.0 ** -13, 2.0 ** -11, 2.0 ** -9, 2.0 ** -7, 2.0 ** -5, 2.0 ** -3, 0.3]
LAST_BOX = (66, 94, 258, 382)          # rows y0:y1, columns x0:x1 under the context's last triangle and the layers it loses to


def build_scene(seed=5):
    """(tris of model A, tris of model B, equal-z24 pairs): triangles as [3][3] object coordinates in draw order; the LAST
    triangle of B is a layer that loses every tie it is in.  Tiles are 64 x 32: 6 x 8 of them."""
    rng = np.random.default_rng(seed)
    A, B = [], []
    # 1. tilted quads over one tile each in tile rows 0-1, z from -0.25 L (behind the near plane: clipped) to 1.5 L, with a
    # little slope in y; each quad's two triangles in different models
    for k, L in enumerate(LEVELS):
        x0, y0 = 64 * (k % 4), 32 * (k // 4)
        zf = (lambda x0, y0, L: lambda x, y: -0.25 * L + 1.75 * L * (x - x0 + 2) / 68.0 + 0.08 * L * (y - y0) / 32.0)(x0, y0, L)
        t1 = plane_tri([(x0 - 2, y0 - 2), (x0 + 66, y0 - 2), (x0 - 2, y0 + 34)], zf)
        t2 = plane_tri([(x0 + 66, y0 - 2), (x0 + 66, y0 + 34), (x0 - 2, y0 + 34)], zf)
        (A if k % 2 == 0 else B).append(t1)
        (B if k % 2 == 0 else A).append(t2)
    # 2. a near triangle over the whole of tile (0, 3) (a near cover, z 2^-10 .. 2^-7), a far wall over tile row 7
    B.append(plane_tri([(-2, 94), (136, 94), (-2, 232)], lambda x, y: 2.0 ** -10 + 2.0 ** -7 * ((x + 2) / 140.0 + (y - 94) / 300.0)))
    A.append(plane_tri([(-600, 222), (1000, 222), (200, 1000)], lambda x, y: 0.86 + 0.0002 * x + 0.0001 * (y - 222)))
    # 3. small far triangles (fragments, window z 0.55 .. 0.95) over the whole frame, alternating between the models
    for i in range(200):
        cx, cy, zz = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0.55, 0.95)
        pts = [(cx + rng.uniform(-3, 3), cy + rng.uniform(-3, 3)) for _ in range(3)]
        (A if i % 2 else B).append(plane_tri(pts, lambda x, y, zz=zz, cx=cx: zz + 0.001 * (x - cx)))
    # 4. identical-z ties (draw order decides, the float is the same): near records across the models in tile (3, 2), far
    # records against fragments of both models in tiles (4, 6) and (5, 6)
    dn = eye_depth(0.004)
    A += front_rect(192, 64, 238, 96, dn)
    B += front_rect(208, 64, 254, 96, dn)
    dfar = eye_depth(0.7)
    B += front_rect(256, 192, 384, 224, dfar)
    for i in range(60):
        cx, cy = 258 + 120 * rng.uniform(), 194 + 26 * rng.uniform()
        (A if i % 2 else B).extend(front_rect(cx, cy, cx + rng.uniform(1, 3), cy + rng.uniform(1, 3), dfar))
    # 5. equal z24, different float: the first-drawn layer keeps the pixel with its larger float; the later ones -- an early
    # layer of B, the context's last triangle -- lie closer by less than one 24-bit step
    (a1, l1, za1, zl1), = tie_depths(0.01, 1)
    (a3, l3, za3, zl3), = tie_depths(0.2, 1)
    A += front_rect(256, 64, 320, 96, a1)               # tile (4, 2): A first
    B += front_rect(320, 64, 384, 96, a1)               # tile (5, 2): early B first
    A += front_rect(128, 128, 192, 160, a3)             # tile (2, 4): A first
    B += front_rect(148, 128, 172, 160, l3)             #   ... an early B layer later
    pairs = [(za1, zl1, LAST_BOX), (za3, zl3, (132, 156, 150, 170))]
    d = float(np.float32(l1))                           # the LAST triangle, later, over tiles (4, 2) and (5, 2)
    B.append([[(x - CX) / FX * d, (y - (H - CY)) / FX * d, d] for x, y in ((254, 62), (560, 62), (254, 140))])
    return A, B, pairs


def as_draw(tris):
    v = np.asarray(tris, np.float32).reshape(-1, 3)
    return v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3)


def load_context(A, B, n_total):
    """Context with models A, padding, B (n_total triangles in all); stream 0 renders A and B."""
    vA, tA = as_draw(A)
    vB, tB = as_draw(B)
    n_pad = n_total - len(tA) - len(tB)
    assert n_pad > 0
    ctx = R.Context(W, H, 1, 0, params(REPLACE, MAX_DIFF))
    ma = ctx.add_model()
    ctx.add_draw(ma, ctx.add_link(ma), vA, tA)
    mp = ctx.add_model()
    pad_v = np.array([[0, 0, -1], [1, 0, -1], [0, 1, -1], [1, 1, -1]], np.float32)     # behind the camera
    pad_t = np.empty((n_pad, 3), np.uint32)
    pad_t[:, 0], pad_t[:, 1], pad_t[:, 2] = 0, 1 + (np.arange(n_pad) & 1), 3
    ctx.add_draw(mp, ctx.add_link(mp), pad_v, pad_t)
    del pad_t
    mb = ctx.add_model()
    ctx.add_draw(mb, ctx.add_link(mb), vB, tB)
    t0 = time.perf_counter()
    ctx.finalize_models()
    t_fin = time.perf_counter() - t0
    ctx.set_stream_models(0, [ma, mb])
    ctx.set_camera(0, P, None, None)
    ctx.set_link_poses(0, ma, IDENT[None])
    ctx.set_link_poses(0, mb, IDENT[None])
    return ctx, t_fin, [(IDENT, 0, [0.0, 0.0, 0.0], vA, tA), (IDENT, 0, [0.0, 0.0, 0.0], vB, tB)]


_scene = {}


def scene():
    """The scene, the oracle's view of it and the sensor plane on its threshold (built once)."""
    if not _scene:
        A, B, pairs = build_scene()
        vA, tA = as_draw(A)
        vB, tB = as_draw(B)
        draws = [(IDENT, 0, [0.0, 0.0, 0.0], vA, tA), (IDENT, 0, [0.0, 0.0, 0.0], vB, tB)]
        zw, prim = oracle_z(draws)
        depth = threshold_sensor(zw)
        depth = np.where(np.isnan(zw), S.sensor_depth(W, H), depth).astype(np.float32)     # (background: the usual plane)
        om, ok, zwin, prim, _ = O.filter_frame(depth, P, draws, max_diff=MAX_DIFF, replace_value=REPLACE, want_debug=True)
        _scene.update(A=A, B=B, pairs=pairs, depth=depth, om=om, ok=ok, zwin=zwin, prim=prim, nA=len(tA), nB=len(tB))
    return _scene


def check_scene_guards(sc, shift):
    """The scene really exercises shift `shift`: drawn near pixels below its exact-z floor and between the floor and 2^23,
    and the equal-z24 pairs won by the first-drawn layer -- the later one of them the context's last triangle."""
    drawn = sc["prim"] >= 0
    z24 = z24_of(np.where(drawn, sc["zwin"], 1.0))
    fl = exact_z_floor(shift)
    below = int((drawn & (z24 < fl)).sum())
    between = int((drawn & (z24 >= fl) & (z24 <= 1 << 23)).sum())
    assert below >= 200 and between >= 2000, (shift, below, between)
    last = sc["nA"] + sc["nB"] - 1                  # the oracle's primitive id of B's last triangle
    for zfirst, zlater, (y0, y1, x0, x1) in sc["pairs"]:
        assert z24_of(zfirst) == z24_of(zlater) and zlater < zfirst
        assert (sc["zwin"][y0:y1, x0:x1].view(np.uint32) == np.float32(zfirst).view(np.uint32)).all()
    y0, y1, x0, x1 = LAST_BOX
    assert (sc["prim"][y0:y1, x0:x1] != last).all()


# (shift, n_tris): the smallest count of each shift (the last order sets the field's top bit), and for four shifts the largest
# (every order bit set)
CASES = [(s, 1 << (31 - s)) for s in range(16, 6, -1)] + [(s, (1 << (32 - s)) - 1) for s in (16, 13, 11, 9)]


@pytest.mark.parametrize("shift,n_tris", CASES, ids=["s%d_n%d" % c for c in CASES])
def test_near_geometry_at_key_shift(shift, n_tris):
    sc = scene()
    assert key_shift_for(n_tris) == shift
    check_scene_guards(sc, shift)
    ctx, t_fin, _ = load_context(sc["A"], sc["B"], n_tris)
    assert ctx.num_triangles() == n_tris
    st = run_modes(ctx, params(REPLACE, MAX_DIFF), sc["depth"][None], sc["om"][None], sc["ok"][None], sc["zwin"][None], sc["prim"][None],
                   "shift %d n %d" % (shift, n_tris))
    assert st["exact_tiles"] > 0, st
    assert st["cover_pass"] and st["cover_tiles"] > 0, st
    print("shift %2d  n_tris %9d  finalize %.2f s  device memory %.0f MB" % (shift, n_tris, t_fin, st["device_bytes"] / 2 ** 20))
    ctx.close()
