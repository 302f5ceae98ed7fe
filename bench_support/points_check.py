"""Expected outputs of the point list batches (include/rtuf.h, POINT LIST BATCHES) in numpy float32, for the tests and
scripts/points_rate.py: from a point list, the stream's pinhole, an optional transform and the virtual depth plane the CPU
oracle gives (empty pixels +inf).  Every operation is a single float32 operation in the header's order.  Also the point
makers the tests share."""
import numpy as np

from bench_support import cloud_check as CC

F = np.float32
KEPT, FILTERED, OUTSIDE = 0, 1, 2
NO_PIXEL = 0xFFFFFFFF
MAX_RADIUS = 4


def stored_intrinsics(fx, fy, cx, cy):
    """(fx, fy, cx, cy) as the points kernel reads them: each double rounded to float."""
    return F(float(fx)), F(float(fy)), F(float(cx)), F(float(cy))


def transformed(points, matrix):
    """[count,3] float32: p'_r = ((m[r] x + m[4+r] y) + m[8+r] z) + m[12+r] with the column-major matrix's 12 used entries
    rounded to float; matrix None: the points as given, untouched."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    if matrix is None:
        return p
    m = np.asarray(matrix, np.float64).reshape(16).astype(np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        out = [(((m[r] * x).astype(F) + (m[4 + r] * y).astype(F)).astype(F) + (m[8 + r] * z).astype(F)).astype(F) + m[12 + r] for r in range(3)]
    return np.stack([o.astype(F) for o in out], axis=1)


def pixel_of(points, intrinsics, W, H):
    """(judged [count] bool, u [count] int64, v [count] int64) of points already in the optical frame; u = v = 0 where the
    point is not judged.  The range tests come before the conversion to int."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    fx, fy, cx, cy = stored_intrinsics(*intrinsics)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        zok = (z > F(0)) & (z < F(np.inf))
        a = (x / z).astype(F)
        b = (y / z).astype(F)
        uf = (((a * fx).astype(F) + cx).astype(F) + F(0.5)).astype(F)
        vf = (((b * fy).astype(F) + cy).astype(F) + F(0.5)).astype(F)
        judged = zok & (uf >= F(0)) & (uf < F(W)) & (vf >= F(0)) & (vf < F(H))
    u = np.where(judged, uf, F(0)).astype(np.int64)
    v = np.where(judged, vf, F(0)).astype(np.int64)
    return judged, u, v


def window_min(plane, r):
    """[H,W] float32: the smallest value of the (2r+1)^2 square around every pixel, clipped to the image (never padded)."""
    plane = np.asarray(plane, np.float32)
    H, W = plane.shape
    pad = np.full((H + 2 * r, W + 2 * r), np.inf, np.float32)      # (+inf never wins a minimum: the same as clipping)
    pad[r:r + H, r:r + W] = plane
    out = plane.copy()
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = np.fmin(out, pad[dy:dy + H, dx:dx + W])
    return out


def verdicts(points, intrinsics, virtual, threshold, r=0, matrix=None):
    """(verdict [count] uint8, pixel [count] uint32) of one stream: virtual is its [H,W] float32 plane with +inf where no link
    drew, threshold rtuf_params.depth_distance_threshold."""
    virtual = np.asarray(virtual, np.float32)
    H, W = virtual.shape
    p = transformed(points, matrix)
    judged, u, v = pixel_of(p, intrinsics, W, H)
    vmin = window_min(virtual, r)[v, u]
    with np.errstate(all="ignore"):
        filtered = p[:, 2] > (vmin - F(threshold)).astype(F)
    verdict = np.where(judged, np.where(filtered, FILTERED, KEPT), OUTSIDE).astype(np.uint8)
    pixel = np.where(judged, v * W + u, NO_PIXEL).astype(np.uint32)
    return verdict, pixel


def summary(verdict):
    """[4] uint32: kept, filtered, outside, count."""
    v = np.asarray(verdict)
    return np.array([(v == KEPT).sum(), (v == FILTERED).sum(), (v == OUTSIDE).sum(), v.size], np.uint32)


# ---- point makers ---------------------------------------------------------------------------------------------------------

def grid_points(sensor, intrinsics):
    """[H*W,3] float32: cloud_point of every pixel of an [H,W] plane with z = the value there, row-major.  Values that carry
    no point (NaN, 0, negatives, +inf) make points that are not judged."""
    s = np.asarray(sensor, np.float32)
    return np.ascontiguousarray(CC.points(s, intrinsics).reshape(-1, 3))


def boundary_points(virtual, threshold, intrinsics):
    """For every pixel a link drew: three points on it, z = V - t exactly, its float neighbour below and the one above ->
    (points [3*k,3], expected verdict [3*k]: kept, kept, filtered).  A window of radius 0 is meant."""
    virtual = np.asarray(virtual, np.float32)
    v, u = np.nonzero(np.isfinite(virtual))
    on = (virtual[v, u] - F(threshold)).astype(F)
    zs = np.stack([on, np.nextafter(on, F(-np.inf)), np.nextafter(on, F(np.inf))], axis=1).reshape(-1)
    uu, vv = np.repeat(u, 3), np.repeat(v, 3)
    pts = CC.points(zs, intrinsics, uu, vv)
    return np.ascontiguousarray(pts, np.float32), np.tile(np.array([KEPT, KEPT, FILTERED], np.uint8), len(u))


EDGE_VALUES = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-42, -1.0, 1.0, 3.0e38, 1e-30], np.float32)


def edge_points():
    """Every triple of the edge values (NaN, +-0, +-inf, subnormals, a negative z, huge and tiny numbers)."""
    e = EDGE_VALUES
    x, y, z = np.meshgrid(e, e, e, indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3))


def random_points(rng, count):
    """A box from -3 to 3 m across and -1 to 9 m deep."""
    p = np.empty((count, 3), np.float32)
    p[:, 0] = rng.uniform(-3.0, 3.0, count)
    p[:, 1] = rng.uniform(-3.0, 3.0, count)
    p[:, 2] = rng.uniform(-1.0, 9.0, count)
    return p


def rigid_transform(rng):
    """[16] float64 column-major: a rotation of up to 0.3 rad about a random axis and a shift of up to 0.2 m."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-0.3, 0.3)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = rng.uniform(-0.2, 0.2, 3)
    return np.ascontiguousarray(M.T.reshape(16))
