"""Expected outputs of the voxel free space (include/rtuf.h, VOXEL FREE SPACE) in numpy float32, for the tests and
scripts/voxel_free_rate.py: from sensor planes, intrinsics, the streams' world_from_optical matrices and the grid.  Every
operation is a single float32 operation in the header's order (the inverse: float64, rounded once at the end); the transform
chain, the pixel and the window minimum are points_check's, valid sensor values are cloud_check's."""
import numpy as np

from bench_support import cloud_check as CC
from bench_support import points_check as PC

F = np.float32
D = np.float64
MAX_RADIUS = 4
FREE, NOT_FREE, NOT_SEEN = 0, 1, 2


def centres(grid):
    """[n_voxels,3] float32 in index order (x fastest): c_r = o_r + ((float)i_r + 0.5f) * (float)voxel_size."""
    o = np.array(grid.origin, D).astype(F)
    size = F(grid.voxel_size)
    axes = [(o[r] + ((np.arange(grid.dims[r]).astype(F) + F(0.5)).astype(F) * size).astype(F)).astype(F) for r in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3))


def inverse_transform(matrix):
    """[16] float32 column-major optical_from_world of a world_from_optical matrix (its 12 used entries rounded to float
    first), or None where it cannot be inverted: det 0 or not finite, or a result that is not finite as a float.  float64:
    cofactors p * q - r * s, det = (a00 C00 + a01 C01) + a02 C02, R = adj / det, t'_r = -((R_r0 t_0 + R_r1 t_1) + R_r2 t_2)."""
    m = np.asarray(matrix, D).reshape(16).astype(F).astype(D)
    a = [[m[4 * c + r] for c in range(3)] for r in range(3)]
    t = [m[12 + r] for r in range(3)]
    with np.errstate(all="ignore"):
        C = [[None] * 3 for _ in range(3)]
        C[0][0] = a[1][1] * a[2][2] - a[1][2] * a[2][1]
        C[0][1] = a[1][2] * a[2][0] - a[1][0] * a[2][2]
        C[0][2] = a[1][0] * a[2][1] - a[1][1] * a[2][0]
        C[1][0] = a[0][2] * a[2][1] - a[0][1] * a[2][2]
        C[1][1] = a[0][0] * a[2][2] - a[0][2] * a[2][0]
        C[1][2] = a[0][1] * a[2][0] - a[0][0] * a[2][1]
        C[2][0] = a[0][1] * a[1][2] - a[0][2] * a[1][1]
        C[2][1] = a[0][2] * a[1][0] - a[0][0] * a[1][2]
        C[2][2] = a[0][0] * a[1][1] - a[0][1] * a[1][0]
        det = (a[0][0] * C[0][0] + a[0][1] * C[0][1]) + a[0][2] * C[0][2]
        if not np.isfinite(det) or det == 0.0:
            return None
        out = np.zeros(16, D)
        for r in range(3):
            R = [C[c][r] / det for c in range(3)]
            out[12 + r] = -((R[0] * t[0] + R[1] * t[1]) + R[2] * t[2])
            for c in range(3):
                out[4 * c + r] = R[c]
        out = out.astype(F)
    return out if np.isfinite(out).all() else None


def projected(intrinsics, matrix, grid, W, H, world=None):
    """(judged [n_voxels] bool, u, v [n_voxels] int64, z [n_voxels] float32) of every voxel centre in one stream's W x H image:
    the centre through the inverse of `matrix` (world_from_optical, or None: as it is), then points_check.pixel_of.  world:
    centres(grid), where the caller has them already."""
    c = centres(grid) if world is None else world
    if matrix is not None:
        inv = inverse_transform(matrix)
        assert inv is not None, "the stream's transform cannot be inverted"
        c = PC.transformed(c, inv.astype(D))
    judged, u, v = PC.pixel_of(c, intrinsics, W, H)
    return judged, u, v, c[:, 2]


def state_of(sensor, proj, margin, r):
    """[n_voxels] uint8 -- FREE, NOT_FREE or NOT_SEEN -- from a stream's sensor values [H,W] and its projected(...) centres."""
    s = np.asarray(sensor, F)
    judged, u, v, z = proj
    valid = CC.kept(s, np.zeros(s.shape, np.uint8))
    emin = PC.window_min(np.where(valid, s, F(np.inf)).astype(F), r)[v, u]
    with np.errstate(all="ignore"):
        free = judged & valid[v, u] & (z < (emin - F(margin)).astype(F))
    return np.where(free, FREE, np.where(judged, NOT_FREE, NOT_SEEN)).astype(np.uint8)


def stream_state(sensor, intrinsics, matrix, grid, margin, r):
    """[n_voxels] uint8 of one stream: FREE, NOT_FREE or NOT_SEEN.  sensor: the [H,W] float32 values the stream reads (16UC1:
    cloud_check.u16_to_metres of the plane); matrix: world_from_optical or None."""
    s = np.asarray(sensor, F)
    return state_of(s, projected(intrinsics, matrix, grid, s.shape[1], s.shape[0]), margin, r)


def stream_free(sensor, intrinsics, matrix, grid, margin, r):
    """[n_voxels] bool: the voxels one stream frees."""
    return stream_state(sensor, intrinsics, matrix, grid, margin, r) == FREE


def pack(free, grid):
    """[n_voxels] bool -> [n_words] uint32, bit i & 31 of word i >> 5."""
    b = np.zeros(grid.n_words * 32, np.uint8)
    b[:grid.n_voxels] = free
    return np.packbits(b, bitorder="little").view("<u4").astype(np.uint32)


def unpack(words, grid):
    return np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little")[:grid.n_voxels].astype(bool)


def expected(sensors, intrinsics, matrices, grid, margin, r):
    """One carve of n streams into an empty free grid: (bits [n_words] uint32, summary [n,4] uint32: free, not free, not seen,
    n_voxels)."""
    states = [stream_state(sensors[s], intrinsics[s], matrices[s], grid, margin, r) for s in range(len(sensors))]
    summary = np.array([[(st == FREE).sum(), (st == NOT_FREE).sum(), (st == NOT_SEEN).sum(), grid.n_voxels] for st in states], np.uint32)
    free = np.zeros(grid.n_voxels, bool)
    for st in states:
        free |= st == FREE
    return pack(free, grid), summary
