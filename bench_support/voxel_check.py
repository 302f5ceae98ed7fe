"""Expected outputs of the voxel occupancy grids (include/rtuf.h, VOXEL OCCUPANCY GRIDS) in numpy float32, for the tests and
scripts/voxel_rate.py: from sensor planes, the masks the filter is expected to give them, intrinsics, optional transforms and
the grid -- or from point lists and verdicts.  Every operation is a single float32 operation in the header's order; points
and kept pixels are cloud_check's, the transform chain is points_check's."""
import numpy as np

from bench_support import cloud_check as CC
from bench_support import points_check as PC

F = np.float32
MAX_DIM = 2048
MAX_VOXELS = 1 << 27


class Grid:
    """origin [3] and voxel_size as doubles, dims (nx, ny, nz): what rtuf_set_voxel_grid is given."""

    def __init__(self, origin, voxel_size, dims):
        self.origin = tuple(float(q) for q in origin)
        self.voxel_size = float(voxel_size)
        self.dims = tuple(int(q) for q in dims)
        self.n_voxels = self.dims[0] * self.dims[1] * self.dims[2]
        self.n_words = (self.n_voxels + 31) // 32

    def stored(self):
        """(origin [3] float32, inv float32): the origin rounded to float, inv = 1.0f / (float)voxel_size."""
        with np.errstate(all="ignore"):
            return np.array(self.origin, np.float64).astype(F), F(F(1.0) / F(self.voxel_size))


def voxel_of(points, grid):
    """(inside [count] bool, index [count] int64, -1 where not inside) of world points [count,3]: g_r = (p_r - o_r) * inv,
    inside iff 0 <= g_r < (float)dims_r for every r, then i_r = (int)g_r.  The range tests come before the conversions."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    o, inv = grid.stored()
    with np.errstate(all="ignore"):
        g = ((p - o[None, :]).astype(F) * inv).astype(F)
        inside = np.ones(len(p), bool)
        for r in range(3):
            inside &= (g[:, r] >= F(0)) & (g[:, r] < F(grid.dims[r]))
    i = np.where(inside[:, None], g, F(0)).astype(np.int64)
    nx, ny, _ = grid.dims
    index = (i[:, 2] * ny + i[:, 1]) * nx + i[:, 0]
    return inside, np.where(inside, index, -1)


def plane_insert(sensor, mask, intrinsics, matrix, grid):
    """One stream's plane form: (indices [inserted] int64 of the inserted pixels, summary [4] uint32: inserted, outside the
    grid, not kept, total).  mask: 0 / non-zero or booleans, the filter's expected mask of the plane."""
    s = np.asarray(sensor, np.float32)
    k = CC.kept(s, mask)
    world = PC.transformed(CC.points(s, intrinsics)[k], matrix)
    inside, index = voxel_of(world, grid)
    n_in = int(inside.sum())
    return index[inside], np.array([n_in, int(k.sum()) - n_in, int((~k).sum()), s.size], np.uint32)


def list_insert(points, verdict, point_matrix, world_matrix, grid):
    """One stream's list form: points [count,3] (the entries j < min(count, capacity)), verdict [count] or None, the stream's
    point transform and world transform (None: none) -> (indices, summary) as plane_insert gives them."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    taken = np.ones(len(p), bool) if verdict is None else np.asarray(verdict) == PC.KEPT
    world = PC.transformed(PC.transformed(p[taken], point_matrix), world_matrix)
    inside, index = voxel_of(world, grid)
    n_in = int(inside.sum())
    return index[inside], np.array([n_in, int(taken.sum()) - n_in, int((~taken).sum()), len(p)], np.uint32)


def accumulate(indices, grid, bits=None, counts=None):
    """ORs and adds lists of voxel indices into (bits [n_words] uint32, counts [n_voxels] uint32): fresh arrays, or the given
    ones continued.  Counts wrap modulo 2^32."""
    total = np.zeros(grid.n_voxels, np.int64) if counts is None else np.asarray(counts).reshape(-1).astype(np.int64)
    for idx in indices:
        total += np.bincount(np.asarray(idx, np.int64), minlength=grid.n_voxels)
    counts = (total & 0xFFFFFFFF).astype(np.uint32)
    occupied = np.zeros(grid.n_words * 32, np.uint8)
    for idx in indices:
        occupied[np.asarray(idx, np.int64)] = 1
    new_bits = np.packbits(occupied, bitorder="little").view("<u4").astype(np.uint32)
    return (new_bits if bits is None else (np.asarray(bits, np.uint32) | new_bits)), counts


def expected_planes(sensors, masks, intrinsics, matrices, grid):
    """A batch: (bits, counts, summary [n,4]) of one insert of n streams into an empty grid."""
    parts = [plane_insert(sensors[s], masks[s], intrinsics[s], matrices[s], grid) for s in range(len(sensors))]
    bits, counts = accumulate([p[0] for p in parts], grid)
    return bits, counts, np.stack([p[1] for p in parts])


def rotation_z(angle, shift=(0.0, 0.0, 0.0)):
    """[16] float64 column-major: a rotation about z by `angle` radians and a shift."""
    M = np.eye(4)
    M[0, 0], M[0, 1], M[1, 0], M[1, 1] = np.cos(angle), -np.sin(angle), np.sin(angle), np.cos(angle)
    M[:3, 3] = shift
    return np.ascontiguousarray(M.T.reshape(16))
