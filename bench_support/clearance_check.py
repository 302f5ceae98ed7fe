"""Expected link clearance tables (include/rtuf.h, LINK CLEARANCE TABLES) in numpy, for the tests and scripts/clearance_rate.py:
brute force over the kept points of cloud_check.compacted and the posed spheres.  The centres come from the doubles of
rtuf_debug_read_poses (or the matrices a test staged) and the camera's offset_inv through explicit elementwise operations --
every product and every sum is one numpy operation, never `@` -- and the clearances are single float32 operations in the
header's order."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
DTYPE = np.dtype([("clearance", "<f4"), ("pixel", "<u4"), ("sphere", "<u4"), ("points_within", "<u4")])


def transform(m, p):
    """Rows 0 .. 2 of a column-major 4x4 (16 doubles) times (p, 1): ((m0 x + m4 y) + m8 z) + m12, p [...,3] float64."""
    m = np.asarray(m, np.float64).reshape(16)
    p = np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        rows = []
        for r in range(3):
            a = m[r] * p[..., 0]
            b = m[4 + r] * p[..., 1]
            c = m[8 + r] * p[..., 2]
            rows.append(((a + b) + c) + m[12 + r])
    return np.stack(rows, axis=-1)


def centre(link_tf, cam_tf, offset_inv, c):
    """Camera-frame centre(s) [...,3] float32 of sphere centre(s) c [...,3] float32 given in the link's vertex frame."""
    p = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return transform(offset_inv, transform(cam_tf, transform(link_tf, p))).astype(np.float32)


def point_sphere(p, c, r):
    """Clearance float32 of points p [...,3] to the sphere c [3], r: sqrt((dx dx + dy dy) + dz dz) - r."""
    p = np.asarray(p, np.float32)
    c = np.asarray(c, np.float32)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[..., 0] - c[0], p[..., 1] - c[1], p[..., 2] - c[2]
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        return (np.sqrt(d2) - F(r)).astype(np.float32)


def posed(link_tf, cam_tf, offset_inv, links, xyz):
    """Camera-frame centres [n,3] float32 of spheres on global links `links` of one stream: link_tf [L,16] doubles."""
    link_tf = np.asarray(link_tf, np.float64).reshape(-1, 16)
    out = np.empty((len(links), 3), np.float32)
    for i, l in enumerate(links):
        out[i] = centre(link_tf[int(l)], cam_tf, offset_inv, np.asarray(xyz, np.float32)[i])
    return out


def _row(points, index, centres, radii, ids, max_distance):
    best = None
    hit = np.zeros(len(points), bool)
    for c, r, i in zip(centres, radii, ids):
        cl = point_sphere(points, c, r)
        with np.errstate(invalid="ignore"):
            inside = cl < F(max_distance)
        if not inside.any():
            continue
        hit |= inside
        cmin = cl[inside].min()
        pix = int(index[inside][cl[inside] == cmin].min())
        cand = (float(cmin), pix, int(i))
        if best is None or cand < best:
            best = cand
    if best is None:
        return (F(np.inf), NONE, NONE, 0)
    return (F(best[0]), best[1], best[2], int(hit.sum()))


def table(points, index, centres, radii, labels, ids, n_labels, max_distance):
    """The [n_labels] rows of one stream: points [N,3] float32 and index [N] of its kept pixels (cloud_check.compacted),
    and the spheres the stream sees: camera-frame centres [M,3], radii, labels and context-global ids.  Spheres of label 0 or
    of labels >= n_labels take no part; row 0 is over all the others together."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    index = np.asarray(index, np.uint32).reshape(-1)
    centres = np.asarray(centres, np.float32).reshape(-1, 3)
    radii = np.asarray(radii, np.float32).reshape(-1)
    labels = np.asarray(labels, np.int64).reshape(-1)
    ids = np.asarray(ids, np.int64).reshape(-1)
    out = np.zeros(n_labels, DTYPE)
    use = (labels >= 1) & (labels < n_labels)
    for row in range(n_labels):
        sel = use if row == 0 else use & (labels == row)
        out[row] = _row(points, index, centres[sel], radii[sel], ids[sel], max_distance)
    return out
