"""An exact integer rasteriser, written from the statement of the fill rule alone (test helper, numpy int64 only).

Coordinates are snapped window coordinates in 1/256 px: the centre of pixel (px, py) is the point (256 px, 256 py).

The rule.  For an ordered pair of vertices (i, j) the edge function is the cross product
    E_ij(p) = (y_i - y_j) (x_i - p_x) - (x_i - x_j) (y_i - p_y),
which is positive on one side of the line through i and j and negative on the other.  A triangle is oriented to positive area
-- E_01(v2) > 0; if it is negative two vertices trade places, if it is zero the triangle covers nothing -- and then each of its
edges (0,1), (1,2), (2,0) is positive at the opposite vertex.  A pixel centre p is covered iff for every edge E(p) > 0, or
E(p) == 0 and the edge owns its boundary.  With dcdx = y_i - y_j and dcdy = x_i - x_j an edge owns its boundary when
    dcdx < 0 or (dcdx == 0 and dcdy > 0)
(llvmpipe's rule: left edges and, of the horizontal ones, the top edge).

Besides coverage the rasteriser keeps a tally of exact ties: the (pixel, edge) pairs with E == 0 at a pixel centre of the frame
that lies in the CLOSED triangle (every E >= 0; a zero further along the edge's line decides nothing), by the edge's direction
class, by whether the edge owns its boundary and by whether the triangle got the pixel."""
import numpy as np

# the eight direction classes of an oriented triangle's edge: (sign of dcdx, sign of dcdy)
CLASSES = {
    (0, 1): "horizontal_top", (0, -1): "horizontal_bottom", (-1, 0): "vertical_left", (1, 0): "vertical_right",
    (-1, 1): "diagonal_left_upper", (-1, -1): "diagonal_left_lower", (1, 1): "diagonal_right_upper", (1, -1): "diagonal_right_lower",
}
CLASS_NAMES = tuple(CLASSES.values())
# the two classes of one line family are the two sides of the same lines
FAMILIES = {"horizontal": ("horizontal_top", "horizontal_bottom"), "vertical": ("vertical_left", "vertical_right"),
            "diagonal_down": ("diagonal_left_lower", "diagonal_right_upper"), "diagonal_up": ("diagonal_left_upper", "diagonal_right_lower")}


def owns_boundary(dcdx, dcdy):
    return dcdx < 0 or (dcdx == 0 and dcdy > 0)


def oriented(tri):
    """The triangle's vertices as Python ints with positive area, or None if its area is zero."""
    (x0, y0), (x1, y1), (x2, y2) = [(int(x), int(y)) for x, y in tri]
    area = (y0 - y1) * (x0 - x2) - (x0 - x1) * (y0 - y2)
    if area == 0:
        return None
    if area < 0:
        (x0, y0), (x1, y1) = (x1, y1), (x0, y0)
    return (x0, y0), (x1, y1), (x2, y2)


def _ceil_div(a, b):
    return -((-a) // b)


class Tally:
    """ties[class][(owned, covered)] -> count of (pixel, edge) pairs."""

    def __init__(self):
        self.ties = {c: {(o, k): 0 for o in (False, True) for k in (False, True)} for c in CLASS_NAMES}

    def add(self, cls, owned, covered, n):
        self.ties[cls][(owned, covered)] += int(n)

    def total(self, cls):
        return sum(self.ties[cls].values())

    def owned(self, cls):
        return self.ties[cls][(True, False)] + self.ties[cls][(True, True)]

    def not_owned(self, cls):
        return self.ties[cls][(False, False)] + self.ties[cls][(False, True)]

    def covered(self, cls):
        return self.ties[cls][(False, True)] + self.ties[cls][(True, True)]

    def not_covered(self, cls):
        return self.ties[cls][(False, False)] + self.ties[cls][(True, False)]


def triangle_coverage(tri, W, H, tally=None):
    """(px0, py0, covered[h, w] bool) of one triangle over the frame, or None where it covers nothing."""
    v = oriented(tri)
    if v is None:
        return None
    xs, ys = [p[0] for p in v], [p[1] for p in v]
    px0, px1 = max(_ceil_div(min(xs), 256), 0), min(max(xs) // 256, W - 1)          # pixel centres in the closed bounding box
    py0, py1 = max(_ceil_div(min(ys), 256), 0), min(max(ys) // 256, H - 1)
    if px1 < px0 or py1 < py0:
        return None
    X = (np.arange(px0, px1 + 1, dtype=np.int64) * 256)[None, :]
    Y = (np.arange(py0, py1 + 1, dtype=np.int64) * 256)[:, None]
    covered = np.ones((py1 - py0 + 1, px1 - px0 + 1), bool)
    closed = covered.copy()
    zeros = []
    for i in range(3):
        j = (i + 1) % 3
        dcdx, dcdy = ys[i] - ys[j], xs[i] - xs[j]
        assert abs(dcdx) < 2 ** 30 and abs(dcdy) < 2 ** 30          # (products below 2^62: exact in int64)
        E = dcdx * (xs[i] - X) - dcdy * (ys[i] - Y)
        own = owns_boundary(dcdx, dcdy)
        covered &= (E >= 0) if own else (E > 0)
        closed &= E >= 0
        zeros.append((E == 0, (int(np.sign(dcdx)), int(np.sign(dcdy))), own))
    if tally is not None:
        for zero, sign, own in zeros:
            on = zero & closed
            n_cov = int((on & covered).sum())
            tally.add(CLASSES[sign], own, True, n_cov)
            tally.add(CLASSES[sign], own, False, int(on.sum()) - n_cov)
    return px0, py0, covered


def rasterise(tris, W, H, z=None):
    """winner[H, W] int32 (triangle index, -1 where nothing covers; the smallest z wins where several do -- the scenes never
    stack two triangles of the same z), count[H, W] int32 (triangles covering each pixel), Tally."""
    winner = np.full((H, W), -1, np.int32)
    best = np.full((H, W), np.inf)
    count = np.zeros((H, W), np.int32)
    tally = Tally()
    for t, tri in enumerate(tris):
        got = triangle_coverage(tri, W, H, tally)
        if got is None:
            continue
        px0, py0, cov = got
        sl = (slice(py0, py0 + cov.shape[0]), slice(px0, px0 + cov.shape[1]))
        count[sl] += cov
        zt = 0.0 if z is None else float(z[t])
        take = cov & (zt < best[sl])
        winner[sl][take] = t
        best[sl][take] = zt
    return winner, count, tally
