"""Expected link residual tables (include/rtuf.h, LINK RESIDUAL TABLES; rtuf_link_residuals_batch*) from the CPU oracle's debug
planes, for the tests and scripts/link_residuals_rate.py.  The oracle's `zwin` is the float window z of every pixel's winner and
`prim` its source triangle (-2: the background quad, -1: no fragment); labels come from labels_check, thresholds from
link_thresholds_check, the virtual depth is the shader's to_linear_depth(z) in numpy float32 with the host's shade_num /
shade_off order of operations (as dilation_check.shade).  Every sum is an integer, so a table is compared for equality.  The
oracle itself is not changed (numpy only)."""
import numpy as np

from bench_support.labels_check import expected_labels
from bench_support.link_thresholds_check import pixel_thresholds

# rtuf_link_residuals: the row's fields in the header's order, 64 bytes
ROW = np.dtype([("pixels", "<u8"), ("invalid", "<u8"), ("filtered", "<u8"), ("in_front", "<u8"), ("behind", "<u8"), ("agree", "<u8"),
                ("sum_residual", "<i8"), ("sum_abs_residual", "<u8")])
Q_SCALE = np.float32(1048576.0)      # q counts 2^-20 m


def u16_to_metres(mm):
    """The 16UC1 calls' sensor value: float32(u16) * 0.001f."""
    return (np.asarray(mm).astype(np.float32) * np.float32(0.001)).astype(np.float32)


def virtual_depth(z, z_near, z_far):
    """num / (z - off) in float32 (rtuf_numerics.h shade_num / shade_off)."""
    f = np.float32
    with np.errstate(all="ignore"):
        num = (f(z_near) * f(z_far)) / (f(z_near) - f(z_far))
        off = f(z_far) / (f(z_far) - f(z_near))
        return (f(num) / (np.asarray(z, np.float32) - f(off))).astype(np.float32)


def quantise(r):
    """q of a float32 residual times 2^20: clipped to the int32 range, round half to even, NaN -> 0."""
    r = np.asarray(r, np.float32).astype(np.float64)
    q = np.rint(np.clip(r, -2147483648.0, 2147483647.0))
    return np.where(np.isnan(r), 0.0, q).astype(np.int64)


def classify(s, v, t):
    """Classes of DRAWN pixels with sensor s, virtual depth v and threshold t (float32 arrays of one shape):
    (invalid, filtered, in_front, behind, agree) as bool arrays and q as int64 (meaningful where agree)."""
    s, v, t = (np.asarray(a, np.float32) for a in (s, v, t))
    with np.errstate(all="ignore"):
        lo = (v - t).astype(np.float32)
        hi = (v + t).astype(np.float32)
        valid = s > 0
        filtered = s > lo
        beyond = s > hi
        q = quantise(((s - v).astype(np.float32) * Q_SCALE).astype(np.float32))
    return ~valid, filtered, valid & ~filtered, valid & filtered & beyond, valid & filtered & ~beyond, q


def table_from_planes(labels, drawn, s, v, t, n_labels):
    """The [n_labels] table of one stream from per-pixel planes: label (uint16), drawn (bool: a fragment reached the pixel,
    the background quad's included), sensor s, virtual depth v and threshold t (float32; v, t unused where not drawn)."""
    labels = np.asarray(labels).astype(np.int64).ravel()
    drawn = np.asarray(drawn, bool).ravel()
    s = np.asarray(s, np.float32).ravel()
    invalid, filtered, in_front, behind, agree, q = classify(s, np.asarray(v, np.float32).ravel(), np.asarray(t, np.float32).ravel())
    with np.errstate(invalid="ignore"):
        invalid = np.where(drawn, invalid, ~(s > 0))
    filtered, in_front, behind, agree = (c & drawn for c in (filtered, in_front, behind, agree))
    assert labels.max(initial=0) < n_labels
    out = np.zeros(n_labels, ROW)
    count = lambda m: np.bincount(labels[m], minlength=n_labels).astype(np.uint64)       # noqa: E731
    out["pixels"] = np.bincount(labels, minlength=n_labels)
    out["invalid"], out["filtered"], out["in_front"] = count(invalid), count(filtered), count(in_front)
    out["behind"], out["agree"] = count(behind), count(agree)
    sq, sa = np.zeros(n_labels, np.int64), np.zeros(n_labels, np.int64)
    np.add.at(sq, labels[agree], q[agree])
    np.add.at(sa, labels[agree], np.abs(q[agree]))
    out["sum_residual"], out["sum_abs_residual"] = sq, sa.astype(np.uint64)
    return out


def expected_table(zwin, prim, sensor, draw_labels, draw_ntris, draw_thr, global_thr, z_near, z_far, n_labels):
    """The [n_labels] table of one stream.  zwin / prim: the oracle's planes; sensor: float32 metres (16UC1: u16_to_metres);
    draw_labels / draw_thr / draw_ntris: label, threshold and triangle count of every draw the oracle was given (labels_check
    / link_thresholds_check .workload_draws; draw_thr None: the global threshold everywhere)."""
    prim = np.asarray(prim)
    labels = expected_labels(prim, draw_labels, draw_ntris)
    if draw_thr is None:
        t = np.full(prim.shape, np.float32(global_thr), np.float32)
    else:
        t = pixel_thresholds(prim, draw_thr, draw_ntris, global_thr)
    return table_from_planes(labels, prim != -1, sensor, virtual_depth(zwin, z_near, z_far), t, n_labels)


def tables_equal(got, want):
    """Equality of two tables field by field; returns (ok, text naming the first rows that differ)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False, "shape / dtype %r %r instead of %r %r" % (got.shape, got.dtype, want.shape, want.dtype)
    bad = np.zeros(got.shape, bool)
    for name in ROW.names:
        bad |= got[name] != want[name]
    if not bad.any():
        return True, ""
    idx = np.argwhere(bad)[:4]
    return False, "%d rows differ; " % int(bad.sum()) + "; ".join("row %s: %s instead of %s" % (tuple(i), got[tuple(i)], want[tuple(i)]) for i in idx)
