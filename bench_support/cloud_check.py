"""Expected outputs of the filtered point clouds (include/rtuf.h, FILTERED POINT CLOUDS) in numpy float32, for the tests and
scripts/cloud_rate.py: from a sensor plane, the mask the filter is expected to give it (0 / 255, or booleans) and the
intrinsics.  Every operation is a single float32 operation in the header's order."""
import numpy as np

F = np.float32
NAN_BITS = 0x7FC00000


def u16_to_metres(mm):
    """uint16 millimetres as every 16UC1 call reads them: float(u16) * 0.001f."""
    return (np.asarray(mm, np.uint16).astype(np.float32) * F(0.001)).astype(np.float32)


def stored_intrinsics(fx, fy, cx, cy):
    """(kx, ky, cx, cy) as rtuf_set_cloud_intrinsics stores them: the reciprocals taken in double, then rounded to float."""
    return F(1.0 / float(fx)), F(1.0 / float(fy)), F(float(cx)), F(float(cy))


def kept(sensor, mask):
    """[H,W] bool: not masked, and a positive finite sensor value."""
    s = np.asarray(sensor, np.float32)
    with np.errstate(invalid="ignore"):
        return (np.asarray(mask) == 0) & (s > 0) & (s < F(np.inf))


def points(sensor, intrinsics, u=None, v=None):
    """[..., 3] float32 point of every pixel of an [H,W] plane (or of the values `sensor` at pixels u, v), kept or not."""
    s = np.asarray(sensor, np.float32)
    kx, ky, cx, cy = stored_intrinsics(*intrinsics)
    if u is None:
        H, W = s.shape
        v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        du = (np.asarray(u).astype(np.float32) - cx).astype(np.float32)
        dv = (np.asarray(v).astype(np.float32) - cy).astype(np.float32)
        x = ((du * s).astype(np.float32) * kx).astype(np.float32)
        y = ((dv * s).astype(np.float32) * ky).astype(np.float32)
    return np.stack([x, y, s], axis=-1)


def organized(sensor, mask, intrinsics):
    """[H,W,3] float32: the point where the pixel is kept, three quiet NaNs (0x7fc00000) elsewhere."""
    p = points(sensor, intrinsics)
    out = np.full(p.shape, NAN_BITS, np.uint32).view(np.float32)
    k = kept(sensor, mask)
    out[k] = p[k]
    return out


def compacted(sensor, mask, intrinsics):
    """(points [count,3] float32, index [count] uint32 = v * W + u, count): the kept pixels in row-major order."""
    k = kept(sensor, mask)
    idx = np.flatnonzero(k.ravel()).astype(np.uint32)
    return organized(sensor, mask, intrinsics)[k], idx, int(k.sum())


def classes(sensor, mask):
    """(kept, filtered, invalid) pixel counts of a plane: filtered = masked; invalid = a sensor value without a point (NaN, 0,
    negative, +inf), masked or not."""
    s = np.asarray(sensor, np.float32)
    with np.errstate(invalid="ignore"):
        valid = (s > 0) & (s < F(np.inf))
    return int(kept(sensor, mask).sum()), int((np.asarray(mask) != 0).sum()), int((~valid).sum())
