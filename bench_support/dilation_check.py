"""Expected outputs of silhouette dilation (rtuf_params.silhouette_dilation_px) from the CPU oracle's debug planes, for the
tests and scripts/dilation_rate.py: the window z where something was drawn, its clipped (2r+1)^2 minimum that ignores NaN,
and the shader's compare in numpy float32 with the host's shade_num / shade_off order of operations (numpy only)."""
import numpy as np


def drawn_z(zwin, prim):
    """The oracle's window z with NaN where nothing was drawn (prim == -1): what the z-surface holds."""
    return np.where(prim == -1, np.float32(np.nan), zwin).astype(np.float32)


def window_min(z, r):
    """Per-plane minimum over the (2r+1)^2 window clipped to the plane, ignoring NaN; NaN where the window holds none."""
    if r == 0:
        return z
    H, W = z.shape
    a = np.where(np.isnan(z), np.float32(np.inf), z).astype(np.float32)
    p = np.full((H, W + 2 * r), np.inf, np.float32)
    p[:, r:r + W] = a
    rows = p[:, 0:W].copy()
    for k in range(1, 2 * r + 1):
        np.minimum(rows, p[:, k:k + W], out=rows)
    q = np.full((H + 2 * r, W), np.inf, np.float32)
    q[r:r + H] = rows
    out = q[0:H].copy()
    for k in range(1, 2 * r + 1):
        np.minimum(out, q[k:k + H], out=out)
    out[np.isinf(out)] = np.nan
    return out


def shade(z, sensor, z_near, z_far, max_diff, replace):
    """masked = sensor > num / (z - off) - max_diff ? replace : sensor in float32 (rtuf_numerics.h shade_num / shade_off);
    masked 0 and mask 0 where z is NaN (nothing drawn: the GL clear colour).  Returns (masked f32, mask u8 0 / 255)."""
    f = np.float32
    with np.errstate(all="ignore"):
        num = (f(z_near) * f(z_far)) / (f(z_near) - f(z_far))
        off = f(z_far) / (f(z_far) - f(z_near))
        thr = (f(num) / (z.astype(np.float32) - f(off))).astype(np.float32) - f(max_diff)
        filt = sensor > thr
    masked = np.where(filt, f(replace), sensor).astype(np.float32)
    undrawn = np.isnan(z)
    masked[undrawn] = 0.0
    filt &= ~undrawn
    return masked, (filt * 255).astype(np.uint8)
