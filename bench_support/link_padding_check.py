"""Expected outputs of link padding (include/rtuf.h, LINK PADDING) from the CPU oracle's debug planes, for the tests and
scripts/link_padding_rate.py.  A drawn pixel q of a padded link spreads its window z over the disc of R2(q) around it, with
R2 = (uint32)(rho * rho), rho = fmin((pad * f) / d, 16), d = num / (z - off): rtuf_numerics.h's link_padding_reach2 in numpy
float32, every operation rounded on its own (tests/link_padding_check.cpp holds the two against each other bit for bit).  The
padded z of a pixel is the smallest z that reaches it, by brute force over the 33 x 33 offsets, and the planes are the
shader's compare of it (dilation_check.shade).  The oracle's `prim` maps primitive -> draw -> link as in
link_thresholds_check.prim_thresholds.  The oracle itself is not changed (numpy only)."""
import numpy as np

from bench_support.dilation_check import drawn_z, shade
from bench_support.link_thresholds_check import prim_thresholds
from bench_support.link_thresholds_check import workload_draws  # noqa: F401  (padding, triangle count) of every draw, for reach2

MAX_PX = 16      # RTUF_MAX_LINK_PADDING_PX


def shade_consts(z_near, z_far):
    """(num, off) of to_linear_depth as the host computes them (rtuf_numerics.h shade_num / shade_off)."""
    f = np.float32
    with np.errstate(all="ignore"):
        return f((f(z_near) * f(z_far)) / (f(z_near) - f(z_far))), f(f(z_far) / (f(z_far) - f(z_near)))


def reach2_values(z, pad, f, num, off):
    """link_padding_reach2 elementwise: z, pad, f float32 arrays (or scalars) that broadcast; num, off float32 scalars."""
    z, pad, f = (np.asarray(a, np.float32) for a in (z, pad, f))
    with np.errstate(all="ignore"):
        d = (np.float32(num) / (z - np.float32(off)).astype(np.float32)).astype(np.float32)
        rho = np.fmin(((pad * f).astype(np.float32) / d).astype(np.float32), np.float32(MAX_PX)).astype(np.float32)
        sq = (rho * rho).astype(np.float32)
        spreads = ~np.isnan(z) & (pad > 0)
        return np.where(spreads, sq, np.float32(0)).astype(np.uint32)


def reach2(zwin, prim, draw_pad, draw_ntris, f, z_near, z_far):
    """[H,W] uint32 R2 of every pixel of one plane: draw_pad[d] the padding of draw d's link, which owns the next draw_ntris[d]
    primitive ids; f = (float)max(fx, fy) of the stream.  0 where the background quad won or nothing was drawn."""
    table = prim_thresholds(draw_pad, draw_ntris)
    pad = np.zeros(prim.shape, np.float32)
    drawn = prim >= 0
    pad[drawn] = table[prim[drawn]]
    num, off = shade_consts(z_near, z_far)
    return reach2_values(drawn_z(zwin, prim), pad, np.float32(f), num, off)


def padded_z(z, R2):
    """z'(p) = min z(q) over q in the plane with z(q) not NaN and |p - q|^2 <= R2(q), NaN where there is none: brute force over
    the 33 x 33 offsets.  z: the z-surface (NaN where nothing was drawn)."""
    H, W = z.shape
    r = MAX_PX
    assert int(R2.max(initial=0)) <= r * r
    zi = np.full((H + 2 * r, W + 2 * r), np.inf, np.float32)
    zi[r:r + H, r:r + W] = np.where(np.isnan(z), np.float32(np.inf), z)
    # a NaN source reaches nobody but itself, and brings nothing there: -1 fails every test
    ri = np.full((H + 2 * r, W + 2 * r), -1, np.int64)
    ri[r:r + H, r:r + W] = np.where(np.isnan(z), -1, R2.astype(np.int64))
    out = np.full((H, W), np.inf, np.float32)
    top = int(R2.max(initial=0))                       # (offsets no source reaches bring nothing)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx * dx + dy * dy > top:
                continue
            src_z = zi[r + dy:r + dy + H, r + dx:r + dx + W]
            src_r = ri[r + dy:r + dy + H, r + dx:r + dx + W]
            np.minimum(out, np.where(dx * dx + dy * dy <= src_r, src_z, np.float32(np.inf)), out=out)
    out[np.isinf(out)] = np.nan
    return out


def expected_planes(zwin, prim, sensor, draw_pad, draw_ntris, f, z_near, z_far, max_diff, replace):
    """(masked f32, mask u8 0 / 255, R2 u32) of one plane with the global threshold max_diff: the GL clear colour (0, 0) where
    no z reaches the pixel."""
    R2 = reach2(zwin, prim, draw_pad, draw_ntris, f, z_near, z_far)
    zp = padded_z(drawn_z(zwin, prim), R2)
    masked, mask = shade(zp, np.asarray(sensor, np.float32), z_near, z_far, max_diff, replace)
    return masked, mask, R2
