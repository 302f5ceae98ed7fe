"""Expected virtual depth planes (include/rtuf.h, VIRTUAL DEPTH; rtuf_render_batch*) from the CPU oracle's debug output, for the
tests and scripts/virtual_rate.py.  The oracle's `zwin` is the float window z of every pixel's winner and `prim` its source
triangle (-2: the background quad, -1: no fragment); the virtual depth is the shader's to_linear_depth(z) in numpy float32 with
the host's shade_num / shade_off order of operations (as dilation_check.shade), the empty value where no link won (numpy only)."""
import numpy as np


def expected_virtual(zwin, prim, z_near, z_far, empty):
    """[..., H, W] float32: num / (zwin - off) where a link's fragment won (prim >= 0), `empty` elsewhere."""
    f = np.float32
    with np.errstate(all="ignore"):
        num = (f(z_near) * f(z_far)) / (f(z_near) - f(z_far))
        off = f(z_far) / (f(z_far) - f(z_near))
        virt = (f(num) / (np.asarray(zwin, np.float32) - f(off))).astype(np.float32)
    return np.where(np.asarray(prim) >= 0, virt, f(empty)).astype(np.float32)


def metres_to_u16(m):
    """The 16UC1 outputs' conversion (cv::Mat::convertTo(CV_16U, 1000.0)): round-half-even of float32(m * 1000), saturated to
    [0, 65535]; NaN and products outside the int32 range give 0."""
    with np.errstate(all="ignore"):
        v = (np.asarray(m, np.float32) * np.float32(1000.0)).astype(np.float32)
        ok = (v >= np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))      # (False for NaN)
        q = np.rint(np.where(ok, v, np.float32(0.0)).astype(np.float64))
    return np.clip(q, 0, 65535).astype(np.uint16)


def expected_virtual_u16(zwin, prim, z_near, z_far, empty):
    """The 16UC1 form: every value of expected_virtual, the empty value included, through metres_to_u16."""
    return metres_to_u16(expected_virtual(zwin, prim, z_near, z_far, empty))


def bits_equal_f32(got, want):
    """Bit-for-bit equality of two float32 arrays; NaN patterns compare equal where both sides are NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    return got.shape == want.shape and bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | both_nan))
