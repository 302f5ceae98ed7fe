"""GPU (-m gpu): depth ranges other than near 0.1 / far 8, covers cut by the far plane, degenerate shader uniforms and the
16UC1 output conversion at its edges -- each against the CPU oracle, bit for bit.

The product builds its projection from the same near / far planes it hands the shader (filter.py getProjectionMatrix), so
other planes move where window z 0.5 (tiles with near geometry, the exact-z pass) and 0.51 fall on the robot, where the
background quad (0.99 x far) sits and whether the compare threshold's fast division is admitted."""
import numpy as np
import pytest

import golden_io
import realtime_urdf_filter_amd as R
import scenes as S
from bench_support import workloads as WL
from gpu_support import bits_equal, params
from gpu_support import run_modes, threshold_sensor
from oracle import bindings as O
from realtime_urdf_filter_amd.filter import depth_f32_to_u16, depth_u16_to_f32

pytestmark = pytest.mark.gpu


def fast_div_admitted(near, far):
    """rtuf_numerics.h fast_div_admitted(shade_num, shade_off), in float32 as the host evaluates it."""
    n, f = np.float32(near), np.float32(far)
    with np.errstate(all="ignore"):
        num = np.float32(np.float32(n * f) / np.float32(n - f))
        off = np.float32(f / np.float32(f - n))
    a = abs(float(num))
    return bool(np.isfinite(num) and np.isfinite(off) and 2.0 ** -40 <= a <= 2.0 ** 40 and 1.0 + 2.0 ** -10 <= off <= 2.0 ** 20)


@pytest.mark.parametrize("near,far", [(0.05, 20.0), (0.3, 3.0), (0.5, 10.0), (0.001, 100.0)])
def test_coupled_planes_on_a_pr2_like_workload(near, far):
    """Projection and uniforms from the same planes (as filter.py builds them): the PR2-like robot with its forearm in front
    of the lens and the two walls, 3 VGA streams; fused, two-kernel (z-surface) and bit-packed, two batches each."""
    W, H, n = 640, 480, 3
    wl = WL.pr2_workload(n, W, H, total_triangles=30000, near_arm=True, walls=True, seed=7)
    fx, fy, cx, cy = WL._intrinsics(W, H)
    Pn, _, _ = R.projection_from_intrinsics(fx, fy, cx, cy, W, H, near, far)
    base = params(wl.replace_value, wl.max_diff, near_plane=near, far_plane=far)
    assert fast_div_admitted(near, far) == ((near, far) != (0.001, 100.0))
    ctx = R.Context(W, H, n, 0, base)
    ids = wl.load_into(ctx)
    wl.stage(ctx, ids)
    ctx.set_cameras(0, np.tile(Pn, (n, 1)), wl.offset_inv, wl.cam_tf)
    depth = wl.depth_batch()
    outs = [O.filter_frame(depth[s], Pn, wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], z_near=near, z_far=far,
                           max_diff=wl.max_diff, replace_value=wl.replace_value, want_debug=True) for s in range(n)]
    om, ok, zwin, prim = (np.stack([o[i] for o in outs]) for i in range(4))
    drawn = prim >= 0
    # the robot reaches both sides of window z 0.5 (eye depth 2nf / (n + f)) -- except at near 0.001, where that depth is
    # 2 mm from the lens -- and something lies beyond 0.51
    assert (drawn & (zwin <= 0.5)).sum() > 500 or near < 0.01, (near, far)
    assert (drawn & (zwin >= 0.51)).sum() > 500, (near, far)
    assert ok.any() and not ok.all()
    st = run_modes(ctx, base, depth, om, ok, zwin, prim, "planes %g / %g" % (near, far))
    if near == 0.05:
        assert st["exact_tiles"] > 0, st          # winners within 2^(26 - shift) z24 steps of the near plane
    ctx.close()


def far_wall_scene(W, H, P, proj_far, seed):
    """Walls tilted through the far plane over whole tiles (their window z runs from 0.97 to 1.03 across the frame), a
    near wall over two tiles, small triangles in front: window-space geometry unprojected through P's planes."""
    near = 0.1
    fx = -P[0] * W / 2
    cx, cy = (1 - P[8]) * W / 2, (P[9] + 1) * H / 2

    def obj(x, y, zw):
        m22, m23 = -(proj_far + near) / (proj_far - near), -2.0 * proj_far * near / (proj_far - near)
        d = m23 / ((2.0 * zw - 1.0) + m22)
        return [(x - cx) / fx * d, (y - (H - cy)) / fx * d, d]

    rng = np.random.default_rng(seed)
    tris = []
    # the far walls: one over the left half, one over the right, z 0.97 .. 1.03 along x and y
    for x0, x1 in ((-300.0, W / 2), (W / 2, W + 300.0)):
        zf = lambda x, y: 0.97 + 0.06 * (x / W) + 0.004 * (y / H)
        tris.append([obj(x0, -50, zf(x0, -50)), obj(x1, -50, zf(x1, -50)), obj(x0, H + 400, zf(x0, H + 400))])
        tris.append([obj(x1, -50, zf(x1, -50)), obj(x1, H + 400, zf(x1, H + 400)), obj(x0, H + 400, zf(x0, H + 400))])
    # small triangles in front of the walls in some tiles
    for _ in range(60):
        cx_, cy_, zz = rng.uniform(0, W), rng.uniform(0, H / 2), rng.uniform(0.6, 0.95)
        tris.append([obj(cx_ + rng.uniform(-4, 4), cy_ + rng.uniform(-4, 4), zz) for _ in range(3)])
    v = np.asarray(tris, np.float32).reshape(-1, 3)
    return v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("background", [True, False], ids=["analytic_background", "background_clipped"])
def test_whole_tile_covers_cut_by_the_far_plane(background):
    """Tiles with nothing but a wall tilted through the far plane (cover-only tiles, resolved from the cover's plane in
    registers) next to tiles with other geometry (resolved from the key tile): (i) with the background quad, (ii) with
    params.far_plane above the projection's far / 0.99, where the quad lies beyond the far plane and pixels the wall does
    not reach have no fragment at all (NaN in the z-surface; the bit-packed output is refused there).  The sensor sits on the
    threshold of the winners.  Where a cover is cut by the far plane its plane can evaluate to z >= 1 on a pixel, but such a
    fragment's 24-bit depth is 2^24 - 1, which never passes GL_LESS against the cleared depth: the cover-only path hands
    shade_threshold and the z-surface only z < 1, as the key path does (tests/golden/far_plane_covers*_160x120.npz pins both
    cases on llvmpipe)."""
    W, H, n = 320, 256, 2
    proj_far = 8.0
    P = S.projection(260.0, 260.0, (W - 1) / 2, (H - 1) / 2, W, H, 0.1, proj_far)
    far = proj_far if background else proj_far / 0.99 * 1.01
    base = params(5.0, 0.05, far_plane=far)
    v, t = far_wall_scene(W, H, P, proj_far, seed=31)
    ident = S.gl(np.eye(4))
    draws = [(ident, 0, [0.0, 0.0, 0.0], v, t)]
    ctx = R.Context(W, H, n, 0, base)
    m = ctx.add_model()
    ctx.add_draw(m, ctx.add_link(m), v, t)
    ctx.finalize_models()
    cams = []
    for s in range(n):
        C = np.eye(4)
        C[:3, 3] = [0.013 * s, -0.007 * s, 0.0]
        cams.append(S.gl(C))
        ctx.set_camera(s, P, None, cams[s])
        ctx.set_link_poses(s, m, ident[None])
    depth, om, ok, zwin, prim = [], [], [], [], []
    for s in range(n):
        _, _, zw, pr, _ = O.filter_frame(np.full((H, W), 3.0, np.float32), P, draws, None, cams[s], z_far=far, want_debug=True)
        d = threshold_sensor(np.where(pr >= 0, zw, np.float32(np.nan)), far=far, seed=s)
        d = np.where(pr >= 0, d, S.sensor_depth(W, H, 0.3 * s)).astype(np.float32)
        o = O.filter_frame(d, P, draws, None, cams[s], z_far=far, max_diff=0.05, replace_value=5.0, want_debug=True)
        depth.append(d)
        om.append(o[0]); ok.append(o[1]); zwin.append(o[2]); prim.append(o[3])
    depth, om, ok, zwin, prim = (np.stack(a) for a in (depth, om, ok, zwin, prim))
    # the wall is cut by the far plane inside the frame, and covers a large part of it
    wall = prim >= 0
    assert wall.mean() > 0.4 and (~wall).sum() > 1000
    assert ((prim == -1).sum() > 1000) == (not background)
    assert (zwin[wall] > np.float32(0.99)).sum() > 1000
    st = run_modes(ctx, base, depth, om, ok, zwin, prim, "far-plane covers, background=%s" % background, bits=background)
    if not background:
        # the bit-packed output cannot say "no fragment": the library refuses it for such a camera
        pin_in = ctx.host_alloc(depth.shape, np.float32)
        pin_bits = ctx.host_alloc((n, ctx.mask_bits_words()), np.uint32)
        pin_in[...] = depth
        with pytest.raises(R.RtufError) as e:
            ctx.filter_batch_bits_async(pin_in, pin_bits)
            ctx.sync()
        assert e.value.code == -6
        ctx.host_free(pin_in)
        ctx.host_free(pin_bits)
    assert st["cover_pass"] and st["cover_tiles"] > 0, st
    ctx.close()


DEGENERATE = ([("near_plane", x) for x in (0.0, -0.1, 8.0, 9.0, 1e-30, float("nan"))]
              + [("depth_distance_threshold", x) for x in (0.0, -0.0, -0.05, float("inf"), float("-inf"), float("nan"), 1e-45)]
              + [("filter_replace_value", x) for x in (float("nan"), -0.0, float("inf"), 1e-45)])


@pytest.mark.parametrize("two_kernel", [False, True])
def test_degenerate_uniforms_between_frames(two_kernel):
    """rtuf_set_params takes any near plane, threshold and replace value, as the reference's shader takes any uniform:
    near 0, behind the camera, at and beyond the far plane, denormal, NaN; thresholds of zero, either sign, infinite, NaN,
    denormal; NaN, -0, infinite and denormal replace values -- each frame the oracle's, NaN for NaN, bit for bit.  The fast
    division is admitted for some of these settings and refused for others."""
    fx = golden_io.Fixture("soup_seed13_160x120")
    ctx = R.Context(fx.width, fx.height, 1, 0, params(fx.replace_value, fx.max_diff, two_kernel=two_kernel))
    m, tfs = fx.load_into(ctx)
    ctx.set_camera(0, fx.projection, fx.offset_inv, fx.cam_tf)
    ctx.set_link_poses(0, m, tfs)
    admitted, counts = set(), set()
    for name, value in DEGENERATE:
        kw = {"near_plane": 0.1, "depth_distance_threshold": fx.max_diff, "filter_replace_value": fx.replace_value}
        kw[name] = value
        p = params(kw["filter_replace_value"], kw["depth_distance_threshold"], two_kernel=two_kernel, near_plane=kw["near_plane"])
        ctx.set_params(p)
        admitted.add(fast_div_admitted(p.near_plane, p.far_plane))
        om, ok = O.filter_frame(fx.depth, fx.projection, fx.draws, fx.offset_inv, fx.cam_tf, z_near=p.near_plane,
                                max_diff=p.depth_distance_threshold, replace_value=p.filter_replace_value)
        counts.add(int((ok > 0).sum()))
        for b in range(2):
            masked, mask = ctx.filter_batch(fx.depth[None])
            assert np.array_equal(mask[0], ok), "%s = %r, batch %d: %d mask pixels differ" % (name, value, b, int((mask[0] != ok).sum()))
            assert bits_equal(masked[0], om), "%s = %r, batch %d: masked depth differs" % (name, value, b)
    assert admitted == {True, False}
    assert 0 in counts and len(counts) >= 4          # the settings are not all alike
    ctx.close()


def u16_geometry(W, H, P):
    fx, cx, cy = 200.0, (W - 1) / 2, (H - 1) / 2
    tris = []
    for x0, x1, y0, y1, d0, d1 in ((10, 120, 20, 230, 0.6, 1.4), (130, 250, 40, 200, 1.5, 6.5)):
        c = []
        for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1)):
            d = d0 + (d1 - d0) * (x - x0) / (x1 - x0)
            c.append([(x - cx) / fx * d, (y - (H - cy)) / fx * d, d])
        tris += [[c[0], c[1], c[3]], [c[1], c[2], c[3]]]
    v = np.asarray(tris, np.float32).reshape(-1, 3)
    return v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("two_kernel", [False, True])
def test_u16_every_value_and_replace_value_edges(two_kernel):
    """16UC1: a 256 x 256 frame holding every uint16 value once, geometry over part of it.  Unfiltered pixels come back
    unchanged; filtered ones hold convertTo(CV_16U, 1000) of the replace value -- at rounding ties (half to even), at and
    beyond the 65535 clamp, at the int range's bound, negative, NaN and infinite."""
    W = H = 256
    P = S.projection(200.0, 200.0, (W - 1) / 2, (H - 1) / 2, W, H)
    v, t = u16_geometry(W, H, P)
    ident = S.gl(np.eye(4))
    draws = [(ident, 0, [0.0, 0.0, 0.0], v, t)]
    mm = np.random.default_rng(17).permutation(65536).astype(np.uint16).reshape(1, H, W)
    d32 = depth_u16_to_f32(mm[0])
    ctx = R.Context(W, H, 1, 0, params(5.0, 0.05, two_kernel=two_kernel))
    m = ctx.add_model()
    ctx.add_draw(m, ctx.add_link(m), v, t)
    ctx.finalize_models()
    ctx.set_camera(0, P, None, None)
    ctx.set_link_poses(0, m, ident[None])
    seen = set()
    for rep in (5.0, 0.0005, 0.0015, 0.0025, 65.5355, 65.5365, 2147483.648, 2147483.5, -1.0, float("nan"), float("inf"), float("-inf")):
        ctx.set_params(params(rep, 0.05, two_kernel=two_kernel))
        out16, mask = ctx.filter_batch_u16(mm)
        om, ok = O.filter_frame(d32, P, draws, replace_value=rep)
        assert np.array_equal(mask[0], ok), rep
        assert 1000 < int((ok > 0).sum()) < W * H - 1000
        want = depth_f32_to_u16(om)
        assert np.array_equal(out16[0], want), "replace %r: %d pixels differ" % (rep, int((out16[0] != want).sum()))
        assert np.array_equal(out16[0][ok == 0], mm[0][ok == 0])          # unfiltered pixels round-trip exactly
        seen.add(int(want[ok > 0][0]))
    # 0.0005 -> 0 and 0.0025 -> 2 (ties to even), 0.0015 -> 2, 65.5355 -> 65535 (65535.5 rounds to even 65536: clamped),
    # beyond the int range / NaN / inf / negative -> 0
    assert {0, 2, 5000, 65535} <= seen
    ctx.close()
