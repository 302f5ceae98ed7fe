"""What more than one GPU test module uses: parameters, comparers, the status-word consumer, workload and scene builders,
OracleScene -- the one class that holds a batch of streams with the CPU oracle's planes of it -- and the expectations and
runners of single batch kinds that a second module needs, each through bench_support/*_check.py on a scene's planes.
A feature's test module keeps its own expectation and its cases; no test module imports another."""
import functools

import numpy as np

import golden_io
import scenes as S
import realtime_urdf_filter_amd as R
from bench_support import cloud_check as CC
from bench_support import workloads as WL
from bench_support.dilation_check import drawn_z, shade, window_min
from bench_support.labels_check import expected_labels
from bench_support.labels_check import workload_draws as label_draws
from bench_support.link_thresholds_check import workload_draws as thr_draws
from bench_support.residuals_check import ROW, expected_table, tables_equal, u16_to_metres
from bench_support.virtual_check import bits_equal_f32, expected_virtual, metres_to_u16
from oracle import bindings as O
from realtime_urdf_filter_amd import urdf
from realtime_urdf_filter_amd.filter import CameraInfo, FilterParameters, RealtimeURDFFilter, depth_f32_to_u16, depth_u16_to_f32


# ---- general helpers ------------------------------------------------------------------------------------------------------

def params(replace=5.0, max_diff=0.05, **kw):
    p = R.default_params()
    p.filter_replace_value = replace
    p.depth_distance_threshold = max_diff
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def torch_device():
    import torch
    return torch, torch.device("cuda:0")


# ---- bit packing ----------------------------------------------------------------------------------------------------------

def pack_bits(mask):
    """[H, W] mask -> [H * ceil(W / 32)] uint32 (pixel x = bit x % 32 of word y * ceil(W / 32) + x / 32)."""
    H, W = mask.shape
    words = (W + 31) // 32
    m = np.zeros((H, words * 32), np.uint8)
    m[:, :W] = mask > 0
    return np.packbits(m, axis=1, bitorder="little").view("<u4").reshape(H, words).reshape(-1)


def unpack_bits(bits, W, H):
    """[..., H * ceil(W / 32)] uint32 -> [..., H, W] bool: the inverse of pack_bits, over any leading axes."""
    bits = np.ascontiguousarray(bits, np.uint32)
    b = np.unpackbits(bits.reshape(bits.shape[:-1] + (H, (W + 31) // 32)).view(np.uint8), axis=-1, bitorder="little")
    return b[..., :W].astype(bool)


# ---- comparers ------------------------------------------------------------------------------------------------------------

def _differ(bad, got, want, what, noun):
    at = np.argwhere(bad)[0]
    where = " ".join("%s %d" % (k, i) for k, i in zip(("stream", "y", "x")[3 - len(at):], at)) if len(at) <= 3 else str(at.tolist())
    raise AssertionError("%s: %d %s pixels differ (first: %s: %r instead of %r)" % (what, int(bad.sum()), noun, where, got[tuple(at)], want[tuple(at)]))


def compare_planes(got, want, what, noun="depth", nan_equal=False):
    """Float planes by bit pattern, 16UC1 planes by value.  nan_equal: a NaN matches a NaN of any payload."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %s planes of shape %s, expected %s" % (what, noun, got.shape, want.shape)
    if want.dtype == np.float32:
        got = np.ascontiguousarray(got, np.float32)
        bad = got.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
        if nan_equal:
            bad &= ~(np.isnan(got) & np.isnan(want))
    else:
        bad = got != want
    if bad.any():
        _differ(bad, got, want, what, noun)


def same_planes(got, want, what):
    """Planes of one dtype, bit for bit, except that a NaN matches a NaN of any payload (an empty value may be one)."""
    assert np.asarray(got).dtype == np.asarray(want).dtype, what
    compare_planes(got, want, what, "plane", nan_equal=True)


def compare_labels(got, want, what, noun="label"):
    """Masks and label planes: equality of every pixel."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %s planes of shape %s, expected %s" % (what, noun, got.shape, want.shape)
    bad = got != want
    if bad.any():
        _differ(bad, got, want, what, noun)


# ---- the status word --------------------------------------------------------------------------------------------------------

class DeviceWord:
    """One uint32 of device memory as a __cuda_array_interface__ object (torch.as_tensor wraps it without a copy)."""
    def __init__(self, ptr):
        self.__cuda_array_interface__ = {"data": (int(ptr), False), "shape": (1,), "typestr": "<i4", "version": 2}


class Consumer:
    """A caller's own HIP stream behind the filter: ordered after the batches on the device, never waits for the host."""
    def __init__(self, ctx):
        import torch
        self.torch, self.ctx, self.stream = torch, ctx, torch.cuda.Stream()

    def read(self, masked, mask):
        """Copies (status word, planes) of the batch enqueued last on the consumer's stream; returns host values."""
        torch = self.torch
        word = torch.as_tensor(DeviceWord(self.ctx.batch_status_device()), device=masked.device)
        self.ctx.order_stream_after_batches(self.stream.cuda_stream)
        with torch.cuda.stream(self.stream):
            w, m, k = word.clone(), masked.clone(), mask.clone()
        self.stream.synchronize()                       # the consumer's stream only: nothing is retired
        return int(w.cpu().numpy()[0]) & 0xffffffff, m.cpu().numpy(), k.cpu().numpy(), word


# ---- workloads --------------------------------------------------------------------------------------------------------------

class _Draw:
    def __init__(self, pre_op, op, verts, tris):
        self.pre_op, self.op, self.verts, self.tris = pre_op, op, verts, tris


def workload_of(name, W, H, geo, link_tf, projection, offset_inv=None, cam_tf=None):
    """One model of one (pre_op, op, verts, tris) draw per link; link_tf [n, links, 16]; identity cameras unless given."""
    n = link_tf.shape[0]
    wl = WL.Workload(name, W, H, n)
    wl.models = [[[_Draw(*g)] for g in geo]]
    wl.link_tf = [np.ascontiguousarray(link_tf, np.float64)]
    wl.projection = np.ascontiguousarray(projection, np.float64)
    wl.offset_inv = np.tile(S.gl(np.eye(4)), (n, 1)) if offset_inv is None else np.ascontiguousarray(offset_inv, np.float64)
    wl.cam_tf = np.tile(S.gl(np.eye(4)), (n, 1)) if cam_tf is None else np.ascontiguousarray(cam_tf, np.float64)
    return wl


def centred_projection(W, H, f=None):
    f = f or 262.5 * W / 320.0
    return S.projection(f, f, (W - 1) / 2.0, (H - 1) / 2.0, W, H)


def quad(x0, x1, y0, y1, z):
    v = np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], np.float32)
    return (0, [0.0, 0.0, 0.0], v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32))


# ---- the scene class ----------------------------------------------------------------------------------------------------------

def oracle_frames(frames, depth):
    """([n,H,W] window z, [n,H,W] prim) of (projection, draws, offset_inv, cam_tf, near, far) frames that no Workload describes
    (a golden fixture, a RankShare posed on the device), on all usable host cores."""
    prep = [O.PreparedFrame(depth[s], P, draws, off, cam, z_near=zn, z_far=zf, want_debug=True)
            for s, (P, draws, off, cam, zn, zf) in enumerate(frames)]
    O.run_prepared(prep, O.usable_threads())
    return np.stack([f.zwin for f in prep]), np.stack([f.prim for f in prep])


class OracleScene:
    """A Workload (one model or several) and optionally its [n,H,W] sensor planes, with the CPU oracle's planes of every stream:
    masked, mask, zwin, prim, each [n,H,W], computed once on first access, all streams on all usable host cores.  Without
    sensor planes only zwin and prim can be read (they do not depend on the sensor)."""

    def __init__(self, wl, depth=None, name=None):
        self.wl, self.name = wl, name or wl.name
        self.W, self.H, self.n = wl.width, wl.height, wl.n_streams
        self.n_links = sum(len(links) for links in wl.models)
        self.depth = None if depth is None else np.ascontiguousarray(depth, np.float32)
        self.ids = None                            # the model ids of the context made last
        self._memo = {}                            # expectations of this module's functions
        self._planes = None

    def _plane(self, i):
        if self._planes is None:
            wl = self.wl
            zero = np.zeros((self.H, self.W), np.float32)
            prep = [O.PreparedFrame(zero if self.depth is None else self.depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s],
                                    z_near=wl.near, z_far=wl.far, max_diff=wl.max_diff, replace_value=wl.replace_value, want_debug=True)
                    for s in range(self.n)]
            O.run_prepared(prep, O.usable_threads())
            self._planes = tuple(np.stack([getattr(f, k) for f in prep]) for k in ("masked", "mask", "zwin", "prim"))
        if i < 2 and self.depth is None:
            raise ValueError("%s has no sensor planes: only zwin and prim can be read" % self.name)
        return self._planes[i]

    masked = property(lambda self: self._plane(0))
    mask = property(lambda self: self._plane(1))
    zwin = property(lambda self: self._plane(2))
    prim = property(lambda self: self._plane(3))

    def context(self, max_streams=None, n=None, global_thr=None, **param_overrides):
        """A context of max_streams (default: every stream) with the workload loaded and the first n streams staged."""
        wl = self.wl
        p = params(replace=wl.replace_value, max_diff=wl.max_diff if global_thr is None else global_thr, **param_overrides)
        p.near_plane, p.far_plane = wl.near, wl.far
        ctx = R.Context(self.W, self.H, max_streams or self.n, 0, p)
        self.ids = wl.load_into(ctx)
        wl.stage(ctx, self.ids, n=n or min(self.n, max_streams or self.n))
        return ctx


# ---- the filter's outputs at silhouette radius r (bench_support/dilation_check.py; r = 0 restates the oracle's own): the dilation,
# ---- point cloud, clearance and batch-kind tests expect these

def zprime(sc, s, r):
    return window_min(drawn_z(sc.zwin[s], sc.prim[s]), r)


def filter_expected(sc, r, u16=False):
    """(masked [n,H,W], mask [n,H,W]) at radius r; 16UC1: the sensor goes through convertTo both ways."""
    key = ("filter", r, u16)
    if key not in sc._memo:
        out = []
        for s in range(sc.n):
            sensor = depth_u16_to_f32(depth_f32_to_u16(sc.depth[s])) if u16 else sc.depth[s]
            m, k = shade(zprime(sc, s, r), sensor, sc.wl.near, sc.wl.far, sc.wl.max_diff, sc.wl.replace_value)
            out.append((depth_f32_to_u16(m) if u16 else m, k))
        sc._memo[key] = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]))
    return sc._memo[key]


def undrawn_at(sc, r):
    return any(np.isnan(zprime(sc, s, r)).any() for s in range(sc.n))


def set_radius(ctx, sc, r, **kw):
    p = params(replace=sc.wl.replace_value, max_diff=sc.wl.max_diff, silhouette_dilation_px=r, **kw)
    p.near_plane, p.far_plane = sc.wl.near, sc.wl.far
    ctx.set_params(p)


# ---- scene builders, memoised: a scene that two modules ask for is rendered once per process.  The key is the call as it is
# ---- spelled (positional and keyword arguments apart), and the scenes are shared: nobody writes to a cached scene's wl or depth.

cached = functools.lru_cache(maxsize=None)


@cached
def soup_scene(seed, W, H, n=3):
    rng = np.random.default_rng(seed)
    geo = S.soup_geometry(rng, n_links=6, tris_per_link=40)
    tfs = np.stack([np.stack(S.random_link_poses(rng, len(geo), near=bool(s & 1))) for s in range(n)])
    cams = [S.random_camera(rng, small=True) for _ in range(n)]
    wl = workload_of("soup%d_%dx%d" % (seed, W, H), W, H, geo, tfs, np.tile(centred_projection(W, H), (n, 1)),
                     np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
    return OracleScene(wl, np.stack([S.sensor_depth(W, H, 0.37 * s + 0.1 * seed) for s in range(n)]))


def edge_focal(W, H):
    """soup_scene's focal length where W : H is at least 4 : 3; taken from the height where the frame is narrower than that."""
    return 262.5 * max(W, 4.0 * H / 3.0) / 320.0


@cached
def edge_scene(seed, W, H, n=3):
    """soup_scene for any frame from 1 x 1 to 2048 x 2048: the same geometry, poses, cameras and sensor planes from the same
    draws in the same order, but the focal length follows the larger of W and 4 H / 3 (centred_projection scales it with W
    alone: a 1 x 2048 soup_scene shows nine robot pixels)."""
    rng = np.random.default_rng(seed)
    geo = S.soup_geometry(rng, n_links=6, tris_per_link=40)
    tfs = np.stack([np.stack(S.random_link_poses(rng, len(geo), near=bool(s & 1))) for s in range(n)])
    cams = [S.random_camera(rng, small=True) for _ in range(n)]
    wl = workload_of("edge%d_%dx%d" % (seed, W, H), W, H, geo, tfs, np.tile(centred_projection(W, H, edge_focal(W, H)), (n, 1)),
                     np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
    return OracleScene(wl, np.stack([S.sensor_depth(W, H, 0.37 * s + 0.1 * seed) for s in range(n)]))


def edge_intrinsics(sc, slot):
    """fx, fy, cx, cy of stream slot `slot` of an edge_scene: intrinsics() with the scene's own focal length."""
    f = edge_focal(sc.W, sc.H)
    return (f + slot, f - 0.5 * slot, (sc.W - 1) / 2.0 + 0.25 * slot, (sc.H - 1) / 2.0 - 0.5 * slot)


@cached
def border_scene(W=160, H=120):
    """Four bars, each crossing one image border (frustum half extents at z = 1: 0.61 x 0.46)."""
    geo = [quad(-0.9, -0.5, -0.7, 0.7, 1.0), quad(0.5, 0.9, -0.7, 0.7, 1.1), quad(-0.9, 0.9, -0.7, -0.38, 1.2),
           quad(-0.9, 0.9, 0.38, 0.7, 1.3)]
    wl = workload_of("borders_%dx%d" % (W, H), W, H, geo, np.tile(S.gl(np.eye(4)), (1, len(geo), 1)), centred_projection(W, H)[None])
    return OracleScene(wl, S.sensor_depth(W, H, 0.3)[None] * np.float32(0.6))


@cached
def neighbour_scene(W=160, H=120):
    """Streams 0 and 2 have a bar along their top and bottom edges, stream 1 between them sees nothing: a window that
    crossed into a neighbouring plane would filter stream 1's first or last rows (sensor 2 m everywhere)."""
    geo = [quad(-0.9, 0.9, -0.7, -0.42, 1.0), quad(-0.9, 0.9, 0.42, 0.7, 1.0)]
    away = np.eye(4)
    away[2, 3] = -5.0                          # behind the camera
    tfs = np.stack([np.tile(S.gl(np.eye(4)), (len(geo), 1)), np.tile(S.gl(away), (len(geo), 1)), np.tile(S.gl(np.eye(4)), (len(geo), 1))])
    wl = workload_of("neighbours_%dx%d" % (W, H), W, H, geo, tfs, np.tile(centred_projection(W, H), (3, 1)))
    return OracleScene(wl, np.full((3, H, W), 2.0, np.float32))


@cached
def undrawn_scene(W=160, H=120):
    """A projection the background quad does not cover (clip-space x shifted): the left part of the image stays at the clear
    colour, and geometry on its edge turns some of it into drawn pixels once dilated."""
    P = centred_projection(W, H)
    P[12] = 160.0
    rng = np.random.default_rng(11)
    geo = S.soup_geometry(rng, n_links=4, tris_per_link=30, scale_lo=0.05, scale_hi=0.3)
    tfs = np.stack([np.stack(S.random_link_poses(rng, len(geo)))])
    wl = workload_of("undrawn_%dx%d" % (W, H), W, H, geo, tfs, P[None])
    return OracleScene(wl, S.sensor_depth(W, H, 0.9)[None])


# (the three scenes of the residual tests: no sensor planes, the tests make theirs from the oracle's planes)

@cached
def small_links_scene(W=160, H=96):
    """A grid of 20 x 12 links of about 6 x 6 pixels each in front of the background: every wave's block of 64 x 4 pixels
    holds ten labels or so, and a 64 x 32 tile more labels than the workgroup keeps rows for."""
    geo = []
    for iy in range(12):
        for ix in range(20):
            x0, y0 = -0.58 + 0.058 * ix, -0.35 + 0.058 * iy          # (a pixel is 0.0076 at z = 1)
            geo.append(quad(x0, x0 + 0.046, y0, y0 + 0.046, 1.0 + 0.01 * ((ix + iy) % 5)))
    return OracleScene(workload_of("small_links_%dx%d" % (W, H), W, H, geo, np.tile(S.gl(np.eye(4)), (1, len(geo), 1)), centred_projection(W, H)[None]))


@cached
def wall_scene(W=192, H=128):
    """A wall over the whole image (cover-only tiles) behind two small links."""
    geo = [quad(-3.0, 3.0, -3.0, 3.0, 1.5), quad(-0.1, 0.0, -0.1, 0.0, 1.0), quad(0.2, 0.3, 0.1, 0.2, 1.2)]
    return OracleScene(workload_of("wall_%dx%d" % (W, H), W, H, geo, np.tile(S.gl(np.eye(4)), (2, len(geo), 1)), np.tile(centred_projection(W, H), (2, 1))))


@cached
def near_quad_scene(W=160, H=128):
    """A link three micrometres behind the near plane (its winners need the exact-z pass) beside one at 1.2 m."""
    geo = [quad(-0.5, -0.3, -0.3, 0.3, 1.2), quad(-0.02, 0.02, -0.015, 0.015, 0.100003)]
    return OracleScene(workload_of("near_quad_%dx%d" % (W, H), W, H, geo, np.tile(S.gl(np.eye(4)), (1, len(geo), 1)), centred_projection(W, H)[None]))


@cached
def fixture_scene(name, n):
    """A golden fixture as n streams: one link per draw, stream s looks from 2 cm * s to the side of the fixture's camera."""
    fx = golden_io.Fixture(name)
    geo = [(pre, op, v, t) for _, pre, op, v, t in fx.draws]
    tfs = np.tile(np.stack([np.asarray(d[0], np.float64).reshape(16) for d in fx.draws])[None], (n, 1, 1))
    cams = np.tile(np.asarray(fx.cam_tf, np.float64).reshape(16), (n, 1))
    cams[:, 12] += 0.02 * np.arange(n)
    wl = workload_of(name, fx.width, fx.height, geo, tfs, np.tile(np.asarray(fx.projection, np.float64).reshape(16), (n, 1)),
                     np.tile(np.asarray(fx.offset_inv, np.float64).reshape(16), (n, 1)), cams)
    wl.near, wl.far, wl.max_diff, wl.replace_value = fx.z_near, fx.z_far, fx.max_diff, fx.replace_value
    return OracleScene(wl, np.tile(fx.depth[None], (n, 1, 1)))


def tie_scene(geo_models, W=160, H=128):
    """geo_models: per model a list of links, per link one (pre_op, op, verts, tris) draw; identity poses, one stream, the
    sensor at 3 m.  Identical triangles in several links or models: the earlier draw wins."""
    wl = WL.Workload("ties", W, H, 1)
    wl.models = [[[_Draw(*g)] for g in links] for links in geo_models]
    wl.link_tf = [np.tile(S.gl(np.eye(4)), (1, len(links), 1)) for links in geo_models]
    wl.projection = centred_projection(W, H)[None]
    wl.offset_inv = S.gl(np.eye(4))[None]
    wl.cam_tf = S.gl(np.eye(4))[None]
    return OracleScene(wl, np.full((1, H, W), 3.0, np.float32))


# ---- label and virtual depth planes -----------------------------------------------------------------------------------------

def label_planes(sc, link_label=None):
    """[n,H,W] label of every pixel: draw -> link -> label, 0 where the background quad won or nothing was drawn."""
    lab, nt = label_draws(sc.wl, link_label)
    return np.stack([expected_labels(sc.prim[s], lab, nt) for s in range(sc.n)])


def virtual_planes(sc, empty=0.0, u16=False):
    v = expected_virtual(sc.zwin, sc.prim, sc.wl.near, sc.wl.far, empty)
    return metres_to_u16(v) if u16 else v


# ---- every kind of batch on a scene with label planes (the fill-rule and the clipper tests) ---------------------------------------

def filter_routes(g, ctx, n, what, two_kernel=False, check_labels=None):
    """Every kind of batch of one context on the first n streams of g, each batch twice (the cover pass has made up its mind
    by the second), every output against the oracle's: plain f32 (in a two-kernel context with the z-surface), 16UC1, mask
    bits, labels, render_batch f32 and 16UC1 with labels, link_residuals_batch pixel counts.  g is an OracleScene whose
    sensor is in whole millimetres, with mm ([n,H,W] uint16), labels, n_labels and zsurface set.  In a two-kernel context the
    mask bits are left out (the API refuses them there); a labelled filter batch takes the z-surface + labels route and the
    compare kernel there, render and residual batches run as in any context.  check_labels(label planes, what), if given,
    sees the label planes of every labelled filter batch.  Returns the statistics of the second plain batch."""
    for rep in range(2):
        w = "%s %s batch %d" % (g.name, what, rep)
        masked, mask = ctx.filter_batch(g.depth[:n])
        same_planes(mask, g.mask[:n], w + ": mask")
        assert bits_equal(masked, g.masked[:n]), w + ": masked depth"
        if two_kernel:
            assert bits_equal_f32(ctx.read_zsurface(n), g.zsurface[:n]), w + ": z surface"
    stats = ctx.stats()
    for rep in range(2):
        w = "%s %s batch %d" % (g.name, what, rep)
        masked, mask = ctx.filter_batch_u16(g.mm[:n])
        same_planes(mask, g.mask[:n], w + ": 16UC1 mask")
        same_planes(masked, depth_f32_to_u16(g.masked[:n]), w + ": 16UC1 masked depth")
        if not two_kernel:
            bits = np.zeros((n, ctx.mask_bits_words()), np.uint32)
            ctx.filter_batch_bits_async(g.depth[:n], bits)
            ctx.sync()
            for s in range(n):
                assert np.array_equal(bits[s], pack_bits(g.mask[s])), "%s: mask bits, stream %d" % (w, s)
        masked, mask, lab = ctx.filter_batch_labels(g.depth[:n])
        same_planes(lab, g.labels[:n], w + ": labels")
        same_planes(mask, g.mask[:n], w + ": mask beside the labels")
        assert bits_equal(masked, g.masked[:n]), w + ": masked depth beside the labels"
        if check_labels is not None:
            check_labels(np.asarray(lab), w)
        for u16 in (False, True):
            v, lab = ctx.render_batch(n, -1.5, labels=True, u16=u16)
            same_planes(v, virtual_planes(g, -1.5, u16)[:n], w + ": virtual depth%s" % (" 16UC1" if u16 else ""))
            same_planes(lab, g.labels[:n], w + ": rendered labels")
        table = ctx.link_residuals_batch(g.depth[:n], g.n_labels)
        for s in range(n):
            want = np.bincount(g.labels[s].reshape(-1), minlength=g.n_labels)
            assert np.array_equal(table[s]["pixels"], want), "%s: residual table pixels, stream %d: %s instead of %s" % (w, s, table[s]["pixels"], want)
    return stats


# ---- residual tables ------------------------------------------------------------------------------------------------------------

def residual_tables(sc, sensor, n_labels, link_label=None, link_thr=None, global_thr=None, n=None):
    """[n, n_labels] expected table; sensor float32 metres or uint16 millimetres."""
    s = u16_to_metres(sensor) if sensor.dtype == np.uint16 else sensor
    lab, nt = label_draws(sc.wl, link_label)
    thr = thr_draws(sc.wl, link_thr)[0] if link_thr is not None else None
    g = sc.wl.max_diff if global_thr is None else global_thr
    return np.stack([expected_table(sc.zwin[i], sc.prim[i], s[i], lab, nt, thr, g, sc.wl.near, sc.wl.far, n_labels)
                     for i in range(n or sc.n)])


def check_tables(got, want, what):
    ok, text = tables_equal(got, want)
    assert ok, "%s: %s" % (what, text)


def table_host(table):
    a = table.cpu().numpy()
    return np.ascontiguousarray(a).view(ROW).reshape(a.shape[0], a.shape[1])


# ---- point clouds ---------------------------------------------------------------------------------------------------------------

CLOUD_SENTINEL = 0x5A5A5A5A


def intrinsics(sc, slot):
    """fx, fy, cx, cy of stream slot `slot`: different for every slot."""
    f = 262.5 * sc.W / 320.0
    return (f + slot, f - 0.5 * slot, (sc.W - 1) / 2.0 + 0.25 * slot, (sc.H - 1) / 2.0 - 0.5 * slot)


def sensor_of(sc, u16):
    return CC.u16_to_metres(depth_f32_to_u16(sc.depth)) if u16 else sc.depth


class CloudExpect:
    """Organized planes and compacted lists of streams `streams` of a scene (in slots 0 ..) for a given mask."""

    def __init__(self, sc, mask, u16, streams):
        sensor = sensor_of(sc, u16)
        self.org = np.stack([CC.organized(sensor[s], mask[s], intrinsics(sc, i)) for i, s in enumerate(streams)])
        self.comp = [CC.compacted(sensor[s], mask[s], intrinsics(sc, i)) for i, s in enumerate(streams)]
        self.counts = np.array([c[2] for c in self.comp], np.uint32)
        cls = np.array([CC.classes(sensor[s], mask[s]) for s in streams])
        # (a vacuous pass must not hide: the batch has kept, filtered and invalid pixels)
        assert (cls.sum(axis=0) > 0).all(), cls


def cloud_expect(sc, r=0, u16=False, streams=None):
    """The cloud of the mask the filter is expected to give at silhouette radius r."""
    streams = tuple(range(sc.n)) if streams is None else tuple(streams)
    key = ("cloud", r, u16, streams)
    if key not in sc._memo:
        sc._memo[key] = CloudExpect(sc, filter_expected(sc, r, u16)[1], u16, streams)
    return sc._memo[key]


def cloud_context(sc, n=None, intr=True, **kw):
    ctx = sc.context(**kw)
    if intr:
        ctx.set_cloud_intrinsics(0, [intrinsics(sc, i) for i in range(n or sc.n)])
    return ctx


def check_org(got, ex, what, n=None):
    got = np.ascontiguousarray(got, np.float32)
    want = ex.org[:n or len(ex.org)]
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert got.shape == want.shape and bad == 0, "%s: %d words differ" % (what, bad)


def check_comp(points, index, counts, ex, cap, what, n=None):
    n = n or len(ex.comp)
    assert np.array_equal(np.asarray(counts)[:n], ex.counts[:n]), "%s: counts %s, expected %s" % (what, counts, ex.counts)
    for s in range(n):
        p, i, c = ex.comp[s]
        m = min(c, cap)
        assert np.array_equal(np.ascontiguousarray(points[s][:m]).view(np.uint32), p[:m].view(np.uint32)), "%s stream %d: points" % (what, s)
        if index is not None:
            assert np.array_equal(np.asarray(index[s][:m]).view(np.uint32), i[:m]), "%s stream %d: index" % (what, s)


class CloudBuffers:
    """Device outputs of one cloud batch, filled with a sentinel."""

    def __init__(self, sc, total, capacity=None):
        torch, dev = torch_device()
        self.cap = capacity
        per = (sc.H, sc.W) if capacity is None else (capacity,)
        self.points = torch.full((total,) + per + (3,), CLOUD_SENTINEL, dtype=torch.int32, device=dev)
        self.index = torch.full((total, capacity), CLOUD_SENTINEL, dtype=torch.int32, device=dev) if capacity else None
        self.counts = torch.full((total,), CLOUD_SENTINEL, dtype=torch.int32, device=dev) if capacity else None

    def host(self):
        f = lambda t, d: None if t is None else np.ascontiguousarray(t.cpu().numpy()).view(d)
        return f(self.points, np.float32), f(self.index, np.uint32), f(self.counts, np.uint32)


def upload(sensor):
    torch, dev = torch_device()
    return torch.from_numpy(sensor.view(np.int16) if sensor.dtype == np.uint16 else sensor).to(dev)


def cloud_enqueue(ctx, d, n, buf, u16=False, index=True):
    if buf.cap is None:
        ctx.cloud_batch_device(n, d.data_ptr(), buf.points.data_ptr(), u16=u16)
    else:
        ctx.cloud_compact_batch_device(n, d.data_ptr(), buf.points.data_ptr(), buf.index.data_ptr() if index else None, buf.counts.data_ptr(), buf.cap, u16=u16)


# ---- BASELINE shares --------------------------------------------------------------------------------------------------------------

def share_frames(share, ctx, n):
    """(projection, draws, offset_inv, cam_tf, near, far) of step 0 of a RankShare's first n streams for oracle_frames,
    from the poses the context holds (the share poses its links on the device: one batch must have run)."""
    link_dev, cam_dev = ctx.read_poses(n, share.n_links_total)
    return [share.oracle_frame(0, s, link_dev, cam_dev) + (share.wl0.near, share.wl0.far) for s in range(n)]


# ---- the filter's modes against given oracle planes ---------------------------------------------------------------------------------

def threshold_sensor(zwin, near=0.1, far=8.0, max_diff=0.05, seed=0):
    """Sensor depth ON the shader's threshold of the oracle's winners (urdf_filter.frag:14-23, in float32), one ulp above or
    below in a third of the pixels each; NaN where nothing but the background won."""
    n, f = np.float32(near), np.float32(far)
    num = np.float32(np.float32(n * f) / np.float32(n - f))
    off = np.float32(f / np.float32(f - n))
    with np.errstate(all="ignore"):
        virt = (num / (zwin - off).astype(np.float32)).astype(np.float32)
        thr = (virt - np.float32(max_diff)).astype(np.float32)
    sel = np.random.default_rng(seed).integers(0, 3, thr.shape)
    d = thr.copy()
    d[sel == 1] = np.nextafter(thr[sel == 1], np.float32(np.inf))
    d[sel == 2] = np.nextafter(thr[sel == 2], np.float32(-np.inf))
    return d.astype(np.float32)


def mode_params(base, two_kernel):
    p = R.Params.from_buffer_copy(base)
    p.flags = (base.flags | R.FLAG_TWO_KERNEL) if two_kernel else (base.flags & ~R.FLAG_TWO_KERNEL)
    return p


def run_modes(ctx, base, depth, om, ok, zwin, prim, what, batches=2, bits=True):
    """Fused, two-kernel (with its z-surface) and bit-packed batches, `batches` of each (the cover pass runs from the
    second on; bits=False: no bit-packed batches), with parameters `base`: every output against the oracle's, bit for bit.  The z-surface holds the winner's
    float z, NaN where nothing was drawn (prim -1: no fragment, not even the background quad's)."""
    n = depth.shape[0]
    for two_kernel in (False, True):
        ctx.set_params(mode_params(base, two_kernel))
        for b in range(batches):
            masked, mask = ctx.filter_batch(depth)
            for s in range(n):
                bad = int((ok[s] != mask[s]).sum())
                assert bad == 0, "%s two_kernel=%d batch %d stream %d: %d mask pixels differ" % (what, two_kernel, b, s, bad)
                assert bits_equal(om[s], masked[s]), "%s two_kernel=%d batch %d stream %d: masked depth differs" % (what, two_kernel, b, s)
            if two_kernel:
                z = ctx.read_zsurface(n)
                for s in range(n):
                    want = np.where(prim[s] == -1, np.float32(np.nan), zwin[s]).astype(np.float32)
                    diff = z[s].view(np.uint32) != want.view(np.uint32)
                    diff &= ~(np.isnan(z[s]) & np.isnan(want))
                    assert not diff.any(), "%s batch %d stream %d: z-surface differs from the oracle's z in %d pixels, first %s" % (
                        what, b, s, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    ctx.set_params(mode_params(base, False))
    if not bits:
        return ctx.stats()
    pin_in = ctx.host_alloc(depth.shape, np.float32)
    pin_bits = ctx.host_alloc((n, ctx.mask_bits_words()), np.uint32)
    pin_in[...] = depth
    for b in range(batches):
        pin_bits[...] = 0xdeadbeef
        ctx.filter_batch_bits_async(pin_in, pin_bits)
        ctx.sync()
        for s in range(n):
            m2, k2 = R.expand_mask_bits(depth[s], pin_bits[s], base.filter_replace_value)
            assert np.array_equal(k2, ok[s]), "%s bits batch %d stream %d: %d mask pixels differ" % (what, b, s, int((k2 != ok[s]).sum()))
            assert bits_equal(m2, om[s]), "%s bits batch %d stream %d: masked depth differs" % (what, b, s)
    ctx.host_free(pin_in)
    ctx.host_free(pin_bits)
    return ctx.stats()


# ---- the façades on the example scene -------------------------------------------------------------------------------------------

INTR = (525.0, 520.0, 319.5, 239.5)


def example_transforms():
    """The example URDF's frames under /EXAMPLE, a fixed frame /world and a camera frame /cam that looks along the world's y."""
    tf = urdf.StaticTransformProvider()
    tf.set_frames(urdf.forward_kinematics(urdf.Model.from_string(WL.EXAMPLE_URDF)), "/EXAMPLE/")
    tf.frames["/world"] = urdf.Transform()
    tf.frames["/cam"] = urdf.Transform(np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]]), (0, 0, 0))
    return tf


def example_facade(labels=False, model_entries=None, **kw):
    """(the Python façade on the example URDF, its transform provider); model_entries: further keys of the model's parameter entry."""
    tf = example_transforms()
    model = dict({"model": "d", "tf_prefix": "/EXAMPLE", "geometry_type": "visual"}, **(model_entries or {}))
    prm = FilterParameters("/world", "/cam", [model], 0.05, filter_replace_value=5.0, **kw)
    return RealtimeURDFFilter(prm, tf, {"d": WL.EXAMPLE_URDF}, labels=labels), tf


def sensor_plane():
    d = np.ascontiguousarray(WL.example_workload(640, 480).depth_batch()[0], np.float32).copy()      # (example_scene's sensor plane)
    d[::9, ::4] = np.nan
    d[5::13, 2::7] = 0.0
    d[7::31, 3::11] = np.inf
    return d


def info(width=640, height=480, intr=INTR):
    return CameraInfo(width, height, [intr[0], 0, intr[2], 0, 0, intr[1], intr[3], 0, 0, 0, 1, 0])
