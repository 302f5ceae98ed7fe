"""GPU (-m gpu, except the scenes' self-check): link clearance tables (include/rtuf.h, LINK CLEARANCE TABLES).

Every table is compared for equality with bench_support/clearance_check.py: brute force over the kept points that
bench_support/cloud_check.py makes from the mask the CPU oracle's planes give (dilation_check / link_thresholds_check where
those features are on) -- never the library's own mask -- and the sphere centres from the matrices the test staged (or, with
on-device forward kinematics, from rtuf_debug_read_poses).  The scene is a small "arm" of six quads with a surface a few
centimetres in front of its first link; each scene's expectation is asserted to hold a finite, an infinite and a negative
clearance, a points_within above 64 and overlapping spheres (row 0 below the sum of the other rows)."""
import numpy as np
import pytest

import realtime_urdf_filter_amd as R
import scenes as S
from bench_support import clearance_check as KC
from bench_support import cloud_check as CC
from bench_support import workloads as WL
from bench_support.link_thresholds_check import expected_planes
from bench_support.link_thresholds_check import workload_draws as thr_draws
from gpu_support import OracleScene, centred_projection, filter_expected, params, quad, torch_device, workload_of
from gpu_support import intrinsics, upload
from oracle import bindings as O
from realtime_urdf_filter_amd.filter import depth_f32_to_u16
from realtime_urdf_filter_amd.geometry import bounding_spheres

gpu = pytest.mark.gpu
INVALID = -1
F = np.float32
LABELS = [1, 2, 2, 0, 3, 7]         # links 1 and 2 share a label, link 3 is ignored, link 5's label is dropped by N_LABELS
N_LABELS = 6                        # rows 0 .. 5: label 4 and 5 have no spheres, label 7 is beyond the table
# (link, x, y, z, r) in the link's vertex frame; ids are list positions
SPHERES = [(0, 0.0, 0.0, 1.2, 0.15), (0, 0.1, 0.0, 1.2, 0.1), (1, -0.45, 0.0, 1.0, 0.05), (2, 0.45, 0.0, 1.0, 0.05), (3, 0.0, 0.0, 1.1, 5.0),
           (4, 0.05, 0.05, 1.2, 0.12), (5, 0.0, 0.0, 1.0, 9.0), (2, 0.45, 0.2, 1.0, 0.0)]


def arm_geometry():
    return [quad(-0.25, 0.25, -0.25, 0.25, 1.2), quad(-0.55, -0.35, -0.3, 0.3, 1.0), quad(0.35, 0.55, -0.3, 0.3, 1.0),
            quad(-0.1, 0.1, 0.3, 0.4, 1.5), quad(-0.2, 0.2, -0.4, -0.3, 1.4), quad(-0.6, -0.5, 0.35, 0.45, 1.6)]


def arm_sensor(W, H, s):
    """2 m everywhere with the usual pixels without a reading, 1.0 m over the side links (on them: filtered) and a patch at
    1.1 m, 10 cm in front of link 0 (kept, and inside its spheres)."""
    d = np.where(np.isfinite(S.sensor_depth(W, H, 0.2 * s)) & (S.sensor_depth(W, H, 0.2 * s) > 0), F(2.0), S.sensor_depth(W, H, 0.2 * s)).astype(F)
    d[d == F(7.9)] = F(2.0)
    f = 262.5 * W / 320.0
    u = lambda x, z: int(round((W - 1) / 2.0 + f * x / z))
    v = lambda y, z: int(round((H - 1) / 2.0 + f * y / z))
    d[v(-0.35, 1.0):v(0.35, 1.0), u(-0.6, 1.0):u(-0.3, 1.0)] = F(1.0)
    d[v(-0.35, 1.0):v(0.35, 1.0), u(0.3, 1.0):u(0.6, 1.0)] = F(1.0)
    d[v(-0.2, 1.1):v(0.2, 1.1), u(-0.2, 1.1):u(0.2, 1.1)] = F(1.1)
    return d


class Arm:
    """The arm scene: n streams, each with a slightly different pose of every link and a camera of its own."""

    def __init__(self, W, H, n, seed=5, models=(6,)):
        rng = np.random.default_rng(seed)
        geo = arm_geometry()
        tfs = np.empty((n, len(geo), 16))
        for s in range(n):
            for l in range(len(geo)):
                T = np.eye(4)
                a = rng.uniform(-0.02, 0.02)
                T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
                T[:3, 3] = rng.uniform(-0.01, 0.01, 3)
                tfs[s, l] = S.gl(T)
        cams = [S.random_camera(rng, small=True) for _ in range(n)]
        off, cam = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
        cam[:, 12:15] *= 0.1                       # (keep the arm in view: the camera moves by centimetres)
        cam[:, [0, 2, 8, 10]] = np.array([1.0, 0.0, 0.0, 1.0])
        wl = workload_of("arm_%dx%d" % (W, H), W, H, geo, tfs, np.tile(centred_projection(W, H), (n, 1)), off, cam)
        if len(models) > 1:                        # the same links split over several models
            links, wl.models, wl.link_tf, b = wl.models[0], [], [], 0
            for m in models:
                wl.models.append(links[b:b + m])
                wl.link_tf.append(np.ascontiguousarray(tfs[:, b:b + m]))
                b += m
        self.wl, self.W, self.H, self.n, self.models = wl, W, H, n, models
        self.depth = np.stack([arm_sensor(W, H, s) for s in range(n)])
        self.link_tf = tfs
        self.scene = OracleScene(wl, self.depth)

    def sensor(self, u16):
        return CC.u16_to_metres(depth_f32_to_u16(self.depth)) if u16 else self.depth

    def mask(self, u16=False, r=0):
        return filter_expected(self.scene, r, u16)[1]

    def context(self, max_streams=None, spheres=SPHERES, labels=LABELS, **kw):
        ctx = self.scene.context(max_streams, **kw)
        ctx.set_cloud_intrinsics(0, [intrinsics(self, i) for i in range(max_streams or self.n)])
        give_spheres(ctx, self, spheres, labels)
        return ctx


def give_spheres(ctx, sc, spheres, labels):
    """Spheres (global link, x, y, z, r) and labels (per global link) go to the models that own the links."""
    base = 0
    for m, nl in enumerate(sc.models):
        if labels is not None:
            ctx.set_link_labels(m, np.array(labels[base:base + nl], np.uint16))
        mine = [(l - base, x, y, z, r) for l, x, y, z, r in spheres if base <= l < base + nl]
        ctx.set_link_spheres(m, [q[0] for q in mine], [q[1:] for q in mine])
        base += nl


def sphere_ids(sc, spheres):
    """Context-global ids: model order, then list order."""
    ids, nxt, base = [0] * len(spheres), 0, 0
    for nl in sc.models:
        for i, q in enumerate(spheres):
            if base <= q[0] < base + nl:
                ids[i] = nxt
                nxt += 1
        base += nl
    return ids


def model_of(sc, link):
    base = 0
    for m, nl in enumerate(sc.models):
        if base <= link < base + nl:
            return m
        base += nl


def expect(sc, mask, max_distance, u16=False, spheres=SPHERES, labels=LABELS, n_labels=N_LABELS, streams=None, stream_models=None, link_tf=None,
           cam_tf=None, check=True):
    """[len(streams), n_labels] expected rows: stream streams[i] of the scene in slot i."""
    streams = list(range(sc.n)) if streams is None else list(streams)
    sensor = sc.sensor(u16)
    ids = sphere_ids(sc, spheres)
    labels = list(range(1, sum(sc.models) + 1)) if labels is None else labels
    out = np.zeros((len(streams), n_labels), KC.DTYPE)
    for i, s in enumerate(streams):
        pts, idx, _ = CC.compacted(sensor[s], mask[s], intrinsics(sc, i))
        seen = [j for j, q in enumerate(spheres) if stream_models is None or model_of(sc, q[0]) in stream_models[i]]
        tf = sc.link_tf[s] if link_tf is None else link_tf[i]
        cam = sc.wl.cam_tf[s] if cam_tf is None else cam_tf[i]
        centres = KC.posed(tf, cam, sc.wl.offset_inv[s], [spheres[j][0] for j in seen], [spheres[j][1:4] for j in seen])
        out[i] = KC.table(pts, idx, centres, [spheres[j][4] for j in seen], [labels[spheres[j][0]] for j in seen], [ids[j] for j in seen], n_labels,
                          max_distance)
    if check:
        conditions(out)
    return out


def conditions(t):
    """What every scene's expectation must show (a vacuous pass must not hide)."""
    c = t["clearance"]
    assert np.isfinite(c).any() and np.isinf(c).any() and (c < 0).any(), c
    assert (t["points_within"] > 64).any()
    assert (t["points_within"][:, 0] < t["points_within"][:, 1:].sum(axis=1)).any(), t["points_within"]


def run_device(ctx, sc, n, max_distance, u16=False, n_labels=N_LABELS, total=None, depth=None, table=None):
    torch, dev = torch_device()
    d = upload(depth_f32_to_u16(sc.depth[:n]) if u16 else sc.depth[:n]) if depth is None else depth
    t = torch.full((total or n, n_labels, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev) if table is None else table
    ctx.link_clearance_batch_device(n, d.data_ptr(), t.data_ptr(), n_labels, max_distance, u16=u16)
    ctx.sync()
    return np.ascontiguousarray(t.cpu().numpy()).view(KC.DTYPE).reshape(t.shape[0], n_labels)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.argwhere(got.view(np.uint32).reshape(got.shape + (4,)) != want.view(np.uint32).reshape(want.shape + (4,)))
    assert len(bad) == 0, "%s: rows differ at %s\ngot  %s\nwant %s" % (what, bad[:4].tolist(), got[tuple(bad[0][:2])], want[tuple(bad[0][:2])])


_arms = {}


def arm(W=160, H=120, n=5, models=(6,)):
    key = (W, H, n, models)
    if key not in _arms:
        _arms[key] = Arm(W, H, n, models=models)
    return _arms[key]


# ---- the scenes themselves (CPU) ---------------------------------------------------------------------------------------------

def test_the_arm_scene_meets_its_conditions_on_the_oracle_alone():
    sc = arm()
    t = expect(sc, sc.mask(), 0.25)
    assert (t["clearance"][:, 1] < 0).all() and (t["points_within"][:, 1] > 64).all()
    assert np.isinf(t["clearance"][:, 4]).all() and np.isinf(t["clearance"][:, 5]).all()      # labels without spheres
    assert (t["sphere"][:, 0] != 4).all() and (t["sphere"][:, 0] != 6).all()                    # label 0 and the dropped label never show
    assert np.isfinite(t["clearance"][:, 2]).any()                                               # the shared label


# ---- sizes, element types, partial batches -------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("lanes", [3, 1])
def test_partial_batch_of_five_in_eight_slots(lanes):
    sc = arm()
    ctx = sc.context(max_streams=8, max_inflight_streams=2, raster_lanes=lanes)
    for u16 in (False, True):
        want = expect(sc, sc.mask(u16), 0.25, u16)
        got = run_device(ctx, sc, 5, 0.25, u16, total=8)
        same(got[:5], want, "device u16=%s lanes=%d" % (u16, lanes))
        assert (got[5:].view(np.uint32) == 0x5A5A5A5A).all()                    # the other streams' rows are left alone
        same(ctx.link_clearance_batch(depth_f32_to_u16(sc.depth) if u16 else sc.depth, N_LABELS, 0.25), want, "host u16=%s" % u16)
    assert ctx.stats()["groups_last_batch"] >= 3
    ctx.close()


@gpu
def test_517x389_f32_and_16uc1():
    sc = arm(517, 389, 1)
    ctx = sc.context()
    for u16 in (False, True):
        same(run_device(ctx, sc, 1, 0.25, u16), expect(sc, sc.mask(u16), 0.25, u16), "517x389 u16=%s" % u16)
    same(ctx.link_clearance_batch(sc.depth, N_LABELS, np.inf), expect(sc, sc.mask(), np.inf), "517x389 host, +inf")
    ctx.close()


# ---- labels, models, many spheres ----------------------------------------------------------------------------------------------

@gpu
def test_default_labels_and_a_smaller_table():
    sc = arm()
    ctx = sc.context(labels=None)
    want = expect(sc, sc.mask(), 0.25, labels=None, n_labels=8)                 # default labels 1 .. 6: the ignored links now count; row 7 is empty
    same(run_device(ctx, sc, 5, 0.25, n_labels=8), want, "default labels")
    assert (want["sphere"][:, 4] == 4).all() and (want["sphere"][:, 6] == 6).all()
    ctx.close()


@gpu
def test_1500_spheres_cross_a_staging_trip():
    sc = arm(n=2)
    rng = np.random.default_rng(9)
    many = list(SPHERES)
    centre = {0: (0, 0, 1.2), 1: (-0.45, 0, 1.0), 2: (0.45, 0, 1.0), 4: (0, -0.35, 1.4)}
    for i in range(1500 - len(SPHERES)):
        l = (0, 1, 2, 4)[i % 4]
        c = np.array(centre[l]) + rng.uniform(-0.2, 0.2, 3) * [1, 1, 0.2]
        many.append((l, float(c[0]), float(c[1]), float(c[2]), float(rng.uniform(0.0, 0.03))))
    ctx = sc.context(spheres=many)
    for dist in (0.05, np.inf):
        same(run_device(ctx, sc, 2, dist), expect(sc, sc.mask(), dist, spheres=many), "1500 spheres, max_distance %s" % dist)
    ctx.close()


@gpu
def test_no_spheres_and_stream_models():
    sc = arm(n=2, models=(3, 3))
    ctx = sc.context(spheres=[])
    empty = run_device(ctx, sc, 2, 0.25)
    assert np.isinf(empty["clearance"]).all() and (empty["pixel"] == KC.NONE).all() and (empty["sphere"] == KC.NONE).all() and (empty["points_within"] == 0).all()
    give_spheres(ctx, sc, SPHERES, LABELS)
    same(run_device(ctx, sc, 2, 0.25), expect(sc, sc.mask(), 0.25), "two models, every stream sees both")
    # stream 1 renders model 0 only: the mask is that of its three links, and the other model's spheres are not there
    ctx.set_stream_models(1, [0])
    wl = sc.wl
    mask = sc.mask().copy()
    draws = [(wl.link_tf[0][1, li], d.pre_op, d.op, d.verts, d.tris) for li, link in enumerate(wl.models[0]) for d in link]
    mask[1] = O.filter_frame(sc.depth[1], wl.projection[1], draws, wl.offset_inv[1], wl.cam_tf[1], z_near=wl.near, z_far=wl.far, max_diff=wl.max_diff,
                             replace_value=wl.replace_value)[1]
    want = expect(sc, mask, np.inf, stream_models=[(0, 1), (0,)])
    assert np.isinf(want["clearance"][1, 3]) and np.isfinite(want["clearance"][0, 3])      # label 3 lives in model 1
    same(run_device(ctx, sc, 2, np.inf), want, "stream 1 restricted to model 0")
    ctx.close()


# ---- other filter features -------------------------------------------------------------------------------------------------------

@gpu
def test_dilation_and_link_thresholds_change_the_kept_set():
    sc = arm(n=2)
    plain = expect(sc, sc.mask(), 0.25)
    ctx = sc.context(silhouette_dilation_px=3)
    want = expect(sc, sc.mask(r=3), 0.25)
    assert (want["points_within"] != plain["points_within"]).any()
    same(run_device(ctx, sc, 2, 0.25), want, "dilation 3")
    same(run_device(ctx, sc, 2, 0.25, True), expect(sc, sc.mask(True, 3), 0.25, True), "dilation 3, 16UC1")
    ctx.close()
    # link 0 with a margin of 0.3 m filters the surface in front of it; link 1 with none keeps the pixels on it
    link_thr = np.array([0.3, np.nan, 0.05, 0.05, 0.05, 0.05], F)
    wl = sc.wl
    thr, nt = thr_draws(wl, link_thr)
    planes = []
    for s in range(sc.n):
        _, _, zwin, prim, _ = O.filter_frame(sc.depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], z_near=wl.near,
                                             z_far=wl.far, max_diff=wl.max_diff, replace_value=wl.replace_value, want_debug=True)
        planes.append(expected_planes(zwin, prim, sc.depth[s], thr, nt, wl.max_diff, wl.near, wl.far, wl.replace_value)[1])
    mask = np.stack(planes)
    want = expect(sc, mask, 0.25)
    assert (want["points_within"] != plain["points_within"]).any() and (want["clearance"][:, 2] < 0).any()
    ctx = sc.context()
    ctx.set_link_thresholds(0, link_thr)
    same(run_device(ctx, sc, 2, 0.25), want, "per-link thresholds")
    ctx.clear_link_thresholds(0)
    same(run_device(ctx, sc, 2, 0.25), plain, "thresholds cleared")
    ctx.close()


@gpu
def test_on_device_forward_kinematics_poses():
    """The PR2-like robot posed from joint positions on the device; bounding spheres of every draw; the sensor shows a surface
    10 cm in front of the robot where it is drawn.  Centres from rtuf_debug_read_poses."""
    n, W, H = 2, 160, 120
    wl = WL.pr2_workload(n, W, H, total_triangles=3000)
    links = wl.models[0]
    spheres = []
    for li, draws in enumerate(links):
        for d in draws:
            # (the spheres live in the link's frame: the draw's glScalef / glTranslatef applied to its vertices)
            v = np.asarray(d.verts, np.float64) * np.asarray(d.op) if d.pre_op == R.OP_SCALE else np.asarray(d.verts, np.float64) + (np.asarray(d.op) if d.pre_op == R.OP_TRANSLATE else 0.0)
            spheres += [(li, float(q[0]), float(q[1]), float(q[2]), float(q[3])) for q in bounding_spheres(v, 2)]
    spheres = spheres[:400]
    assert len(spheres) >= 20
    p = params(replace=wl.replace_value, max_diff=wl.max_diff)
    ctx = R.Context(W, H, n, 0, p)
    ids = wl.load_into(ctx)
    wl.load_kinematics(ctx, ids)
    wl.stage_joint_positions(ctx, ids)
    virt, _ = ctx.render_batch(n, empty_value=3.0)
    depth = np.where(virt < 3.0, virt - F(0.1), F(3.0)).astype(F)
    depth[:, ::7, ::5] = np.nan

    class Sc:
        pass
    sc = Sc()
    sc.W, sc.H, sc.n, sc.models, sc.wl, sc.depth = W, H, n, tuple(len(m) for m in wl.models), wl, depth
    sc.sensor = lambda u16: depth
    ctx.set_cloud_intrinsics(0, [intrinsics(sc, i) for i in range(n)])
    mine = [(q[0],) + q[1:] for q in spheres]
    ctx.set_link_spheres(0, [q[0] for q in mine], [q[1:] for q in mine])
    n_labels = len(links) + 1 + sum(len(m) for m in wl.models[1:])
    got = run_device(ctx, sc, n, 0.3, n_labels=n_labels, depth=upload(depth))
    tf, cam = ctx.read_poses(n, sum(sc.models))
    mask = np.stack([O.filter_frame(depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], z_near=wl.near, z_far=wl.far,
                                    max_diff=wl.max_diff, replace_value=wl.replace_value)[1] for s in range(n)])
    want = expect(sc, mask, 0.3, spheres=spheres, labels=None, n_labels=n_labels, link_tf=tf, cam_tf=cam)
    same(got, want, "on-device FK")
    ctx.close()


# ---- max_distance ------------------------------------------------------------------------------------------------------------------

@gpu
def test_max_distance_small_infinite_and_exactly_at_a_pair():
    sc = arm(n=2)
    ctx = sc.context()
    far = expect(sc, sc.mask(), np.inf)
    same(run_device(ctx, sc, 2, np.inf), far, "+inf")
    same(run_device(ctx, sc, 2, 0.02), expect(sc, sc.mask(), 0.02), "0.02 m")
    c = far["clearance"][0, 2]                     # the nearest pair of label 2 in stream 0: a real pair's clearance, positive
    assert np.isfinite(c) and c > 0
    at, above = expect(sc, sc.mask(), c), expect(sc, sc.mask(), np.nextafter(c, F(np.inf)))
    assert np.isinf(at["clearance"][0, 2]) and above["clearance"][0, 2] == c and above["points_within"][0, 2] >= 1
    same(run_device(ctx, sc, 2, c), at, "max_distance at a pair's clearance")
    same(run_device(ctx, sc, 2, np.nextafter(c, F(np.inf))), above, "one ulp above it")
    ctx.close()


# ---- repeated batches ----------------------------------------------------------------------------------------------------------------

@gpu
def test_graph_replay_rezeroes_the_rows():
    torch, dev = torch_device()
    sc = arm(n=2)
    ctx = sc.context(max_streams=1, raster_lanes=1, pipelines=2)
    d = torch.empty((1, sc.H, sc.W), dtype=torch.float32, device=dev)
    t = torch.zeros((1, N_LABELS, 4), dtype=torch.int32, device=dev)
    wants = [expect(sc, sc.mask(), 0.25, streams=(s,)) for s in range(2)]
    assert (wants[0].view(np.uint32) != wants[1].view(np.uint32)).any()
    for i, s in enumerate((0, 1, 0, 0, 1, 0, 1, 1, 0)):
        ctx.set_cameras(0, sc.wl.projection[s:s + 1], sc.wl.offset_inv[s:s + 1], sc.wl.cam_tf[s:s + 1])
        ctx.set_link_poses_batch(0, 0, sc.wl.link_tf[0][s:s + 1])
        d.copy_(torch.from_numpy(sc.depth[s:s + 1]))
        torch.cuda.synchronize()
        same(run_device(ctx, sc, 1, 0.25, depth=d, table=t), wants[s], "batch %d (stream %d)" % (i, s))
    st = ctx.stats()
    assert st["graphs_enabled"] == 1 and st["graph_hits"] >= 1, st
    ctx.close()


@gpu
def test_a_rerun_after_regrown_bins_ends_with_the_same_table():
    sc = arm(n=2)
    ctx = sc.context(bin_capacity=1)
    want = expect(sc, sc.mask(), 0.25)
    got = run_device(ctx, sc, 2, 0.25)
    st = ctx.stats()
    assert st["batch_reruns"] >= 1 and st["batch_status"] != 0, st
    same(got, want, "re-run")
    same(run_device(ctx, sc, 2, 0.25), want, "the batch after it")
    assert ctx.stats()["batch_status"] == 0
    ctx.close()


# ---- invalid input ---------------------------------------------------------------------------------------------------------------------

@gpu
def test_invalid_input_is_refused_and_the_context_stays_usable():
    sc = arm(n=2)
    ctx = sc.context()
    want = expect(sc, sc.mask(), 0.25)

    def refused(call):
        with pytest.raises(R.RtufError) as e:
            call()
        assert e.value.code == INVALID, e.value

    one = [[0.0, 0.0, 1.0, 0.1]]
    refused(lambda: ctx.set_link_spheres(0, [6], one))                          # bad link index
    refused(lambda: ctx.set_link_spheres(0, [-1], one))
    refused(lambda: ctx.set_link_spheres(1, [0], one))                          # bad model
    refused(lambda: ctx.set_link_spheres(0, [0], [[np.nan, 0, 1, 0.1]]))
    refused(lambda: ctx.set_link_spheres(0, [0], [[0, np.inf, 1, 0.1]]))
    refused(lambda: ctx.set_link_spheres(0, [0], [[0, 0, 1, -0.1]]))
    refused(lambda: ctx.set_link_spheres(0, [0], [[0, 0, 1, np.inf]]))
    refused(lambda: ctx.set_link_spheres(0, [0] * 4097, one * 4097))            # 4,097 spheres
    for bad in (np.nan, 0.0, -1.0):
        refused(lambda: ctx.link_clearance_batch(sc.depth, N_LABELS, bad))
    refused(lambda: ctx.link_clearance_batch(sc.depth, 0, 0.25))
    same(run_device(ctx, sc, 2, 0.25), want, "after the refusals: the list is what it was")
    ctx.set_link_spheres(0, [0] * 4096, one * 4096)                             # 4,096 are fine
    ctx.close()
    # 257 distinct labels: a robot of 257 links with default labels and a sphere on each
    wl = workload_of("many_links", 160, 120, [quad(-0.1, 0.1, -0.1, 0.1, 1.0 + 0.001 * i) for i in range(257)], np.tile(S.gl(np.eye(4)), (1, 257, 1)),
                   centred_projection(160, 120)[None])
    ctx = R.Context(160, 120, 1, 0, params())
    wl.load_into(ctx)
    refused(lambda: ctx.set_link_spheres(0, list(range(257)), one * 257))
    ctx.set_link_spheres(0, list(range(256)), one * 256)
    ctx.close()
