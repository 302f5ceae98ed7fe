"""GPU (-m gpu): link residual tables (include/rtuf.h, LINK RESIDUAL TABLES; rtuf_link_residuals_batch*).

The expectation is bench_support/residuals_check.py on the CPU oracle's debug planes (zwin, prim), the labels of labels_check
and the thresholds of link_thresholds_check.  Every sum of a table is an integer, so every comparison is equality of the whole
table.  The sensor planes are built from the oracle's planes: per pixel a valid value around the virtual depth, NaN, 0, a
negative value, +inf, or a value at or one ulp either side of lo = v - t and hi = v + t.

Run as a script (RTUF_SMALL_LAUNCH=0 python tests/test_link_residuals_gpu.py) the scene checks go through the 256-thread tile
kernels: the threshold is read once per process, so test_scenes_256_thread_kernels starts one."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import golden_io
import realtime_urdf_filter_amd as R
import scenes as S
from bench_support.labels_check import workload_draws as label_draws
from bench_support.link_thresholds_check import pixel_thresholds
from bench_support.link_thresholds_check import workload_draws as thr_draws
from bench_support.residuals_check import ROW, expected_table, tables_equal, u16_to_metres, virtual_depth
from oracle import bindings as O
from test_batch_status_gpu import Consumer, params
from test_silhouette_dilation_gpu import _centred, _quad, _workload, soup_scene, undrawn_scene

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -6
SENTINEL = 0x5a5a5a5a5a5a5a5a
F = np.float32


def _torch():
    import torch
    return torch, torch.device("cuda:0")


# ---- scenes and expectations -----------------------------------------------------------------------------------------------

class RScene:
    """A Workload with the oracle's zwin / prim of every stream (they do not depend on the sensor plane)."""

    def __init__(self, wl):
        self.wl, self.name = wl, wl.name
        self.W, self.H, self.n = wl.width, wl.height, wl.n_streams
        zero = np.zeros((self.H, self.W), np.float32)
        prep = [O.PreparedFrame(zero, wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], z_near=wl.near, z_far=wl.far,
                                max_diff=wl.max_diff, replace_value=wl.replace_value, want_debug=True) for s in range(self.n)]
        O.run_prepared(prep, O.usable_threads())
        self.zwin, self.prim = np.stack([f.zwin for f in prep]), np.stack([f.prim for f in prep])
        self.n_links = sum(len(links) for links in wl.models)
        self.virt = virtual_depth(self.zwin, wl.near, wl.far)

    def thresholds(self, link_thr=None, global_thr=None):
        """[n,H,W] threshold of every pixel."""
        g = self.wl.max_diff if global_thr is None else global_thr
        if link_thr is None:
            return np.full(self.prim.shape, F(g), np.float32)
        thr, nt = thr_draws(self.wl, link_thr)
        return np.stack([pixel_thresholds(self.prim[s], thr, nt, g) for s in range(self.n)])

    def sensor(self, seed, link_thr=None, global_thr=None):
        """[n,H,W] float32: the mix of valid values, invalid ones and the edges of every pixel's [lo, hi]."""
        rng = np.random.default_rng(seed)
        t = self.thresholds(link_thr, global_thr)
        v = self.virt
        with np.errstate(all="ignore"):
            lo, hi = (v - t).astype(np.float32), (v + t).astype(np.float32)
            near = (v + rng.uniform(-0.12, 0.12, v.shape).astype(np.float32)).astype(np.float32)
        inf = F(np.inf)
        choices = [near, near, near, np.full_like(v, np.nan), np.zeros_like(v), np.full_like(v, -1.5), np.full_like(v, inf),
                   lo, np.nextafter(lo, -inf), np.nextafter(lo, inf), hi, np.nextafter(hi, -inf), np.nextafter(hi, inf),
                   rng.uniform(0.2, 7.0, v.shape).astype(np.float32), np.full_like(v, -0.0)]
        pick = rng.integers(0, len(choices), v.shape)
        return np.ascontiguousarray(np.choose(pick, choices).astype(np.float32))

    def sensor_u16(self, seed):
        """[n,H,W] uint16 millimetres around the virtual depth, with 0 and 65535."""
        rng = np.random.default_rng(seed)
        with np.errstate(all="ignore"):
            mm = np.clip(np.nan_to_num(self.virt * F(1000.0), nan=0.0, posinf=65535.0, neginf=0.0) + rng.integers(-120, 121, self.virt.shape), 0, 65535)
        pick = rng.integers(0, 8, mm.shape)
        mm = np.where(pick == 0, 0, np.where(pick == 1, 65535, np.where(pick == 2, rng.integers(1, 9000, mm.shape), mm)))
        return np.ascontiguousarray(mm.astype(np.uint16))

    def want(self, sensor, n_labels, link_label=None, link_thr=None, global_thr=None, n=None):
        """[n, n_labels] expected table; sensor float32 metres or uint16 millimetres."""
        s = u16_to_metres(sensor) if sensor.dtype == np.uint16 else sensor
        lab, nt = label_draws(self.wl, link_label)
        thr = thr_draws(self.wl, link_thr)[0] if link_thr is not None else None
        g = self.wl.max_diff if global_thr is None else global_thr
        return np.stack([expected_table(self.zwin[i], self.prim[i], s[i], lab, nt, thr, g, self.wl.near, self.wl.far, n_labels)
                         for i in range(n or self.n)])

    def context(self, max_streams=None, n=None, **kw):
        p = params(replace=self.wl.replace_value, max_diff=self.wl.max_diff, **kw)
        p.near_plane, p.far_plane = self.wl.near, self.wl.far
        ctx = R.Context(self.W, self.H, max_streams or self.n, 0, p)
        self.ids = self.wl.load_into(ctx)
        self.wl.stage(ctx, self.ids, n=n or min(self.n, max_streams or self.n))
        return ctx


def fixture_scene(name, n=2):
    """A golden fixture as n streams: one link per draw, stream s looks from 2 cm * s to the side of the fixture's camera."""
    fx = golden_io.Fixture(name)
    geo = [(pre, op, v, t) for _, pre, op, v, t in fx.draws]
    tfs = np.tile(np.stack([np.asarray(d[0], np.float64).reshape(16) for d in fx.draws])[None], (n, 1, 1))
    cams = np.tile(np.asarray(fx.cam_tf, np.float64).reshape(16), (n, 1))
    cams[:, 12] += 0.02 * np.arange(n)
    wl = _workload(name, fx.width, fx.height, geo, tfs, np.tile(np.asarray(fx.projection, np.float64).reshape(16), (n, 1)),
                   np.tile(np.asarray(fx.offset_inv, np.float64).reshape(16), (n, 1)), cams)
    wl.near, wl.far, wl.max_diff, wl.replace_value = fx.z_near, fx.z_far, fx.max_diff, fx.replace_value
    return RScene(wl)


def small_links_scene(W=160, H=96):
    """A grid of 20 x 12 links of about 6 x 6 pixels each in front of the background: every wave's block of 64 x 4 pixels
    holds ten labels or so, and a 64 x 32 tile more labels than the workgroup keeps rows for."""
    geo = []
    for iy in range(12):
        for ix in range(20):
            x0, y0 = -0.58 + 0.058 * ix, -0.35 + 0.058 * iy          # (a pixel is 0.0076 at z = 1)
            geo.append(_quad(x0, x0 + 0.046, y0, y0 + 0.046, 1.0 + 0.01 * ((ix + iy) % 5)))
    wl = _workload("small_links_%dx%d" % (W, H), W, H, geo, np.tile(S.gl(np.eye(4)), (1, len(geo), 1)), _centred(W, H)[None])
    return RScene(wl)


def wall_scene(W=192, H=128):
    """A wall over the whole image (cover-only tiles) behind two small links."""
    geo = [_quad(-3.0, 3.0, -3.0, 3.0, 1.5), _quad(-0.1, 0.0, -0.1, 0.0, 1.0), _quad(0.2, 0.3, 0.1, 0.2, 1.2)]
    wl = _workload("wall_%dx%d" % (W, H), W, H, geo, np.tile(S.gl(np.eye(4)), (2, len(geo), 1)), np.tile(_centred(W, H), (2, 1)))
    return RScene(wl)


def near_quad_scene(W=160, H=128):
    """A link three micrometres behind the near plane (its winners need the exact-z pass) beside one at 1.2 m."""
    geo = [_quad(-0.5, -0.3, -0.3, 0.3, 1.2), _quad(-0.02, 0.02, -0.015, 0.015, 0.100003)]
    wl = _workload("near_quad_%dx%d" % (W, H), W, H, geo, np.tile(S.gl(np.eye(4)), (1, len(geo), 1)), _centred(W, H)[None])
    return RScene(wl)


_scenes = {}


def scene(name):
    if name not in _scenes:
        if name == "undrawn":
            _scenes[name] = RScene(undrawn_scene().wl)
        elif name == "small_links":
            _scenes[name] = small_links_scene()
        elif name == "wall":
            _scenes[name] = wall_scene()
        elif name == "near_quad":
            _scenes[name] = near_quad_scene()
        elif name == "soup":
            _scenes[name] = RScene(soup_scene(31, 160, 120).wl)
        elif name == "soup_164x100":
            _scenes[name] = RScene(soup_scene(32, 164, 100).wl)
        elif name == "soup_49_streams":
            _scenes[name] = RScene(soup_scene(33, 128, 96, n=49).wl)
        else:
            _scenes[name] = fixture_scene(name)
    return _scenes[name]


def check(got, want, what):
    ok, text = tables_equal(got, want)
    assert ok, "%s: %s" % (what, text)


def run_device(ctx, sensor, n_labels, n=None, total=None, table=None):
    """One residual batch with device planes; returns (host table [total, n_labels], the device table)."""
    torch, dev = _torch()
    u16 = sensor.dtype == np.uint16
    d = torch.from_numpy(sensor.view(np.int16) if u16 else sensor).to(dev)
    if table is None:
        table = torch.full((total or sensor.shape[0], n_labels, 8), SENTINEL, dtype=torch.int64, device=dev)
    fn = ctx.link_residuals_batch_device_u16 if u16 else ctx.link_residuals_batch_device
    fn(n or sensor.shape[0], d.data_ptr(), table.data_ptr(), n_labels)
    ctx.sync()
    return host(table), table


def host(table):
    a = table.cpu().numpy()
    return np.ascontiguousarray(a).view(ROW).reshape(a.shape[0], a.shape[1])


# ---- scenes: many labels per wave, tile edges, cover-only and exact-z tiles, undrawn pixels -------------------------------------

SCENES = ["soup", "small_links", "wall", "near_quad", "near_range_ties_160x120", "near_large_shapes_517x389", "soup_164x100", "undrawn", "mesh_links_seed21_160x120"]


def scene_checks(name, lanes):
    sc = scene(name)
    ctx = sc.context(raster_lanes=lanes)
    n_labels = sc.n_links + 1
    for rep in range(2):                       # (the second round runs after the cover pass has gone to sleep where no tile has a cover)
        s = sc.sensor(100 + rep)
        want = sc.want(s, n_labels)
        got, _ = run_device(ctx, s, n_labels)
        check(got, want, "%s lanes %d f32 device round %d" % (name, lanes, rep))
        assert (got["pixels"].sum(axis=1) == sc.W * sc.H).all()
        check(ctx.link_residuals_batch(s, n_labels), want, "%s f32 host" % name)
        if sc.W % 4 == 0:
            mm = sc.sensor_u16(200 + rep)
            want = sc.want(mm, n_labels)
            got, _ = run_device(ctx, mm, n_labels)
            check(got, want, "%s lanes %d 16UC1 device round %d" % (name, lanes, rep))
            assert (got["pixels"].sum(axis=1) == sc.W * sc.H).all()
            check(ctx.link_residuals_batch(mm, n_labels), want, "%s 16UC1 host" % name)
        assert ctx.stats()["batch_status"] == 0
    st = ctx.stats()
    if name == "near_quad":
        assert st["exact_tiles"] > 0, st
    if name == "wall":
        assert st["cover_tiles"] > 0, st
    if name == "undrawn":
        assert (sc.prim == -1).any() and (sc.prim == -2).any()
    if name == "small_links":                  # (more labels in one 64 x 32 tile than the workgroup keeps rows for)
        assert len(np.unique(label_plane(sc)[0, :32, :64])) > 16
    ctx.close()


def label_plane(sc, link_label=None):
    from bench_support.labels_check import expected_labels
    lab, nt = label_draws(sc.wl, link_label)
    return np.stack([expected_labels(sc.prim[s], lab, nt) for s in range(sc.n)])


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("name", SCENES)
def test_scenes(name, lanes):
    scene_checks(name, lanes)


def test_scenes_256_thread_kernels():
    """The same checks with RTUF_SMALL_LAUNCH=0: every launch takes the 256-thread tile kernels."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=600,
                       env=dict(os.environ, RTUF_SMALL_LAUNCH="0"))
    assert r.returncode == 0 and "scenes ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- thresholds and labels --------------------------------------------------------------------------------------------------------

def test_per_link_thresholds_special_values_and_clear():
    sc = scene("soup")
    ctx = sc.context()
    n_labels = sc.n_links + 1
    link_thr = np.array([np.nan, -np.inf, np.inf, 0.0, 0.2, 0.01][:sc.n_links], np.float32)
    ctx.set_link_thresholds(sc.ids[0], link_thr)
    s = sc.sensor(7, link_thr)
    want = sc.want(s, n_labels, link_thr=link_thr)
    got, _ = run_device(ctx, s, n_labels)
    check(got, want, "thresholds f32")
    for link, row in enumerate(got[0][1:]):
        valid = row["pixels"] - row["invalid"]
        if link < 2:                           # NaN, -inf: every valid pixel in front
            assert row["in_front"] == valid and row["agree"] == 0 and row["behind"] == 0 and row["filtered"] == 0
        if link == 2:                          # +inf: every valid pixel agrees
            assert row["agree"] == valid and row["in_front"] == 0 and row["behind"] == 0
    assert got["pixels"][:, 1:].sum() > 500
    mm = sc.sensor_u16(8)
    check(run_device(ctx, mm, n_labels)[0], sc.want(mm, n_labels, link_thr=link_thr), "thresholds 16UC1")
    check(ctx.link_residuals_batch(s, n_labels), want, "thresholds host")
    ctx.clear_link_thresholds(sc.ids[0])
    check(run_device(ctx, s, n_labels)[0], sc.want(s, n_labels), "after clear")
    ctx.close()


def test_custom_labels_grouping_zero_and_spare_rows():
    sc = scene("soup")
    ctx = sc.context()
    labels = np.array([3, 3, 0, 7, 1, 7][:sc.n_links], np.uint16)
    ctx.set_link_labels(sc.ids[0], labels)
    s = sc.sensor(9)
    got, _ = run_device(ctx, s, 8)
    check(got, sc.want(s, 8, link_label=labels), "custom labels")
    assert (got["pixels"][:, [2, 4, 5, 6]] == 0).all() and (got["pixels"][:, [3, 7]] > 0).all()
    got, _ = run_device(ctx, s, 40)            # more rows than labels: the spare rows are all zero
    check(got, sc.want(s, 40, link_label=labels), "spare rows")
    assert not np.ascontiguousarray(got[:, 8:]).view(np.uint64).any()
    ctx.close()


def test_refusals_write_nothing_and_leave_the_context_usable():
    torch, dev = _torch()
    sc = scene("soup")
    p = params(replace=sc.wl.replace_value, max_diff=sc.wl.max_diff)
    p.near_plane, p.far_plane = sc.wl.near, sc.wl.far
    ctx = R.Context(sc.W, sc.H, sc.n, 0, p)
    s = sc.sensor(10)
    d = torch.from_numpy(s).to(dev)
    n_labels = sc.n_links + 1
    table = torch.full((sc.n, n_labels, 8), SENTINEL, dtype=torch.int64, device=dev)

    def refused(code, call):
        with pytest.raises(R.RtufError) as e:
            call()
        assert e.value.code == code, e.value
    refused(STATE, lambda: ctx.link_residuals_batch_device(sc.n, d.data_ptr(), table.data_ptr(), n_labels))         # before finalize
    ids = sc.wl.load_into(ctx)
    sc.wl.stage(ctx, ids)
    refused(INVALID, lambda: ctx.link_residuals_batch_device(sc.n, d.data_ptr(), table.data_ptr(), n_labels - 1))    # a link's label >= n_labels
    refused(INVALID, lambda: ctx.link_residuals_batch_device_u16(sc.n, d.data_ptr(), table.data_ptr(), n_labels - 1))
    refused(INVALID, lambda: ctx.link_residuals_batch_device(sc.n, d.data_ptr(), table.data_ptr(), 0))
    refused(INVALID, lambda: ctx.link_residuals_batch_device(sc.n, d.data_ptr(), table.data_ptr(), -3))
    refused(INVALID, lambda: ctx.link_residuals_batch(s, n_labels - 1))
    refused(INVALID, lambda: ctx.link_residuals_batch(s, 0))
    refused(INVALID, lambda: ctx.link_residuals_batch_device(sc.n, None, table.data_ptr(), n_labels))                # NULL plane / table
    refused(INVALID, lambda: ctx.link_residuals_batch_device(sc.n, d.data_ptr(), None, n_labels))
    refused(INVALID, lambda: ctx.link_residuals_batch_device(0, d.data_ptr(), table.data_ptr(), n_labels))           # n out of range
    refused(INVALID, lambda: ctx.link_residuals_batch_device(sc.n + 1, d.data_ptr(), table.data_ptr(), n_labels))
    p.silhouette_dilation_px = 2
    ctx.set_params(p)
    refused(INVALID, lambda: ctx.link_residuals_batch_device(sc.n, d.data_ptr(), table.data_ptr(), n_labels))        # silhouette dilation
    refused(INVALID, lambda: ctx.link_residuals_batch(s, n_labels))
    ctx.sync()
    torch.cuda.synchronize()
    assert (table.cpu().numpy() == SENTINEL).all()
    p.silhouette_dilation_px = 0
    ctx.set_params(p)
    ctx.set_link_labels(ids[0], np.array([1, 2, 0, 0, 2, 1][:sc.n_links], np.uint16))                              # now three rows are enough
    got, _ = run_device(ctx, s, 3)
    check(got, sc.want(s, 3, link_label=np.array([1, 2, 0, 0, 2, 1][:sc.n_links])), "after the refusals")
    ctx.close()


# ---- batch rules -------------------------------------------------------------------------------------------------------------------

def test_three_lanes_several_groups_partial_batch():
    sc = scene("soup_49_streams")
    ctx = sc.context(max_streams=64, n=49, max_inflight_streams=8, raster_lanes=3)
    n_labels = sc.n_links + 3
    s = sc.sensor(11)
    got, _ = run_device(ctx, s, n_labels, n=49, total=64)
    check(got[:49], sc.want(s, n_labels), "49 of 64 streams")
    assert (np.ascontiguousarray(got[49:]).view(np.uint64) == SENTINEL).all()                    # rows of streams beyond n are not touched
    assert ctx.stats()["groups_last_batch"] > 3
    mm = sc.sensor_u16(12)
    check(run_device(ctx, mm, n_labels, n=49, total=64)[0][:49], sc.want(mm, n_labels), "49 of 64 streams 16UC1")
    ctx.close()


def test_two_pipelines_batches_in_flight_with_tables_of_their_own():
    torch, dev = _torch()
    sc = scene("soup")
    ctx = sc.context(pipelines=2)
    n_labels = sc.n_links + 1
    rounds = []
    for i in range(4):
        s = sc.sensor(20 + i)
        d = torch.from_numpy(s).to(dev)
        table = torch.full((sc.n, n_labels, 8), SENTINEL, dtype=torch.int64, device=dev)
        ctx.link_residuals_batch_device(sc.n, d.data_ptr(), table.data_ptr(), n_labels)
        rounds.append((s, d, table))
    ctx.sync()
    for i, (s, _, table) in enumerate(rounds):
        check(host(table), sc.want(s, n_labels), "round %d" % i)
    ctx.close()


def test_regrown_bins_rerun_leaves_the_single_run_table():
    sc = scene("mesh_links_seed21_160x120")
    ctx = sc.context(bin_capacity=1)
    n_labels = sc.n_links + 1
    s = sc.sensor(30)
    got, _ = run_device(ctx, s, n_labels)
    st = ctx.stats()
    assert st["regrowths"] > 0 and st["batch_reruns"] > 0 and st["batch_status"] != 0, st
    check(got, sc.want(s, n_labels), "re-run")
    check(ctx.link_residuals_batch(s, n_labels), sc.want(s, n_labels), "after the re-run, host planes")
    ctx.close()


def test_regrown_bins_rerun_host_planes():
    sc = scene("mesh_links_seed21_160x120")
    ctx = sc.context(bin_capacity=1)
    n_labels = sc.n_links + 1
    mm = sc.sensor_u16(31)
    got = ctx.link_residuals_batch(mm, n_labels)
    assert ctx.stats()["batch_reruns"] > 0
    check(got, sc.want(mm, n_labels), "re-run, host planes")
    ctx.close()


def test_a_table_is_overwritten_never_accumulated():
    sc = scene("soup")
    ctx = sc.context()
    n_labels = sc.n_links + 1
    a, b = sc.sensor(40), sc.sensor(41)
    got_a, table = run_device(ctx, a, n_labels)
    check(got_a, sc.want(a, n_labels), "first")
    got_b, _ = run_device(ctx, b, n_labels, table=table)
    check(got_b, sc.want(b, n_labels), "second, same table")
    assert not tables_equal(got_a, got_b)[0]
    ctx.close()


def test_graph_replay_of_small_batches():
    """One raster lane, pipelines = 2, one stream: small batches replay a captured graph, the zeroing of the table included."""
    torch, dev = _torch()
    sc = scene("soup")
    ctx = sc.context(max_streams=1, n=1, raster_lanes=1, pipelines=2)
    n_labels = sc.n_links + 1
    d = torch.empty((1, sc.H, sc.W), dtype=torch.float32, device=dev)
    ta = torch.full((1, n_labels, 8), SENTINEL, dtype=torch.int64, device=dev)
    tb = torch.full((1, n_labels, 8), SENTINEL, dtype=torch.int64, device=dev)
    for i in range(8):
        s = sc.sensor(50 + i)[:1]
        d.copy_(torch.from_numpy(s))
        torch.cuda.synchronize()
        table = tb if i >= 6 else ta
        ctx.link_residuals_batch_device(1, d.data_ptr(), table.data_ptr(), n_labels)
        ctx.sync()
        check(host(table), sc.want(s, n_labels, n=1), "replay %d" % i)
    st = ctx.stats()
    assert st["graphs_enabled"] == 1 and st["graph_hits"] > 0, st
    ctx.close()


def test_status_word_is_zero_behind_a_final_residual_batch():
    torch, dev = _torch()
    sc = scene("soup")
    ctx = sc.context()
    n_labels = sc.n_links + 1
    s = sc.sensor(60)
    ctx.link_residuals_batch(s, n_labels)      # (bins sized)
    d = torch.from_numpy(s).to(dev)
    table = torch.full((sc.n, n_labels, 8), SENTINEL, dtype=torch.int64, device=dev)
    user = Consumer(ctx)
    ctx.link_residuals_batch_device(sc.n, d.data_ptr(), table.data_ptr(), n_labels)
    word, early, _, _ = user.read(table, table)
    assert word == 0, hex(word)
    check(np.ascontiguousarray(early).view(ROW).reshape(sc.n, n_labels), sc.want(s, n_labels), "behind the batch")
    ctx.sync()
    st = ctx.stats()
    assert st["batch_status"] == 0 and st["batch_reruns"] == 0, st
    ctx.close()


def test_timings_land_in_ms_raster():
    sc = scene("soup")
    ctx = sc.context()
    ctx.enable_timing(1)
    ctx.link_residuals_batch(sc.sensor(61), sc.n_links + 1)
    st = ctx.stats()
    assert st["ms_raster"] > 0 and st["ms_compare"] == 0, st
    ctx.close()


# ---- agreement with the filter on the device, contexts whose filter batches take other routes -----------------------------------

@pytest.mark.parametrize("with_thresholds", [False, True])
def test_pixels_and_filtered_equal_the_bincounts_of_the_label_filter(with_thresholds):
    torch, dev = _torch()
    sc = scene("soup")
    ctx = sc.context()
    n_labels = sc.n_links + 1
    link_thr = np.linspace(-0.1, 0.3, sc.n_links).astype(np.float32) if with_thresholds else None
    if with_thresholds:
        ctx.set_link_thresholds(sc.ids[0], link_thr)
    s = sc.sensor(70, link_thr)
    d = torch.from_numpy(s).to(dev)
    m, k = torch.empty_like(d), torch.empty(d.shape, dtype=torch.uint8, device=dev)
    lab = torch.empty(d.shape, dtype=torch.int16, device=dev)
    ctx.filter_batch_device_labels(sc.n, d.data_ptr(), m.data_ptr(), k.data_ptr(), lab.data_ptr())
    ctx.sync()
    got, table = run_device(ctx, s, n_labels)
    for i in range(sc.n):
        li = lab[i].to(torch.int64).flatten() & 0xffff
        assert torch.equal(torch.bincount(li, minlength=n_labels), table[i, :, 0])
        assert torch.equal(torch.bincount(li[k[i].flatten() == 255], minlength=n_labels), table[i, :, 2])
    check(got, sc.want(s, n_labels, link_thr=link_thr), "table")
    ctx.close()


@pytest.mark.parametrize("with_thresholds", [False, True])
def test_two_kernel_context_is_accepted_and_gives_the_same_table(with_thresholds):
    sc = scene("soup")
    n_labels = sc.n_links + 1
    link_thr = np.array([0.3, np.nan, 0.0, 0.1, -0.2, np.inf][:sc.n_links], np.float32) if with_thresholds else None
    s = sc.sensor(80, link_thr)
    tables = []
    for flags in (0, R.FLAG_TWO_KERNEL):
        ctx = sc.context(flags=flags)
        if with_thresholds:
            ctx.set_link_thresholds(sc.ids[0], link_thr)
        tables.append(run_device(ctx, s, n_labels)[0])
        if flags and not with_thresholds:      # the context filters as before, and the residual batch again behind it
            masked, mask = ctx.filter_batch(s)
            assert mask.any()
            check(run_device(ctx, s, n_labels)[0], tables[0], "behind a two-kernel filter batch")
        ctx.close()
    check(tables[1], tables[0], "two-kernel context")
    check(tables[0], sc.want(s, n_labels, link_thr=link_thr), "fused context")


if __name__ == "__main__":
    for name in SCENES:
        scene_checks(name, 1)
    print("scenes ok")
