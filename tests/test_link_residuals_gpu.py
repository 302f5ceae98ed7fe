"""GPU (-m gpu): link residual tables (include/rtuf.h, LINK RESIDUAL TABLES; rtuf_link_residuals_batch*).

The expectation is bench_support/residuals_check.py on the CPU oracle's debug planes (zwin, prim), the labels of labels_check
and the thresholds of link_thresholds_check.  Every sum of a table is an integer, so every comparison is equality of the whole
table.  The sensor planes are built from the oracle's planes: per pixel a valid value around the virtual depth, NaN, 0, a
negative value, +inf, or a value at or one ulp either side of lo = v - t and hi = v + t.

Run as a script (RTUF_SMALL_LAUNCH=0 python tests/test_link_residuals_gpu.py) the scene checks go through the 256-thread tile
kernels: the threshold is read once per process, so test_scenes_256_thread_kernels starts one."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import realtime_urdf_filter_amd as R
from bench_support.link_thresholds_check import pixel_thresholds
from bench_support.link_thresholds_check import workload_draws as thr_draws
from bench_support.residuals_check import ROW, tables_equal, virtual_depth
from gpu_support import (Consumer, OracleScene, cached, check_tables, fixture_scene, label_planes, near_quad_scene, params, residual_tables, small_links_scene,
                         soup_scene, table_host, torch_device, undrawn_scene, wall_scene)

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -6
SENTINEL = 0x5a5a5a5a5a5a5a5a
F = np.float32


# ---- scenes and expectations -----------------------------------------------------------------------------------------------

class RScene(OracleScene):
    """A workload without sensor planes (zwin and prim do not depend on them) and the sensors the tests make from the oracle's."""

    @functools.cached_property
    def virt(self):
        return virtual_depth(self.zwin, self.wl.near, self.wl.far)

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


BUILDERS = {"undrawn": undrawn_scene, "small_links": small_links_scene, "wall": wall_scene, "near_quad": near_quad_scene,
            "soup": lambda: soup_scene(31, 160, 120), "soup_164x100": lambda: soup_scene(32, 164, 100),
            "soup_49_streams": lambda: soup_scene(33, 128, 96, n=49)}


@cached
def scene(name):
    return RScene((BUILDERS[name]() if name in BUILDERS else fixture_scene(name, 2)).wl)


def run_device(ctx, sensor, n_labels, n=None, total=None, table=None):
    """One residual batch with device planes; returns (host table [total, n_labels], the device table)."""
    torch, dev = torch_device()
    u16 = sensor.dtype == np.uint16
    d = torch.from_numpy(sensor.view(np.int16) if u16 else sensor).to(dev)
    if table is None:
        table = torch.full((total or sensor.shape[0], n_labels, 8), SENTINEL, dtype=torch.int64, device=dev)
    fn = ctx.link_residuals_batch_device_u16 if u16 else ctx.link_residuals_batch_device
    fn(n or sensor.shape[0], d.data_ptr(), table.data_ptr(), n_labels)
    ctx.sync()
    return table_host(table), table


# ---- scenes: many labels per wave, tile edges, cover-only and exact-z tiles, undrawn pixels -------------------------------------

SCENES = ["soup", "small_links", "wall", "near_quad", "near_range_ties_160x120", "near_large_shapes_517x389", "soup_164x100", "undrawn", "mesh_links_seed21_160x120"]


def scene_checks(name, lanes):
    sc = scene(name)
    ctx = sc.context(raster_lanes=lanes)
    n_labels = sc.n_links + 1
    for rep in range(2):                       # (the second round runs after the cover pass has gone to sleep where no tile has a cover)
        s = sc.sensor(100 + rep)
        want = residual_tables(sc, s, n_labels)
        got, _ = run_device(ctx, s, n_labels)
        check_tables(got, want, "%s lanes %d f32 device round %d" % (name, lanes, rep))
        assert (got["pixels"].sum(axis=1) == sc.W * sc.H).all()
        check_tables(ctx.link_residuals_batch(s, n_labels), want, "%s f32 host" % name)
        if sc.W % 4 == 0:
            mm = sc.sensor_u16(200 + rep)
            want = residual_tables(sc, mm, n_labels)
            got, _ = run_device(ctx, mm, n_labels)
            check_tables(got, want, "%s lanes %d 16UC1 device round %d" % (name, lanes, rep))
            assert (got["pixels"].sum(axis=1) == sc.W * sc.H).all()
            check_tables(ctx.link_residuals_batch(mm, n_labels), want, "%s 16UC1 host" % name)
        assert ctx.stats()["batch_status"] == 0
    st = ctx.stats()
    if name == "near_quad":
        assert st["exact_tiles"] > 0, st
    if name == "wall":
        assert st["cover_tiles"] > 0, st
    if name == "undrawn":
        assert (sc.prim == -1).any() and (sc.prim == -2).any()
    if name == "small_links":                  # (more labels in one 64 x 32 tile than the workgroup keeps rows for)
        assert len(np.unique(label_planes(sc)[0, :32, :64])) > 16
    ctx.close()


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
    want = residual_tables(sc, s, n_labels, link_thr=link_thr)
    got, _ = run_device(ctx, s, n_labels)
    check_tables(got, want, "thresholds f32")
    for link, row in enumerate(got[0][1:]):
        valid = row["pixels"] - row["invalid"]
        if link < 2:                           # NaN, -inf: every valid pixel in front
            assert row["in_front"] == valid and row["agree"] == 0 and row["behind"] == 0 and row["filtered"] == 0
        if link == 2:                          # +inf: every valid pixel agrees
            assert row["agree"] == valid and row["in_front"] == 0 and row["behind"] == 0
    assert got["pixels"][:, 1:].sum() > 500
    mm = sc.sensor_u16(8)
    check_tables(run_device(ctx, mm, n_labels)[0], residual_tables(sc, mm, n_labels, link_thr=link_thr), "thresholds 16UC1")
    check_tables(ctx.link_residuals_batch(s, n_labels), want, "thresholds host")
    ctx.clear_link_thresholds(sc.ids[0])
    check_tables(run_device(ctx, s, n_labels)[0], residual_tables(sc, s, n_labels), "after clear")
    ctx.close()


def test_custom_labels_grouping_zero_and_spare_rows():
    sc = scene("soup")
    ctx = sc.context()
    labels = np.array([3, 3, 0, 7, 1, 7][:sc.n_links], np.uint16)
    ctx.set_link_labels(sc.ids[0], labels)
    s = sc.sensor(9)
    got, _ = run_device(ctx, s, 8)
    check_tables(got, residual_tables(sc, s, 8, link_label=labels), "custom labels")
    assert (got["pixels"][:, [2, 4, 5, 6]] == 0).all() and (got["pixels"][:, [3, 7]] > 0).all()
    got, _ = run_device(ctx, s, 40)            # more rows than labels: the spare rows are all zero
    check_tables(got, residual_tables(sc, s, 40, link_label=labels), "spare rows")
    assert not np.ascontiguousarray(got[:, 8:]).view(np.uint64).any()
    ctx.close()


def test_refusals_write_nothing_and_leave_the_context_usable():
    torch, dev = torch_device()
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
    check_tables(got, residual_tables(sc, s, 3, link_label=np.array([1, 2, 0, 0, 2, 1][:sc.n_links])), "after the refusals")
    ctx.close()


# ---- batch rules -------------------------------------------------------------------------------------------------------------------

def test_three_lanes_several_groups_partial_batch():
    sc = scene("soup_49_streams")
    ctx = sc.context(max_streams=64, n=49, max_inflight_streams=8, raster_lanes=3)
    n_labels = sc.n_links + 3
    s = sc.sensor(11)
    got, _ = run_device(ctx, s, n_labels, n=49, total=64)
    check_tables(got[:49], residual_tables(sc, s, n_labels), "49 of 64 streams")
    assert (np.ascontiguousarray(got[49:]).view(np.uint64) == SENTINEL).all()                    # rows of streams beyond n are not touched
    assert ctx.stats()["groups_last_batch"] > 3
    mm = sc.sensor_u16(12)
    check_tables(run_device(ctx, mm, n_labels, n=49, total=64)[0][:49], residual_tables(sc, mm, n_labels), "49 of 64 streams 16UC1")
    ctx.close()


def test_two_pipelines_batches_in_flight_with_tables_of_their_own():
    torch, dev = torch_device()
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
        check_tables(table_host(table), residual_tables(sc, s, n_labels), "round %d" % i)
    ctx.close()


def test_regrown_bins_rerun_leaves_the_single_run_table():
    sc = scene("mesh_links_seed21_160x120")
    ctx = sc.context(bin_capacity=1)
    n_labels = sc.n_links + 1
    s = sc.sensor(30)
    got, _ = run_device(ctx, s, n_labels)
    st = ctx.stats()
    assert st["regrowths"] > 0 and st["batch_reruns"] > 0 and st["batch_status"] != 0, st
    check_tables(got, residual_tables(sc, s, n_labels), "re-run")
    check_tables(ctx.link_residuals_batch(s, n_labels), residual_tables(sc, s, n_labels), "after the re-run, host planes")
    ctx.close()


def test_regrown_bins_rerun_host_planes():
    sc = scene("mesh_links_seed21_160x120")
    ctx = sc.context(bin_capacity=1)
    n_labels = sc.n_links + 1
    mm = sc.sensor_u16(31)
    got = ctx.link_residuals_batch(mm, n_labels)
    assert ctx.stats()["batch_reruns"] > 0
    check_tables(got, residual_tables(sc, mm, n_labels), "re-run, host planes")
    ctx.close()


def test_a_table_is_overwritten_never_accumulated():
    sc = scene("soup")
    ctx = sc.context()
    n_labels = sc.n_links + 1
    a, b = sc.sensor(40), sc.sensor(41)
    got_a, table = run_device(ctx, a, n_labels)
    check_tables(got_a, residual_tables(sc, a, n_labels), "first")
    got_b, _ = run_device(ctx, b, n_labels, table=table)
    check_tables(got_b, residual_tables(sc, b, n_labels), "second, same table")
    assert not tables_equal(got_a, got_b)[0]
    ctx.close()


def test_graph_replay_of_small_batches():
    """One raster lane, pipelines = 2, one stream: small batches replay a captured graph, the zeroing of the table included."""
    torch, dev = torch_device()
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
        check_tables(table_host(table), residual_tables(sc, s, n_labels, n=1), "replay %d" % i)
    st = ctx.stats()
    assert st["graphs_enabled"] == 1 and st["graph_hits"] > 0, st
    ctx.close()


def test_status_word_is_zero_behind_a_final_residual_batch():
    torch, dev = torch_device()
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
    check_tables(np.ascontiguousarray(early).view(ROW).reshape(sc.n, n_labels), residual_tables(sc, s, n_labels), "behind the batch")
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
    torch, dev = torch_device()
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
    check_tables(got, residual_tables(sc, s, n_labels, link_thr=link_thr), "table")
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
            check_tables(run_device(ctx, s, n_labels)[0], tables[0], "behind a two-kernel filter batch")
        ctx.close()
    check_tables(tables[1], tables[0], "two-kernel context")
    check_tables(tables[0], residual_tables(sc, s, n_labels, link_thr=link_thr), "fused context")


if __name__ == "__main__":
    for name in SCENES:
        scene_checks(name, 1)
    print("scenes ok")
