"""GPU (-m gpu, except the check of the case list): every kernel route a batch can take (csrc/rtuf_routes.h), once, small.

A route is the variant of the tile kernel a batch runs and what runs behind it.  The cases are the rows of the header's table
with every modifier the API admits for them: full planes (label plane x per-link thresholds x 16UC1), full planes in
two-kernel mode (label plane x 16UC1), mask bits, render (label plane), residual tables, organized clouds and clearance tables
(per-link thresholds where the kind reads them, 16UC1), and the four kinds that honour a silhouette radius with one.  Each case
runs five batches on a context of its own and checks the first and the last.  The scene has triangles over whole tiles (five
cover tiles in stream 1), so on its own it would keep the cover pass on for ever: the three batches in between pose the links
100 m away, outside the frustum, where nothing covers a tile, and the cover pass switches itself off after those three idle
batches.  The first batch so runs the route's kernel with the cover code, the last -- the scene as in the first -- the one
without (stats()["cover_pass"] is asserted 1 and 0).  In this process the 36 tiles of a batch take the 1,024-thread kernels; run as a script
(RTUF_SMALL_LAUNCH=0 python tests/test_kernel_routes_gpu.py) the same cases take the 256-thread ones: the threshold is read
once per process, so test_every_route_256_thread_kernels starts one.

These are the routes as they stood before link padding, scene planes and point lists: the table has since got the Pad stage
behind the tile kernel, the scene stage behind the compare stage and the Points tail, and neither cases() nor the `behind`
set of test_the_cases_are_the_routes_of_the_table knows them.  Those routes are held by tests/test_link_padding_gpu.py (Pad),
tests/test_scene_planes_gpu.py (the scene stage, in every mode) and tests/test_point_lists_gpu.py (Points), each against the
oracle in the same way; tests/test_frame_sizes_gpu.py runs all of them, and the kinds of this module, at the smallest,
thinnest and widest frames a context accepts, where this module has one frame of 160 x 120.

One scene, soup_scene(1, 160, 120), three streams: 2.5 x 3.75 tiles of 64 x 32.  Every expectation comes from the CPU oracle's
planes through tests/gpu_support.py and bench_support/*_check.py, never from the library; every comparison is for equality, of
bit patterns where the output is a float."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import gpu_support as K
import realtime_urdf_filter_amd as R
from bench_support import clearance_check as KC
from bench_support import cloud_check as CC
from bench_support.link_thresholds_check import expected_planes
from bench_support.link_thresholds_check import workload_draws as thr_draws
from realtime_urdf_filter_amd.filter import depth_f32_to_u16, depth_u16_to_f32

gpu = pytest.mark.gpu
LINK_LABEL = (3, 7, 7, 1, 12, 5)             # of the scene's six links: two share a label, the order is not the links'
N_LABELS = 13
LINK_THR = (0.30, -0.02, 0.05, 0.60, 0.0, 0.12)      # per link; the global threshold is 0.05
EMPTY = 0.25
RADIUS = 2
MAX_DISTANCE = 1.5
BATCHES = 5
SENT = {1: 0x5a, 2: 0x5a5a, 4: 0x5a5a5a5a, 8: 0x5a5a5a5a5a5a5a5a}


def cases():
    """(kind, modifiers) of every route: 40."""
    out = []
    for u16 in (False, True):
        for labels in (False, True):
            for thresh in (False, True):
                out.append(("filter", dict(labels=labels, thresh=thresh, u16=u16)))
            out.append(("filter", dict(labels=labels, u16=u16, two_kernel=True)))
            out.append(("render", dict(labels=labels, u16=u16)))
        for thresh in (False, True):
            for kind in ("bits", "residual", "cloud", "clearance"):
                out.append((kind, dict(thresh=thresh, u16=u16)))
        for kind in ("filter", "bits", "cloud", "clearance"):
            out.append((kind, dict(u16=u16, radius=RADIUS)))
    return out


def case_id(case):
    kind, mod = case
    return "-".join([kind] + [k if v is True else "%s%d" % (k, v) for k, v in sorted(mod.items()) if v])


def test_the_cases_are_the_routes_of_the_table():
    """The tile kernel's 22 variants are all met (with the cover code and without: the five batches), and so is every kernel
    behind it with every tail -- of the table as it stood before link padding, scene planes and point lists (the module's
    docstring names the modules that hold the Pad stage, the scene stage and the Points tail)."""
    variants, behind = set(), set()
    for kind, mod in cases():
        labels, thresh, u16 = mod.get("labels", False), mod.get("thresh", False), mod.get("u16", False)
        zsurface = mod.get("two_kernel", False) or mod.get("radius", 0) > 0
        out = "zsurface" if zsurface else {"filter": "planes", "render": "render", "residual": "residual"}.get(kind, "bits")
        variants.add((out, labels, thresh, u16 and not zsurface))
        behind.add(("dilate" if mod.get("radius", 0) else "compare" if zsurface else None, kind if kind in ("cloud", "clearance") else None))
    assert len(cases()) == 40 == len(set(map(case_id, cases())))
    assert len(variants) == 22
    assert behind == {(None, None), ("compare", None), ("dilate", None), (None, "cloud"), (None, "clearance"), ("dilate", "cloud"), ("dilate", "clearance")}


class World:
    """The scene, its spheres and the expectations of every case, each computed once."""

    def __init__(self):
        self.sc = K.soup_scene(1, 160, 120)
        sc = self.sc
        assert sc.n == 3 and len(LINK_LABEL) == len(LINK_THR) == sc.n_links
        self.labels = K.label_planes(sc, LINK_LABEL)
        # one sphere at the middle of every link's vertices, a second one on link 0: (link, x, y, z, r) in the link's vertex frame
        self.spheres = [(l, *np.asarray(links[0].verts, np.float64).mean(axis=0), 0.08) for l, links in enumerate(sc.wl.models[0])]
        self.spheres.append((0, *(np.asarray(sc.wl.models[0][0][0].verts, np.float64)[0]), 0.03))
        self._memo = {}

    def context(self, thresh=False, two_kernel=False, radius=0):
        ctx = K.cloud_context(self.sc, flags=R.FLAG_TWO_KERNEL if two_kernel else 0, silhouette_dilation_px=radius)
        ctx.set_link_labels(0, np.array(LINK_LABEL, np.uint16))
        ctx.set_link_spheres(0, [q[0] for q in self.spheres], [q[1:] for q in self.spheres])
        if thresh:
            ctx.set_link_thresholds(0, np.array(LINK_THR, np.float32))
        return ctx

    def sensor(self, u16):
        return depth_f32_to_u16(self.sc.depth) if u16 else self.sc.depth

    def planes(self, thresh, radius, u16):
        """(masked, mask) of a filter batch: float32 metres, or uint16 millimetres."""
        if not thresh:
            return K.filter_expected(self.sc, radius, u16)
        key = ("thresh", u16)
        if key not in self._memo:
            sc, wl = self.sc, self.sc.wl
            thr, nt = thr_draws(wl, LINK_THR)
            out = []
            for s in range(sc.n):
                sensor = depth_u16_to_f32(depth_f32_to_u16(sc.depth[s])) if u16 else sc.depth[s]
                m, k = expected_planes(sc.zwin[s], sc.prim[s], sensor, thr, nt, wl.max_diff, wl.near, wl.far, wl.replace_value)
                out.append((depth_f32_to_u16(m) if u16 else m, k))
            self._memo[key] = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]))
            plain = K.filter_expected(sc, 0, u16)[1]
            assert ((self._memo[key][1] > 0) != (plain > 0)).sum() > 100      # (the thresholds change the mask: a kernel without them would show)
        return self._memo[key]

    def residuals(self, thresh, u16):
        key = ("residual", thresh, u16)
        if key not in self._memo:
            self._memo[key] = K.residual_tables(self.sc, self.sensor(u16), N_LABELS, link_label=LINK_LABEL, link_thr=LINK_THR if thresh else None)
        return self._memo[key]

    def cloud(self, thresh, radius, u16):
        key = ("cloud", thresh, radius, u16)
        if key not in self._memo:
            self._memo[key] = K.CloudExpect(self.sc, self.planes(thresh, radius, u16)[1], u16, (0, 1, 2))
        return self._memo[key]

    def clearance(self, thresh, radius, u16):
        key = ("clearance", thresh, radius, u16)
        if key not in self._memo:
            sc, wl = self.sc, self.sc.wl
            sensor, mask = K.sensor_of(sc, u16), self.planes(thresh, radius, u16)[1]
            links, xyz, radii = [q[0] for q in self.spheres], [q[1:4] for q in self.spheres], [q[4] for q in self.spheres]
            out = np.zeros((sc.n, N_LABELS), KC.DTYPE)
            for s in range(sc.n):
                pts, idx, _ = CC.compacted(sensor[s], mask[s], K.intrinsics(sc, s))
                centres = KC.posed(wl.link_tf[0][s], wl.cam_tf[s], wl.offset_inv[s], links, xyz)
                out[s] = KC.table(pts, idx, centres, radii, [LINK_LABEL[l] for l in links], list(range(len(links))), N_LABELS, MAX_DISTANCE)
            assert np.isfinite(out["clearance"]).any() and (out["points_within"] > 0).any()      # (not a table of "nothing near")
            self._memo[key] = out
        return self._memo[key]


_world = []


def world():
    if not _world:
        _world.append(World())
    return _world[0]


def run_case(w, kind, labels=False, thresh=False, u16=False, two_kernel=False, radius=0):
    torch, dev = K.torch_device()
    sc = w.sc
    what = case_id((kind, dict(labels=labels, thresh=thresh, u16=u16, two_kernel=two_kernel, radius=radius)))
    shape = (sc.n, sc.H, sc.W)
    plane_t = torch.int16 if u16 else torch.int32
    full = lambda sh, dt: torch.full(sh, SENT[torch.empty((), dtype=dt).element_size()], dtype=dt, device=dev)
    d = K.upload(w.sensor(u16))
    out = {}
    if kind == "filter":
        out["masked"], out["mask"] = full(shape, plane_t), full(shape, torch.uint8)
    elif kind == "bits":
        out["bits"] = full((sc.n, len(K.pack_bits(np.zeros((sc.H, sc.W), np.uint8)))), torch.int32)
    elif kind == "render":
        out["virtual"] = full(shape, plane_t)
    elif kind == "residual":
        out["table"] = full((sc.n, N_LABELS, 8), torch.int64)
    elif kind == "clearance":
        out["clearance"] = full((sc.n, N_LABELS, 4), torch.int32)
    if labels:
        out["labels"] = full(shape, torch.int16)
    cloud = K.CloudBuffers(sc, sc.n) if kind == "cloud" else None
    ptr = {k: t.data_ptr() for k, t in out.items()}

    def enqueue(ctx):
        n = sc.n
        if kind == "filter" and labels:
            ctx.filter_batch_device_labels(n, d.data_ptr(), ptr["masked"], ptr["mask"], ptr["labels"], u16=u16)
        elif kind == "filter":
            (ctx.filter_batch_device_u16 if u16 else ctx.filter_batch_device)(n, d.data_ptr(), ptr["masked"], ptr["mask"])
        elif kind == "bits":
            ctx.filter_batch_device_bits(n, d.data_ptr(), ptr["bits"], u16=u16)
        elif kind == "render":
            (ctx.render_batch_device_u16 if u16 else ctx.render_batch_device)(n, ptr["virtual"], ptr.get("labels"), EMPTY)
        elif kind == "residual":
            (ctx.link_residuals_batch_device_u16 if u16 else ctx.link_residuals_batch_device)(n, d.data_ptr(), ptr["table"], N_LABELS)
        elif kind == "cloud":
            K.cloud_enqueue(ctx, d, n, cloud, u16)
        else:
            ctx.link_clearance_batch_device(n, d.data_ptr(), ptr["clearance"], N_LABELS, MAX_DISTANCE, u16=u16)

    def check(batch):
        at = "%s, batch %d" % (what, batch)
        host = {k: t.cpu().numpy() for k, t in out.items()}
        plane = lambda a: a.view(np.uint16) if u16 else a.view(np.float32)
        if kind == "filter":
            masked, mask = w.planes(thresh, radius, u16)
            K.compare_planes(plane(host["masked"]), masked, at, "masked")
            K.compare_labels(host["mask"], mask, at, "mask")
        elif kind == "bits":
            want = np.stack([K.pack_bits(m) for m in w.planes(thresh, radius, u16)[1]])
            assert np.array_equal(host["bits"].view(np.uint32), want), "%s: mask bits" % at
        elif kind == "render":
            K.same_planes(plane(host["virtual"]), K.virtual_planes(sc, EMPTY, u16), at)
        elif kind == "residual":
            K.check_tables(K.table_host(out["table"]), w.residuals(thresh, u16), at)
        elif kind == "cloud":
            K.check_org(cloud.host()[0], w.cloud(thresh, radius, u16), at)
        else:
            want = w.clearance(thresh, radius, u16)
            got = np.ascontiguousarray(host["clearance"]).view(np.uint32).reshape(sc.n, N_LABELS, 4)
            bad = np.argwhere(got != want.view(np.uint32).reshape(sc.n, N_LABELS, 4))
            assert len(bad) == 0, "%s: clearance rows differ at %s" % (at, bad[:4].tolist())
        if labels:
            K.compare_labels(host["labels"].view(np.uint16), w.labels, at)

    ctx = w.context(thresh, two_kernel, radius)
    away = sc.wl.link_tf[0].copy()
    away[:, :, 14] += 100.0                    # every link 100 m along z: outside the frustum
    for batch in range(BATCHES):
        last = batch == BATCHES - 1
        ctx.set_link_poses_batch(0, sc.ids[0], sc.wl.link_tf[0] if batch == 0 or last else away)
        if last:                               # (what the first batch wrote must not pass for the last one's)
            for t in list(out.values()) + ([cloud.points] if cloud else []):
                t.fill_(SENT[t.element_size()])
        enqueue(ctx)
        ctx.sync()
        torch.cuda.synchronize()
        if batch == 0 or last:
            st = ctx.stats()
            assert st["cover_pass"] == (1 if batch == 0 else 0), "%s, batch %d: cover pass %d, cover tiles %d" % (what, batch, st["cover_pass"], st["cover_tiles"])
            check(batch)
    ctx.close()


@gpu
@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_route(case):
    run_case(world(), case[0], **case[1])


@gpu
def test_every_route_256_thread_kernels():
    """The same cases with RTUF_SMALL_LAUNCH=0: every launch takes the 256-thread tile kernels."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=600,
                       env=dict(os.environ, RTUF_SMALL_LAUNCH="0"))
    assert r.returncode == 0 and "routes ok 40" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


if __name__ == "__main__":
    for route_case in cases():
        run_case(world(), route_case[0], **route_case[1])
    print("routes ok %d" % len(cases()))
