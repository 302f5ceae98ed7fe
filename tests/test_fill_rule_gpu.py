"""GPU (-m gpu): the fill rule on exact ties in every coverage path, on the lattice scenes of tests/lattice_scenes.py.

Every scene's triangles lie on the 1/256 px lattice, edge to edge, one robot link per colour with neighbours in different
colours, so the label plane and the virtual depth plane show which triangle got every pixel.  The expectation is the CPU
oracle's (tests/test_fill_rule_cpu.py shows it equal to the integer rasteriser of tests/fill_rule.py; the prim plane is
checked against that here as well), compared bit for bit on every route that rasterises.  The sensor plane lies half a metre
behind the front layer of the geometry, so the mask is the coverage.

Each scene runs in two draw orders.  Where two triangles claim one pixel at one depth the earlier draw keeps it, so a
triangle that wrongly covers a neighbour's pixel shows only if it is drawn first: in one of the two orders it is.

ctx.stats() pins the path a scene is built for (fragments, records, the cover pass, the exact-z pass), so that a scene cannot
take another route unnoticed.

Run as a script (RTUF_SMALL_LAUNCH=0 python tests/test_fill_rule_gpu.py) every scene goes through the 256-thread tile kernels:
the threshold is read once per process, so test_every_scene_256_thread_kernels starts one."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import lattice_scenes as L
import realtime_urdf_filter_amd as R
from gpu_support import OracleScene, filter_routes, label_planes
from realtime_urdf_filter_amd.filter import depth_f32_to_u16, depth_u16_to_f32

pytestmark = pytest.mark.gpu
REPLACE, MAX_DIFF = 5.0, 0.05


def build(name, reverse):
    """A lattice scene as a batch of identical streams under different sensor planes, with the oracle's planes of each."""
    sc = L.scene(name)
    n = 1 if name.startswith("limit") else 3
    wl, _ = L.workload(name, n, reverse)
    assert (wl.near, wl.far, wl.max_diff, wl.replace_value) == (L.NEAR, L.FAR, MAX_DIFF, REPLACE)
    front = min(sc.zs)
    yy, xx = np.mgrid[0:sc.H, 0:sc.W]
    mm = np.stack([(int(round((front + 0.5) * 1000)) + 7 * s + (xx + yy) % 3).astype(np.uint16) for s in range(n)])
    g = OracleScene(wl, depth_u16_to_f32(mm), name + ("_reversed" if reverse else ""))          # whole millimetres: one oracle run serves f32 and 16UC1
    g.sc, g.mm = sc, mm
    assert np.array_equal(depth_f32_to_u16(g.depth), mm)
    want = L.expected_prim(name, n, reverse)
    for s in range(n):
        assert np.array_equal(g.prim[s], want), "%s: the oracle and the integer rule differ" % g.name
    winner = L.reference(name)[0]
    assert np.array_equal(g.mask[0] > 0, (winner >= 0) & (np.asarray(sc.zs)[np.maximum(winner, 0)] == front))       # the mask is the front layer's coverage
    g.labels = label_planes(g)
    g.n_labels = len(wl.models[0]) + 1
    g.zsurface = np.where(g.prim == -1, np.float32(np.nan), g.zwin).astype(np.float32)
    return g


_scenes = {}


def gscene(name, reverse=False):
    if (name, reverse) not in _scenes:
        _scenes[(name, reverse)] = build(name, reverse)
    return _scenes[(name, reverse)]


def path_checks(name, g, st, n):
    """What ctx.stats() must show after the scene's second plain filter batch of n streams."""
    kind, sc = L.kind_of(name), g.sc
    winner = L.reference(name)[0]
    assert st["batch_status"] == 0, (name, st)
    if kind in ("tiny", "small"):
        frag_pixels = int(np.isin(winner, np.flatnonzero(sc.fragment_sized())).sum())
        assert frag_pixels > 0 and st["fragments_binned"] == n * frag_pixels, (name, frag_pixels, n, st)
        if kind == "small":          # the squares across tile borders are records
            assert st["triangles_binned"] > 0 and st["bin_entries"] > 0, (name, st)
    elif kind == "near":
        assert st["fragments_binned"] == 0 and st["exact_tiles"] > 0, (name, st)
    elif kind == "records":
        assert st["triangles_binned"] > 0 and st["bin_entries"] > 0, (name, st)
    elif kind == "tiles":
        assert st["cover_pass"] == 1, (name, st)
        if L.covered_tiles(name):
            assert st["cover_tiles"] > 0, (name, st)
        if "_cover_" in name:
            assert st["occluded_entries"] > 0, (name, st)


def run_scene(name):
    limit = name.startswith("limit")
    g = gscene(name)
    # a batch of one stream
    ctx = g.context(1, 1)
    st = filter_routes(g, ctx, 1, "one stream")
    path_checks(name, g, st, 1)
    ctx.close()
    # two-kernel mode
    ctx = g.context(g.n, g.n, flags=R.FLAG_TWO_KERNEL)
    st = filter_routes(g, ctx, g.n, "two-kernel", two_kernel=True)
    path_checks(name, g, st, g.n)
    ctx.close()
    if limit:
        return
    # a batch of 3 in a context of 4 with three raster lanes
    ctx = g.context(4, 3, raster_lanes=3)
    st = filter_routes(g, ctx, 3, "3 of 4 streams, 3 lanes")
    path_checks(name, g, st, 3)
    ctx.close()
    # the other draw order
    g = gscene(name, reverse=True)
    ctx = g.context(4, 3, raster_lanes=3)
    filter_routes(g, ctx, 3, "3 of 4 streams, 3 lanes")
    ctx.close()


@pytest.mark.parametrize("name", L.NAMES)
def test_every_route_gives_every_pixel_to_the_triangle_the_rule_names(name):
    run_scene(name)


def test_every_scene_256_thread_kernels():
    """The same checks with RTUF_SMALL_LAUNCH=0: every launch takes the 256-thread tile kernels (the 2048 x 2048 scene does
    anyway)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, timeout=600,
                       env=dict(os.environ, RTUF_SMALL_LAUNCH="0"))
    assert r.returncode == 0 and "scenes ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


if __name__ == "__main__":
    for scene_name in L.NAMES:
        if not scene_name.startswith("limit"):
            run_scene(scene_name)
    print("scenes ok")
