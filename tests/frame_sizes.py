"""The frames, inputs and expectations of the frame-size tests: every batch kind at the smallest, thinnest and widest frames
a context accepts (rtuf_create: 1 x 1 to 2048 x 2048).  tests/test_frame_sizes_cpu.py asserts on the CPU oracle's planes alone
that these inputs discriminate (a case whose expectation is all-kept, all-filtered or nothing-drawn proves nothing);
tests/test_frame_sizes_gpu.py runs them.  Every expectation comes from the oracle's planes of gpu_support.edge_scene(SEED, W, H)
through tests/gpu_support.py, tests/link_padding_scenes.py and bench_support/*_check.py, never from the library."""
import numpy as np

import gpu_support as K
import link_padding_scenes as LP
from bench_support import clearance_check as KC
from bench_support import cloud_check as CC
from bench_support import points_check as PC
from bench_support import scene_check as SC
from bench_support import voxel_check as VC
from bench_support import voxel_free_check as VF
from bench_support.dilation_check import shade
from bench_support.link_thresholds_check import expected_planes as thresh_planes
from bench_support.link_thresholds_check import workload_draws as thr_draws
from realtime_urdf_filter_amd.filter import depth_f32_to_u16, depth_u16_to_f32

F = np.float32
SEED = 1
# (W, H), each for a reason of its own: the minimum; narrower than a quad; one quad in one row; two quads; just under one 64 x 32
# tile; exactly one; one column and one row into the next tiles; the same with W % 4 == 0; one column at the largest height; the
# largest height with W % 4 == 0; the widest frame that is no multiple of 4; the widest frame; the widest single row
FRAMES = ((1, 1), (3, 5), (4, 1), (8, 2), (60, 31), (64, 32), (65, 33), (68, 33), (1, 2048), (36, 2048), (2047, 3), (2048, 3), (2048, 1))
SMALL_FRAMES = FRAMES[:4]                          # the per-link thresholds change nothing there
MAX_DILATION_FRAMES = FRAMES[:8] + ((2048, 3),)
VOXEL_FRAMES = ((3, 5), (8, 2), (1, 2048), (2047, 3), (2048, 1))

LINK_LABEL = (3, 7, 7, 1, 12, 5)                   # of the scene's six links: two share a label, the order is not the links'
N_LABELS = 13
LINK_THR = (0.30, -0.02, 0.05, 0.60, 0.0, 0.12)    # per link; the global threshold is 0.05
EMPTY = 0.25
MAX_DISTANCE = 1.5
MAX_DILATION = 16                                  # kMaxDilation
PADS = (0.02, 0.05, 0.0, 0.03, 0.08, 0.01)         # link_padding_scenes' paddings of the soup
PAD_FOCAL = 200.0                                  # the padded contexts' focal length is at least this: 0.08 m reach the clamp within 1 m
MARGINS = np.array([(0.02, 0.01), (0.03, 0.0), (0.0, 0.02)], F)       # scene margins {abs_m, rel} of the three streams
# 13 x 9 x 24 voxels of 25 cm around the optical axis, from 0.25 m to 6.25 m: the centres of column 6 have x = 0 and those of
# row 4 y = 0 exactly, so that a frame of one column or one row still sees voxel centres; 2,808 voxels end inside a word
GRID = VC.Grid((-1.625, -1.125, 0.25), 0.25, (13, 9, 24))
VOXEL_TRANSFORMS = (None, VC.rotation_z(0.3, (0.1, 0.0, 0.0)), VC.rotation_z(0.6, (0.0, 0.1, 0.0)))
CARVE_MARGIN, CARVE_RADIUS = 0.05, 1
POINT_RADII = (0, PC.MAX_RADIUS)
MODES = ("plain", "thresh", "dilate2", "dilate16", "pad", "scene")


def frame_id(frame):
    return "%dx%d" % frame


def admits_u16(W):
    """The 16UC1 filter, render and residual forms, the mask bits, the clouds and scene learning need a width that is a
    multiple of 4 (include/rtuf.h); clearance tables, point lists and the voxel calls take any width."""
    return W % 4 == 0


class World:
    """One frame: the scene and every expectation, each computed once."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.sc = sc = K.edge_scene(SEED, W, H)
        self.n = sc.n
        assert sc.n == 3 and len(LINK_LABEL) == len(LINK_THR) == len(PADS) == sc.n_links
        self.intr = [K.edge_intrinsics(sc, i) for i in range(sc.n)]
        f = max(K.edge_focal(W, H), PAD_FOCAL)
        self.pad_intr = [(f + i, f - 0.5 * i, self.intr[i][2], self.intr[i][3]) for i in range(sc.n)]
        # one sphere at the middle of every link's vertices, a second one on link 0: (link, x, y, z, r) in the link's vertex frame
        self.spheres = [(l, *np.asarray(links[0].verts, np.float64).mean(axis=0), 0.08) for l, links in enumerate(sc.wl.models[0])]
        self.spheres.append((0, *(np.asarray(sc.wl.models[0][0][0].verts, np.float64)[0]), 0.03))
        self._memo = {}

    def memo(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    # ---- inputs
    def sensor(self, u16):
        """What a call is given: float32 metres or uint16 millimetres."""
        return self.memo(("sensor", u16), lambda: depth_f32_to_u16(self.sc.depth) if u16 else self.sc.depth)

    def metres(self, u16):
        """The sensor planes as the kernels read them."""
        return self.memo(("metres", u16), lambda: CC.u16_to_metres(self.sensor(True)) if u16 else self.sc.depth)

    def learn_frame(self, u16):
        """The frame the scene is learned from: the sensor planes a quarter nearer in two pixels of three, a quarter further in
        the third, so that the scene filters some of what the robot filter keeps and keeps the rest."""
        def make():
            y, x = np.mgrid[0:self.H, 0:self.W]
            a = np.stack([self.sc.depth[s] * np.where((x + 2 * y + s) % 3 == 0, F(1.25), F(0.75)).astype(F) for s in range(self.n)]).astype(F)
            return depth_f32_to_u16(a) if u16 else a
        return self.memo(("learn_frame", u16), make)

    # ---- the filter's planes
    def _shaded(self, z_of, u16, sensor=None):
        sc, wl = self.sc, self.sc.wl
        out = []
        for s in range(sc.n):
            sen = (depth_u16_to_f32(depth_f32_to_u16(sc.depth[s])) if u16 else sc.depth[s]) if sensor is None else sensor[s]
            m, k = shade(z_of(s), sen, wl.near, wl.far, wl.max_diff, wl.replace_value)
            out.append((depth_f32_to_u16(m) if u16 else m, k))
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def learned(self, u16):
        """The scene planes one learn call on learn_frame leaves in a fresh context (bench_support/scene_check.py)."""
        def make():
            a = self.learn_frame(u16)
            metres = CC.u16_to_metres(a) if u16 else a
            robot = self._shaded(lambda s: K.zprime(self.sc, s, 0), False, metres)[1]
            return SC.learned(np.full(a.shape, np.inf, F), a if not u16 else metres, robot)
        return self.memo(("learned", u16), make)

    def scene_planes(self):
        """The planes the scene contexts filter with: learned from the 16UC1 frame where the width admits learning (the last
        learn call the test makes), else given through rtuf_set_scene_planes."""
        return self.learned(admits_u16(self.W))

    def planes(self, mode, u16):
        """(masked, mask) [n,H,W] of a filter batch in a context of `mode`: float32 metres, or uint16 millimetres."""
        def make():
            sc, wl = self.sc, self.sc.wl
            if mode in ("plain", "dilate2", "dilate16"):
                return K.filter_expected(sc, {"plain": 0, "dilate2": 2, "dilate16": MAX_DILATION}[mode], u16)
            if mode == "thresh":
                thr, nt = thr_draws(wl, LINK_THR)
                out = []
                for s in range(sc.n):
                    sensor = depth_u16_to_f32(depth_f32_to_u16(sc.depth[s])) if u16 else sc.depth[s]
                    m, k = thresh_planes(sc.zwin[s], sc.prim[s], sensor, thr, nt, wl.max_diff, wl.near, wl.far, wl.replace_value)
                    out.append((depth_f32_to_u16(m) if u16 else m, k))
                return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
            if mode == "pad":
                ex = self.padded(u16)
                return ex.masked, ex.mask
            if mode == "scene":
                rm, rk = self.planes("plain", u16)
                return SC.expected(rm, rk, sc.depth, self.scene_planes(), MARGINS, wl.replace_value, u16=u16)
            raise KeyError(mode)
        return self.memo(("planes", mode, u16), make)

    def padded(self, u16):
        return self.memo(("padded", u16), lambda: LP.expected(self.sc, PADS, u16, focals=[max(i[0], i[1]) for i in self.pad_intr]))

    def bits(self, mode, u16):
        return self.memo(("bits", mode, u16), lambda: np.stack([K.pack_bits(m) for m in self.planes(mode, u16)[1]]))

    def labels(self):
        return self.memo("labels", lambda: K.label_planes(self.sc, LINK_LABEL))

    def virtual(self, u16):
        return self.memo(("virtual", u16), lambda: K.virtual_planes(self.sc, EMPTY, u16))

    def residuals(self, thresh, u16):
        return self.memo(("residual", thresh, u16), lambda: K.residual_tables(self.sc, self.sensor(u16), N_LABELS, link_label=LINK_LABEL,
                                                                               link_thr=LINK_THR if thresh else None))

    # ---- clouds and clearance tables
    def cloud(self, mode, u16):
        """(organized [n,H,W,3], [(points, index, count)] per stream) of the mask of `mode`."""
        def make():
            sensor, mask = self.metres(u16), self.planes(mode, u16)[1]
            return (np.stack([CC.organized(sensor[s], mask[s], self.intr[s]) for s in range(self.n)]),
                    [CC.compacted(sensor[s], mask[s], self.intr[s]) for s in range(self.n)])
        return self.memo(("cloud", mode, u16), make)

    def capacity(self, mode, u16):
        """Of the compacted cloud: below the largest stream's count and above the smallest's where two counts differ by two or
        more, and always within 1 .. W * H."""
        counts = [c[2] for c in self.cloud(mode, u16)[1]]
        return int(min(max((min(counts) + max(counts)) // 2, 1), self.W * self.H))

    def clearance(self, mode, u16):
        def make():
            wl = self.sc.wl
            links, xyz, radii = [q[0] for q in self.spheres], [q[1:4] for q in self.spheres], [q[4] for q in self.spheres]
            out = np.zeros((self.n, N_LABELS), KC.DTYPE)
            for s in range(self.n):
                pts, idx, _ = self.cloud(mode, u16)[1][s]
                centres = KC.posed(wl.link_tf[0][s], wl.cam_tf[s], wl.offset_inv[s], links, xyz)
                out[s] = KC.table(pts, idx, centres, radii, [LINK_LABEL[l] for l in links], list(range(len(links))), N_LABELS, MAX_DISTANCE)
            return out
        return self.memo(("clearance", mode, u16), make)

    # ---- point lists
    def point_lists(self):
        """Per stream: the point of every pixel of the sensor plane (pixels without a reading make points that are not judged),
        then points on the first and last pixel of rows and columns, half a pixel either side of the border and one pixel outside
        it, at 1 m and 3 m; stream s's list is 5 s points shorter, so that the lists end at different places."""
        def make():
            W, H = self.W, self.H
            along = lambda n: np.unique(np.linspace(0, n - 1, min(n, 48)).round()).astype(F)
            across = lambda n: np.array([-1.0, -0.51, -0.49, 0.0, n - 1.0, n - 0.51, n - 0.49, float(n)], F)
            out = []
            for s in range(self.n):
                parts = [PC.grid_points(self.sc.depth[s], self.intr[s])]
                for z in (1.0, 3.0):
                    for u, v in ((across(W), along(H)), (along(W), across(H))):
                        uu, vv = np.meshgrid(u, v, indexing="ij")
                        parts.append(CC.points(np.full(uu.size, z, F), self.intr[s], uu.ravel(), vv.ravel()))
                p = np.ascontiguousarray(np.concatenate(parts), F)
                out.append(p[:len(p) - 5 * s])
            return out
        return self.memo("point_lists", make)

    def point_verdicts(self, r):
        """[(verdict, pixel)] per stream at window radius r (bench_support/points_check.py on the oracle's virtual depth)."""
        def make():
            virt = K.virtual_planes(self.sc, empty=np.inf)
            return [PC.verdicts(p, self.intr[s], virt[s], self.sc.wl.max_diff, r) for s, p in enumerate(self.point_lists())]
        return self.memo(("verdicts", r), make)

    # ---- voxels
    def voxel_insert(self, u16):
        """(bits, counts, summary [n,4]) of one insert into the empty grid."""
        return self.memo(("insert", u16), lambda: VC.expected_planes(list(self.metres(u16)), list(self.planes("plain", u16)[1]), self.intr,
                                                                     VOXEL_TRANSFORMS, GRID))

    def voxel_carve(self, u16):
        """(free bits, summary [n,4]) of one carve into the empty free words."""
        return self.memo(("carve", u16), lambda: VF.expected(list(self.metres(u16)), self.intr, list(VOXEL_TRANSFORMS), GRID, CARVE_MARGIN,
                                                             CARVE_RADIUS))


_worlds = {}


def world(frame):
    if frame not in _worlds:
        _worlds[frame] = World(*frame)
    return _worlds[frame]
