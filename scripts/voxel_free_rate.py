"""Cycle times of the voxel free space carve (rtuf_voxel_carve_batch_device) on the c3 workload: 256 VGA streams, device-resident
sensor planes, the grid of scripts/voxel_rate.py -- 200 x 150 x 200 = 6.0 M voxels of 2 cm from (-2.0, -1.5, 0.3), every camera
looking into the same frustum, each rolled and shifted a little by a transform of its own.  Legs, alternating round by round in
one process:
  carve r0 summary / carve r0 : clear + carve at radius_px 0, with the per-stream summary and without (the early-out);
  carve r2 summary / carve r2 : the same at radius_px 2 (25 gathers per voxel and stream);
  insert                      : clear + rtuf_voxel_insert_batch_device with counts, the cycle of scripts/voxel_rate.py;
  torch                       : what a caller does without the call, giving the same free words at radius 0 -- per stream the centres
                                through the stream's inverse, project, gather, compare; OR over the streams; pack.
The margin is 2 cm (more than half the voxel diagonal).  Every leg runs `--rounds` times, each time for at least `--steps`
cycles and about `--window` seconds; spread = (max - min) / mean of a leg's rounds.  The WHOLE free grid of every carve leg's last cycle, its summary rows, and the torch baseline's words are held against
bench_support/voxel_free_check.py for equality (the insert leg must leave the cleared free words zero); a mismatch fails.  No
ratio is asserted: the last lines say plainly whether the carve beats the torch baseline and how it stands beside the insert.

usage: python scripts/voxel_free_rate.py [--streams 256] [--steps 10] [--window 1.0] [--warmup 2] [--rounds 3] [--out profiles/voxel_free_rate_c3.txt]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from bench_support import voxel_check as VC  # noqa: E402
from bench_support import voxel_free_check as VF  # noqa: E402
from bench_support import workloads as WL  # noqa: E402

INTR = (525.0, 525.0, 319.5, 239.5)
GRID = VC.Grid((-2.0, -1.5, 0.3), 0.02, (200, 150, 200))
MARGIN = 0.02
LEGS = ("carve r0 summary", "carve r0", "carve r2 summary", "carve r2", "insert", "torch")
RADIUS = {"carve r0 summary": 0, "carve r0": 0, "carve r2 summary": 2, "carve r2": 2, "torch": 0}


def transforms(n):
    return [VC.rotation_z(0.05 * ((s % 13) - 6), (0.01 * (s % 7), -0.01 * (s % 5), 0.0)) for s in range(n)]


def expectation(depth, matrices, grid, radii, threads):
    """{r: (bits, summary [n,4])} of one carve of every stream into the empty free grid, the projection of a stream shared by
    the radii, the streams spread over `threads` threads."""
    n, H, W = depth.shape
    world = VF.centres(grid)

    def one(s):
        proj = VF.projected(INTR, matrices[s], grid, W, H, world)
        return [VF.state_of(depth[s], proj, MARGIN, r) for r in radii]

    free = {r: np.zeros(grid.n_voxels, bool) for r in radii}
    summary = {r: np.zeros((n, 4), np.uint32) for r in radii}
    with ThreadPoolExecutor(threads) as pool:
        for s, states in enumerate(pool.map(one, range(n))):
            for r, st in zip(radii, states):
                free[r] |= st == VF.FREE
                summary[r][s] = [(st == VF.FREE).sum(), (st == VF.NOT_FREE).sum(), (st == VF.NOT_SEEN).sum(), grid.n_voxels]
    return {r: (VF.pack(free[r], grid), summary[r]) for r in radii}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds a leg's timed window lasts at least")
    ap.add_argument("--dims", type=int, nargs=3, default=list(GRID.dims), help="a smaller grid, for a rehearsal")
    ap.add_argument("--expect-only", action="store_true", help="compute the expectation and stop: needs no GPU")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_free_rate_c3.txt"))
    args = ap.parse_args()
    n, W, H = args.streams, 640, 480
    grid = VC.Grid(GRID.origin, GRID.voxel_size, args.dims)
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# python scripts/voxel_free_rate.py (%d VGA streams of c3, device planes, grid %d x %d x %d voxels of %g m from %s, margin %g m, %d rounds per leg, each at least %d "
        "timed cycles and %g s, %d warm-up); one MI355X" % ((n,) + grid.dims + (grid.voxel_size, grid.origin, MARGIN, args.rounds, args.steps, args.window, args.warmup)))
    wl = WL.pr2_workload(n, W, H, total_triangles=args.triangles)
    depth = wl.depth_batch().astype(np.float32)
    matrices = transforms(n)
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    t0 = time.perf_counter()
    want = expectation(depth, matrices, grid, (0, 2), threads)
    for r in (0, 2):
        s = want[r][1]
        say("# expectation at radius %d (all %d streams, %.1f s for both radii on %d threads): per stream %d .. %d free, %d .. %d not free, %d .. %d not seen; "
            "%d of %d voxels free for some stream" % ((r, n, time.perf_counter() - t0, threads) + tuple(int(f(s[:, k])) for k in range(3) for f in (np.min, np.max))
                                                     + (int(VF.unpack(want[r][0], grid).sum()), grid.n_voxels)))
        assert (s[:, :3] > 0).all()
    assert not np.array_equal(want[0][0], want[2][0])
    if args.expect_only:
        return

    import torch
    import realtime_urdf_filter_amd as R
    dev = torch.device("cuda:0")
    d_depth = torch.from_numpy(depth).to(dev)
    d_summary = torch.zeros((n, 4), dtype=torch.int32, device=dev)

    # the torch baseline's inputs: the centres, the inverses' 12 used entries, the margin, all float32 on the device
    centres = torch.from_numpy(VF.centres(grid)).to(dev)
    cx_, cy_, cz_ = (centres[:, k].contiguous() for k in range(3))
    inv = torch.from_numpy(np.stack([VF.inverse_transform(m) for m in matrices])).to(dev)      # [n,16] column-major
    margin_t = torch.tensor(MARGIN, dtype=torch.float32, device=dev)
    fx, fy, cx, cy = INTR
    weights = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, dtype=torch.int64, device=dev)).view(1, 32)
    planes = d_depth.view(n, W * H)

    def torch_free():
        """-> the free words [n_words] int64 (below 2^32) of one carve at radius 0 into an empty grid."""
        free = torch.zeros(grid.n_words * 32, dtype=torch.bool, device=dev)
        for s in range(n):
            m = inv[s]
            x, y, z = (((m[r] * cx_ + m[4 + r] * cy_) + m[8 + r] * cz_) + m[12 + r] for r in range(3))
            uf = ((x / z) * fx + cx) + 0.5
            vf = ((y / z) * fy + cy) + 0.5
            judged = (z > 0) & (z < float("inf")) & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
            zero = torch.zeros_like(uf)
            pixel = torch.where(judged, vf, zero).long() * W + torch.where(judged, uf, zero).long()
            sv = planes[s][pixel]
            free[:grid.n_voxels] |= judged & (sv > 0) & (sv < float("inf")) & (z < sv - margin_t)
        return (free.view(-1, 32).long() * weights).sum(dim=1)

    p = R.default_params()
    p.filter_replace_value, p.depth_distance_threshold = wl.replace_value, wl.max_diff
    p.raster_lanes = 1
    ctx = R.Context(W, H, n, 0, p)
    ids = wl.load_into(ctx)
    wl.stage(ctx, ids)
    ctx.set_cloud_intrinsics(0, [INTR] * n)
    ctx.set_voxel_transforms(0, np.stack(matrices))
    ctx.set_voxel_grid(grid.origin, grid.voxel_size, grid.dims, True)
    results = []
    for rnd in range(args.rounds):
        for what in LEGS:
            last = {}

            def cycle():
                if what == "torch":
                    last["words"] = torch_free()
                elif what == "insert":
                    ctx.voxel_clear()
                    ctx.voxel_insert_batch_device(n, d_depth.data_ptr(), None)
                else:
                    ctx.voxel_clear()
                    ctx.voxel_carve_batch_device(n, d_depth.data_ptr(), MARGIN, RADIUS[what], d_summary.data_ptr() if what.endswith("summary") else None)

            def finish():
                ctx.sync()
                torch.cuda.synchronize()

            for _ in range(args.warmup):
                cycle()
            finish()
            t = time.perf_counter()
            cycle()
            finish()
            # (a leg's timed window is at least args.steps cycles and at least about args.window seconds)
            steps = max(args.steps, int(args.window / max(time.perf_counter() - t, 1e-4)) + 1)
            t = time.perf_counter()
            for _ in range(steps):
                cycle()
            finish()
            el = time.perf_counter() - t
            if what == "torch":
                bad = int((last["words"].cpu().numpy().astype(np.uint32) != want[0][0]).sum())
            elif what == "insert":
                bad = int(np.count_nonzero(ctx.voxel_free()))
            else:
                bad = int((ctx.voxel_free() != want[RADIUS[what]][0]).sum())
                if what.endswith("summary"):
                    bad += int((d_summary.cpu().numpy().view(np.uint32) != want[RADIUS[what]][1]).sum())
            last.clear()
            row = {"round": rnd, "leg": what, "cycles": steps, "cycle_ms": round(1e3 * el / steps, 3), "frames_per_s": round(n * steps / el, 1),
                   "free_words_checked": grid.n_words, "mismatches": bad}
            results.append(row)
            say(json.dumps(row))
            if bad:
                raise SystemExit("%s: the last cycle differs from the expectation" % what)
    ctx.set_voxel_grid(None, 0.0, None)
    ctx.close()
    say("# cycle times in ms; spread = (max - min) / mean of a leg's rounds:")
    stat = {}
    for what in LEGS:
        ms = [r["cycle_ms"] for r in results if r["leg"] == what]
        stat[what] = (sum(ms) / len(ms), (max(ms) - min(ms)) / (sum(ms) / len(ms)))
        say("#   %-17s rounds %s  mean %.3f  spread %.3f" % (what, " ".join("%.3f" % v for v in ms), stat[what][0], stat[what][1]))
    parts = []
    for what in LEGS[:4]:
        ms, spread = stat[what]
        vs_torch, vs_insert = stat["torch"][0] / ms, ms / stat["insert"][0]
        beats = stat["torch"][0] - ms > (spread + stat["torch"][1]) * stat["torch"][0]
        say("#   %s: %.1f x as fast as the torch baseline%s (%s it by more than the two legs' spreads together, %.3f + %.3f); %.2f of an insert cycle's time; "
            "%.1f G voxel-stream pairs/s" % (what, vs_torch, "" if RADIUS[what] == 0 else " (which is a radius-0 baseline)", "beats" if beats else "DOES NOT beat", spread,
                                            stat["torch"][1], vs_insert, grid.n_voxels * n / (ms * 1e-3) / 1e9))
        parts.append("%s %.3f ms (%.1f x torch, %.2f of insert, spread %.3f)" % (what, ms, vs_torch, vs_insert, spread))
    say("# c3 clear + carve cycles, %d streams into one %d x %d x %d grid of 2 cm voxels: %s; insert cycle %.3f ms (spread %.3f), torch baseline %.3f ms (spread %.3f)"
        % ((n,) + grid.dims + ("; ".join(parts), stat["insert"][0], stat["insert"][1], stat["torch"][0], stat["torch"][1])))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
