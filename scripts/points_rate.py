"""Frames/s of the point list batches (rtuf_points_batch_device) on the c3 workload: 256 VGA streams of the 250 k-triangle
PR2-like robot, 65,536 points per stream -- cloud_point of a seeded sample of the workload's own sensor pixels -- device
resident, radius 0 and 4, one raster lane and the default lanes, against two legs of the same run:
  (a) render alone: rtuf_render_batch_device into a caller's plane, the floor the batch is built on;
  (b) the torch baseline: that render batch followed by torch ops that produce the same verdict bytes (project, round, gather,
      compare, and for radius 4 a min-pool of the plane), ordered behind the batch on the device.

Every leg runs `--rounds` times, the legs alternating (a, points, b, a, ...); a leg is warm-up, then `--steps` timed batches
between two synchronisations (two output sets alternating, as bench.py), and its spread is (max - min) / mean of its rounds.
A pass with rtuf_enable_timing(2) gives the kernels' share: ms_raster is the tile kernel, ms_compare the points kernel (with
the summary's zeroing) of a batch.  The verdicts of EVERY stream of each leg's last batch -- the torch baseline's too -- are
held against bench_support/points_check.py on the CPU oracle's virtual depth planes; a mismatch fails.  The lines go to stdout
and to --out.

usage: python scripts/points_rate.py [--streams 256] [--points 65536] [--steps 100] [--warmup 10] [--rounds 3] [--out profiles/points_rate_c3.txt]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import realtime_urdf_filter_amd as R  # noqa: E402
from bench_support import cloud_check as CC  # noqa: E402
from bench_support import points_check as PC  # noqa: E402
from bench_support import workloads as WL  # noqa: E402
from bench_support.virtual_check import expected_virtual  # noqa: E402
from oracle import bindings as O  # noqa: E402

INTR = (525.0, 525.0, 319.5, 239.5)
LEGS = (("render", 0), ("points", 0), ("torch", 0), ("points", 4), ("torch", 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=250000)
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timed-steps", type=int, default=16, help="batches of the rtuf_enable_timing(2) pass")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_rate_c3.txt"))
    args = ap.parse_args()
    n, W, H, cap = args.streams, 640, 480, args.points
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# python scripts/points_rate.py (%d VGA streams of c3, %d points per stream, device resident, %d rounds of %d timed steps per leg, %d warm-up, "
        "%d with rtuf_enable_timing(2)); one MI355X" % (n, cap, args.rounds, args.steps, args.warmup, args.timed_steps))
    wl = WL.pr2_workload(n, W, H, total_triangles=args.triangles)
    dev = torch.device("cuda:0")
    depth = wl.depth_batch().astype(np.float32)
    rng = np.random.default_rng(65536)
    pick = np.sort(rng.choice(W * H, cap, replace=False))            # the same pixels in every stream, in row-major order
    pts = np.stack([CC.points(depth[s].ravel()[pick], INTR, pick % W, pick // W) for s in range(n)]).astype(np.float32)
    d_points = torch.from_numpy(pts).to(dev)
    d_counts = torch.full((n,), cap, dtype=torch.int32, device=dev)
    sets = [dict(plane=torch.empty((n, H, W), dtype=torch.float32, device=dev), verdict=torch.empty((n, cap), dtype=torch.uint8, device=dev),
                 pixel=torch.empty((n, cap), dtype=torch.int32, device=dev), summary=torch.empty((n, 4), dtype=torch.int32, device=dev)) for _ in range(2)]

    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    t0 = time.perf_counter()
    frames = [O.PreparedFrame(depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], z_near=wl.near, z_far=wl.far,
                              max_diff=wl.max_diff, replace_value=wl.replace_value, want_debug=True) for s in range(n)]
    O.run_prepared(frames, threads)
    want = {r: [] for r in (0, 4)}
    for s, f in enumerate(frames):
        virt = expected_virtual(f.zwin, f.prim, wl.near, wl.far, np.inf)
        for r in want:
            want[r].append(PC.verdicts(pts[s], INTR, virt, wl.max_diff, r))
    del frames
    totals = {r: np.sum([PC.summary(v) for v, _ in want[r]], axis=0) for r in want}
    say("# oracle planes and expected verdicts of all %d streams: %.1f s on %d threads; kept / filtered / outside at r = 0: %d / %d / %d, r = 4: %d / %d / %d"
        % (n, time.perf_counter() - t0, threads, totals[0][0], totals[0][1], totals[0][2], totals[4][0], totals[4][1], totals[4][2]))

    fx, fy, cx, cy = (float(v) for v in PC.stored_intrinsics(*INTR))
    thr = float(np.float32(wl.max_diff))
    px, py, pz = d_points[..., 0].contiguous(), d_points[..., 1].contiguous(), d_points[..., 2].contiguous()

    def torch_verdicts(plane, r):
        """The torch ops of a caller without the points call, on the rendered plane (+inf where no link drew)."""
        uf = ((px / pz) * fx + cx) + 0.5
        vf = ((py / pz) * fy + cy) + 0.5
        judged = (pz > 0) & torch.isfinite(pz) & (uf >= 0) & (uf < float(W)) & (vf >= 0) & (vf < float(H))
        idx = torch.where(judged, vf.to(torch.int64) * W + uf.to(torch.int64), 0)
        if r:
            plane = -torch.nn.functional.max_pool2d(-plane.unsqueeze(1), 2 * r + 1, stride=1, padding=r).squeeze(1)      # (padded with -inf: +inf for the minimum)
        vmin = plane.reshape(n, W * H).gather(1, idx)
        return torch.where(judged, (pz > vmin - thr).to(torch.uint8), 2).to(torch.uint8)

    results = []
    for lanes in (1, 0):
        p = R.default_params()
        p.filter_replace_value, p.depth_distance_threshold = wl.replace_value, wl.max_diff
        p.raster_lanes = lanes
        ctx = R.Context(W, H, n, 0, p)
        ids = wl.load_into(ctx)
        wl.stage(ctx, ids)
        ctx.set_cloud_intrinsics(0, [INTR] * n)
        for rnd in range(args.rounds):
            for what, r in LEGS:
                last = {}

                def submit(k):
                    o = sets[k % 2]
                    if what == "points":
                        ctx.points_batch_device(n, d_points.data_ptr(), d_counts.data_ptr(), cap, r, o["verdict"].data_ptr(), o["pixel"].data_ptr(), o["summary"].data_ptr())
                    else:
                        ctx.render_batch_device(n, o["plane"].data_ptr(), None, float("inf"))
                        if what == "torch":
                            ctx.order_stream_after_batches(torch.cuda.current_stream().cuda_stream)
                            last["out"] = torch_verdicts(o["plane"], r)

                def finish():
                    ctx.sync()
                    torch.cuda.synchronize()

                for k in range(args.warmup):
                    submit(k)
                finish()
                t = time.perf_counter()
                for k in range(args.steps):
                    submit(k)
                finish()
                el = time.perf_counter() - t
                bad = 0
                if what != "render":
                    got = (last["out"] if what == "torch" else sets[(args.steps - 1) % 2]["verdict"]).cpu().numpy()
                    bad = sum(int((got[s] != want[r][s][0]).sum()) for s in range(n))
                    if what == "points":
                        gp = sets[(args.steps - 1) % 2]["pixel"].cpu().numpy().view(np.uint32)
                        bad += sum(int((gp[s] != want[r][s][1]).sum()) for s in range(n))
                last.clear()
                ms_tile = ms_points = 0.0
                if what != "torch" and rnd == 0:
                    ctx.enable_timing(2)                  # (starts the sums again)
                    for k in range(args.timed_steps):
                        submit(k)
                    finish()
                    st = ctx.stats()
                    ctx.enable_timing(0)
                    nb = max(1, st["timed_batches"])
                    ms_tile, ms_points = st["sum_ms_raster"] / nb, (st["sum_ms_compare"] / nb if what == "points" else 0.0)
                st = ctx.stats()
                row = {"raster_lanes": st["raster_lanes"], "round": rnd, "batch": what, "radius": r, "frames_per_s": round(n * args.steps / el, 1),
                       "batch_ms": round(1e3 * el / args.steps, 3), "ms_tile_per_batch": round(ms_tile, 4), "ms_points_kernel_per_batch": round(ms_points, 4),
                       "launch_groups": st["groups_last_batch"], "streams_checked": 0 if what == "render" else n, "mismatches": bad}
                results.append(row)
                say(json.dumps(row))
                if bad:
                    raise SystemExit("lanes %d %s r=%d: the last batch differs from the expectation" % (lanes, what, r))
        ctx.close()

    # bytes a point costs the points kernel: 12 in, 1 verdict and 4 pixel out, and (2r+1)^2 plane values of 4 bytes gathered
    say("# frames/s per lane setting; spread = (max - min) / mean of a leg's own rounds:")
    summary = []
    for lanes in sorted(set(r["raster_lanes"] for r in results)):
        rs = [r for r in results if r["raster_lanes"] == lanes]

        def leg(what, rad):
            f = [r["frames_per_s"] for r in rs if r["batch"] == what and r["radius"] == rad]
            mean = sum(f) / len(f)
            return f, mean, (max(f) - min(f)) / mean
        rl, rmean, rspread = leg("render", 0)
        say("#   lanes %d  (a) render alone: rounds %s, spread %.3f" % (lanes, " ".join("%.0f" % v for v in rl), rspread))
        parts = []
        for rad in (0, 4):
            tl, tmean, tspread = leg("torch", rad)
            pl, pmean, pspread = leg("points", rad)
            ms = next(r for r in rs if r["batch"] == "points" and r["radius"] == rad and r["round"] == 0)
            streamed = n * cap * 17.0
            gathered = n * cap * 4.0 * (2 * rad + 1) ** 2
            k_ms = ms["ms_points_kernel_per_batch"]
            slower = pmean < tmean and (tmean - pmean) / tmean > max(tspread, pspread)
            say("#   lanes %d  r = %d  (b) render + torch: rounds %s, spread %.3f" % (lanes, rad, " ".join("%.0f" % v for v in tl), tspread))
            say("#   lanes %d  r = %d  points batch:      rounds %s, spread %.3f = %.3f of (a), %.2f x (b): %s"
                % (lanes, rad, " ".join("%.0f" % v for v in pl), pspread, pmean / rmean, pmean / tmean,
                   "SLOWER than (b) beyond the legs' spread" if slower else "not slower than (b) beyond the legs' spread"))
            say("#   lanes %d  r = %d  tile kernel %.4f ms + points kernel %.4f ms per batch (sums over the lanes' launches); per point 17 bytes streamed + %d gathered: "
                "%.1f GB/s streamed, %.1f GB/s with the gathers counted as 4 bytes each" % (lanes, rad, ms["ms_tile_per_batch"], k_ms, 4 * (2 * rad + 1) ** 2,
                                                                                         streamed / (k_ms * 1e6) if k_ms else 0.0, (streamed + gathered) / (k_ms * 1e6) if k_ms else 0.0))
            parts.append("r=%d points %.0f (%.2f of render, %.2f x torch; spreads %.3f / %.3f)" % (rad, pmean, pmean / rmean, pmean / tmean, pspread, tspread))
        summary.append("%d lane(s): render %.0f (spread %.3f), %s" % (lanes, rmean, rspread, ", ".join(parts)))
    say("# c3 frames/s, %d points per stream, " % cap + "; ".join(summary))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
