"""Frames/s and kernel times of silhouette dilation (rtuf_params.silhouette_dilation_px) on the c3 workload: 256 VGA streams
of the 250 k-triangle PR2-like robot, device-resident planes (f32 masked + mask), one raster lane and the default lanes, at
r = 0, 1, 4 and 16 -- plus r = 0 with RTUF_FLAG_TWO_KERNEL, the z-surface route without the dilation, which separates what
the route and its one batch in flight cost from what the dilate kernel costs.

Per configuration: warm-up, `--steps` timed batches (two output sets alternating, as bench.py), then a pass with
rtuf_enable_timing(2) for the tile kernel (ms_raster) and the compare / dilate kernel (ms_compare) per batch.  Every stream of
the last timed batch is checked against the CPU oracle's debug planes (bench_support/dilation_check.py); a mismatch fails.

usage: python scripts/dilation_rate.py [--streams 256] [--steps 40] [--warmup 10] [--radii 0,1,4,16]"""
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
from bench_support import workloads as WL  # noqa: E402
from bench_support.dilation_check import drawn_z, shade, window_min  # noqa: E402
from oracle import bindings as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timed-steps", type=int, default=16, help="batches of the rtuf_enable_timing(2) pass")
    ap.add_argument("--radii", default="0,1,4,16")
    args = ap.parse_args()
    radii = [int(x) for x in args.radii.split(",")]
    n, W, H = args.streams, 640, 480
    wl = WL.pr2_workload(n, W, H, total_triangles=args.triangles)
    dev = torch.device("cuda:0")
    depth = wl.depth_batch().astype(np.float32)
    d_depth = torch.from_numpy(depth).to(dev)
    sets = [(torch.empty((n, H, W), dtype=torch.float32, device=dev), torch.empty((n, H, W), dtype=torch.uint8, device=dev)) for _ in range(2)]

    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    t0 = time.perf_counter()
    frames = [O.PreparedFrame(depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], max_diff=wl.max_diff,
                              replace_value=wl.replace_value, want_debug=True) for s in range(n)]
    O.run_prepared(frames, threads)
    zs = [drawn_z(f.zwin, f.prim) for f in frames]
    print("# oracle debug planes of %d streams: %.1f s on %d threads" % (n, time.perf_counter() - t0, threads), flush=True)

    configs = []
    for lanes in (1, 0):
        configs.append((lanes, 0, True))
        configs += [(lanes, r, False) for r in radii]
    results = []
    for lanes, r, two in configs:
        p = R.default_params()
        p.filter_replace_value, p.depth_distance_threshold = wl.replace_value, wl.max_diff
        p.raster_lanes = lanes
        p.silhouette_dilation_px = r
        if two:
            p.flags |= R.FLAG_TWO_KERNEL
        ctx = R.Context(W, H, n, 0, p)
        wl.stage(ctx, wl.load_into(ctx))

        def submit(k):
            m, kk = sets[k % 2]
            ctx.filter_batch_device(n, d_depth.data_ptr(), m.data_ptr(), kk.data_ptr())

        for k in range(args.warmup):
            submit(k)
        ctx.sync()
        t = time.perf_counter()
        for k in range(args.steps):
            submit(k)
        ctx.sync()
        el = time.perf_counter() - t
        fps = n * args.steps / el
        k_last = args.steps - 1
        ctx.enable_timing(2)
        for k in range(args.timed_steps):
            submit(k)
        ctx.sync()
        st = ctx.stats()
        tb = max(1, st["timed_batches"])
        ms_tile, ms_cmp = st["sum_ms_raster"] / tb, st["sum_ms_compare"] / tb
        ctx.close()
        # parity: every stream of the last timed batch (every batch has the same inputs, so the timing pass rewrote the same values)
        hm, hk = sets[k_last % 2][0].cpu().numpy(), sets[k_last % 2][1].cpu().numpy()
        bad = 0
        for s in range(n):
            em, ek = shade(window_min(zs[s], r), depth[s], wl.near, wl.far, wl.max_diff, wl.replace_value)
            bad += int((ek != hk[s]).sum()) + int((em.view(np.uint32) != hm[s].view(np.uint32)).sum())
        row = {"raster_lanes": st["raster_lanes"], "radius": r, "two_kernel_flag": two, "frames_per_s": round(fps, 1),
               "batch_ms": round(1e3 * el / args.steps, 3), "ms_tile_per_batch": round(ms_tile, 4), "ms_compare_or_dilate_per_batch": round(ms_cmp, 4),
               "launch_groups": st["groups_last_batch"], "frames_checked": n, "mismatching_values": bad}
        results.append(row)
        print(json.dumps(row), flush=True)
        if bad:
            raise SystemExit("lanes %d r %d: %d values differ from the oracle" % (lanes, r, bad))
    print("# frames/s relative to r = 0 (fused) of the same lanes:")
    for row in results:
        base = next(x for x in results if x["raster_lanes"] == row["raster_lanes"] and x["radius"] == 0 and not x["two_kernel_flag"])
        print("#   lanes %d  r %2d%s  %.3f" % (row["raster_lanes"], row["radius"], " two-kernel" if row["two_kernel_flag"] else "           ",
                                           row["frames_per_s"] / base["frames_per_s"]))


if __name__ == "__main__":
    main()
