"""Frames/s and tile kernel time of link labels (rtuf_filter_batch_device_labels) on the c3 workload: 256 VGA streams of the
250 k-triangle PR2-like robot, device-resident planes (f32 masked + mask, + the uint16 label plane), one raster lane and the
default lanes, fused and with RTUF_FLAG_TWO_KERNEL, each without and with labels.

Per configuration: warm-up, `--steps` timed batches (two output sets alternating, as bench.py), then a pass with
rtuf_enable_timing(2) for the tile kernel (ms_raster) per batch.  Every stream of the last timed batch is checked against the
CPU oracle: masked / mask bit for bit, and the labels against its winning triangles mapped through draw -> link -> label
(bench_support/labels_check.py); a mismatch fails.

usage: python scripts/labels_rate.py [--streams 256] [--steps 40] [--warmup 10]"""
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
from bench_support.labels_check import expected_labels, workload_draws  # noqa: E402
from oracle import bindings as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timed-steps", type=int, default=16, help="batches of the rtuf_enable_timing(2) pass")
    args = ap.parse_args()
    n, W, H = args.streams, 640, 480
    wl = WL.pr2_workload(n, W, H, total_triangles=args.triangles)
    dev = torch.device("cuda:0")
    depth = wl.depth_batch().astype(np.float32)
    d_depth = torch.from_numpy(depth).to(dev)
    sets = [(torch.empty((n, H, W), dtype=torch.float32, device=dev), torch.empty((n, H, W), dtype=torch.uint8, device=dev),
             torch.empty((n, H, W), dtype=torch.int16, device=dev)) for _ in range(2)]

    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    t0 = time.perf_counter()
    frames = [O.PreparedFrame(depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], max_diff=wl.max_diff,
                              replace_value=wl.replace_value, want_debug=True) for s in range(n)]
    O.run_prepared(frames, threads)
    dlab, dtris = workload_draws(wl)
    want_labels = [expected_labels(f.prim, dlab, dtris) for f in frames]
    print("# oracle planes of %d streams: %.1f s on %d threads" % (n, time.perf_counter() - t0, threads), flush=True)

    results = []
    for lanes in (1, 0):
        for two in (False, True):
            for labels in (False, True):
                p = R.default_params()
                p.filter_replace_value, p.depth_distance_threshold = wl.replace_value, wl.max_diff
                p.raster_lanes = lanes
                if two:
                    p.flags |= R.FLAG_TWO_KERNEL
                ctx = R.Context(W, H, n, 0, p)
                wl.stage(ctx, wl.load_into(ctx))

                def submit(k):
                    m, kk, lab = sets[k % 2]
                    if labels:
                        ctx.filter_batch_device_labels(n, d_depth.data_ptr(), m.data_ptr(), kk.data_ptr(), lab.data_ptr())
                    else:
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
                hl = sets[k_last % 2][2].cpu().numpy().view(np.uint16)
                bad = bad_labels = 0
                for s in range(n):
                    bad += int((frames[s].mask != hk[s]).sum()) + int((frames[s].masked.view(np.uint32) != hm[s].view(np.uint32)).sum())
                    if labels:
                        bad_labels += int((want_labels[s] != hl[s]).sum())
                row = {"raster_lanes": st["raster_lanes"], "two_kernel_flag": two, "labels": labels, "frames_per_s": round(fps, 1),
                       "batch_ms": round(1e3 * el / args.steps, 3), "ms_tile_per_batch": round(ms_tile, 4), "ms_compare_per_batch": round(ms_cmp, 4),
                       "launch_groups": st["groups_last_batch"], "frames_checked": n, "mismatching_values": bad,
                       "mismatching_labels": bad_labels if labels else None}
                results.append(row)
                print(json.dumps(row), flush=True)
                if bad or bad_labels:
                    raise SystemExit("lanes %d two-kernel %s labels %s: %d values, %d labels differ from the oracle" % (lanes, two, labels, bad, bad_labels))
    print("# frames/s with labels relative to the same route and lanes without:")
    for row in results:
        if row["labels"]:
            base = next(x for x in results if x["raster_lanes"] == row["raster_lanes"] and x["two_kernel_flag"] == row["two_kernel_flag"] and not x["labels"])
            fused = next(x for x in results if x["raster_lanes"] == row["raster_lanes"] and not x["two_kernel_flag"] and not x["labels"])
            print("#   lanes %d  %s  %.3f of the same route, %.3f of the plain fused path, tile kernel %.4f -> %.4f ms"
                  % (row["raster_lanes"], "two-kernel" if row["two_kernel_flag"] else "fused     ", row["frames_per_s"] / base["frames_per_s"],
                     row["frames_per_s"] / fused["frames_per_s"], base["ms_tile_per_batch"], row["ms_tile_per_batch"]))


if __name__ == "__main__":
    main()
