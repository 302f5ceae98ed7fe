"""Frames/s and tile kernel time of per-link depth thresholds (rtuf_set_link_thresholds) on the c3 workload: 256 VGA streams of
the 250 k-triangle PR2-like robot, device-resident planes (f32 masked + mask), fused route, one raster lane and the default
lanes.  Every link gets a threshold of its own (0.02 .. 0.30 m); the plain fused path runs on the same box, alternating with it
round by round, so box-to-box and drift differences cancel in the ratio.

Per configuration and round: warm-up, `--steps` timed batches (two output sets alternating, as bench.py), then a pass with
rtuf_enable_timing(2) for the tile kernel (ms_raster) per batch.  Every stream of the last timed batch is checked: the plain
path against the CPU oracle bit for bit, the threshold path against the oracle's winners mapped through draw -> link ->
threshold and shaded in numpy float32 (bench_support/link_thresholds_check.py); a mismatch fails.

usage: python scripts/link_thresholds_rate.py [--streams 256] [--steps 40] [--warmup 10] [--rounds 3]"""
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
from bench_support.link_thresholds_check import expected_planes, workload_draws  # noqa: E402
from oracle import bindings as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3, help="plain / thresholds alternations per lane setting")
    ap.add_argument("--timed-steps", type=int, default=16, help="batches of the rtuf_enable_timing(2) pass")
    args = ap.parse_args()
    n, W, H = args.streams, 640, 480
    wl = WL.pr2_workload(n, W, H, total_triangles=args.triangles)
    dev = torch.device("cuda:0")
    depth = wl.depth_batch().astype(np.float32)
    d_depth = torch.from_numpy(depth).to(dev)
    sets = [(torch.empty((n, H, W), dtype=torch.float32, device=dev), torch.empty((n, H, W), dtype=torch.uint8, device=dev))
            for _ in range(2)]
    n_links = sum(len(links) for links in wl.models)
    link_thr = np.linspace(0.02, 0.30, n_links).astype(np.float32)

    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    t0 = time.perf_counter()
    frames = [O.PreparedFrame(depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], max_diff=wl.max_diff,
                              replace_value=wl.replace_value, want_debug=True) for s in range(n)]
    O.run_prepared(frames, threads)
    dthr, dtris = workload_draws(wl, link_thr)
    want = [expected_planes(f.zwin, f.prim, depth[s], dthr, dtris, wl.max_diff, wl.near, wl.far, wl.replace_value)
            for s, f in enumerate(frames)]
    print("# oracle planes of %d streams: %.1f s on %d threads" % (n, time.perf_counter() - t0, threads), flush=True)

    results = []
    for lanes in (1, 0):
        for rnd in range(args.rounds):
            for thresholds in (False, True):
                p = R.default_params()
                p.filter_replace_value, p.depth_distance_threshold = wl.replace_value, wl.max_diff
                p.raster_lanes = lanes
                ctx = R.Context(W, H, n, 0, p)
                ids = wl.load_into(ctx)
                wl.stage(ctx, ids)
                if thresholds:
                    base = 0
                    for m in ids:
                        nl = ctx.num_links(m)
                        ctx.set_link_thresholds(m, link_thr[base:base + nl])
                        base += nl

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
                ms_tile = st["sum_ms_raster"] / tb
                ctx.close()
                hm, hk = sets[k_last % 2][0].cpu().numpy(), sets[k_last % 2][1].cpu().numpy()
                bad = 0
                for s in range(n):
                    em, ek = want[s] if thresholds else (frames[s].masked, frames[s].mask)
                    bad += int((ek != hk[s]).sum()) + int((em.view(np.uint32) != hm[s].view(np.uint32)).sum())
                filtered = int(sum(int((w[1] != f.mask).sum()) for w, f in zip(want, frames))) if thresholds else 0
                row = {"raster_lanes": st["raster_lanes"], "round": rnd, "link_thresholds": thresholds, "frames_per_s": round(fps, 1),
                       "batch_ms": round(1e3 * el / args.steps, 3), "ms_tile_per_batch": round(ms_tile, 4),
                       "launch_groups": st["groups_last_batch"], "frames_checked": n, "mismatching_values": bad,
                       "mask_pixels_changed_by_thresholds": filtered if thresholds else None}
                results.append(row)
                print(json.dumps(row), flush=True)
                if bad:
                    raise SystemExit("lanes %d thresholds %s: %d values differ from the expectation" % (lanes, thresholds, bad))
    print("# frames/s with per-link thresholds relative to the plain fused path (same lanes, means over the rounds):")
    for lanes in sorted({r["raster_lanes"] for r in results}):
        def mean(key, thr):
            v = [r[key] for r in results if r["raster_lanes"] == lanes and r["link_thresholds"] == thr]
            return sum(v) / len(v)
        print("#   lanes %d  %.3f of the plain fused path (%.0f -> %.0f frames/s), tile kernel %.4f -> %.4f ms"
              % (lanes, mean("frames_per_s", True) / mean("frames_per_s", False), mean("frames_per_s", False), mean("frames_per_s", True),
                 mean("ms_tile_per_batch", False), mean("ms_tile_per_batch", True)))


if __name__ == "__main__":
    main()
