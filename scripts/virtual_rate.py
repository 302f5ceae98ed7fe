"""Frames/s and tile kernel time of virtual depth planes (rtuf_render_batch_device*) on the c3 workload: 256 VGA streams of the
250 k-triangle PR2-like robot, device-resident planes, one raster lane and the default lanes: the plain fused filter (f32
masked + mask) first, then render batches f32 and 16UC1, each without and with the uint16 label plane.

Per configuration: warm-up, `--steps` timed batches (two output sets alternating, as bench.py), then a pass with
rtuf_enable_timing(2) for the tile kernel (ms_raster) per batch.  Every stream of the last timed batch is checked against the
CPU oracle: the filter's masked / mask bit for bit, the virtual depth against bench_support/virtual_check.py and the labels
against bench_support/labels_check.py; a mismatch fails.  The lines go to stdout and to --out.

usage: python scripts/virtual_rate.py [--streams 256] [--steps 40] [--warmup 10] [--out profiles/virtual_rate_c3.txt]"""
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
from bench_support.virtual_check import expected_virtual, metres_to_u16  # noqa: E402
from oracle import bindings as O  # noqa: E402

EMPTY = 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timed-steps", type=int, default=16, help="batches of the rtuf_enable_timing(2) pass")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "virtual_rate_c3.txt"))
    args = ap.parse_args()
    n, W, H = args.streams, 640, 480
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# python scripts/virtual_rate.py (%d VGA streams of c3, device planes, %d timed steps, %d warm-up, %d with rtuf_enable_timing(2)); one MI355X"
        % (n, args.steps, args.warmup, args.timed_steps))
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
    want_virtual = [expected_virtual(f.zwin, f.prim, wl.near, wl.far, EMPTY) for f in frames]
    say("# oracle planes of %d streams: %.1f s on %d threads" % (n, time.perf_counter() - t0, threads))

    results = []
    for lanes in (1, 0):
        for what, u16, labels in (("filter", False, False), ("render", False, False), ("render", False, True), ("render", True, False), ("render", True, True)):
            p = R.default_params()
            p.filter_replace_value, p.depth_distance_threshold = wl.replace_value, wl.max_diff
            p.raster_lanes = lanes
            ctx = R.Context(W, H, n, 0, p)
            wl.stage(ctx, wl.load_into(ctx))

            def submit(k):
                m, kk, lab = sets[k % 2]
                if what == "filter":
                    ctx.filter_batch_device(n, d_depth.data_ptr(), m.data_ptr(), kk.data_ptr())
                else:           # (the 16UC1 plane takes the first half of the f32 buffer)
                    (ctx.render_batch_device_u16 if u16 else ctx.render_batch_device)(n, m.data_ptr(), lab.data_ptr() if labels else None, EMPTY)

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
            ms_tile = st["sum_ms_raster"] / max(1, st["timed_batches"])
            ctx.close()
            # parity: every stream of the last timed batch (every batch has the same inputs, so the timing pass rewrote the same values)
            hm, hk = sets[k_last % 2][0].cpu().numpy(), sets[k_last % 2][1].cpu().numpy()
            hl = sets[k_last % 2][2].cpu().numpy().view(np.uint16)
            bad = bad_labels = 0
            for s in range(n):
                if what == "filter":
                    bad += int((frames[s].mask != hk[s]).sum()) + int((frames[s].masked.view(np.uint32) != hm[s].view(np.uint32)).sum())
                elif u16:
                    bad += int((metres_to_u16(want_virtual[s]) != hm.reshape(-1).view(np.uint16)[s * H * W:(s + 1) * H * W].reshape(H, W)).sum())
                else:
                    bad += int((want_virtual[s].view(np.uint32) != hm[s].view(np.uint32)).sum())
                if labels:
                    bad_labels += int((want_labels[s] != hl[s]).sum())
            row = {"raster_lanes": st["raster_lanes"], "batch": what, "u16": u16, "labels": labels, "frames_per_s": round(fps, 1),
                   "batch_ms": round(1e3 * el / args.steps, 3), "ms_tile_per_batch": round(ms_tile, 4), "launch_groups": st["groups_last_batch"],
                   "frames_checked": n, "mismatching_values": bad, "mismatching_labels": bad_labels if labels else None}
            results.append(row)
            say(json.dumps(row))
            if bad or bad_labels:
                raise SystemExit("lanes %d %s u16 %s labels %s: %d values, %d labels differ from the oracle" % (lanes, what, u16, labels, bad, bad_labels))
    say("# render frames/s relative to the plain fused filter of the same lanes:")
    ratios = []
    for row in results:
        if row["batch"] == "render":
            base = next(x for x in results if x["raster_lanes"] == row["raster_lanes"] and x["batch"] == "filter")
            ratios.append(row["frames_per_s"] / base["frames_per_s"])
            say("#   lanes %d  %s %s  %.3f of the filter's frames/s, tile kernel %.4f -> %.4f ms"
                % (row["raster_lanes"], "16UC1" if row["u16"] else "f32  ", "+ labels" if row["labels"] else "        ", ratios[-1],
                   base["ms_tile_per_batch"], row["ms_tile_per_batch"]))
    fused = [x for x in results if x["batch"] == "filter"]
    plain = [x for x in results if x["batch"] == "render" and not x["u16"] and not x["labels"]]
    say("# c3 frames/s, filter -> render f32: " + ", ".join("%d lane(s) %.0f -> %.0f" % (a["raster_lanes"], a["frames_per_s"], b["frames_per_s"])
                                                           for a, b in zip(fused, plain))
        + "; render / filter over all forms %.3f .. %.3f" % (min(ratios), max(ratios)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
