"""Frames/s and tile kernel time of link residual tables (rtuf_link_residuals_batch_device*) on the c3 workload: 256 VGA streams
of the 250 k-triangle PR2-like robot, device-resident planes, one raster lane and the default lanes.  Per lane setting the
plain fused filter (f32 masked + mask) runs three times -- first, in the middle and last: their spread is the run-to-run
spread the residual legs are read against -- and between them residual batches f32 and 16UC1, without and with a threshold on
every link.

Per leg: warm-up, `--steps` timed batches (two output sets alternating, as bench.py), then a pass with rtuf_enable_timing(2)
for the tile kernel (ms_raster) per batch.  A sample of the last timed batch's streams is checked against the CPU oracle: the
filter's masked / mask bit for bit, the residual tables against bench_support/residuals_check.py for equality; a mismatch
fails.  The lines go to stdout and to --out.

usage: python scripts/link_residuals_rate.py [--streams 256] [--steps 40] [--warmup 10] [--out profiles/link_residuals_rate_c3.txt]"""
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
from bench_support.labels_check import workload_draws as label_draws  # noqa: E402
from bench_support.link_thresholds_check import workload_draws as thr_draws  # noqa: E402
from bench_support.residuals_check import ROW, expected_table, tables_equal, u16_to_metres  # noqa: E402
from oracle import bindings as O  # noqa: E402

LEGS = (("filter", False, False), ("residuals", False, False), ("residuals", True, False), ("filter", False, False),
        ("residuals", False, True), ("residuals", True, True), ("filter", False, False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timed-steps", type=int, default=16, help="batches of the rtuf_enable_timing(2) pass")
    ap.add_argument("--checked", type=int, default=24, help="streams of the last batch held against the oracle")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_residuals_rate_c3.txt"))
    args = ap.parse_args()
    n, W, H = args.streams, 640, 480
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# python scripts/link_residuals_rate.py (%d VGA streams of c3, device planes, %d timed steps, %d warm-up, %d with rtuf_enable_timing(2)); one MI355X"
        % (n, args.steps, args.warmup, args.timed_steps))
    wl = WL.pr2_workload(n, W, H, total_triangles=args.triangles)
    dev = torch.device("cuda:0")
    depth = wl.depth_batch().astype(np.float32)
    depth_mm = np.clip(np.rint(np.nan_to_num(depth, nan=0.0, posinf=65.535, neginf=0.0) * 1000.0), 0, 65535).astype(np.uint16)
    d_depth = torch.from_numpy(depth).to(dev)
    d_depth_mm = torch.from_numpy(depth_mm.view(np.int16)).to(dev)
    n_links = sum(len(links) for links in wl.models)
    n_labels = n_links + 1
    link_thr = np.linspace(0.02, 0.2, n_links).astype(np.float32)
    sets = [(torch.empty((n, H, W), dtype=torch.float32, device=dev), torch.empty((n, H, W), dtype=torch.uint8, device=dev),
             torch.empty((n, n_labels, 8), dtype=torch.int64, device=dev)) for _ in range(2)]

    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    sample = sorted(set(np.linspace(0, n - 1, min(n, args.checked)).astype(int).tolist()))
    t0 = time.perf_counter()
    frames = {s: O.PreparedFrame(depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], max_diff=wl.max_diff,
                                 replace_value=wl.replace_value, want_debug=True) for s in sample}
    O.run_prepared(list(frames.values()), threads)
    dlab, dtris = label_draws(wl)
    dthr = thr_draws(wl, link_thr)[0]
    want = {}
    for u16 in (False, True):
        for thr in (False, True):
            sens = u16_to_metres(depth_mm) if u16 else depth
            want[(u16, thr)] = np.stack([expected_table(frames[s].zwin, frames[s].prim, sens[s], dlab, dtris, dthr if thr else None, wl.max_diff,
                                                        wl.near, wl.far, n_labels) for s in sample])
    say("# oracle planes and expected tables of %d streams (%d labels): %.1f s on %d threads" % (len(sample), n_labels, time.perf_counter() - t0, threads))

    results = []
    for lanes in (1, 0):
        for what, u16, thr in LEGS:
            p = R.default_params()
            p.filter_replace_value, p.depth_distance_threshold = wl.replace_value, wl.max_diff
            p.raster_lanes = lanes
            ctx = R.Context(W, H, n, 0, p)
            ids = wl.load_into(ctx)
            wl.stage(ctx, ids)
            if thr:
                base = 0
                for m, links in zip(ids, wl.models):
                    ctx.set_link_thresholds(m, link_thr[base:base + len(links)])
                    base += len(links)

            def submit(k):
                m, kk, table = sets[k % 2]
                if what == "filter":
                    ctx.filter_batch_device(n, d_depth.data_ptr(), m.data_ptr(), kk.data_ptr())
                elif u16:
                    ctx.link_residuals_batch_device_u16(n, d_depth_mm.data_ptr(), table.data_ptr(), n_labels)
                else:
                    ctx.link_residuals_batch_device(n, d_depth.data_ptr(), table.data_ptr(), n_labels)

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
            # parity: the sampled streams of the last timed batch (every batch has the same inputs)
            bad = 0
            if what == "filter":
                hm, hk = sets[k_last % 2][0][sample].cpu().numpy(), sets[k_last % 2][1][sample].cpu().numpy()
                for i, s in enumerate(sample):
                    bad += int((frames[s].mask != hk[i]).sum()) + int((frames[s].masked.view(np.uint32) != hm[i].view(np.uint32)).sum())
            else:
                got = np.ascontiguousarray(sets[k_last % 2][2][sample].cpu().numpy()).view(ROW).reshape(len(sample), n_labels)
                ok, text = tables_equal(got, want[(u16, thr)])
                bad = 0 if ok else 1
                if not ok:
                    say("# " + text)
            row = {"raster_lanes": st["raster_lanes"], "batch": what, "u16": u16, "link_thresholds": thr, "frames_per_s": round(fps, 1),
                   "batch_ms": round(1e3 * el / args.steps, 3), "ms_tile_per_batch": round(ms_tile, 4), "launch_groups": st["groups_last_batch"],
                   "frames_checked": len(sample), "mismatches": bad}
            results.append(row)
            say(json.dumps(row))
            if bad:
                raise SystemExit("lanes %d %s u16 %s thresholds %s: the last batch differs from the oracle" % (lanes, what, u16, thr))
    say("# residual frames/s relative to the plain fused filter of the same lanes (mean of its three legs; spread = (max - min) / mean):")
    ratios, summary = [], []
    for lanes in sorted(set(r["raster_lanes"] for r in results)):
        fl = [r for r in results if r["raster_lanes"] == lanes and r["batch"] == "filter"]
        mean = sum(r["frames_per_s"] for r in fl) / len(fl)
        spread = (max(r["frames_per_s"] for r in fl) - min(r["frames_per_s"] for r in fl)) / mean
        say("#   lanes %d  filter legs %s frames/s, spread %.3f, tile kernel %.4f ms" % (lanes, " ".join("%.0f" % r["frames_per_s"] for r in fl), spread,
                                                                                     sum(r["ms_tile_per_batch"] for r in fl) / len(fl)))
        for r in results:
            if r["raster_lanes"] == lanes and r["batch"] == "residuals":
                ratios.append(r["frames_per_s"] / mean)
                say("#   lanes %d  %s %s  %.3f of the filter's frames/s, tile kernel %.4f ms"
                    % (lanes, "16UC1" if r["u16"] else "f32  ", "+ link thresholds" if r["link_thresholds"] else "                 ", ratios[-1],
                       r["ms_tile_per_batch"]))
        plain = next(r for r in results if r["raster_lanes"] == lanes and r["batch"] == "residuals" and not r["u16"] and not r["link_thresholds"])
        summary.append("%d lane(s) %.0f -> %.0f (filter spread %.3f)" % (lanes, mean, plain["frames_per_s"], spread))
    say("# c3 frames/s, filter -> residuals f32: " + ", ".join(summary) + "; residuals / filter over all forms %.3f .. %.3f" % (min(ratios), max(ratios)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
