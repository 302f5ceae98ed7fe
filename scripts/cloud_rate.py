"""Frames/s of the filtered point clouds (rtuf_cloud_batch_device*, rtuf_cloud_compact_batch_device*) on the c3 workload: 256 VGA
streams of the 250 k-triangle PR2-like robot, device-resident planes, one raster lane and the default lanes, against two
yardsticks from the same run:
  (a) the mask-bits device batch the cloud batches are built on (three legs per lane setting: first, middle, last -- their
      spread is the run-to-run spread everything else is read against);
  (b) what a caller does today: rtuf_filter_batch_device (masked + mask) followed by torch ops that build the same organized
      tensor (keep = mask == 0 & valid sensor; stack of x, y, z; where(keep, xyz, NaN)), or the same compacted output directly
      from the stacked points without the NaN plane (one nonzero of keep, a gather, index = v * W + u, counts by bincount),
      all streams of the batch concatenated (two legs each; both are checked against the expectation like the cloud legs).

Per leg: warm-up, `--steps` timed batches (two output sets alternating, as bench.py), then a pass with rtuf_enable_timing(2):
ms_raster is the tile kernel, ms_compare the cloud kernels of a batch.  A sample of the last timed batch's streams is checked
against bench_support/cloud_check.py on the CPU oracle's mask, bit for bit; a mismatch of a cloud leg fails.  The lines go to
stdout and to --out.

usage: python scripts/cloud_rate.py [--streams 256] [--steps 40] [--warmup 10] [--out profiles/cloud_rate_c3.txt]"""
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
from bench_support import workloads as WL  # noqa: E402
from oracle import bindings as O  # noqa: E402

# (batch, 16UC1)
LEGS = (("bits", False), ("today organized", False), ("today compacted", False), ("cloud organized", False), ("cloud organized", True), ("bits", False),
        ("cloud compacted", False), ("cloud compacted", True), ("today organized", False), ("today compacted", False), ("bits", False))
FX, FY, CX, CY = 525.0, 525.0, 319.5, 239.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timed-steps", type=int, default=16, help="batches of the rtuf_enable_timing(2) pass")
    ap.add_argument("--checked", type=int, default=8, help="streams of the last batch held against the expectation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_rate_c3.txt"))
    args = ap.parse_args()
    n, W, H = args.streams, 640, 480
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# python scripts/cloud_rate.py (%d VGA streams of c3, device planes, %d timed steps, %d warm-up, %d with rtuf_enable_timing(2)); one MI355X"
        % (n, args.steps, args.warmup, args.timed_steps))
    wl = WL.pr2_workload(n, W, H, total_triangles=args.triangles)
    dev = torch.device("cuda:0")
    depth = wl.depth_batch().astype(np.float32)
    depth_mm = np.clip(np.rint(np.nan_to_num(depth, nan=0.0, posinf=65.535, neginf=0.0) * 1000.0), 0, 65535).astype(np.uint16)
    d_depth = torch.from_numpy(depth).to(dev)
    d_depth_mm = torch.from_numpy(depth_mm.view(np.int16)).to(dev)
    cap = W * H
    sets = [dict(masked=torch.empty((n, H, W), dtype=torch.float32, device=dev), mask=torch.empty((n, H, W), dtype=torch.uint8, device=dev),
                 bits=torch.empty((n, H * ((W + 31) // 32)), dtype=torch.int32, device=dev), points=torch.empty((n, H, W, 3), dtype=torch.float32, device=dev),
                 index=torch.empty((n, cap), dtype=torch.int32, device=dev), counts=torch.empty((n,), dtype=torch.int32, device=dev)) for _ in range(2)]
    kx, ky, cx, cy = (float(v) for v in CC.stored_intrinsics(FX, FY, CX, CY))
    uu = (torch.arange(W, dtype=torch.float32, device=dev) - cx).view(1, 1, W)
    vv = (torch.arange(H, dtype=torch.float32, device=dev) - cy).view(1, H, 1)
    nan = torch.tensor(float("nan"), dtype=torch.float32, device=dev)

    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    sample = sorted(set(np.linspace(0, n - 1, min(n, args.checked)).astype(int).tolist()))
    t0 = time.perf_counter()
    want = {}
    for u16 in (False, True):
        sens = CC.u16_to_metres(depth_mm) if u16 else depth
        frames = [O.PreparedFrame(sens[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], max_diff=wl.max_diff,
                                  replace_value=wl.replace_value) for s in sample]
        O.run_prepared(frames, threads)
        want[u16] = [(CC.organized(sens[s], f.mask, (FX, FY, CX, CY)),) + CC.compacted(sens[s], f.mask, (FX, FY, CX, CY)) for s, f in zip(sample, frames)]
    say("# oracle masks and expected clouds of %d streams: %.1f s on %d threads" % (len(sample), time.perf_counter() - t0, threads))

    def today(o, compact):
        """The torch ops of a caller without the cloud calls, on the filter's masked plane and mask."""
        s = d_depth
        keep = (o["mask"] == 0) & (s > 0) & torch.isfinite(s)
        x = ((uu * s) * kx)
        y = ((vv * s) * ky)
        xyz = torch.stack((x, y, s), dim=-1)
        if not compact:
            return torch.where(keep.unsqueeze(-1), xyz, nan), None, None
        # the compacted tensor alone: one nonzero, a gather from the stacked points (no NaN plane in between), the index
        # v * W + u of every entry and the counts per stream
        nz = keep.nonzero(as_tuple=True)
        return xyz[nz], nz[1] * W + nz[2], torch.bincount(nz[0], minlength=n)

    results = []
    for lanes in (1, 0):
        p = R.default_params()
        p.filter_replace_value, p.depth_distance_threshold = wl.replace_value, wl.max_diff
        p.raster_lanes = lanes
        ctx = R.Context(W, H, n, 0, p)
        ids = wl.load_into(ctx)
        wl.stage(ctx, ids)
        ctx.set_cloud_intrinsics(0, [(FX, FY, CX, CY)] * n)
        for what, u16 in LEGS:
            last = {}

            def submit(k):
                o = sets[k % 2]
                d = d_depth_mm if u16 else d_depth
                if what == "bits":
                    ctx.filter_batch_device_bits(n, d.data_ptr(), o["bits"].data_ptr(), u16=u16)
                elif what == "cloud organized":
                    ctx.cloud_batch_device(n, d.data_ptr(), o["points"].data_ptr(), u16=u16)
                elif what == "cloud compacted":
                    ctx.cloud_compact_batch_device(n, d.data_ptr(), o["points"].data_ptr(), o["index"].data_ptr(), o["counts"].data_ptr(), cap, u16=u16)
                else:
                    ctx.filter_batch_device(n, d_depth.data_ptr(), o["masked"].data_ptr(), o["mask"].data_ptr())
                    ctx.order_stream_after_batches(torch.cuda.current_stream().cuda_stream)
                    last["out"] = today(o, what == "today compacted")

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
            fps = n * args.steps / el
            k_last = args.steps - 1
            o = sets[k_last % 2]
            bad = 0
            if what == "cloud organized":
                got = o["points"][sample].cpu().numpy()
                bad = sum(int((got[i].view(np.uint32) != want[u16][i][0].view(np.uint32)).sum()) for i in range(len(sample)))
            elif what == "cloud compacted":
                gp, gi, gc = o["points"].view(n, cap, 3)[sample].cpu().numpy(), o["index"][sample].cpu().numpy().view(np.uint32), o["counts"][sample].cpu().numpy()
                for i in range(len(sample)):
                    _, wp, wi, wc = want[u16][i]
                    bad += int(gc[i] != wc) + int((gp[i][:wc].view(np.uint32) != wp.view(np.uint32)).sum()) + int((gi[i][:wc] != wi).sum())
            elif what == "today organized":
                got = last["out"][0][sample].cpu().numpy()
                bad = sum(int((got[i].view(np.uint32) != want[False][i][0].view(np.uint32)).sum()) for i in range(len(sample)))
            elif what == "today compacted":
                tp, ti, tc = last["out"]
                start = torch.cumsum(tc, 0) - tc
                for i, st_ in enumerate(sample):
                    _, wp, wi, wc = want[False][i]
                    a = int(start[st_])
                    bad += int(int(tc[st_]) != wc)
                    bad += int((tp[a:a + wc].cpu().numpy().view(np.uint32) != wp.view(np.uint32)).sum()) + int((ti[a:a + wc].cpu().numpy() != wi).sum())
            last.clear()
            ms_tile = ms_cloud = 0.0
            if not what.startswith("today"):
                ctx.enable_timing(2)                  # (starts the sums again)
                for k in range(args.timed_steps):
                    submit(k)
                finish()
                st = ctx.stats()
                ctx.enable_timing(0)
                nb = max(1, st["timed_batches"])
                ms_tile = st["sum_ms_raster"] / nb
                ms_cloud = st["sum_ms_compare"] / nb if what.startswith("cloud") else 0.0
            st = ctx.stats()
            row = {"raster_lanes": st["raster_lanes"], "batch": what, "u16": u16, "frames_per_s": round(fps, 1), "batch_ms": round(1e3 * el / args.steps, 3),
                   "ms_tile_per_batch": round(ms_tile, 4), "ms_cloud_kernels_per_batch": round(ms_cloud, 4), "launch_groups": st["groups_last_batch"],
                   "frames_checked": len(sample), "mismatches": bad}
            results.append(row)
            say(json.dumps(row))
            if bad and what.startswith("cloud"):
                raise SystemExit("lanes %d %s u16 %s: the last batch differs from the expectation" % (lanes, what, u16))
        ctx.close()
    say("# frames/s per lane setting; spread = (max - min) / mean of a yardstick's own legs:")
    summary = []
    for lanes in sorted(set(r["raster_lanes"] for r in results)):
        rs = [r for r in results if r["raster_lanes"] == lanes]

        def legs(what):
            f = [r["frames_per_s"] for r in rs if r["batch"] == what]
            mean = sum(f) / len(f)
            return f, mean, (max(f) - min(f)) / mean
        bl, bmean, bspread = legs("bits")
        say("#   lanes %d  (a) mask-bits legs %s, spread %.3f" % (lanes, " ".join("%.0f" % v for v in bl), bspread))
        parts = []
        for form in ("organized", "compacted"):
            tl, tmean, tspread = legs("today " + form)
            say("#   lanes %d  (b) filter + torch, %s: legs %s, spread %.3f" % (lanes, form, " ".join("%.0f" % v for v in tl), tspread))
            for r in rs:
                if r["batch"] == "cloud " + form:
                    beats = r["frames_per_s"] > max(tl) and (r["frames_per_s"] - tmean) / tmean > tspread
                    say("#   lanes %d  cloud %s %s  %.0f frames/s = %.3f of (a), %.2f x (b) (%s (b) by more than its spread); tile %.4f ms + cloud kernels %.4f ms"
                        % (lanes, form, "16UC1" if r["u16"] else "f32  ", r["frames_per_s"], r["frames_per_s"] / bmean, r["frames_per_s"] / tmean,
                           "beats" if beats else "DOES NOT beat", r["ms_tile_per_batch"], r["ms_cloud_kernels_per_batch"]))
                    if not r["u16"]:
                        parts.append("%s %.0f (%.2f of bits, %.1f x today)" % (form, r["frames_per_s"], r["frames_per_s"] / bmean, r["frames_per_s"] / tmean))
        summary.append("%d lane(s): bits %.0f (spread %.3f), cloud f32 %s" % (lanes, bmean, bspread, ", ".join(parts)))
    say("# c3 frames/s, " + "; ".join(summary))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
