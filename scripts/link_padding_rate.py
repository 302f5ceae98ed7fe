"""Frames/s of link padding (rtuf_set_link_padding) on the c3 workload: 256 VGA streams of the 250 k-triangle PR2-like robot,
device-resident planes, one raster lane and the default lanes.  The legs alternate round by round in one process on one
context per lane setting:
  bits            the mask-bits device batch without padding (the fused route)
  dilated r       the same with silhouette_dilation_px = r, for r the largest reach floor(sqrt(max R2)) the workload shows at 2 cm
                  and at 5 cm (one leg if they are equal): the yardstick -- the z-surface route with a window of that size everywhere
  pad 2 cm        the same with 2 cm of padding on every link
  pad 5 cm        ... with 5 cm
  cloud 2 cm      a compacted cloud batch with 2 cm on every link
Per leg and round: warm-up, then `--steps` timed batches (two output sets alternating, as bench.py).  After the rounds a pass
with rtuf_enable_timing(2): ms_raster is the tile kernel, ms_compare what runs behind it -- dilate_compare_kernel or
pad_compare_kernel (plus the cloud kernels for the cloud leg).  A leg's spread is (max - min) / mean of its rounds.

Every stream of the last batch of every dilated, padded and cloud leg is checked against the expectation from the CPU
oracle's planes (bench_support/dilation_check.py, link_padding_check.py, cloud_check.py), bit for bit; a mismatch fails.  The
reach histogram (mean and largest sqrt(R2) over the drawn link pixels, share of clamped sources) comes from the same planes.
The lines go to stdout and to --out.

usage: python scripts/link_padding_rate.py [--streams 256] [--steps 40] [--warmup 10] [--rounds 3] [--out profiles/link_padding_rate_c3.txt]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import realtime_urdf_filter_amd as R  # noqa: E402
from bench_support import cloud_check as CC  # noqa: E402
from bench_support import link_padding_check as PC  # noqa: E402
from bench_support import workloads as WL  # noqa: E402
from bench_support.dilation_check import drawn_z, shade, window_min  # noqa: E402
from oracle import bindings as O  # noqa: E402

FX, FY, CX, CY = 525.0, 525.0, 319.5, 239.5
PADS = (0.02, 0.05)


def pack_bits(mask):
    H, W = mask.shape
    words = (W + 31) // 32
    m = np.zeros((H, words * 32), np.uint8)
    m[:, :W] = mask > 0
    return np.packbits(m, axis=1, bitorder="little").view("<u4").reshape(-1)


def padded_z_cropped(z, R2):
    """link_padding_check.padded_z on the bounding box of the spreading sources plus their reach: the same values, less work."""
    ys, xs = np.nonzero(R2)
    if len(ys) == 0:
        return z
    r = PC.MAX_PX
    y0, y1, x0, x1 = max(0, ys.min() - r), min(z.shape[0], ys.max() + r + 1), max(0, xs.min() - r), min(z.shape[1], xs.max() + r + 1)
    out = z.copy()
    out[y0:y1, x0:x1] = PC.padded_z(z[y0:y1, x0:x1], R2[y0:y1, x0:x1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timed-steps", type=int, default=16, help="batches of the rtuf_enable_timing(2) pass")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_padding_rate_c3.txt"))
    args = ap.parse_args()
    n, W, H = args.streams, 640, 480
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# python scripts/link_padding_rate.py (%d VGA streams of c3, device planes, %d rounds of %d timed steps, %d warm-up, %d with rtuf_enable_timing(2)); one MI355X"
        % (n, args.rounds, args.steps, args.warmup, args.timed_steps))
    wl = WL.pr2_workload(n, W, H, total_triangles=args.triangles)
    dev = torch.device("cuda:0")
    depth = wl.depth_batch().astype(np.float32)
    d_depth = torch.from_numpy(depth).to(dev)
    words = H * ((W + 31) // 32)
    cap = W * H
    sets = [dict(bits=torch.empty((n, words), dtype=torch.int32, device=dev), points=torch.empty((n, cap, 3), dtype=torch.float32, device=dev),
                 index=torch.empty((n, cap), dtype=torch.int32, device=dev), counts=torch.empty((n,), dtype=torch.int32, device=dev)) for _ in range(2)]

    # the expectation of every stream, from the oracle's planes
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    t0 = time.perf_counter()
    frames = [O.PreparedFrame(depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], max_diff=wl.max_diff,
                              replace_value=wl.replace_value, want_debug=True) for s in range(n)]
    O.run_prepared(frames, threads)
    n_links = sum(len(links) for links in wl.models)
    f32max = np.float32(max(FX, FY))

    def padded(s, pad):
        fr = frames[s]
        draw_pad, ntris = PC.workload_draws(wl, [pad] * n_links)
        R2 = PC.reach2(fr.zwin, fr.prim, draw_pad, ntris, f32max, wl.near, wl.far)
        zp = padded_z_cropped(drawn_z(fr.zwin, fr.prim), R2)
        mask = shade(zp, depth[s], wl.near, wl.far, wl.max_diff, wl.replace_value)[1]
        src = R2[fr.prim >= 0]
        return mask, np.sqrt(src.astype(np.float64)), int((src == PC.MAX_PX ** 2).sum())

    want, reach = {}, {}
    with ThreadPoolExecutor(threads) as pool:
        for pad in PADS:
            got = list(pool.map(lambda s: padded(s, pad), range(n)))
            want[("pad", pad)] = [g[0] for g in got]
            r_all = np.concatenate([g[1] for g in got])
            reach[pad] = (float(r_all.mean()), float(r_all.max()), sum(g[2] for g in got) / max(1, len(r_all)), len(r_all))
        radii = sorted(set(int(np.floor(reach[pad][1])) for pad in PADS if reach[pad][1] >= 1))
        for r in radii:
            want[("dil", r)] = list(pool.map(lambda s: shade(window_min(drawn_z(frames[s].zwin, frames[s].prim), r), depth[s], wl.near, wl.far,
                                                             wl.max_diff, wl.replace_value)[1], range(n)))
    say("# oracle planes and expectations of %d streams: %.1f s on %d threads" % (n, time.perf_counter() - t0, threads))
    for pad in PADS:
        say("# reach at %g cm, f = %g: mean sqrt(R2) %.2f px, largest %.2f px, %.4f of the %d drawn link pixels clamped at %d px"
            % (100 * pad, float(f32max), reach[pad][0], reach[pad][1], reach[pad][2], reach[pad][3], PC.MAX_PX))

    legs = [("bits", None)] + [("dilated", r) for r in radii] + [("pad", pad) for pad in PADS] + [("cloud", PADS[0])]

    def leg_name(leg):
        what, v = leg
        return {"bits": "bits", "dilated": "dilated r=%s" % v, "pad": "pad %g cm" % (100 * (v or 0)), "cloud": "cloud %g cm" % (100 * (v or 0))}[what]

    results, timing = [], {}
    for lanes in (1, 0):
        p = R.default_params()
        p.filter_replace_value, p.depth_distance_threshold = wl.replace_value, wl.max_diff
        p.raster_lanes = lanes
        ctx = R.Context(W, H, n, 0, p)
        ids = wl.load_into(ctx)
        wl.stage(ctx, ids)
        ctx.set_cloud_intrinsics(0, [(FX, FY, CX, CY)] * n)

        def configure(leg):
            what, v = leg
            for m in ids:
                ctx.clear_link_padding(m)
            p.silhouette_dilation_px = v if what == "dilated" else 0
            ctx.set_params(p)
            if what in ("pad", "cloud"):
                for m in ids:
                    ctx.set_link_padding(m, np.full(ctx.num_links(m), v, np.float32))

        def submit(leg, k):
            o = sets[k % 2]
            if leg[0] == "cloud":
                ctx.cloud_compact_batch_device(n, d_depth.data_ptr(), o["points"].data_ptr(), o["index"].data_ptr(), o["counts"].data_ptr(), cap)
            else:
                ctx.filter_batch_device_bits(n, d_depth.data_ptr(), o["bits"].data_ptr())

        def finish():
            ctx.sync()
            torch.cuda.synchronize()

        def mismatches(leg, o):
            what, v = leg
            if what == "bits":
                return 0, 0
            if what == "cloud":
                gp, gi, gc = o["points"].cpu().numpy(), o["index"].cpu().numpy().view(np.uint32), o["counts"].cpu().numpy()
                bad = 0
                for s in range(n):
                    wp, wi, wc = CC.compacted(depth[s], want[("pad", v)][s], (FX, FY, CX, CY))
                    bad += int(gc[s] != wc) + int((gp[s][:wc].view(np.uint32) != wp.view(np.uint32)).sum()) + int((gi[s][:wc] != wi).sum())
                return bad, n
            got = o["bits"].cpu().numpy().view(np.uint32)
            masks = want[("dil", v)] if what == "dilated" else want[("pad", v)]
            return sum(int((got[s] != pack_bits(masks[s])).sum()) for s in range(n)), n

        for rnd in range(args.rounds):
            for leg in legs:
                configure(leg)
                for k in range(args.warmup):
                    submit(leg, k)
                finish()
                t = time.perf_counter()
                for k in range(args.steps):
                    submit(leg, k)
                finish()
                el = time.perf_counter() - t
                bad, checked = mismatches(leg, sets[(args.steps - 1) % 2]) if rnd == args.rounds - 1 else (0, 0)
                st = ctx.stats()
                row = {"raster_lanes": st["raster_lanes"], "round": rnd, "leg": leg_name(leg), "frames_per_s": round(n * args.steps / el, 1),
                       "batch_ms": round(1e3 * el / args.steps, 3), "launch_groups": st["groups_last_batch"], "frames_checked": checked, "mismatches": bad}
                results.append(row)
                say(json.dumps(row))
                if bad:
                    raise SystemExit("lanes %d %s: the last batch differs from the expectation" % (lanes, leg_name(leg)))
        for leg in legs:
            configure(leg)
            submit(leg, 0)
            finish()
            ctx.enable_timing(2)                      # (starts the sums again)
            for k in range(args.timed_steps):
                submit(leg, k)
            finish()
            st = ctx.stats()
            ctx.enable_timing(0)
            nb = max(1, st["timed_batches"])
            timing[(st["raster_lanes"], leg_name(leg))] = (st["sum_ms_raster"] / nb, st["sum_ms_compare"] / nb)
            say(json.dumps({"raster_lanes": st["raster_lanes"], "leg": leg_name(leg), "ms_tile_per_batch": round(st["sum_ms_raster"] / nb, 4),
                            "ms_behind_tile_per_batch": round(st["sum_ms_compare"] / nb, 4)}))
        ctx.close()

    say("# frames/s per lane setting, mean of the rounds; spread = (max - min) / mean of a leg's own rounds; behind = the kernels behind the tile kernel:")
    summary = []
    for lanes in sorted(set(r["raster_lanes"] for r in results)):
        def fps(name):
            f = [r["frames_per_s"] for r in results if r["raster_lanes"] == lanes and r["leg"] == name]
            mean = sum(f) / len(f)
            return mean, (max(f) - min(f)) / mean
        parts = []
        for leg in legs:
            name = leg_name(leg)
            mean, spread = fps(name)
            tile, behind = timing[(lanes, name)]
            say("#   lanes %d  %-14s %9.0f frames/s, spread %.3f; tile %.4f ms, behind %.4f ms per batch" % (lanes, name, mean, spread, tile, behind))
        bits_mean = fps("bits")[0]
        for pad in PADS:
            r = int(np.floor(reach[pad][1]))
            pm, ps = fps(leg_name(("pad", pad)))
            if r < 1:
                continue
            dm, ds = fps(leg_name(("dilated", r)))
            verdict = "slower than the dilated leg by more than the spread" if (dm - pm) / dm > max(ps, ds) else (
                "faster than the dilated leg by more than the spread" if (pm - dm) / dm > max(ps, ds) else "within the spread of the dilated leg")
            say("#   lanes %d  pad %g cm = %.3f of dilated r=%d, %.3f of bits (%s); pad_compare_kernel %.4f ms, dilate_compare_kernel %.4f ms per batch"
                % (lanes, 100 * pad, pm / dm, r, pm / bits_mean, verdict, timing[(lanes, leg_name(("pad", pad)))][1], timing[(lanes, leg_name(("dilated", r)))][1]))
            parts.append("pad %g cm %.0f (%.2f of dilated r=%d, %.2f of bits)" % (100 * pad, pm, pm / dm, r, pm / bits_mean))
        cm = fps(leg_name(("cloud", PADS[0])))[0]
        parts.append("cloud %g cm %.0f (%.2f of bits)" % (100 * PADS[0], cm, cm / bits_mean))
        summary.append("%d lane(s): bits %.0f, %s" % (lanes, bits_mean, ", ".join(parts)))
    say("# c3 frames/s, " + "; ".join(summary))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
