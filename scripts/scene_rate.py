"""Frames/s of batches with scene planes in effect (include/rtuf.h, SCENE PLANES) on the c3 workload: 256 VGA streams of the
250 k-triangle PR2-like robot, device-resident planes, one raster lane and the default lanes.  The scene is LEARNED from the
workload's own sensor planes (rtuf_learn_scene_batch_device), so nearly every pixel the robot filter keeps is scene-filtered:
the dense case.  The legs alternate round by round in one process:
  plain        the fused filter without a scene, three legs per round (first, middle, last): their spread is the yardstick
  +scene       the same batch with the scene in effect, f32 and 16UC1 (scene_apply_planes_kernel behind the tile kernel)
  bits         the mask-bits batch without and with the scene (scene_apply_bits_kernel), and the compacted cloud on top of either
  two-kernel   RTUF_FLAG_TWO_KERNEL without a scene: compare_kernel, the project's measured streaming kernel of this shape, for
               the bytes / time comparison of a rocprofv3 run (--kernel-stats)
  today        what a caller does without the feature: rtuf_filter_batch_device followed by torch ops that build the same planes
Checking: the learned planes and EVERY stream of the last +scene / bits+scene batch are held against bench_support/scene_check.py
for equality; the robot filter's own planes that the expectation is built on are the plain leg's of the same run, themselves held
against the CPU oracle on a sample of streams.  A mismatch fails.

  --kernel-stats CSV RUN   instead of running: append to --out the bytes / time of the apply kernels and of compare_kernel from the
                       kernel_stats.csv of a `rocprofv3 --kernel-trace --stats -- python scripts/scene_rate.py --out RUN ...` run
  --append FILE ...    instead of running: append the given files' lines to --out (the same-box headline comparison)

usage: python scripts/scene_rate.py [--streams 256] [--steps 20] [--rounds 3] [--out profiles/scene_rate_c3.txt]"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LEGS = ("plain", "+scene f32", "+scene 16UC1", "today", "bits", "plain", "bits+scene", "cloud", "cloud+scene", "two-kernel", "plain")
ABS_M, REL = 0.02, 0.01
W, H = 640, 480


def kernel_stats(path, run_file, out):
    """Bytes / time of the apply kernels beside compare_kernel's, from the kernel_stats.csv of a rocprofv3 run of this script whose
    own output is run_file.  Every leg runs (warm-up + steps) x rounds batches of all streams in both lane settings, whatever
    the launches they are split into, so a kernel's pixels follow from the legs that launch it, and bytes / time from its
    TotalDurationNs -- per-launch averages would mix launches of 256 and of 85 streams."""
    run = None
    for line in open(run_file):
        if line.startswith("# run "):
            run = json.loads(line[6:])
    px_per_leg = 2 * run["rounds"] * (run["warmup"] + run["steps"]) * run["streams"] * W * H
    share = run["share"]
    # kernel -> (label, legs that launch it, algorithmic bytes per pixel: read + written at the run's scene-filtered share)
    kernels = {"scene_apply_planes_kernel<false, true>": ("scene_apply_planes_kernel f32", 1, 8 + 5 * share),
               "scene_apply_planes_kernel<true, true>": ("scene_apply_planes_kernel 16UC1", 1, 6 + 3 * share),
               "scene_apply_bits_kernel<false, true>": ("scene_apply_bits_kernel f32", 2, 8 + 0.25 * share),
               "compare_kernel<false>": ("compare_kernel f32 (two-kernel leg)", 1, 13.0)}
    lines = ["# rocprofv3 --kernel-trace --stats of this script, a run of its own with no counters (%d rounds of %d + %d batches per leg, scene-filtered share %.3f):"
             % (run["rounds"], run["warmup"], run["steps"], share)]
    for r in csv.DictReader(open(path)):
        for pat, (label, legs, b) in kernels.items():
            if pat in r["Name"]:
                total_ns = float(r["TotalDurationNs"])
                row = {"kernel": label, "launches": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 1), "algorithmic_bytes_per_px": round(b, 3),
                       "ps_per_px": round(1e3 * total_ns / (legs * px_per_leg), 3), "TB_per_s": round(b * legs * px_per_leg / total_ns / 1e3, 3)}
                lines.append(json.dumps(row))
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--checked", type=int, default=8, help="streams whose robot planes are held against the CPU oracle")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_rate_c3.txt"))
    ap.add_argument("--kernel-stats", nargs=2)
    ap.add_argument("--append", nargs="*")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats[0], args.kernel_stats[1], args.out)
    if args.append is not None:
        with open(args.out, "a") as f:
            for path in args.append:
                f.write(open(path).read().rstrip("\n") + "\n")
        return
    import torch

    import realtime_urdf_filter_amd as R
    from bench_support import scene_check as SC
    from bench_support import workloads as WL
    from oracle import bindings as O

    n = args.streams
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# python scripts/scene_rate.py (%d VGA streams of c3, device planes, %d rounds of %d timed steps per leg, %d warm-up); one MI355X"
        % (n, args.rounds, args.steps, args.warmup))
    wl = WL.pr2_workload(n, W, H, total_triangles=args.triangles)
    dev = torch.device("cuda:0")
    depth = wl.depth_batch().astype(np.float32)
    depth_mm = np.clip(np.rint(np.nan_to_num(depth, nan=0.0, posinf=65.535, neginf=0.0) * 1000.0), 0, 65535).astype(np.uint16)
    d_depth = torch.from_numpy(depth).to(dev)
    d_depth_mm = torch.from_numpy(depth_mm.view(np.int16)).to(dev)
    cap = W * H
    words = H * ((W + 31) // 32)
    sets = [dict(masked=torch.empty((n, H, W), dtype=torch.float32, device=dev), masked_mm=torch.empty((n, H, W), dtype=torch.int16, device=dev),
                 mask=torch.empty((n, H, W), dtype=torch.uint8, device=dev), bits=torch.empty((n, words), dtype=torch.int32, device=dev),
                 points=torch.empty((n, cap, 3), dtype=torch.float32, device=dev), index=torch.empty((n, cap), dtype=torch.int32, device=dev),
                 counts=torch.empty((n,), dtype=torch.int32, device=dev)) for _ in range(2)]
    margins = np.tile(np.array([[ABS_M, REL]], np.float32), (n, 1))
    rep = torch.tensor(wl.replace_value, dtype=torch.float32, device=dev)
    d_scene = torch.empty((n, H, W), dtype=torch.float32, device=dev)

    def today(o):
        """The torch ops of a caller without the feature, on the filter's masked plane and mask: the same planes."""
        thr = d_scene - (ABS_M + REL * d_scene)
        sf = d_depth > thr
        return torch.where(sf, rep, o["masked"]), torch.where(sf, torch.tensor(255, dtype=torch.uint8, device=dev), o["mask"])

    results = []
    for lanes in (1, 0):
        p = R.default_params()
        p.filter_replace_value, p.depth_distance_threshold = wl.replace_value, wl.max_diff
        p.raster_lanes = lanes
        ctx = R.Context(W, H, n, 0, p)
        ids = wl.load_into(ctx)
        wl.stage(ctx, ids)
        ctx.set_cloud_intrinsics(0, [(525.0, 525.0, 319.5, 239.5)] * n)
        ctx.filter_batch_device(n, d_depth.data_ptr(), sets[0]["masked"].data_ptr(), sets[0]["mask"].data_ptr())      # (the first batch sizes the tile bins)
        ctx.sync()
        bytes_before = ctx.stats()["device_bytes"]
        ctx.learn_scene_batch_device(n, d_depth.data_ptr())
        ctx.get_scene_planes_device(0, n, d_scene.data_ptr())
        scene_bytes = ctx.stats()["device_bytes"] - bytes_before
        state = {"scene": None, "two": None}

        def configure(scene, two):
            if state["two"] != two:
                q = R.Params.from_buffer_copy(p)
                q.flags = (p.flags | R.FLAG_TWO_KERNEL) if two else p.flags
                ctx.set_params(q)
                state["two"] = two
            if state["scene"] != scene:
                ctx.set_scene_margins(0, margins if scene else None, n=n)
                state["scene"] = scene

        last = {}

        def submit(what, k):
            o = sets[k % 2]
            if what in ("plain", "+scene f32", "two-kernel", "today"):
                ctx.filter_batch_device(n, d_depth.data_ptr(), o["masked"].data_ptr(), o["mask"].data_ptr())
                if what == "today":
                    ctx.order_stream_after_batches(torch.cuda.current_stream().cuda_stream)
                    last["today"] = today(o)
            elif what == "+scene 16UC1":
                ctx.filter_batch_device_u16(n, d_depth_mm.data_ptr(), o["masked_mm"].data_ptr(), o["mask"].data_ptr())
            elif what.startswith("bits"):
                ctx.filter_batch_device_bits(n, d_depth.data_ptr(), o["bits"].data_ptr())
            else:
                ctx.cloud_compact_batch_device(n, d_depth.data_ptr(), o["points"].data_ptr(), o["index"].data_ptr(), o["counts"].data_ptr(), cap)

        def finish():
            ctx.sync()
            torch.cuda.synchronize()

        frames = {i: 0 for i in range(len(LEGS))}
        seconds = {i: 0.0 for i in range(len(LEGS))}
        per_round = {i: [] for i in range(len(LEGS))}
        kept = {}
        for rnd in range(args.rounds):
            for i, what in enumerate(LEGS):
                configure("+scene" in what or what.endswith("+scene"), what == "two-kernel")
                for k in range(args.warmup):
                    submit(what, k)
                finish()
                t = time.perf_counter()
                for k in range(args.steps):
                    submit(what, k)
                finish()
                el = time.perf_counter() - t
                frames[i] += n * args.steps
                seconds[i] += el
                per_round[i].append(n * args.steps / el)
                if rnd == args.rounds - 1 and not args.no_check:            # the last batch of the leg's last round, for the check below
                    o = sets[(args.steps - 1) % 2]
                    if what == "plain" and "plain" not in kept:
                        kept["plain"] = (o["masked"].cpu().numpy(), o["mask"].cpu().numpy())
                    elif what == "+scene f32":
                        kept[what] = (o["masked"].cpu().numpy(), o["mask"].cpu().numpy())
                    elif what == "+scene 16UC1":
                        kept[what] = (o["masked_mm"].cpu().numpy().view(np.uint16), o["mask"].cpu().numpy())
                    elif what == "bits+scene":
                        kept[what] = o["bits"].cpu().numpy().view(np.uint32)
                    elif what == "today":
                        kept[what] = tuple(a.cpu().numpy() for a in last["today"])
                last.clear()
        st = ctx.stats()
        scene_host = d_scene.cpu().numpy()
        bad = {}
        share = float((d_depth > (d_scene - (ABS_M + REL * d_scene))).float().mean())
        say("# run " + json.dumps({"streams": n, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "share": round(share, 4)}))
        if not args.no_check:
            rm, rk = kept["plain"]
            # the robot filter's own planes: a sample against the CPU oracle
            sample = sorted(set(np.linspace(0, n - 1, min(n, args.checked)).astype(int).tolist()))
            prep = [O.PreparedFrame(depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], max_diff=wl.max_diff, replace_value=wl.replace_value)
                    for s in sample]
            O.run_prepared(prep, max(1, min(16, len(os.sched_getaffinity(0)))))
            bad["plain vs oracle (%d streams)" % len(sample)] = sum(int((f.mask != rk[s]).sum()) + int((f.masked.view(np.uint32) != rm[s].view(np.uint32)).sum())
                                                                     for s, f in zip(sample, prep))
            want_scene = SC.learned(np.full((n, H, W), np.inf, np.float32), depth, rk)
            bad["learned planes"] = int((want_scene.view(np.uint32) != scene_host.view(np.uint32)).sum())
            em, ek = SC.expected(rm, rk, depth, scene_host, margins, wl.replace_value)
            gm, gk = kept["+scene f32"]
            bad["+scene f32"] = int((gm.view(np.uint32) != em.view(np.uint32)).sum()) + int((gk != ek).sum())
            tm, tk = kept["today"]
            bad["today"] = int((tm.view(np.uint32) != em.view(np.uint32)).sum()) + int((tk != ek).sum())
            gb = kept["bits+scene"]
            bits_want = np.packbits(ek > 0, axis=-1, bitorder="little").reshape(n, -1).view("<u4")
            bad["bits+scene"] = int((gb != bits_want).sum())
            # 16UC1: the robot's planes on the millimetre sensor are the f32 ones wherever the sensor is a whole millimetre
            # multiple; they are not in general, so the 16UC1 leg is held against the definition on ITS robot mask, read from the
            # batch itself where the scene does not filter, and must agree with the scene's verdict everywhere it does
            g16, k16 = kept["+scene 16UC1"]
            sens16 = SC.sensor_metres(depth, True)
            sf16 = SC.scene_filtered(sens16, scene_host, ABS_M, REL)
            rep16 = int(np.clip(np.rint(wl.replace_value * 1000.0), 0, 65535))
            bad["+scene 16UC1 (scene pixels)"] = int((k16[sf16] != 255).sum()) + int((g16[sf16] != rep16).sum())
            bad["+scene 16UC1 (kept pixels)"] = int((g16[k16 == 0] != depth_mm[k16 == 0]).sum())
            bad["+scene 16UC1 (filtered pixels)"] = int((g16[k16 == 255] != rep16).sum()) + int(((k16 != 0) & (k16 != 255)).sum())
        for i, what in enumerate(LEGS):
            row = {"raster_lanes": st["raster_lanes"], "leg": i, "batch": what, "frames_per_s": round(frames[i] / seconds[i], 1),
                   "per_round": [round(v) for v in per_round[i]], "launch_groups": st["groups_last_batch"]}
            results.append(row)
            say(json.dumps(row))
        say("# lanes %d: scene planes + streams' table + learning scratch %.1f MB; scene-filtered share of all pixels %s; mismatches %s"
            % (st["raster_lanes"], scene_bytes / 1e6, "%.3f" % share, json.dumps(bad)))
        if any(bad.values()):
            raise SystemExit("lanes %d: the last batch differs from the expectation: %s" % (lanes, bad))
        ctx.close()
    say("# frames/s per lane setting; spread = (max - min) / mean over the plain legs of every round:")
    summary = []
    for lanes in sorted(set(r["raster_lanes"] for r in results)):
        rs = [r for r in results if r["raster_lanes"] == lanes]
        plain = [v for r in rs if r["batch"] == "plain" for v in r["per_round"]]
        pmean = sum(plain) / len(plain)
        spread = (max(plain) - min(plain)) / pmean
        by = {r["batch"]: r["frames_per_s"] for r in rs if r["batch"] != "plain"}
        say("#   lanes %d  plain legs %s: mean %.0f, spread %.3f" % (lanes, " ".join("%.0f" % v for v in plain), pmean, spread))
        say("#   lanes %d  +scene f32 %.0f (%.3f of plain), 16UC1 %.0f; today (filter + torch) %.0f (+scene is %.2f x); bits %.0f -> +scene %.0f (%.3f); "
            "compacted cloud %.0f -> +scene %.0f (%.3f); two-kernel %.0f"
            % (lanes, by["+scene f32"], by["+scene f32"] / pmean, by["+scene 16UC1"], by["today"], by["+scene f32"] / by["today"], by["bits"], by["bits+scene"],
               by["bits+scene"] / by["bits"], by["cloud"], by["cloud+scene"], by["cloud+scene"] / by["cloud"], by["two-kernel"]))
        summary.append("%d lane(s): plain %.0f (spread %.3f), +scene %.0f (%.2f of plain, %.1f x filter + torch), bits %.0f -> %.0f, compacted cloud %.0f -> %.0f"
                       % (lanes, pmean, spread, by["+scene f32"], by["+scene f32"] / pmean, by["+scene f32"] / by["today"], by["bits"], by["bits+scene"], by["cloud"],
                          by["cloud+scene"]))
    say("# c3 frames/s with a learned scene in effect, " + "; ".join(summary))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
