"""Frames/s of the link clearance tables (rtuf_link_clearance_batch_device) on the c3 workload: 256 VGA streams of the
250 k-triangle PR2-like robot, device-resident planes, spheres from geometry.bounding_spheres of every draw (segments 1 and
4), one raster lane and the default lanes, all legs from the same run:
  (a) the mask-bits device batch the clearance batch is built on (three legs per lane setting: their spread is the
      run-to-run spread everything else is read against);
  (b) clearance batches at max_distance 0.25 m and +inf;
  (c) what a caller does today: rtuf_cloud_compact_batch_device, then per stream torch ops -- the pairwise distances of the
      kept points to the posed centres minus the radii, the per-label minimum and the count of points within max_distance
      (fewer steps: it is slow).  Its clearance and points_within are checked against the same expectation.
A sample of the last batch's streams is checked against bench_support/clearance_check.py on the CPU oracle's mask for
equality; a mismatch of a clearance leg fails.  The lines go to stdout and to --out.

usage: python scripts/clearance_rate.py [--streams 256] [--steps 20] [--warmup 5] [--out profiles/clearance_rate_c3.txt]"""
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
from bench_support import clearance_check as KC  # noqa: E402
from bench_support import cloud_check as CC  # noqa: E402
from bench_support import workloads as WL  # noqa: E402
from oracle import bindings as O  # noqa: E402
from realtime_urdf_filter_amd.geometry import bounding_spheres  # noqa: E402

INTR = (525.0, 525.0, 319.5, 239.5)
LEGS = ("bits", "clearance 0.25", "clearance inf", "bits", "today 0.25", "today inf", "bits")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--today-steps", type=int, default=2)
    ap.add_argument("--checked", type=int, default=2, help="streams of the last batch held against the expectation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance_rate_c3.txt"))
    args = ap.parse_args()
    n, W, H = args.streams, 640, 480
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# python scripts/clearance_rate.py (%d VGA streams of c3, device planes, %d timed steps, %d warm-up; torch legs %d steps); one MI355X"
        % (n, args.steps, args.warmup, args.today_steps))
    wl = WL.pr2_workload(n, W, H, total_triangles=args.triangles)
    dev = torch.device("cuda:0")
    depth = wl.depth_batch().astype(np.float32)
    d_depth = torch.from_numpy(depth).to(dev)
    n_links = sum(len(m) for m in wl.models)
    n_labels = n_links + 1
    link_tf = np.concatenate([tf for tf in wl.link_tf if tf.shape[1]], axis=1)      # [n, links, 16]
    sample = sorted(set(np.linspace(0, n - 1, min(n, args.checked)).astype(int).tolist()))
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    frames = [O.PreparedFrame(depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], max_diff=wl.max_diff,
                              replace_value=wl.replace_value) for s in sample]
    O.run_prepared(frames, threads)
    kept = [CC.compacted(depth[s], f.mask, INTR) for s, f in zip(sample, frames)]
    sets = [dict(bits=torch.empty((n, H * ((W + 31) // 32)), dtype=torch.int32, device=dev), table=torch.empty((n, n_labels, 4), dtype=torch.int32, device=dev),
                 points=torch.empty((n, W * H, 3), dtype=torch.float32, device=dev), counts=torch.empty((n,), dtype=torch.int32, device=dev)) for _ in range(2)]
    results = []
    for segments in (1, 4):
        spheres, base = [], 0                      # (model, link in model, global link, xyzr)
        for m, links in enumerate(wl.models):
            for li, draws in enumerate(links):
                for d in draws:
                    # (the spheres live in the link's frame: the draw's glScalef / glTranslatef applied to its vertices)
                    v = np.asarray(d.verts, np.float64)
                    v = v * np.asarray(d.op) if d.pre_op == R.OP_SCALE else (v + np.asarray(d.op) if d.pre_op == R.OP_TRANSLATE else v)
                    spheres += [(m, li, base + li, q) for q in bounding_spheres(v, segments)]
            base += len(links)
        assert len(spheres) <= 4096 and n_links <= 256, (len(spheres), n_links)      # (the context's limits: spheres, distinct labels)
        glob = np.array([q[2] for q in spheres])
        xyzr = np.array([q[3] for q in spheres], np.float32)
        labels = glob + 1
        want = {}
        for dist in (0.25, np.inf):
            want[dist] = [KC.table(kept[i][0], kept[i][1], KC.posed(link_tf[s], wl.cam_tf[s], wl.offset_inv[s], glob, xyzr[:, :3]), xyzr[:, 3], labels,
                                   np.arange(len(spheres)), n_labels, dist) for i, s in enumerate(sample)]
        centres_all = torch.from_numpy(np.stack([KC.posed(link_tf[s], wl.cam_tf[s], wl.offset_inv[s], glob, xyzr[:, :3]) for s in range(n)])).to(dev)
        t_r = torch.from_numpy(xyzr[:, 3].copy()).to(dev)
        t_lab = torch.from_numpy(labels.astype(np.int64)).to(dev)
        for lanes in (1, 0):
            p = R.default_params()
            p.filter_replace_value, p.depth_distance_threshold = wl.replace_value, wl.max_diff
            p.raster_lanes = lanes
            ctx = R.Context(W, H, n, 0, p)
            ids = wl.load_into(ctx)
            wl.stage(ctx, ids)
            ctx.set_cloud_intrinsics(0, [INTR] * n)
            for m in ids:
                mine = [q for q in spheres if q[0] == m]
                ctx.set_link_spheres(m, [q[1] for q in mine], [q[3] for q in mine])
            for what in LEGS:
                dist = np.inf if what.endswith("inf") else 0.25
                last = {}

                def today(o):
                    """Per stream: pairwise clearances [kept, spheres], minimum and count per label (row 0: all labels)."""
                    counts = o["counts"].cpu()
                    out_c = torch.full((n, n_labels), float("inf"), device=dev)
                    out_n = torch.zeros((n, n_labels), dtype=torch.int64, device=dev)
                    for s in range(n):
                        pts = o["points"][s, :int(counts[s])]
                        if not pts.shape[0]:
                            continue
                        d = pts[:, None, :] - centres_all[s][None, :, :]
                        c = torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) - t_r[None, :]
                        inside = c < dist
                        cm = torch.where(inside, c, torch.full_like(c, float("inf")))
                        out_c[s].scatter_reduce_(0, t_lab, cm.min(dim=0).values, "amin")
                        out_c[s, 0] = cm.min()
                        per = torch.zeros((pts.shape[0], n_labels), dtype=torch.int32, device=dev).index_add_(1, t_lab, inside.to(torch.int32))
                        out_n[s] = (per > 0).sum(dim=0)
                        out_n[s, 0] = inside.any(dim=1).sum()
                    return out_c, out_n

                def submit(k):
                    o = sets[k % 2]
                    if what == "bits":
                        ctx.filter_batch_device_bits(n, d_depth.data_ptr(), o["bits"].data_ptr())
                    elif what.startswith("clearance"):
                        ctx.link_clearance_batch_device(n, d_depth.data_ptr(), o["table"].data_ptr(), n_labels, dist)
                    else:
                        ctx.cloud_compact_batch_device(n, d_depth.data_ptr(), o["points"].data_ptr(), None, o["counts"].data_ptr(), W * H)
                        ctx.order_stream_after_batches(torch.cuda.current_stream().cuda_stream)
                        last["out"] = today(o)

                def finish():
                    ctx.sync()
                    torch.cuda.synchronize()

                steps = args.today_steps if what.startswith("today") else args.steps
                for k in range(1 if what.startswith("today") else args.warmup):
                    submit(k)
                finish()
                t = time.perf_counter()
                for k in range(steps):
                    submit(k)
                finish()
                el = time.perf_counter() - t
                bad = 0
                if what.startswith("clearance"):
                    got = sets[(steps - 1) % 2]["table"][sample].cpu().numpy().view(np.uint32)
                    bad = sum(int((got[i] != want[dist][i].view(np.uint32).reshape(n_labels, 4)).any(axis=1).sum()) for i in range(len(sample)))
                elif what.startswith("today"):
                    tc, tn = last["out"]
                    for i, s in enumerate(sample):
                        bad += int((tc[s].cpu().numpy() != want[dist][i]["clearance"]).sum()) + int((tn[s].cpu().numpy() != want[dist][i]["points_within"]).sum())
                last.clear()
                st = ctx.stats()
                row = {"segments": segments, "spheres": len(spheres), "raster_lanes": st["raster_lanes"], "batch": what, "frames_per_s": round(n * steps / el, 1),
                       "batch_ms": round(1e3 * el / steps, 3), "steps": steps, "frames_checked": len(sample), "mismatched_rows": bad}
                results.append(row)
                say(json.dumps(row))
                if bad and what.startswith("clearance"):
                    raise SystemExit("segments %d lanes %d %s: the last batch differs from the expectation" % (segments, lanes, what))
            ctx.close()
    say("# frames/s; spread = (max - min) / mean of the mask-bits legs of the same context:")
    for segments in (1, 4):
        for lanes in sorted(set(r["raster_lanes"] for r in results)):
            rs = [r for r in results if r["raster_lanes"] == lanes and r["segments"] == segments]
            b = [r["frames_per_s"] for r in rs if r["batch"] == "bits"]
            bm = sum(b) / len(b)
            f = {r["batch"]: r["frames_per_s"] for r in rs}
            say("#   segments %d (%d spheres) lanes %d: bits %s (spread %.3f); clearance 0.25 m %.0f = %.3f of bits, %.1f x torch (%.0f); +inf %.0f = %.3f of bits, %.1f x torch (%.0f)"
                % (segments, rs[0]["spheres"], lanes, " ".join("%.0f" % v for v in b), (max(b) - min(b)) / bm, f["clearance 0.25"], f["clearance 0.25"] / bm,
                   f["clearance 0.25"] / f["today 0.25"], f["today 0.25"], f["clearance inf"], f["clearance inf"] / bm, f["clearance inf"] / f["today inf"], f["today inf"]))
    def ratio(segments, lanes, leg, over):
        rs = {r["batch"]: r["frames_per_s"] for r in results if r["raster_lanes"] == lanes and r["segments"] == segments and r["batch"] != "bits"}
        b = [r["frames_per_s"] for r in results if r["raster_lanes"] == lanes and r["segments"] == segments and r["batch"] == "bits"]
        return rs[leg] / (sum(b) / len(b) if over == "bits" else rs[over])
    lanes_all = sorted(set(r["raster_lanes"] for r in results))
    say("# c3 frames/s of a clearance batch: " + "; ".join(
        "%d segment(s), %d lane(s): 0.25 m %.2f of bits, %.0f x torch; +inf %.2f of bits, %.0f x torch"
        % (sg, ln, ratio(sg, ln, "clearance 0.25", "bits"), ratio(sg, ln, "clearance 0.25", "today 0.25"), ratio(sg, ln, "clearance inf", "bits"),
           ratio(sg, ln, "clearance inf", "today inf")) for sg in (1, 4) for ln in lanes_all))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
