"""Frames/s of the voxel occupancy grid inserts (rtuf_voxel_insert_batch_device) on the c3 workload: 256 VGA streams of the
250 k-triangle PR2-like robot, device-resident planes, ONE grid of 2 cm voxels over the workload's reach -- 200 x 150 x 200 =
6.0 M voxels from (-2.0, -1.5, 0.3): every camera looks into the same frustum, each rolled and shifted a little by a transform
of its own, so all 256 streams hit the same voxels: the contended case.  With and without counts, one raster lane and the
default lanes, against the yardsticks of the same run:
  (a) the plain mask-bits device batch, asynchronous as callers run it: the ceiling, since the insert contains it;
  (a') the same batch with a sync after every batch: what the insert's synchronous order alone costs;
  (b) what a caller does today: rtuf_cloud_compact_batch_device, then torch ops that give the same count tensor -- the transform
      chain, the subtract and multiply, the range test, the index and one bincount over all streams.
A cycle of an insert leg is clear -> insert, as a mapper runs it; a cycle of (b) builds its count tensor from nothing.  Every leg
runs `--rounds` times; spread = (max - min) / mean of a leg's rounds.  The grid of each insert leg's last cycle and the count
tensor of each (b) leg's last cycle are held against bench_support/voxel_check.py on the CPU oracle's masks of EVERY stream,
for equality; a mismatch fails.  The kernel's own time is what a cycle takes beyond (a'): the clear and the insert kernel.

usage: python scripts/voxel_rate.py [--streams 256] [--steps 20] [--warmup 4] [--rounds 3] [--out profiles/voxel_rate_c3.txt]"""
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
from bench_support import voxel_check as VC  # noqa: E402
from bench_support import workloads as WL  # noqa: E402
from oracle import bindings as O  # noqa: E402

FX, FY, CX, CY = 525.0, 525.0, 319.5, 239.5
GRID = VC.Grid((-2.0, -1.5, 0.3), 0.02, (200, 150, 200))
LEGS = ("bits", "bits synced", "today", "insert counts", "insert bits only")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_rate_c3.txt"))
    args = ap.parse_args()
    n, W, H = args.streams, 640, 480
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# python scripts/voxel_rate.py (%d VGA streams of c3, device planes, grid %d x %d x %d voxels of %g m from %s, %d rounds of %d timed cycles per leg, "
        "%d warm-up); one MI355X" % ((n,) + GRID.dims + (GRID.voxel_size, GRID.origin, args.rounds, args.steps, args.warmup)))
    wl = WL.pr2_workload(n, W, H, total_triangles=args.triangles)
    dev = torch.device("cuda:0")
    depth = wl.depth_batch().astype(np.float32)
    d_depth = torch.from_numpy(depth).to(dev)
    cap = W * H
    matrices = [VC.rotation_z(0.05 * ((s % 13) - 6), (0.01 * (s % 7), -0.01 * (s % 5), 0.0)) for s in range(n)]

    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    t0 = time.perf_counter()
    frames = [O.PreparedFrame(depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], max_diff=wl.max_diff,
                              replace_value=wl.replace_value) for s in range(n)]
    O.run_prepared(frames, threads)
    want_bits, want_counts, want_summary = VC.expected_planes(depth, [f.mask for f in frames], [(FX, FY, CX, CY)] * n, matrices, GRID)
    del frames
    say("# oracle masks and the expected grid of all %d streams: %.1f s on %d threads; per stream %d .. %d inserted, %d .. %d outside the grid, "
        "%d .. %d not kept; %d voxels occupied, largest count %d"
        % ((n, time.perf_counter() - t0, threads) + tuple(int(f(want_summary[:, k])) for k in range(3) for f in (np.min, np.max))
           + (int((want_counts > 0).sum()), int(want_counts.max()))))
    assert (want_summary[:, :3] > 0).all()

    # (b)'s inputs: the 12 used matrix entries, the grid's origin and inv as float32 tensors
    m = torch.from_numpy(np.stack(matrices).astype(np.float32)).to(dev)          # [n,16] column-major
    o, inv = GRID.stored()
    o_t, inv_t = torch.from_numpy(o).to(dev), float(inv)
    nx, ny, nz = GRID.dims
    pts = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    bits_out = [torch.empty((n, H * ((W + 31) // 32)), dtype=torch.int32, device=dev) for _ in range(2)]
    lane_of_cap = torch.arange(cap, device=dev).view(1, cap)

    def today():
        """The torch ops of a caller without the voxel calls, on the compacted cloud: -> counts [n_voxels] int64."""
        x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
        w = [((m[:, r, None] * x + m[:, 4 + r, None] * y) + m[:, 8 + r, None] * z) + m[:, 12 + r, None] for r in range(3)]
        g = [(w[r] - o_t[r]) * inv_t for r in range(3)]
        inside = (lane_of_cap < cnt.view(n, 1)) & (g[0] >= 0) & (g[0] < nx) & (g[1] >= 0) & (g[1] < ny) & (g[2] >= 0) & (g[2] < nz)
        idx = (g[2][inside].long() * ny + g[1][inside].long()) * nx + g[0][inside].long()
        return torch.bincount(idx, minlength=GRID.n_voxels)

    results = []
    for lanes in (1, 0):
        p = R.default_params()
        p.filter_replace_value, p.depth_distance_threshold = wl.replace_value, wl.max_diff
        p.raster_lanes = lanes
        ctx = R.Context(W, H, n, 0, p)
        ids = wl.load_into(ctx)
        wl.stage(ctx, ids)
        ctx.set_cloud_intrinsics(0, [(FX, FY, CX, CY)] * n)
        ctx.set_voxel_transforms(0, np.stack(matrices))
        for rnd in range(args.rounds):
            for what in LEGS:
                last = {}
                if what.startswith("insert"):
                    ctx.set_voxel_grid(GRID.origin, GRID.voxel_size, GRID.dims, what == "insert counts")

                def cycle(k):
                    if what == "bits" or what == "bits synced":
                        ctx.filter_batch_device_bits(n, d_depth.data_ptr(), bits_out[k % 2].data_ptr())
                        if what == "bits synced":
                            ctx.sync()
                    elif what == "today":
                        ctx.cloud_compact_batch_device(n, d_depth.data_ptr(), pts.data_ptr(), None, cnt.data_ptr(), cap)
                        ctx.order_stream_after_batches(torch.cuda.current_stream().cuda_stream)
                        last["counts"] = today()
                    else:
                        ctx.voxel_clear()
                        ctx.voxel_insert_batch_device(n, d_depth.data_ptr(), None)

                def finish():
                    ctx.sync()
                    torch.cuda.synchronize()

                for k in range(args.warmup):
                    cycle(k)
                finish()
                t = time.perf_counter()
                for k in range(args.steps):
                    cycle(k)
                finish()
                el = time.perf_counter() - t
                bad = 0
                if what == "today":
                    bad = int((last["counts"].cpu().numpy() != want_counts.astype(np.int64)).sum())
                elif what.startswith("insert"):
                    got_bits, got_counts = ctx.voxel_grid()
                    bad = int((got_bits != want_bits).sum()) + (int((got_counts.reshape(-1) != want_counts).sum()) if got_counts is not None else 0)
                last.clear()
                st = ctx.stats()
                row = {"raster_lanes": st["raster_lanes"], "round": rnd, "leg": what, "frames_per_s": round(n * args.steps / el, 1),
                       "cycle_ms": round(1e3 * el / args.steps, 3), "launch_groups": st["groups_last_batch"], "streams_checked": n if what in LEGS[2:] else 0,
                       "mismatches": bad}
                results.append(row)
                say(json.dumps(row))
                if bad:
                    raise SystemExit("lanes %d %s: the last cycle differs from the expectation" % (lanes, what))
        ctx.set_voxel_grid(None, 0.0, None)
        ctx.close()
    say("# frames/s per lane setting; spread = (max - min) / mean of a leg's rounds:")
    summary = []
    ok = True
    for lanes in sorted(set(r["raster_lanes"] for r in results)):
        stat = {}
        for what in LEGS:
            f = [r["frames_per_s"] for r in results if r["raster_lanes"] == lanes and r["leg"] == what]
            ms = [r["cycle_ms"] for r in results if r["raster_lanes"] == lanes and r["leg"] == what]
            stat[what] = (sum(f) / len(f), (max(f) - min(f)) / (sum(f) / len(f)), sum(ms) / len(ms))
            say("#   lanes %d  %-16s rounds %s  mean %.0f  spread %.3f  cycle %.3f ms" % (lanes, what, " ".join("%.0f" % v for v in f), stat[what][0], stat[what][1], stat[what][2]))
        px_bytes = n * W * H * (4.0 + 1.0 / 8.0)
        parts = []
        for what in LEGS[3:]:
            fps, spread, ms = stat[what]
            own_ms = ms - stat["bits synced"][2]
            beats = fps - stat["today"][0] > (spread + stat["today"][1]) * stat["today"][0]
            ok = ok and beats
            say("#   lanes %d  %s: %.3f of bits, %.3f of bits synced, %.2f x today (%s today by more than the two legs' spreads together, %.3f + %.3f); "
                "clear + insert kernel %.3f ms per cycle = %.2f TB/s of the sensor planes and mask bits it reads (compare_kernel: 4.96 TB/s of its 13 B/px on c3)"
                % (lanes, what, fps / stat["bits"][0], fps / stat["bits synced"][0], fps / stat["today"][0], "beats" if beats else "DOES NOT beat", spread,
                   stat["today"][1], own_ms, px_bytes / (own_ms * 1e-3) / 1e12 if own_ms > 0 else float("nan")))
            parts.append("%s %.0f (%.2f of bits, %.1f x today, spread %.3f, clear + kernel %.3f ms)" % (what, fps, fps / stat["bits"][0], fps / stat["today"][0], spread, own_ms))
        summary.append("%d lane(s): bits %.0f (spread %.3f), bits synced %.0f, today %.0f (spread %.3f), %s"
                       % (lanes, stat["bits"][0], stat["bits"][1], stat["bits synced"][0], stat["today"][0], stat["today"][1], ", ".join(parts)))
    say("# c3 frames/s, one 200 x 150 x 200 grid of 2 cm voxels, " + "; ".join(summary))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("an insert leg does not beat the torch baseline by more than the two legs' spreads together")


if __name__ == "__main__":
    main()
