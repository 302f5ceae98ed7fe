#!/bin/bash
# Which wave of a workgroup does the work, and on which SIMD it runs: setup_kernel and tile_kernel<fused> on one C3 batch,
# counted by the instrumented library of scripts/lane_util.sh (-DRTUF_LANECOUNT -DRTUF_COUNT; never the product).
#   - per kernel, two 4 x 4 tables of the waves started: wave index (threadIdx.x >> 6, modulo 4) against hardware SIMD, over the
#     whole chip and on a single CU
#   - per instrumented loop, the trips that had a live lane, by wave index
#   usage (GPU box): scripts/wave_roles.sh >> profiles/wave_roles_c3.txt
#   (rebuilt unless LANE_LIB names an instrumented library built beforehand; LANE_FLAGS adds -D switches, as in lane_util.sh)
here="$(cd "$(dirname "$0")/.." && pwd)"
lib=$here/realtime_urdf_filter_amd/lib/variants/librtuf_lanes.so
if [ -n "$LANE_LIB" ]; then lib=$LANE_LIB; else
(cd $here/realtime_urdf_filter_amd/csrc && mkdir -p ../lib/variants && hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -I../../include -I. \
   -Wno-unused-value -Wno-unused-result -DRTUF_LANECOUNT -DRTUF_COUNT $LANE_FLAGS rtuf_kernels.hip rtuf_api.cpp -o $lib) || exit 1
fi
cd $here && RTUF_LIB=$lib python - "$@" <<'PY'
import ctypes, os, sys
sys.path.insert(0, os.getcwd())
import torch
import realtime_urdf_filter_amd as R
from realtime_urdf_filter_amd import _capi
from bench_support import configs as CF
LOOPS = 48; TABLES = 2
NAMES = {0: "tile: record load+unpack", 1: "tile: lane-walk quad trips", 3: "tile: quarter-wave pair trips", 5: "tile: whole-wave pair trips",
         7: "tile: parked (workgroup) trips", 9: "tile: fragment list", 10: "tile: resolve passes",
         11: "setup: phase 1 vertices", 12: "setup: phase 2 triangles", 13: "setup: small boxes (coverage)", 15: "setup: fragment store loop",
         16: "setup: fragment group-finding trips", 17: "setup: records (set-up)", 19: "setup: record tile trips", 20: "setup: record group-finding trips"}
TABLE_NAMES = ["wave index x SIMD, whole chip", "wave index x SIMD, one CU (the one the first wave ran on)"]
lib = _capi.load_library()
lib.rtuf_debug_wave_roles.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
lib.rtuf_debug_wave_roles.restype = ctypes.c_int
share = CF.build("c3", 1, 0)
n, W, H = share.n, share.width, share.height
p = R.default_params(); p.filter_replace_value = share.wl0.replace_value; p.depth_distance_threshold = share.wl0.max_diff
p.raster_lanes = 1
ctx = R.Context(W, H, n, 0, p)
share.load(ctx)
dev = torch.device("cuda:0")
d = torch.from_numpy(share.depth_host(0)).to(dev)
m = torch.empty((n, H, W), dtype=torch.float32, device=dev); k = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
for step in (0, 1, 2):
    share.stage(ctx, step)
    ctx.filter_batch_device(n, d.data_ptr(), m.data_ptr(), k.data_ptr()); ctx.sync()
words = (ctypes.c_uint64 * (4 * LOOPS + 2 * TABLES * 16 + 2))()
lib.rtuf_debug_wave_roles(ctx._h, words, len(words))
print("C3 (%d streams %dx%d), one batch, one raster lane; flags: %s" % (n, W, H, os.environ.get("LANE_FLAGS", "(none)")))
for kern, kname in enumerate(("setup_kernel", "tile_kernel<fused>")):
    for t in range(TABLES):
        tab = [[int(words[4 * LOOPS + (kern * TABLES + t) * 16 + r * 4 + s]) for s in range(4)] for r in range(4)]
        tot = sum(map(sum, tab)) or 1
        worst = max(abs(16.0 * v / tot - 1.0) for row in tab for v in row)
        print("%s, waves started, %s (largest deviation from equal shares: %.1f %%)" % (kname, TABLE_NAMES[t], 100 * worst))
        print("            SIMD 0      SIMD 1      SIMD 2      SIMD 3")
        for r in range(4):
            print("  %d  " % r + "".join("%12d" % v for v in tab[r]))
print("trips with a live lane, by wave index (threadIdx.x >> 6, modulo 4)")
print("  %-40s %11s %11s %11s %11s   relative to wave 0" % ("loop", "wave 0", "wave 1", "wave 2", "wave 3"))
for i in sorted(NAMES):
    row = [int(words[4 * i + r]) for r in range(4)]
    if sum(row):
        print("  %-40s" % NAMES[i] + "".join(" %11d" % v for v in row) + "   " + " ".join("%.2f" % (v / max(row[0], 1)) for v in row))
ctx.close()
PY
