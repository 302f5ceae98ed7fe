#!/bin/bash
# Two trees on ONE box: bench lines of a checkout beside the working tree (e.g. `git worktree add .r05tree <round-5 commit>`,
# built there), alternating, so that box-to-box differences (this pool: up to 20 % on the tile kernel) cancel.
#   usage: scripts/same_box.sh .r05tree [bench args...]
here="$(cd "$(dirname "$0")/.." && pwd)"
other=$here/$1; shift
Q="--cpu-seconds 0 --host-copy-seconds 0 --min-seconds 3 --check-frames 8 --isolated-seconds 1.5 --other-configs off"
full() { grep -q '"--full"' "$1/bench.py" && echo --full; }      # (checkouts from before --full run every leg by default)
line() { python -c "
import sys,json
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); r=d.get('roofline') or {}
print('%9.0f frames/s  tile %.4f ms  mem %.2f GB  mismatches %s  %s' % (d['value'], r.get('avg_launch_ms', float('nan')), d['device_memory_bytes']/1e9, (d.get('parity') or {}).get('mismatching_values'), d.get('step_ms')))"; }
# one bench line of the tree in $2, under a time limit of its own; a leg that fails (or faults the GPU) ends the comparison there
set -o pipefail
leg() {
  printf "%-10s " "$1"; local dir=$2; shift 2
  (cd $dir && timeout -k 10 300 python bench.py $Q "$@" 2>/dev/null | line) || { echo "leg failed: stopping"; exit 1; }
}
for rep in 1 2; do
  leg other $other $(full $other) "$@"
  leg this $here --full "$@"
  leg this-v2 $here --full --variants 2 "$@"
done
