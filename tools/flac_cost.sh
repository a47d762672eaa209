#!/bin/bash
# tools/flac_cost.sh [out dir] [pool cache .npz]: the numbers of DESIGN.md 4.19 -- one rocprofv3 kernel trace (no counters) of a
# 512-file batch for the three decode kernels' durations, then the same batch without the profiler for
# afx_batch_create_from_raw's wall time (FLAC against native twin) and the link rate, then the C4-share crawl as WAV and as
# FLAC, eight alternating rounds, with the workers' phase timers.  Every GPU step has its own time limit and the chain stops
# at the first step that fails.
set -u
cd "$(dirname "$0")/.."
OUT=${1:-${TMPDIR:-/tmp}/flac_cost}
CACHE=${2:-$OUT/pool.npz}
mkdir -p "$OUT"
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/flac_512x1s" -o p -- python3 tools/flac_cost.py worker 512 "$CACHE" > "$OUT/flac_512x1s.json" &&
python3 tools/flac_cost.py report "$OUT" &&
echo "# wall times without the profiler:" &&
timeout -k 10 200 python3 tools/flac_cost.py worker 512 "$CACHE" &&
echo "# crawl, WAV beside FLAC:" &&
AFEC_CRAWL_TIMING=1 timeout -k 10 400 python3 tools/flac_cost.py crawl 12500 8 "$CACHE"
