#!/bin/bash
# tools/rawpcm_cost.sh [out dir]: the numbers of DESIGN.md 4.18 -- one rocprofv3 kernel trace (no counters) per batch shape
# for raw_native_kernel's duration (512 one-second stereo I16_BE files, 1 000 two-second stereo I24_BE files), then the same
# shapes without the profiler for afx_batch_create_from_raw's wall time, foreign against native twin, then the C4-share crawl
# as WAV and as AIFF.  Every GPU step has its own time limit and the chain stops at the first step that fails.
set -u
cd "$(dirname "$0")/.."
OUT=${1:-${TMPDIR:-/tmp}/rawpcm_cost}
mkdir -p "$OUT"
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/i16_512x1s" -o p -- python3 tools/rawpcm_cost.py worker 512 1 i16 > "$OUT/i16_512x1s.json" &&
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/i24_1000x2s" -o p -- python3 tools/rawpcm_cost.py worker 1000 2 i24 > "$OUT/i24_1000x2s.json" &&
python3 tools/rawpcm_cost.py report "$OUT" &&
echo "# wall times without the profiler:" &&
timeout -k 10 200 python3 tools/rawpcm_cost.py worker 512 1 i16 &&
timeout -k 10 200 python3 tools/rawpcm_cost.py worker 1000 2 i24 &&
echo "# crawl, WAV beside AIFF:" &&
timeout -k 10 300 python3 tools/rawpcm_cost.py crawl 12500
