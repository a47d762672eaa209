#!/bin/bash
# tools/class_signature_cost.sh [out dir]: the numbers of DESIGN.md's class-signature section -- one rocprofv3 kernel trace
# (no counters) per batch shape for the kernels' durations, then the same shapes without the profiler for the calls' wall
# times: the crawler's 512 one-second files, and 1 000 two-second files.  Every GPU step has its own time limit and the
# chain stops at the first step that fails.
set -u
cd "$(dirname "$0")/.."
OUT=${1:-${TMPDIR:-/tmp}/class_signature_cost}
mkdir -p "$OUT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/files512x1s" -o p -- python3 tools/class_signature_cost.py worker 512 1 > "$OUT/files512x1s.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/files1000x2s" -o p -- python3 tools/class_signature_cost.py worker 1000 2 > "$OUT/files1000x2s.json" &&
python3 tools/class_signature_cost.py report "$OUT" &&
echo "# wall times without the profiler:" &&
timeout -k 10 300 python3 tools/class_signature_cost.py worker 512 1 &&
timeout -k 10 300 python3 tools/class_signature_cost.py worker 1000 2
