#!/bin/bash
# tools/devio_file_cost.sh [out dir]: the numbers of DESIGN.md 4.23 -- one rocprofv3 kernel trace (no counters) of the worker
# for the durations of devio_file_export_kernel (512 one-second files, AFX_D_HIGH_LEVEL_INPUTS | AFX_D_CLASSIFICATION_INPUTS),
# their share of the rate a device copy reaches, then the same worker without the profiler for the HIP-event brackets of the
# host fetches beside the device export.  Every GPU step has its own time limit and the chain stops at the first step that fails.
set -u
cd "$(dirname "$0")/.."
OUT=${1:-${TMPDIR:-/tmp}/devio_file_cost}
mkdir -p "$OUT"
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -o p -- python3 tools/devio_file_cost.py worker 512 1 > "$OUT/worker_traced.json" &&
python3 tools/devio_file_cost.py report "$OUT/trace" "$OUT/worker_traced.json" | tee "$OUT/kernels.jsonl" &&
echo "# brackets without the profiler:" &&
timeout -k 10 200 python3 tools/devio_file_cost.py worker 512 1 | tee "$OUT/worker.json"
