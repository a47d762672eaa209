#!/bin/bash
# tools/devio_raw_cost.sh [out dir]: the numbers of DESIGN.md 4.21 -- one rocprofv3 kernel trace (no counters) of the worker for
# the durations of devio_raw_gather_kernel (512 one-second stereo files: I16 aligned, I16 two bytes off, I24 one byte off, F32
# planar) and devio_samples_kernel, their share of the rate a device copy reaches; the same with misaligned sources going
# element by element (AFX_DEVIO_RAW_ELEMENTWISE) for the comparison of the two forms; then the worker without the profiler for
# the HIP-event brackets of afx_batch_create_from_raw_device beside afx_batch_create_from_raw from page-locked memory.
# Every GPU step has its own time limit and the chain stops at the first step that fails.
set -u
cd "$(dirname "$0")/.."
OUT=${1:-${TMPDIR:-/tmp}/devio_raw_cost}
mkdir -p "$OUT"
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -o p -- python3 tools/devio_raw_cost.py worker 512 1 device-only > "$OUT/worker_traced.json" &&
python3 tools/devio_raw_cost.py report "$OUT/trace" "$OUT/worker_traced.json" | tee "$OUT/kernels.jsonl" &&
AFX_DEVIO_RAW_ELEMENTWISE=1 timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_elementwise" -o p -- python3 tools/devio_raw_cost.py worker 512 1 device-only > "$OUT/worker_traced_elementwise.json" &&
python3 tools/devio_raw_cost.py report "$OUT/trace_elementwise" "$OUT/worker_traced_elementwise.json" | tee "$OUT/kernels_elementwise.jsonl" &&
echo "# brackets without the profiler:" &&
timeout -k 10 240 python3 tools/devio_raw_cost.py worker 512 1 | tee "$OUT/worker.json"
