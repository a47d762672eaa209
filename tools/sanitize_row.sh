#!/bin/bash
# tools/sanitize_row.sh [plain] -- afec_amd/csrc/afx_high_level_row.cpp (afx_batch_fetch_high_level_row,
# afx_batch_high_level_row_capacity, afx_format_class_json) and afec_amd/host/HighLevelPool.cpp under AddressSanitizer + UBSan
# on the CPU: one stand-alone program, tests/sanitize/row_main.cpp, on the mock device of tests/sanitize/hipstub, linked as
# tests/sanitize/build.sh links the C-ABI's and the host layer's code, with a mock text kernel of its own that writes the
# reference's text into the slots the host sized.  `plain` builds it without a sanitizer (what
# tests/test_high_level_row_cpu.py runs).
set -eu
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
KIND=asan
if [ "${1:-}" = plain ]; then SAN=""; KIND=plain; shift; fi
OUT=${AFX_SAN_DIR:-/tmp/afx_san}
mkdir -p "$OUT"
ABI="afec_amd/csrc/afx_plan.cpp afec_amd/csrc/afx_workspace.cpp afec_amd/csrc/afx_batch_plan.cpp afec_amd/csrc/afx_batch_create.cpp afec_amd/csrc/afx_batch_run.cpp afec_amd/csrc/afx_batch_fetch.cpp afec_amd/csrc/afx_high_level.cpp afec_amd/csrc/afx_classification.cpp afec_amd/csrc/afx_class_decision.cpp afec_amd/csrc/afx_model.cpp afec_amd/csrc/afx_high_level_text.cpp afec_amd/csrc/afx_high_level_row.cpp"
MOCK="tests/sanitize/mock_kernels.cpp tests/sanitize/hipstub/hip_stub.cpp"
HOST="afec_amd/host/Crawler.cpp afec_amd/host/SampleAnalyser.cpp afec_amd/host/DescriptorColumns.cpp afec_amd/host/SqlitePool.cpp afec_amd/host/WaveFile.cpp afec_amd/host/SyntheticInput.cpp afec_amd/host/HighLevelPool.cpp"
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer $SAN -Itests/sanitize/hipstub -Iinclude -DAFX_SRC_HASH=\"mock\" \
    -o "$OUT/row_main_$KIND" tests/sanitize/row_main.cpp $MOCK $ABI $HOST -lpthread -ldl
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/row_main_$KIND" "$OUT/row_main_$KIND.db"
