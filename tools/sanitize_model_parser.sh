#!/bin/bash
# tools/sanitize_model_parser.sh [plain] [LightGBM text file ...] -- afec_amd/csrc/afx_model.cpp (the LightGBM text reader,
# afx_model_create_from_lightgbm / _get_info / _destroy) under AddressSanitizer + UBSan on the CPU: a stand-alone program
# (tests/sanitize/model_parser_main.cpp) on the mock device of tests/sanitize/hipstub, linked as tests/sanitize/build.sh
# links the C-ABI's host code.  Without files it runs the built-in texts; with the decompressed members of a model file it
# also truncates and mutates those.  `plain` builds without a sanitizer (what tests/test_gbdt_ref_cpu.py runs).
set -eu
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
KIND=asan
if [ "${1:-}" = plain ]; then SAN=""; KIND=plain; shift; fi
OUT=${AFX_SAN_DIR:-/tmp/afx_san}
mkdir -p "$OUT"
ABI="afec_amd/csrc/afx_plan.cpp afec_amd/csrc/afx_workspace.cpp afec_amd/csrc/afx_batch_plan.cpp afec_amd/csrc/afx_batch_create.cpp afec_amd/csrc/afx_batch_run.cpp afec_amd/csrc/afx_batch_fetch.cpp"
MOCK="tests/sanitize/mock_kernels.cpp tests/sanitize/hipstub/hip_stub.cpp"
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer $SAN -Itests/sanitize/hipstub -Iinclude -DAFX_SRC_HASH=\"mock\" \
    -o "$OUT/model_parser_$KIND" tests/sanitize/model_parser_main.cpp afec_amd/csrc/afx_model.cpp $MOCK $ABI -lpthread
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/model_parser_$KIND" "$@"
