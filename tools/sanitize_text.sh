#!/bin/bash
# tools/sanitize_text.sh [plain] -- afec_amd/csrc/afx_high_level_text.cpp (afx_batch_fetch_high_level_text,
# afx_format_json_g9) and the number formatter afec_amd/csrc/text/afx_g9.h under AddressSanitizer + UBSan on the CPU: two
# stand-alone programs.  tests/sanitize/text_main.cpp drives the entry points on the mock device of tests/sanitize/hipstub,
# linked as tests/sanitize/build.sh links the C-ABI's host code, with a mock text kernel of its own that formats with the
# device's header; tests/host/test_g9_format.cpp holds that header against snprintf("%.9g") on 30 million values.
# `plain` builds both without a sanitizer (what tests/test_text_format_cpu.py runs).
set -eu
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
KIND=asan
if [ "${1:-}" = plain ]; then SAN=""; KIND=plain; shift; fi
OUT=${AFX_SAN_DIR:-/tmp/afx_san}
mkdir -p "$OUT"
ABI="afec_amd/csrc/afx_plan.cpp afec_amd/csrc/afx_workspace.cpp afec_amd/csrc/afx_batch_plan.cpp afec_amd/csrc/afx_batch_create.cpp afec_amd/csrc/afx_batch_run.cpp afec_amd/csrc/afx_batch_fetch.cpp afec_amd/csrc/afx_high_level.cpp afec_amd/csrc/afx_classification.cpp afec_amd/csrc/afx_class_decision.cpp afec_amd/csrc/afx_model.cpp afec_amd/csrc/afx_high_level_text.cpp"
MOCK="tests/sanitize/mock_kernels.cpp tests/sanitize/hipstub/hip_stub.cpp"
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer $SAN -Itests/sanitize/hipstub -Iinclude -DAFX_SRC_HASH=\"mock\" \
    -o "$OUT/text_main_$KIND" tests/sanitize/text_main.cpp $MOCK $ABI -lpthread
g++ -std=c++17 -O2 -g -fno-omit-frame-pointer $SAN -o "$OUT/test_g9_format_$KIND" tests/host/test_g9_format.cpp -lpthread
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/text_main_$KIND"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/test_g9_format_$KIND" "$@"
