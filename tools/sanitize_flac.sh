#!/bin/bash
# tools/sanitize_flac.sh [plain] [mutations per image] [seed] -- the FLAC indexer (afec_amd/csrc/flac/afx_flac_index.cpp) and
# the decoder the GPU runs (afec_amd/csrc/flac/afx_flac_decode.h) under AddressSanitizer + UBSan on the CPU: the stand-alone
# program tests/sanitize/flac_decode_main.cpp takes every fixture of tests/golden/flac, every truncation of it and seeded
# single-byte mutations, with the indexer's own index and with a truncated or changed one.  No device, no Python.
# `plain` builds without a sanitizer.
set -eu
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
KIND=asan
if [ "${1:-}" = plain ]; then SAN=""; KIND=plain; shift; fi
OUT=${AFX_SAN_DIR:-/tmp/afx_san}
mkdir -p "$OUT"
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer $SAN -Iinclude \
    -o "$OUT/flac_decode_$KIND" tests/sanitize/flac_decode_main.cpp afec_amd/csrc/flac/afx_flac_index.cpp
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/flac_decode_$KIND" "${1:-2000}" "${2:-1}" tests/golden/flac/*.flac
