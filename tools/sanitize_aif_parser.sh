#!/bin/bash
# tools/sanitize_aif_parser.sh [plain] [mutations per image] [seed] -- afec_amd/host/AifFile.cpp (the AIFF / AIFF-C reader)
# under AddressSanitizer + UBSan on the CPU: the stand-alone program tests/sanitize/aif_parser_main.cpp parses generated
# valid images of every accepted encoding, their truncations and single-byte mutations, as images and from a temporary
# file.  No device, no Python.  `plain` builds without a sanitizer.
set -eu
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
KIND=asan
if [ "${1:-}" = plain ]; then SAN=""; KIND=plain; shift; fi
OUT=${AFX_SAN_DIR:-/tmp/afx_san}
mkdir -p "$OUT"
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer $SAN -Iinclude \
    -o "$OUT/aif_parser_$KIND" tests/sanitize/aif_parser_main.cpp afec_amd/host/AifFile.cpp afec_amd/host/WaveFile.cpp
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/aif_parser_$KIND" "$@"
