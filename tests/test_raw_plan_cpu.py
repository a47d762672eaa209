"""The plan of the raw arena (afec_amd/csrc/afx_raw_plan.h): every offset the ingest kernels later trust, decided on the host
before anything is enqueued.  tests/host/raw_plan_main.cpp holds the checks -- literal offsets of hand-made batches, and the
layout's invariants over seeded random ones, for all four combinations of the optional launchers; here it is compiled by
g++, plain and with AddressSanitizer + UBSan, and run as a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build(directory, name, flags):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(directory / name)
    include = ["-I" + os.path.join(ROOT, *p) for p in (("include",), ("afec_amd", "csrc"), ("tests", "sanitize", "hipstub"))]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + include +
                          ["-o", exe, os.path.join(ROOT, "tests", "host", "raw_plan_main.cpp")])
    return exe


def run(exe, batches, seed):
    out = subprocess.run([exe, str(batches), str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-2000:], out.stderr.decode()[-4000:])
    word = out.stdout.decode().split()
    assert word[0] == "ok" and int(word[2]) >= 4 * batches and int(word[4]) > 100 * batches, out.stdout
    return out


def test_hand_made_offsets_and_the_invariants_of_random_batches(tmp_path):
    run(build(tmp_path, "raw_plan_main", ["-O2"]), 400, 1)


def test_the_same_under_asan_and_ubsan(tmp_path):
    out = run(build(tmp_path, "raw_plan_main_asan", SANITIZE), 300, 2)
    assert b"runtime error" not in out.stderr and b"AddressSanitizer" not in out.stderr
