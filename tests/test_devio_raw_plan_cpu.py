"""The planning of LoadSample on device-resident audio (afec_amd/csrc/devio/afx_devio_raw_plan.h): the caller's buffers as
afx_batch_create_from_raw's own rule is to see them, every refusal with its status, the gather's table and tile prefix, the
sample export's extent, decided on the host before anything is enqueued.  tests/host/devio_raw_plan_main.cpp holds the
checks; here it is compiled by g++, plain and with AddressSanitizer + UBSan, and run as a program of its own."""
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
                          ["-o", exe, os.path.join(ROOT, "tests", "host", "devio_raw_plan_main.cpp")])
    return exe


def run(exe):
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, (out.stdout.decode()[-3000:], out.stderr.decode()[-4000:])
    word = out.stdout.decode().split()
    assert word[0] == "ok" and int(word[1]) > 100, out.stdout
    return out


def test_refusals_statuses_tile_prefix_and_extents(tmp_path):
    run(build(tmp_path, "devio_raw_plan_main", ["-O2"]))


def test_the_same_under_asan_and_ubsan(tmp_path):
    out = run(build(tmp_path, "devio_raw_plan_main_asan", SANITIZE))
    assert b"runtime error" not in out.stderr and b"AddressSanitizer" not in out.stderr
