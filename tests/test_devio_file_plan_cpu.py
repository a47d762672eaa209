"""The planning of the per-file results' export into device memory (afec_amd/csrc/devio/afx_devio_file_plan.h): the export
kernel's table for each kind, the widths, the kernels a call needs, the extent of every destination and every refusal with
the destination its text names, decided on the host before anything is enqueued.  tests/host/devio_file_plan_main.cpp
holds the checks; here it is compiled by g++, plain and with AddressSanitizer + UBSan, and run as a program of its own."""
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
                          ["-o", exe, os.path.join(ROOT, "tests", "host", "devio_file_plan_main.cpp")])
    return exe


def run(exe):
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, (out.stdout.decode()[-3000:], out.stderr.decode()[-4000:])
    word = out.stdout.decode().split()
    assert word[0] == "ok" and int(word[1]) > 100, out.stdout
    return out


def test_tables_widths_extents_and_every_refusal(tmp_path):
    run(build(tmp_path, "devio_file_plan_main", ["-O2"]))


def test_the_same_under_asan_and_ubsan(tmp_path):
    out = run(build(tmp_path, "devio_file_plan_main_asan", SANITIZE))
    assert b"runtime error" not in out.stderr and b"AddressSanitizer" not in out.stderr
