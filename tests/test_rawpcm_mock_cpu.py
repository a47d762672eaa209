"""The big-endian formats on the mock device of tests/sanitize.  Its builds link afec_amd/csrc/afx_batch_create.cpp and
afec_amd/host/Crawler.cpp from a fixed list of files, without the byte-order kernel's launcher and without the AIFF reader:
both are weak references there, found null, and a file that needs one is refused like any other file that cannot be taken
-- its neighbours are analysed.  (tests/sanitize/build.sh and mock_kernels.cpp are as they were.)"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import ctypes, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
from afec_amd import capi, hostlib
from tests._aiff import aiff_bytes
from tests._wav import wav_bytes

L = ctypes.CDLL(sys.argv[1])
vp, i32, i64, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32
L.afx_plan_create.argtypes = [ctypes.POINTER(capi._PlanDesc), ctypes.POINTER(vp)]
L.afx_batch_create_from_raw.argtypes = [vp, ctypes.POINTER(capi._Raw), i32, u32, ctypes.POINTER(vp), ctypes.POINTER(capi._LoadInfo)]
L.afx_batch_total_frames.restype = i64
L.afx_batch_total_frames.argtypes = [vp]
L.afx_batch_run.argtypes = [vp]
L.afx_batch_fetch.argtypes = [vp, ctypes.POINTER(capi._Out)]
L.afx_batch_destroy.argtypes = [vp]
L.afx_plan_destroy.argtypes = [vp]

desc = capi._PlanDesc(44100, 2048, 1024, 0, capi.PRECISION_F64, 0, capi.FRAME_KERNEL_AUTO, 0)
plan = vp()
assert L.afx_plan_create(ctypes.byref(desc), ctypes.byref(plan)) == 0
x = ((np.arange(6000) %% 251 - 125) * 100).astype(np.int16)
foreign = x.byteswap()
raws = (capi._Raw * 3)()
for i, (data, fmt) in enumerate([(x, capi.RAW_I16), (foreign, capi.RAW_I16_BE), (x, capi.RAW_I16)]):
    raws[i].data, raws[i].format, raws[i].channels, raws[i].sample_rate, raws[i].n_frames = data.ctypes.data, fmt, 1, 0, x.size
info = (capi._LoadInfo * 3)()
batch = vp()
assert L.afx_batch_create_from_raw(plan, raws, 3, capi.D_MFCC, ctypes.byref(batch), info) == 0
assert L.afx_batch_run(batch) == 0
out, res = capi._alloc_out(capi.D_MFCC, int(L.afx_batch_total_frames(batch)), 3)
assert L.afx_batch_fetch(batch, ctypes.byref(out)) == 0
L.afx_batch_destroy(batch)
L.afx_plan_destroy(plan)

# the crawler above it: an AIFF among WAVs
hostlib._lib = hostlib._bind(L)
wav = wav_bytes(x, 1, 16)
crawl = hostlib.crawl([wav, aiff_bytes(x, 1, 16), wav], names=["a.wav", "b.aif", "c.wav"], files_per_batch=8)
print(json.dumps({"status": res["buf_status"].tolist(), "frame_offset": res["frame_offset"].tolist(),
                  "n_samples": [int(info[i].n_samples) for i in range(3)], "files": crawl["files"], "failed": crawl["failed"]}))
"""


def test_a_big_endian_buffer_is_unsupported_on_the_mock_and_its_neighbours_are_analysed(tmp_path):
    env = dict(os.environ, AFX_SAN_DIR=str(tmp_path / "afx_san"))
    out = subprocess.run([os.path.join(ROOT, "tests", "sanitize", "build.sh"), "plain", "host_lib"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600, env=env)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    mock = out.stdout.decode().split()[-1]
    script = tmp_path / "mock_be.py"
    script.write_text(SCRIPT % {"root": ROOT})
    r = subprocess.run([sys.executable, str(script), mock], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    got = json.loads(r.stdout.decode().splitlines()[-1])
    assert got["status"] == [0, -2, 0]                                  # AFX_OK, AFX_ERR_UNSUPPORTED, AFX_OK
    frames = got["frame_offset"]
    assert frames[1] - frames[0] == frames[3] - frames[2] > 0 and frames[2] == frames[1]
    assert got["n_samples"][0] == got["n_samples"][2] > 0 and got["n_samples"][1] == 0
    assert got["files"] == 3 and got["failed"] == 1                      # the AIFF: no reader in that build
