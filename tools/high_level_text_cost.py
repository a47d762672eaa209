#!/usr/bin/env python3
"""What the text of the high-level vector columns costs on the GPU next to what a caller pays who downloads the doubles and
formats them on the host (DESIGN.md, high-level text columns).

  high_level_text_cost.py <files> <seconds>   one batch of <files> files of <seconds> s (LoadSample front end, the mask
                                              AFX_D_HIGH_LEVEL_INPUTS): prints one JSON line with, as medians of 7 after 3
                                              warm-up rounds, each behind a batch synchronise,
      (a) the wall time of afx_batch_fetch_high_level into page-locked memory, and of formatting its three vector columns
          of all files on one host thread (tools/host_format/host_format.cpp), once with snprintf("%.9g") and once with
          std::to_chars(general, 9);
      (b) where the loaded library has it, the wall time of afx_batch_fetch_high_level_text into page-locked memory, the
          bytes it downloads and the bytes of them that are text; its text is compared with the host's, byte for byte.

AFX_TREE names another checkout to import afec_amd from: run it once on a built checkout of the parent commit for (a) and once
on this tree for (a) and (b), alternating, in one visit."""
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.environ.get("AFX_TREE") or os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def host_formatter():
    lib = os.path.join(HERE, "host_format", "libhost_format.so")
    src = os.path.join(HERE, "host_format", "host_format.cpp")
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", lib, src])
    L = ctypes.CDLL(lib)
    L.host_format_columns.restype = ctypes.c_int64
    L.host_format_columns.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    return L


def main(files, seconds):
    import numpy as np
    import afec_amd as afx
    from afec_amd import capi
    rng = np.random.default_rng(1)
    n = int(44100 * seconds)
    t = np.arange(n)
    pool = []
    for k in range(8):
        tone = np.sin(2 * np.pi * (110.0 * (k + 1)) * t / 44100.0) * np.exp(-(t % 11025) / 4000.0)
        pool.append(np.round(12000 * tone + 2000 * rng.uniform(-1, 1, n) * (t % 22050 < 6000)).astype(np.int16))
    H = host_formatter()
    plan = afx.Plan()
    b, infos = plan.batch_from_raw([(pool[i % 8], 1) for i in range(files)], afx.D_HIGH_LEVEL_INPUTS)
    L = b.L
    b.run()
    frame_offset = np.ascontiguousarray(b.fetch()["frame_offset"], dtype=np.int64)
    levels = (capi._LoadInfo * files)()
    for i, d in enumerate(infos):
        levels[i].peak_value, levels[i].rms_value = d["peak_value"], d["rms_value"]
    # (a) the doubles into page-locked memory, as a pipeline keeps it
    shapes = {"scalars": (files, 15), "signature": (files, 64, 14), "pitch": (b.total_frames,), "peak": (b.total_frames,)}
    pinned = {k: capi.pinned_array(s, np.float64) for k, s in shapes.items()}
    status = np.zeros(files, dtype=np.int32)
    high = capi._HighOut(status=status.ctypes.data, **{k: a.ctypes.data for k, (a, _) in pinned.items()})
    n_values = files * 896 + 2 * b.total_frames
    host_text = np.zeros(33 * n_values + 6 * files, dtype=np.uint8)
    # (b) the text into page-locked memory
    with_text = hasattr(b, "fetch_high_level_text") and hasattr(L, "afx_batch_fetch_high_level_text")
    if with_text:
        capacity = b.high_level_text_capacity()
        text, keep_text = capi.pinned_array((max(1, capacity),), np.uint8)
        scalars = np.zeros((files, 15))
        begin, length = np.zeros((files, 3), dtype=np.int64), np.zeros((files, 3), dtype=np.int32)
        tout = capi._HighTextOut(scalars=scalars.ctypes.data, text=text.ctypes.data, text_capacity=capacity, begin=begin.ctypes.data,
                                 length=length.ctypes.data, status=status.ctypes.data)
    times = {"fetch_high_level": [], "format_snprintf": [], "format_to_chars": [], "fetch_high_level_text": []}
    text_bytes = {}
    for _ in range(10):
        b.run()
        b.sync()
        t0 = time.perf_counter()
        assert L.afx_batch_fetch_high_level(b.h, levels, ctypes.byref(high)) == 0
        times["fetch_high_level"].append((time.perf_counter() - t0) * 1e3)
        for mode, name in ((0, "format_snprintf"), (1, "format_to_chars")):
            t0 = time.perf_counter()
            text_bytes[name] = H.host_format_columns(pinned["signature"][0].ctypes.data, pinned["pitch"][0].ctypes.data, pinned["peak"][0].ctypes.data,
                                                     frame_offset.ctypes.data, files, mode, host_text.ctypes.data)
            times[name].append((time.perf_counter() - t0) * 1e3)
        if with_text:                                # alternating, so that both see the same machine
            b.run()
            b.sync()
            t0 = time.perf_counter()
            assert L.afx_batch_fetch_high_level_text(b.h, levels, ctypes.byref(tout)) == 0
            times["fetch_high_level_text"].append((time.perf_counter() - t0) * 1e3)
    out = {"files": files, "seconds": seconds, "frames": b.total_frames, "values": n_values, "build": afx.build_info(),
           "doubles_bytes": int(sum(a.nbytes for a, _ in pinned.values()))}
    for name, ms in times.items():
        if ms:
            out[name + "_ms"] = statistics.median(ms[3:])
    out["host_snprintf_total_ms"] = out["fetch_high_level_ms"] + out["format_snprintf_ms"]
    out["host_to_chars_total_ms"] = out["fetch_high_level_ms"] + out["format_to_chars_ms"]
    out["host_text_bytes"] = int(text_bytes["format_snprintf"])
    assert text_bytes["format_snprintf"] == text_bytes["format_to_chars"]
    if with_text:
        # the GPU's text is the host's: the columns behind one another are the same bytes
        joined = b"".join(text[begin[i, c]:begin[i, c] + length[i, c]].tobytes() for i in range(files) for c in range(3))
        assert joined == host_text[:out["host_text_bytes"]].tobytes(), "the GPU's text differs from snprintf's"
        out["text_bytes"] = int(length.sum())
        out["downloaded_bytes"] = int(capacity + begin.nbytes + length.nbytes + scalars.nbytes)
    b.close()
    plan.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(sys.argv[1]), float(sys.argv[2]))
