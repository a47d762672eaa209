#!/usr/bin/env python3
"""What afx_batch_fetch_high_level costs next to what a caller paid before it existed (DESIGN.md, high-level descriptors).

  high_level_cost.py worker <files> <seconds>   one batch of <files> files of <seconds> s (LoadSample front end, the mask
                                                AFX_D_HIGH_LEVEL_INPUTS: the smallest records a caller could download):
                                                prints one JSON line with (a) the device time of afx_batch_run, (b) the wall
                                                time of afx_batch_fetch_records into page-locked memory, and the wall time of
                                                afx_batch_fetch_high_level (medians of 7 after 3 warm-up rounds)
  high_level_cost.py report <dir>               the kernel's own duration from the rocprofv3 kernel trace under <dir>

tools/high_level_cost.sh runs the worker under `rocprofv3 --kernel-trace --stats` for the two batch shapes and then the report."""
import csv
import ctypes
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(files, seconds):
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
    plan = afx.Plan()
    b, infos = plan.batch_from_raw([(pool[i % 8], 1) for i in range(files)], afx.D_HIGH_LEVEL_INPUTS)
    L = b.L
    stride = ctypes.c_int32()
    L.afx_batch_record_layout.argtypes = [ctypes.c_void_p] * 4
    L.afx_batch_record_layout(b.h, ctypes.byref(stride), None, None)
    records, keep = capi.pinned_array((b.total_frames, stride.value), np.float64)
    L.afx_batch_fetch_records.argtypes = [ctypes.c_void_p] * 6
    # both fetches as the C calls they are, into memory that exists already (the records' page-locked, as a pipeline
    # keeps it; the high-level results' ordinary arrays)
    b.run()
    hl = b.fetch_high_level(infos)
    out_struct = capi._HighOut()
    for k, v in hl.items():
        setattr(out_struct, k, v.ctypes.data)
    levels = (capi._LoadInfo * files)()
    for i, d in enumerate(infos):
        levels[i].peak_value, levels[i].rms_value = d["peak_value"], d["rms_value"]
    run_ms, records_ms, high_ms = [], [], []
    for round_ in range(10):
        run_ms.append(b.run_timed(1))
        t0 = time.perf_counter()
        st = L.afx_batch_fetch_records(b.h, records.ctypes.data, None, None, None, None)
        t1 = time.perf_counter()
        st2 = L.afx_batch_fetch_high_level(b.h, levels, ctypes.byref(out_struct))
        t2 = time.perf_counter()
        assert st == 0 and st2 == 0
        records_ms.append((t1 - t0) * 1e3)
        high_ms.append((t2 - t1) * 1e3)
    assert np.all(hl["status"] == 0) and np.all(np.isfinite(hl["scalars"]))
    out = {"files": files, "seconds": seconds, "frames": b.total_frames, "record_stride": stride.value,
           "records_bytes": int(records.nbytes), "high_level_bytes": int(sum(v.nbytes for k, v in hl.items() if k != "status")),
           "batch_run_ms": statistics.median(run_ms[3:]), "fetch_records_ms": statistics.median(records_ms[3:]),
           "fetch_high_level_ms": statistics.median(high_ms[3:]), "build": afx.build_info()}
    del keep
    b.close()
    plan.close()
    print(json.dumps(out))


def report(directory):
    for trace in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        runs = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(open(trace)) if "high_level_kernel" in r["Kernel_Name"]]
        steady = runs[3:] or runs
        print(json.dumps({"trace": os.path.relpath(trace, directory), "high_level_kernel_launches": len(runs),
                          "median_us": statistics.median(steady) / 1e3 if steady else None,
                          "min_us": min(steady) / 1e3 if steady else None, "max_us": max(steady) / 1e3 if steady else None}))


if __name__ == "__main__":
    if sys.argv[1] == "worker":
        worker(int(sys.argv[2]), float(sys.argv[3]))
    else:
        report(sys.argv[2])
