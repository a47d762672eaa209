#!/usr/bin/env python3
"""What afx_batch_fetch_classification_features costs next to what a caller paid before it existed (DESIGN.md,
classification features).

  classification_cost.py worker <files> <seconds>   one batch of <files> files of <seconds> s (LoadSample front end, the mask
                                                    AFX_D_CLASSIFICATION_INPUTS: the smallest records a caller could
                                                    download): prints one JSON line with (a) the device time of
                                                    afx_batch_run, (b) the wall time of what a caller does today on the same
                                                    build -- afx_batch_fetch_records of records + statistics + effective
                                                    lengths into page-locked memory, then afx_batch_fetch_rhythm -- and (c)
                                                    the wall time of afx_batch_fetch_classification_features, with the
                                                    bytes each brings to the host (medians of 7 after 3 warm-up rounds)
  classification_cost.py report <dir>               the kernel's own duration from the rocprofv3 kernel trace under <dir>

tools/classification_cost.sh runs the worker under `rocprofv3 --kernel-trace --stats` for the two batch shapes and then the report."""
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
    b, _ = plan.batch_from_raw([(pool[i % 8], 1) for i in range(files)], afx.D_CLASSIFICATION_INPUTS)
    L = b.L
    stride = ctypes.c_int32()
    L.afx_batch_record_layout.argtypes = [ctypes.c_void_p] * 4
    L.afx_batch_record_layout(b.h, ctypes.byref(stride), None, None)
    # every destination exists before the clock starts: the records' and statistics' page-locked, as a pipeline keeps them
    records, keep1 = capi.pinned_array((b.total_frames, stride.value), np.float64)
    stats, keep2 = capi.pinned_array((files, stride.value, 13), np.float64)
    lengths, scalars = np.zeros((files, 3)), np.zeros((files, len(afx.RHYTHM_SCALARS)))
    features, counts = np.zeros((files, afx.NUM_CLASSIFICATION_FEATURES)), np.zeros(files, dtype=np.int32)
    L.afx_batch_fetch_records.argtypes = [ctypes.c_void_p] * 6
    b.run()
    run_ms, today_ms, features_ms = [], [], []
    for round_ in range(10):
        run_ms.append(b.run_timed(1))
        t0 = time.perf_counter()
        st = L.afx_batch_fetch_records(b.h, records.ctypes.data, stats.ctypes.data, None, None, lengths.ctypes.data)
        st1 = L.afx_batch_fetch_rhythm(b.h, None, scalars.ctypes.data, None)
        t1 = time.perf_counter()
        st2 = L.afx_batch_fetch_classification_features(b.h, features.ctypes.data, counts.ctypes.data, None)
        t2 = time.perf_counter()
        assert st == 0 and st1 == 0 and st2 == 0
        today_ms.append((t1 - t0) * 1e3)
        features_ms.append((t2 - t1) * 1e3)
    assert np.all(counts == 0) and np.all(np.isfinite(features)) and np.any(features != 0.0)
    out = {"files": files, "seconds": seconds, "frames": b.total_frames, "record_stride": stride.value,
           "today_bytes": int(records.nbytes + stats.nbytes + lengths.nbytes + scalars.nbytes),
           "features_bytes": int(features.nbytes + counts.nbytes),
           "batch_run_ms": statistics.median(run_ms[3:]), "fetch_today_ms": statistics.median(today_ms[3:]),
           "fetch_classification_features_ms": statistics.median(features_ms[3:]), "build": afx.build_info()}
    del keep1, keep2
    b.close()
    plan.close()
    print(json.dumps(out))


def report(directory):
    for trace in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        runs = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(open(trace))
                if "classification_features_kernel" in r["Kernel_Name"]]
        steady = runs[3:] or runs
        print(json.dumps({"trace": os.path.relpath(trace, directory), "classification_features_kernel_launches": len(runs),
                          "median_us": statistics.median(steady) / 1e3 if steady else None,
                          "min_us": min(steady) / 1e3 if steady else None, "max_us": max(steady) / 1e3 if steady else None}))


if __name__ == "__main__":
    if sys.argv[1] == "worker":
        worker(int(sys.argv[2]), float(sys.argv[3]))
    else:
        report(sys.argv[2])
