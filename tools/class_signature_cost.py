#!/usr/bin/env python3
"""What afx_batch_fetch_class_signature costs next to what a caller could do before it existed (class signature).

  class_signature_cost.py worker <files> <seconds>   one batch of <files> files of <seconds> s (LoadSample front end, the
                                                     mask AFX_D_CLASSIFICATION_INPUTS) and the reference's OneShot-vs-Loops
                                                     bagging (tests/golden/oneshot_vs_loops_model.npz): prints one JSON line
                                                     with (a) the wall time of afx_batch_fetch_classification_features into
                                                     page-locked memory -- after which that caller still has 1 718 trees per
                                                     file to walk on the CPU, which is not timed here -- and (b) the wall
                                                     time of afx_batch_fetch_class_signature, with the bytes each brings to
                                                     the host (medians of 7 after 3 warm-up rounds)
  class_signature_cost.py report <dir>               the two kernels' own durations from the rocprofv3 kernel trace under <dir>

tools/class_signature_cost.sh runs the worker under `rocprofv3 --kernel-trace --stats` (no counters) for the two batch shapes,
then the report, then the worker without the profiler for the wall times."""
import csv
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
    from tests import _gbdt_ref as ref
    rng = np.random.default_rng(1)
    n = int(44100 * seconds)
    t = np.arange(n)
    pool = []
    for k in range(8):
        tone = np.sin(2 * np.pi * (110.0 * (k + 1)) * t / 44100.0) * np.exp(-(t % 11025) / 4000.0)
        pool.append(np.round(12000 * tone + 2000 * rng.uniform(-1, 1, n) * (t % 22050 < 6000)).astype(np.int16))
    z = np.load(os.path.join(ROOT, "tests", "golden", "oneshot_vs_loops_model.npz"))
    plan = afx.Plan()
    model = afx.Model(plan, [ref.write_lightgbm(m) for m in ref.unpack_models(z)], z["scale"], z["offset"], z["limits"])
    b, _ = plan.batch_from_raw([(pool[i % 8], 1) for i in range(files)], afx.D_CLASSIFICATION_INPUTS)
    L = b.L
    features, keep = capi.pinned_array((files, afx.NUM_CLASSIFICATION_FEATURES), np.float64)
    counts = np.zeros(files, dtype=np.int32)
    signature = np.zeros((files, model.n_classes), dtype=np.float32)
    used, bad = np.zeros((files, model.n_models), dtype=np.int32), np.zeros(files, dtype=np.int32)
    b.run()
    features_ms, signature_ms = [], []
    for _ in range(10):
        b.run()
        L.afx_batch_sync(b.h)
        t0 = time.perf_counter()
        st1 = L.afx_batch_fetch_classification_features(b.h, features.ctypes.data, counts.ctypes.data, None)
        t1 = time.perf_counter()
        st2 = L.afx_batch_fetch_class_signature(b.h, model.h, signature.ctypes.data, used.ctypes.data, bad.ctypes.data)
        t2 = time.perf_counter()
        assert st1 == 0 and st2 == 0
        features_ms.append((t1 - t0) * 1e3)
        signature_ms.append((t2 - t1) * 1e3)
    assert np.all(bad == 0) and np.all(used > 0) and np.all(np.abs(signature.sum(axis=1) - 1.0) < 1e-5)
    out = {"files": files, "seconds": seconds, "frames": b.total_frames, "trees_per_file": sum(model.trees_per_model),
           "features_bytes": int(features.nbytes + counts.nbytes), "signature_bytes": int(signature.nbytes + used.nbytes + bad.nbytes),
           "fetch_classification_features_ms": statistics.median(features_ms[3:]),
           "fetch_class_signature_ms": statistics.median(signature_ms[3:]),
           "iterations_used_mean": float(used.mean()), "build": afx.build_info()}
    del keep
    model.close()
    b.close()
    plan.close()
    print(json.dumps(out))


def report(directory):
    for trace in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        rows = list(csv.DictReader(open(trace)))
        for kernel in ("classification_features_kernel", "class_signature_kernel"):
            runs = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]]
            steady = runs[3:] or runs
            print(json.dumps({"trace": os.path.relpath(trace, directory), "kernel": kernel, "launches": len(runs),
                              "median_us": statistics.median(steady) / 1e3 if steady else None,
                              "min_us": min(steady) / 1e3 if steady else None, "max_us": max(steady) / 1e3 if steady else None}))


if __name__ == "__main__":
    if sys.argv[1] == "worker":
        worker(int(sys.argv[2]), float(sys.argv[3]))
    else:
        report(sys.argv[2])
