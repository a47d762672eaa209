#!/usr/bin/env python3
"""What the per-file results cost on their way into device memory next to the host fetches.

  devio_file_cost.py worker [files] [seconds]   one batch of <files> (512) float files of <seconds> (1) s under
                                                AFX_D_HIGH_LEVEL_INPUTS | AFX_D_CLASSIFICATION_INPUTS and a small generated model.
                                                Each in a bracket of HIP events of its own, medians of 7 after 3 warm-up rounds:
                                                the three host fetches of the same results (afx_batch_fetch_high_level,
                                                afx_batch_fetch_classification_features, afx_batch_fetch_class_signature);
                                                afx_batch_export_file_results_device "embedding" (signature + normalised features
                                                + class signature as float, into a consumer stream) and "everything" (all eight
                                                kinds, the float kinds as double, tracks padded).  One JSON line, with the bytes
                                                the export kernel reads and writes.
  devio_file_cost.py report <dir> <worker.json> devio_file_export_kernel's own durations from the rocprofv3 kernel trace under
                                                <dir>, and their share of the rate a copy reaches on this part
                                                (profiles/r02/ubench_hbm_stream.txt: 4.7 TB/s of read + write)

tools/devio_file_cost.sh runs the worker under `rocprofv3 --kernel-trace --stats` (no counters), then the report, then the
worker without the profiler for the brackets."""
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.devio_cost import COPY_RATE, Bracket  # noqa: E402

VARIANTS = ["embedding f32", "everything f64"]


def worker(files, seconds):
    import ctypes
    import numpy as np
    import afec_amd as afx
    from afec_amd import device
    from tests import _gbdt_ref as ref
    from tests.test_gpu_file_results_device import stump_models, vectors
    rng = np.random.default_rng(1)
    n = int(44100 * seconds)
    H = device.hip()
    vp = ctypes.c_void_p
    H.hipEventCreate.argtypes, H.hipEventRecord.argtypes, H.hipEventSynchronize.argtypes = [ctypes.POINTER(vp)], [vp, vp], [vp]
    H.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    mask = afx.D_HIGH_LEVEL_INPUTS | afx.D_CLASSIFICATION_INPUTS
    plan = afx.Plan()
    stream = device.Stream()
    bracket = Bracket(H, stream.handle)
    pool = [(0.5 * np.sin(2 * np.pi * 110.0 * (k + 1) * np.arange(n) / 44100.0) + 0.1 * rng.uniform(-1, 1, n)).astype(np.float32) for k in range(8)]
    norm = vectors()
    model = afx.Model(plan, [ref.write_lightgbm(m) for m in stump_models()], *norm)
    batch = plan.batch([pool[i % 8] for i in range(files)], mask)
    batch.run()
    batch.sync()
    fo, _ = device.frame_offsets(batch)
    frames, longest = int(fo[-1]), int(np.diff(fo).max())
    K, W_SIG, W_FEAT, k = device.FILE_KIND_INDEX, device.SIGNATURE_WIDTH, afx.NUM_CLASSIFICATION_FEATURES, model.n_classes
    total = W_SIG + W_FEAT + k
    one = device.DeviceArray((files, total), np.float32)
    embedding = [(one.ptr, K["spectrum_signature"], afx.PCM_F32, total, 0), (one.ptr + W_SIG * 4, K["features_normalised"], afx.PCM_F32, total, 0),
                 (one.ptr + (W_SIG + W_FEAT) * 4, K["class_signature"], afx.PCM_F32, total, 0)]
    widths = {"high_scalars": afx.NUM_HL_SCALARS, "spectrum_signature": W_SIG, "features": W_FEAT, "features_normalised": W_FEAT, "class_signature": k}
    dests = {name: device.DeviceArray((files, w), np.float64) for name, w in widths.items()}
    dests.update({name: device.DeviceArray((files, longest), np.float64) for name in ("pitch", "peak")})
    dests["non_finite"] = device.DeviceArray((files,), np.int32)
    everything = [(dests[name], K[name], afx.PCM_F64, widths.get(name, 1), longest if name in ("pitch", "peak") else 0) for name in device.FILE_KINDS]

    def host_fetches():
        batch.fetch_high_level(None)
        batch.fetch_classification_features()
        batch.fetch_class_signature(model)

    ms = {key: [] for key in ["host fetches"] + VARIANTS}
    for _ in range(10):
        ms["host fetches"].append(bracket(host_fetches))
        ms["embedding f32"].append(bracket(lambda: device.file_results_into(batch, embedding, model, None, device.EXPORT_PACKED, 0, 0.0, stream)))
        ms["everything f64"].append(bracket(lambda: device.file_results_into(batch, everything, model, None, device.EXPORT_PADDED, longest, 0.0, stream)))
    features, _, _ = batch.fetch_classification_features()
    got = one.download()
    assert np.array_equal(got[:, W_SIG:W_SIG + W_FEAT], ref.normalise(features, *norm).astype(np.float32))
    assert np.array_equal(dests["features"].download(), features)
    per_file = 15 + W_SIG + 2 * W_FEAT
    print(json.dumps({"files": files, "seconds": seconds, "frames": frames, "max_frames": longest,
                      "median_ms": {key: statistics.median(v[3:]) for key, v in ms.items()},
                      "min_ms": {key: min(v[3:]) for key, v in ms.items()}, "max_ms": {key: max(v[3:]) for key, v in ms.items()},
                      "bytes": {"results_to_host": files * ((15 + W_SIG + W_FEAT) * 8 + k * 4 + 8) + 2 * frames * 8,
                                "embedding f32": files * ((W_SIG + W_FEAT) * (8 + 4) + k * 8) + 3 * W_FEAT * 8,
                                "everything f64": files * (per_file * 16 + k * 12 + 8) + 3 * W_FEAT * 8 + 2 * (frames * 8 + files * longest * 8)},
                      "build": afx.build_info()}))
    batch.close()
    model.close()
    plan.close()


def report(directory, worker_json):
    w = json.loads(open(worker_json).read().strip().splitlines()[-1])
    for trace in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        rows = list(csv.DictReader(open(trace)))
        runs = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "devio_file_export_kernel" in r["Kernel_Name"]]
        for i, key in enumerate(VARIANTS):   # the worker's launches alternate
            steady = runs[i::2][3:] or runs[i::2]
            med = statistics.median(steady) / 1e3 if steady else None
            print(json.dumps({"kernel": "devio_file_export_kernel " + key, "launches": len(runs[i::2]), "median_us": med,
                              "min_us": min(steady) / 1e3 if steady else None, "max_us": max(steady) / 1e3 if steady else None,
                              "bytes_read_plus_written": w["bytes"][key], "TB_per_s": w["bytes"][key] / (med * 1e-6) / 1e12 if med else None,
                              "share_of_copy_rate_4.7TB_s": w["bytes"][key] / (med * 1e-6) / COPY_RATE if med else None}))


if __name__ == "__main__":
    if sys.argv[1] == "worker":
        worker(int(sys.argv[2]) if len(sys.argv) > 2 else 512, float(sys.argv[3]) if len(sys.argv) > 3 else 1.0)
    else:
        report(sys.argv[2], sys.argv[3])
