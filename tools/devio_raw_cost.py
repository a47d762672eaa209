#!/usr/bin/env python3
"""What LoadSample on device-resident audio costs next to the host path.

  devio_raw_cost.py worker [files] [seconds]   <files> (512) stereo files of <seconds> (1) s under AFX_D_ALL_LOW_LEVEL.  Gather cases,
                                           each 3 warm-up + 7 creations in a bracket of HIP events: I16 aligned, I16 two bytes
                                           behind a 16-byte boundary, packed I24 one byte behind one, F32 planar; the same I16
                                           batch at 44.1 kHz and at 48 kHz through afx_batch_create_from_raw from page-locked
                                           memory (skipped with `device-only`: a library without the device call runs
                                           `host-only`); afx_batch_export_samples_device padded F32.  One JSON line, with the
                                           bytes each kernel reads and writes.
  devio_raw_cost.py report <dir> <worker.json>   the kernels' own durations from the rocprofv3 kernel trace under <dir> and their
                                           share of the rate a copy reaches on this part (profiles/r02/ubench_hbm_stream.txt:
                                           4.7 TB/s of read + write)

tools/devio_raw_cost.sh runs the worker under `rocprofv3 --kernel-trace --stats` (no counters), the same with
AFX_DEVIO_RAW_ELEMENTWISE set (misaligned interleaved sources element by element), then the worker without the profiler for the
brackets.  Every source is uploaded once and read by every creation: 90 to 180 MB a case, within the 256 MB the part's
last-level cache holds -- the sources are cache-resident at best, never fresh from a producer."""
import csv
import ctypes
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 4.7e12   # bytes read + written per second by a device copy (profiles/r02/ubench_hbm_stream.txt)
CASES = ["i16_aligned", "i16_off_2", "i24_off_1", "f32_planar"]


def worker(files, seconds, which):
    import numpy as np
    import afec_amd as afx
    from afec_amd import capi, device
    from devio_cost import Bracket   # tools/devio_cost.py, beside this file
    rng = np.random.default_rng(1)
    n = int(44100 * seconds)
    H = device.hip()
    vp = ctypes.c_void_p
    H.hipEventCreate.argtypes, H.hipEventRecord.argtypes, H.hipEventSynchronize.argtypes = [ctypes.POINTER(vp)], [vp, vp], [vp]
    H.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    mask = afx.D_ALL_LOW_LEVEL
    plan = afx.Plan()
    stream = device.Stream()
    bracket = Bracket(H, stream.handle)
    t = np.arange(n)[:, None]
    pool = [0.5 * np.sin(2 * np.pi * 110.0 * (k + 1) * t / 44100.0 + np.array([0.0, 0.7])[None, :]) + 0.1 * rng.uniform(-1, 1, (n, 2)) for k in range(8)]
    ms, nbytes = {}, {}

    def timed(name, make):
        ms[name] = []
        for _ in range(10):
            made = []
            ms[name].append(bracket(lambda: made.append(make())))
            made[0][0].close()

    i16 = [np.round(p * 30000).astype(np.int16) for p in pool]
    if which != "device-only":
        pinned, owner = capi.pinned_array((files, n, 2), np.int16)
        for i in range(files):
            pinned[i] = i16[i % 8]
        for rate in (44100, 48000):
            timed("create_from_raw_pinned_%d" % rate, lambda: plan.batch_from_raw([(pinned[i], 2, rate) for i in range(files)], mask))
    if which != "host-only":
        inter, planar = device.RAW_INTERLEAVED, device.RAW_PLANAR
        # one allocation a case, the files back to back from `off` bytes behind a 16-byte boundary (hipMalloc's is aligned)
        def resident(per_file, off):
            host = np.zeros(off + sum(a.size for a in per_file), dtype=np.uint8)
            first, at = [], off
            for a in per_file:
                first.append(at)
                host[at:at + a.size] = a
                at += a.size
            d = device.DeviceArray.from_numpy(host)
            return d, [d.ptr + f for f in first]
        as_bytes = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        i24 = [np.round(p * 8000000).astype("<i4").view(np.uint8).reshape(n, 2, 4)[:, :, :3] for p in pool]
        f32p = [np.ascontiguousarray(p.astype(np.float32).T) for p in pool]
        sources = {"i16_aligned": (resident([as_bytes(i16[i % 8]) for i in range(files)], 0), capi.RAW_I16, inter, 2),
                   "i16_off_2": (resident([as_bytes(i16[i % 8]) for i in range(files)], 2), capi.RAW_I16, inter, 2),
                   "i24_off_1": (resident([as_bytes(i24[i % 8]) for i in range(files)], 1), capi.RAW_I24, inter, 3),
                   "f32_planar": (resident([as_bytes(f32p[i % 8]) for i in range(files)], 0), capi.RAW_F32, planar, 4)}
        for name in CASES:
            (d, ptrs), fmt, layout, bps = sources[name]
            for rate in ((44100, 48000) if name == "i16_aligned" else (44100,)):
                specs = [(p, fmt, 2, rate, layout, n, n if layout == planar else 0) for p in ptrs]
                timed("create_from_raw_device_%s_%d" % (name, rate), lambda: afx.create_batch_from_raw_device(plan, specs, mask=mask))
            nbytes["devio_raw_gather_kernel " + name] = 2 * files * n * 2 * bps
        (d, ptrs), fmt, layout, bps = sources["i16_off_2"]
        batch, infos = afx.create_batch_from_raw_device(plan, [(p, fmt, 2, 0, layout, n, 0) for p in ptrs], mask=mask)
        used = afx.sample_counts(batch).download()
        longest = int(used.max())
        padded = device.DeviceArray((files, longest + 64), np.float32)
        ms["export_samples_padded_f32"] = [bracket(lambda: capi._check(H, H.afx_batch_export_samples_device(
            batch.h, padded.ptr, afx.PCM_F32, longest + 64, 0.0, stream.handle))) for _ in range(10)]
        nbytes["devio_samples_kernel padded f32"] = int(used.sum()) * 4 + padded.nbytes
        want = np.stack([np.pad(batch.fetch_samples(i, int(used[i])).astype(np.float32), (0, longest + 64 - int(used[i]))) for i in (0, files - 1)])
        assert np.array_equal(padded.download()[[0, files - 1]], want)
        batch.close()
    print(json.dumps({"files": files, "seconds": seconds, "which": which, "elementwise": "AFX_DEVIO_RAW_ELEMENTWISE" in os.environ,
                      "median_ms": {k: statistics.median(v[3:]) for k, v in ms.items()}, "min_ms": {k: min(v[3:]) for k, v in ms.items()},
                      "bytes": nbytes, "build": afx.build_info()}))
    plan.close()


def report(directory, worker_json):
    w = json.loads(open(worker_json).read().strip().splitlines()[-1])
    for trace in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
        gathers = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "devio_raw_gather_kernel" in r["Kernel_Name"]]
        # the worker's launches in order: ten a case and rate (i16_aligned at two rates), then the export's batch
        series, at = {}, 0
        for name in CASES:
            for rate in ((44100, 48000) if name == "i16_aligned" else (44100,)):
                series.setdefault("devio_raw_gather_kernel " + name, []).extend(gathers[at + 3:at + 10])
                at += 10
        series["devio_samples_kernel padded f32"] = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "devio_samples_kernel" in r["Kernel_Name"]][3:]
        for key, r in series.items():
            med = statistics.median(r) / 1e3 if r else None
            print(json.dumps({"kernel": key, "elementwise": w["elementwise"], "launches": len(r), "median_us": med, "min_us": min(r) / 1e3 if r else None,
                              "max_us": max(r) / 1e3 if r else None, "bytes_read_plus_written": w["bytes"][key],
                              "TB_per_s": w["bytes"][key] / (med * 1e-6) / 1e12 if med else None,
                              "share_of_copy_rate_4.7TB_s": w["bytes"][key] / (med * 1e-6) / COPY_RATE if med else None}))


if __name__ == "__main__":
    if sys.argv[1] == "worker":
        worker(int(sys.argv[2]) if len(sys.argv) > 2 else 512, float(sys.argv[3]) if len(sys.argv) > 3 else 1.0,
               sys.argv[4] if len(sys.argv) > 4 else "both")
    else:
        report(sys.argv[2], sys.argv[3])
