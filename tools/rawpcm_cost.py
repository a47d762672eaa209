#!/usr/bin/env python3
"""What big-endian PCM costs next to its native twin.

  rawpcm_cost.py worker <files> <seconds> <i16|i24>   one batch of <files> stereo files of <seconds> s, laid out as a staging
                                                      buffer, created by afx_batch_create_from_raw once with its samples in
                                                      Motorola order (AFX_RAW_*_BE) and once as the native twin: prints one
                                                      JSON line with the medians of 7 wall times of either call (after 3
                                                      warm-up rounds, alternating, same process, same build)
  rawpcm_cost.py report <dir>                         raw_native_kernel's own duration from the rocprofv3 kernel trace under <dir>
  rawpcm_cost.py crawl <files> [rounds]               the C4-share shape (<files> one-second stereo 16-bit files in memory, no
                                                      database) crawled as WAV and as AIFF, alternating, rounds - 1 times each after one warm-up round:
                                                      files/s and busy host CPUs

tools/rawpcm_cost.sh runs the worker under `rocprofv3 --kernel-trace --stats` for the two batch shapes, then the report, then
the workers and the crawl without the profiler."""
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(files, seconds, kind):
    import numpy as np
    import afec_amd as afx
    from afec_amd import capi
    rng = np.random.default_rng(1)
    frames = int(44100 * seconds)
    width, native_fmt, foreign_fmt = (2, capi.RAW_I16, capi.RAW_I16_BE) if kind == "i16" else (3, capi.RAW_I24, capi.RAW_I24_BE)
    slot = (frames * 2 * width + 15) & ~15
    staging = {"native": np.zeros(files * slot, dtype=np.uint8), "foreign": np.zeros(files * slot, dtype=np.uint8)}
    pool = [rng.integers(0, 256, frames * 2 * width, dtype=np.uint8) for _ in range(8)]
    for i in range(files):
        staging["native"][i * slot:i * slot + pool[i % 8].size] = pool[i % 8]
        staging["foreign"][i * slot:i * slot + pool[i % 8].size] = pool[i % 8].reshape(-1, width)[:, ::-1].reshape(-1)
    plan = afx.Plan()
    ms = {"native": [], "foreign": []}
    for round_ in range(10):
        for which, fmt in (("native", native_fmt), ("foreign", foreign_fmt)):
            raws = [(staging[which][i * slot:i * slot + frames * 2 * width], 2, 0, fmt) for i in range(files)]
            t0 = time.perf_counter()
            b, infos = plan.batch_from_raw(raws, afx.D_MFCC)
            ms[which].append((time.perf_counter() - t0) * 1e3)      # (with the binding's packing of the table, the same for both)
            b.close()
    payload = files * frames * 2 * width
    print(json.dumps({"files": files, "seconds": seconds, "kind": kind, "payload_bytes": payload,
                      "create_native_ms": statistics.median(ms["native"][3:]), "create_foreign_ms": statistics.median(ms["foreign"][3:]),
                      "derived_kernel_us_at_4.7TB_s": 2 * payload / 4.7e12 * 1e6, "build": afx.build_info()}))
    plan.close()


def report(directory):
    for trace in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        runs = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(open(trace)) if "raw_native_kernel" in r["Kernel_Name"]]
        steady = runs[3:] or runs
        print(json.dumps({"trace": os.path.relpath(trace, directory), "raw_native_kernel_launches": len(runs),
                          "median_us": statistics.median(steady) / 1e3 if steady else None,
                          "min_us": min(steady) / 1e3 if steady else None, "max_us": max(steady) / 1e3 if steady else None}))


def crawl(files, rounds=4):
    import numpy as np
    from afec_amd import hostlib
    from tests._aiff import aiff_bytes
    from tests._wav import wav_bytes
    rng = np.random.default_rng(2)
    t = np.arange(44100)
    pool = []
    for k in range(16):
        tone = np.sin(2 * np.pi * (110.0 * (k + 1)) * t / 44100.0) * np.exp(-(t % 11025) / 4000.0)
        mono = 12000 * tone + 2000 * rng.uniform(-1, 1, t.size)
        pool.append(np.round(np.stack([mono, 0.8 * np.roll(mono, 5)], axis=1)).astype(np.int16))
    sets = {"wav": ([wav_bytes(x, 2, 16) for x in pool], ".wav"), "aiff": ([aiff_bytes(x, 2, 16) for x in pool], ".aif")}
    rates = {"wav": [], "aiff": []}
    for round_ in range(rounds):
        for which, (images, ext) in sets.items():
            st = hostlib.crawl([images[i % 16] for i in range(files)], [f"f{i:06d}{ext}" for i in range(files)], files_per_batch=512)
            assert st["failed"] == 0 and st["files"] == files
            if round_:
                rates[which].append({"files_per_s": st["files"] / st["seconds"], "busy_cpus": st["cpu_seconds"] / st["seconds"]})
    hostlib.release()
    print(json.dumps({"files": files, **{k: v for k, v in rates.items()}}))


if __name__ == "__main__":
    if sys.argv[1] == "worker":
        worker(int(sys.argv[2]), float(sys.argv[3]), sys.argv[4])
    elif sys.argv[1] == "crawl":
        crawl(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 4)
    else:
        report(sys.argv[2])
