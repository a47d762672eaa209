#!/usr/bin/env python3
"""What FLAC input costs next to the same audio as WAV.

  flac_cost.py crawl <files> [rounds] [cache.npz]   the C4-share content (<files> one-second stereo 16-bit files, images in
                                                    memory, no database) crawled as WAV and as FLAC, alternating in one
                                                    process, rounds - 1 times each after one warm-up round: files/s, busy host
                                                    CPUs and uploaded bytes per file of either container.  The FLAC images are
                                                    written by tests/_flac.py (FIXED-2 / Rice): no libFLAC is needed.  cache.npz:
                                                    the encoded pool is kept there (pure-Python encoding takes seconds per file)
  flac_cost.py worker <files> [cache.npz]           one batch of <files> such files through afx_batch_create_from_raw, as FLAC
                                                    and as the native twin, alternating: the medians of 7 wall times after 3
                                                    warm-up rounds, and the host-to-device rate of a page-locked copy of the
                                                    bytes a FLAC batch saves, measured in the same run
  flac_cost.py report <dir>                         the three decode kernels' durations from the rocprofv3 kernel trace under <dir>

tools/flac_cost.sh runs the worker under `rocprofv3 --kernel-trace --stats`, the report, and the crawl with
AFEC_CRAWL_TIMING=1 (the workers' parse-phase seconds go to stderr)."""
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POOL = 8


def pool_of_files(cache=None):
    """POOL one-second stereo 16-bit signals -> (PCM arrays, WAV images, FLAC images)"""
    import numpy as np
    from tests import _flac
    from tests._wav import wav_bytes
    rng = np.random.default_rng(2)
    t = np.arange(44100)
    pcm = []
    for k in range(POOL):
        tone = np.sin(2 * np.pi * (110.0 * (k + 1)) * t / 44100.0) * np.exp(-(t % 11025) / 4000.0)
        mono = 12000 * tone + 2000 * rng.uniform(-1, 1, t.size)
        pcm.append(np.round(np.stack([mono, 0.8 * np.roll(mono, 5)], axis=1)).astype(np.int16))
    flac = None
    if cache and os.path.exists(cache):
        with np.load(cache) as z:
            flac = [z["f%d" % k].tobytes() for k in range(POOL)]
    if flac is None:
        flac = [_flac.fixed2_stream(x, 16, 44100, 4096) for x in pcm]
        if cache:
            np.savez(cache, **{"f%d" % k: np.frombuffer(f, dtype=np.uint8) for k, f in enumerate(flac)})
    return pcm, [wav_bytes(x, 2, 16) for x in pcm], flac


def crawl(files, rounds=8, cache=None):
    from afec_amd import hostlib
    _, wav, flac = pool_of_files(cache)
    sets = {"wav": (wav, ".wav"), "flac": (flac, ".flac")}
    rates = {"wav": [], "flac": []}
    for round_ in range(rounds):
        for which, (images, ext) in sets.items():
            st = hostlib.crawl([images[i % POOL] for i in range(files)], [f"f{i:06d}{ext}" for i in range(files)], files_per_batch=512)
            assert st["failed"] == 0 and st["files"] == files, st
            if round_:
                rates[which].append({"files_per_s": st["files"] / st["seconds"], "busy_cpus": st["cpu_seconds"] / st["seconds"],
                                     "uploaded_bytes_per_file": st["pcm_bytes"] / st["files"]})
    hostlib.release()
    print(json.dumps({"files": files, "file_bytes": {"wav": statistics.mean(len(i) for i in wav), "flac": statistics.mean(len(i) for i in flac)},
                      "median_files_per_s": {k: statistics.median(r["files_per_s"] for r in v) for k, v in rates.items()}, **rates}))


def worker(files, cache=None):
    import numpy as np
    import torch
    import afec_amd as afx
    from afec_amd import capi
    pcm, _, flac = pool_of_files(cache)
    plan = afx.Plan()
    native = [(pcm[i % POOL].view(np.uint8).reshape(-1), 2, 44100, capi.RAW_I16) for i in range(files)]
    streams = [capi.flac_stream(f, plan.L) for f in flac]
    coded = [(streams[i % POOL][0], 2, 44100, capi.RAW_FLAC, 44100) for i in range(files)]
    ms = {"native": [], "flac": []}
    for round_ in range(10):
        for which, raws in (("native", native), ("flac", coded)):
            t0 = time.perf_counter()
            b, infos = plan.batch_from_raw(raws, afx.D_MFCC)
            ms[which].append((time.perf_counter() - t0) * 1e3)
            b.close()
    up_native = sum(r[0].size for r in native)
    up_flac = sum(((streams[i % POOL][0].frames_bytes + 15) & ~15) + 16 * (streams[i % POOL][0].n_index + 1) for i in range(files))
    saved = up_native - up_flac
    host = torch.empty(max(saved, 1), dtype=torch.uint8).pin_memory()
    dev = torch.empty(max(saved, 1), dtype=torch.uint8, device="cuda")
    copy_ms = []
    for _ in range(8):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.copy_(host, non_blocking=True)
        torch.cuda.synchronize()
        copy_ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"files": files, "uploaded_bytes": {"native": up_native, "flac": up_flac}, "create_native_ms": statistics.median(ms["native"][3:]),
                      "create_flac_ms": statistics.median(ms["flac"][3:]), "saved_bytes": saved, "saved_bytes_copy_ms": statistics.median(copy_ms[2:]),
                      "link_GB_s": saved / statistics.median(copy_ms[2:]) / 1e6, "build": afx.build_info()}))
    plan.close()


def report(directory):
    for trace in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        rows = list(csv.DictReader(open(trace)))
        for kernel in ("flac_walk_kernel", "flac_restore_kernel", "flac_output_kernel"):
            runs = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]]
            steady = runs[3:] or runs
            print(json.dumps({"trace": os.path.relpath(trace, directory), "kernel": kernel, "launches": len(runs),
                              "median_us": statistics.median(steady) / 1e3 if steady else None,
                              "min_us": min(steady) / 1e3 if steady else None, "max_us": max(steady) / 1e3 if steady else None}))


if __name__ == "__main__":
    if sys.argv[1] == "crawl":
        crawl(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 8, sys.argv[4] if len(sys.argv) > 4 else None)
    elif sys.argv[1] == "worker":
        worker(int(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        report(sys.argv[2])
