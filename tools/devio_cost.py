#!/usr/bin/env python3
"""What device-resident input and output cost next to the host paths.

  devio_cost.py worker [files] [seconds]   one batch of <files> (512) float files of <seconds> (1) s under AFX_D_ALL_PER_FRAME |
                                           AFX_D_STATISTICS.  Each in a bracket of HIP events of its own, medians of 7 after 3
                                           warm-up rounds: afx_batch_fetch_records into page-locked memory;
                                           afx_batch_export_device packed F64 and padded F32 (every series, one call each);
                                           afx_batch_create from page-locked memory; afx_batch_create_from_device.  One JSON line,
                                           with the bytes each kernel reads and writes.
  devio_cost.py report <dir> <worker.json> the kernels' own durations from the rocprofv3 kernel trace under <dir>, and their share
                                           of the rate a copy reaches on this part (profiles/r02/ubench_hbm_stream.txt: 4.7 TB/s of
                                           read + write), from the worker's byte counts

tools/devio_cost.sh runs the worker under `rocprofv3 --kernel-trace --stats` (no counters), then the report, then the worker
without the profiler for the brackets."""
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


class Bracket:
    """two HIP events on a stream of the tool's own around one call; the call either waits on the host (the bracket is then
    its wall time as the device saw it) or makes that stream wait for its launch"""

    def __init__(self, H, stream):
        self.H, self.stream = H, stream
        self.ev = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.ev:
            assert H.hipEventCreate(ctypes.byref(e)) == 0

    def __call__(self, call):
        H = self.H
        assert H.hipEventRecord(self.ev[0], self.stream) == 0
        call()
        assert H.hipEventRecord(self.ev[1], self.stream) == 0
        assert H.hipEventSynchronize(self.ev[1]) == 0
        ms = ctypes.c_float()
        assert H.hipEventElapsedTime(ctypes.byref(ms), self.ev[0], self.ev[1]) == 0
        return ms.value


def worker(files, seconds):
    import numpy as np
    import afec_amd as afx
    from afec_amd import capi, device
    rng = np.random.default_rng(1)
    n = int(44100 * seconds)
    H = device.hip()
    vp = ctypes.c_void_p
    H.hipEventCreate.argtypes, H.hipEventRecord.argtypes, H.hipEventSynchronize.argtypes = [ctypes.POINTER(vp)], [vp, vp], [vp]
    H.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    H.afx_batch_fetch_records.argtypes = [vp] * 6
    H.afx_batch_record_layout.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), vp, vp]
    mask = afx.D_ALL_PER_FRAME | afx.D_STATISTICS
    plan = afx.Plan()
    stream = device.Stream()
    bracket = Bracket(H, stream.handle)
    pool = [(0.5 * np.sin(2 * np.pi * 110.0 * (k + 1) * np.arange(n) / 44100.0) + 0.1 * rng.uniform(-1, 1, n)).astype(np.float32) for k in range(8)]
    pinned, owner = capi.pinned_array((files, n), np.float32)
    for i in range(files):
        pinned[i] = pool[i % 8]
    resident = device.DeviceArray.from_numpy(pinned)
    host_bufs = [pinned[i] for i in range(files)]

    batch = afx.create_batch_from_device(plan, resident, mask, lengths=[n] * files)
    batch.run()
    batch.sync()
    fo, _ = device.frame_offsets(batch)
    frames, longest = int(fo[-1]), int(np.diff(fo).max())
    stride = ctypes.c_int32()
    capi._check(plan.L, plan.L.afx_batch_record_layout(batch.h, ctypes.byref(stride), None, None))
    stride = stride.value
    records, owner2 = capi.pinned_array((frames, stride), np.float64)
    stats, owner3 = capi.pinned_array((files, stride, afx.NUM_STATISTICS), np.float64)
    names = device.SERIES
    packed = device.DeviceArray((frames, stride), np.float64)
    padded = device.DeviceArray((files, longest, stride), np.float32)
    cols, col = {}, 0
    for s, name in enumerate(names):
        cols[s] = col
        col += device.SERIES_WIDTH[name]
    assert col == stride
    outs64 = [(packed.ptr + cols[s] * 8, s, afx.PCM_F64, stride, 0) for s in range(len(names))]
    outs32 = [(padded.ptr + cols[s] * 4, s, afx.PCM_F32, stride, longest * stride) for s in range(len(names))]
    ms = {k: [] for k in ("fetch_records_pinned", "export_packed_f64", "export_padded_f32", "create_host_pinned", "create_from_device")}
    for round_ in range(10):
        ms["fetch_records_pinned"].append(bracket(lambda: capi._check(plan.L, plan.L.afx_batch_fetch_records(
            batch.h, records.ctypes.data, stats.ctypes.data, None, None, None))))
        ms["export_packed_f64"].append(bracket(lambda: device.export_into(batch, outs64, device.EXPORT_PACKED, 0, 0.0, stream)))
        ms["export_padded_f32"].append(bracket(lambda: device.export_into(batch, outs32, device.EXPORT_PADDED, longest, 0.0, stream)))
        made = []
        ms["create_host_pinned"].append(bracket(lambda: made.append(plan.batch(host_bufs, mask))))
        ms["create_from_device"].append(bracket(lambda: made.append(afx.create_batch_from_device(plan, resident, mask, lengths=[n] * files))))
        for b in made:
            b.close()
    want = batch.fetch()
    got = packed.download()
    assert all(np.array_equal(got[:, cols[s]:cols[s] + device.SERIES_WIDTH[name]].reshape(want[name].shape), want[name]) for s, name in enumerate(names))
    info = batch.info()
    print(json.dumps({"files": files, "seconds": seconds, "frames": frames, "stride": stride, "max_frames": longest,
                      "median_ms": {k: statistics.median(v[3:]) for k, v in ms.items()},
                      "min_ms": {k: min(v[3:]) for k, v in ms.items()},
                      "bytes": {"records_and_statistics_to_host": records.nbytes + stats.nbytes,
                                "devio_export_kernel packed f64": 2 * frames * stride * 8,
                                "devio_export_kernel padded f32": frames * stride * 8 + files * longest * stride * 4,
                                "devio_gather_kernel": 2 * info["arena_bytes"], "pcm_to_device": files * n * 4},
                      "build": afx.build_info()}))
    batch.close()
    plan.close()


def report(directory, worker_json):
    w = json.loads(open(worker_json).read().strip().splitlines()[-1])
    for trace in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        rows = list(csv.DictReader(open(trace)))
        for kernel, keys in (("devio_gather_kernel", ["devio_gather_kernel"]),
                             ("devio_export_kernel", ["devio_export_kernel packed f64", "devio_export_kernel padded f32"])):
            runs = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]]
            # the worker's launches alternate packed, padded; the gather's first launch is the resident batch's
            series = {keys[0]: runs[1:]} if len(keys) == 1 else {keys[0]: runs[0::2], keys[1]: runs[1::2]}
            for key, r in series.items():
                steady = r[3:] or r
                med = statistics.median(steady) / 1e3 if steady else None
                print(json.dumps({"kernel": key, "launches": len(r), "median_us": med, "min_us": min(steady) / 1e3 if steady else None,
                                  "max_us": max(steady) / 1e3 if steady else None, "bytes_read_plus_written": w["bytes"][key],
                                  "TB_per_s": w["bytes"][key] / (med * 1e-6) / 1e12 if med else None,
                                  "share_of_copy_rate_4.7TB_s": w["bytes"][key] / (med * 1e-6) / COPY_RATE if med else None}))


if __name__ == "__main__":
    if sys.argv[1] == "worker":
        worker(int(sys.argv[2]) if len(sys.argv) > 2 else 512, float(sys.argv[3]) if len(sys.argv) > 3 else 1.0)
    else:
        report(sys.argv[2], sys.argv[3])
