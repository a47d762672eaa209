#!/usr/bin/env python3
"""What the whole high-level row costs out of one fetch next to the two fetches it replaces plus the host's formatting of the
six class columns (the high-level row).

  high_level_row_cost.py <files> <seconds> [rows]   one batch of <files> files of <seconds> s (LoadSample front end, the mask
                                              AFX_D_CLASS_DECISION_INPUTS | AFX_D_HIGH_LEVEL_INPUTS), the reference's
                                              OneShot-vs-Loops bagging and a 16-class category model of one-leaf trees: prints
                                              one JSON line with, over 7 rounds after 3 warm-up rounds, each behind a batch
                                              synchronise, a host clock around calls that end in the download,
      (a) afx_batch_fetch_high_level_text into page-locked memory, afx_batch_fetch_class_decision, and the six class columns
          of all files formatted on one host thread (tools/host_format/host_format.cpp, snprintf("%.9g")): median, minimum
          and maximum of the sum, and the medians of the three parts;
      (b) where the loaded library has it, afx_batch_fetch_high_level_row into page-locked memory: median, minimum, maximum;
          its text is compared with (a)'s, byte for byte;
      and, with (b), the rows per second of the high-level pool's InsertHighLevelRows for <rows> rows (default 12 500, the
      batch's rows over and over under distinct file names) into a fresh database in one transaction.

AFX_TREE names another checkout to import afec_amd from: run it on a built checkout of the parent commit for (a) and on this
tree for (a) and (b), alternating, in one visit."""
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.environ.get("AFX_TREE") or os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

CLASS_NAMES = ["Loop", "OneShot"]
CATEGORY_NAMES = ["None", "Bass", "Kick", "Snare", "Clap", "Hi Hat", "Cymbal", "Tom", "Percussion", "Chord", "Pad", "Lead", "Pluck", "Vocal",
                  "FX", "Texture"]
WEIGHTS = [0.01, 0.22, 0.2, 0.15, 0.1, 0.08, 0.06, 0.05, 0.04, 0.03, 0.02, 0.012, 0.011, 0.01, 0.004, 0.003]


def host_formatter():
    lib = os.path.join(HERE, "host_format", "libhost_format.so")
    src = os.path.join(HERE, "host_format", "host_format.cpp")
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", lib, src])
    L = ctypes.CDLL(lib)
    L.host_format_class_columns.restype = ctypes.c_int64
    L.host_format_class_columns.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int32] + [ctypes.c_void_p] * 3 + [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    return L


def main(files, seconds, pool_rows):
    import math
    import numpy as np
    import afec_amd as afx
    from afec_amd import capi
    from tests import _gbdt_ref as gbdt
    rng = np.random.default_rng(1)
    n = int(44100 * seconds)
    t = np.arange(n)
    pcm = []
    for k in range(8):
        tone = np.sin(2 * np.pi * (110.0 * (k + 1)) * t / 44100.0) * np.exp(-(t % 11025) / 4000.0)
        pcm.append(np.round(12000 * tone + 2000 * rng.uniform(-1, 1, n) * (t % 22050 < 6000)).astype(np.int16))
    H = host_formatter()
    plan = afx.Plan()
    z = np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", "oneshot_vs_loops_model.npz"))
    class_model = afx.Model(plan, [gbdt.write_lightgbm(m) for m in gbdt.unpack_models(z)], z["scale"], z["offset"], z["limits"])
    identity = (np.ones(1680), np.zeros(1680), np.full(1680, 1e300))
    category_model = afx.Model(plan, [gbdt.write_lightgbm(gbdt.make_model([math.log(w) for w in WEIGHTS], len(WEIGHTS)))], *identity)
    K = len(WEIGHTS)
    b, infos = plan.batch_from_raw([(pcm[i % 8], 1) for i in range(files)], afx.D_CLASS_DECISION_INPUTS | afx.D_HIGH_LEVEL_INPUTS)
    L = b.L
    b.run()
    levels = (capi._LoadInfo * files)()
    for i, d in enumerate(infos):
        levels[i].peak_value, levels[i].rms_value = d["peak_value"], d["rms_value"]
    status = np.zeros(files, dtype=np.int32)
    # (a) the vector columns' text into page-locked memory, the decision's arrays, the host's text of them
    capacity = b.high_level_text_capacity()
    text, keep_text = capi.pinned_array((max(1, capacity),), np.uint8)
    scalars = np.zeros((files, 15))
    begin, length = np.zeros((files, 3), dtype=np.int64), np.zeros((files, 3), dtype=np.int32)
    tout = capi._HighTextOut(scalars=scalars.ctypes.data, text=text.ctypes.data, text_capacity=capacity, begin=begin.ctypes.data,
                             length=length.ctypes.data, status=status.ctypes.data)
    desc = capi._DecisionDesc(class_model=class_model.h, loop_class=0, oneshot_class=1, use_heuristics=1, category_model=category_model.h,
                              category_none_class=0)
    dout, decision = capi._decision_out(files, True, K)
    names = [s.encode("utf-8") for s in CLASS_NAMES + CATEGORY_NAMES]
    name_bytes = np.frombuffer(b"".join(names), dtype=np.uint8).copy()
    name_length = np.array([len(s) for s in names], dtype=np.int32)
    name_offset = (np.cumsum(name_length) - name_length).astype(np.int32)
    host_text = np.zeros(files * (4 * 34 + 2 * 34 * K + 8 + int(name_length.sum()) + 3 * len(names)), dtype=np.uint8)
    # (b) the whole row into page-locked memory
    with_row = hasattr(b, "fetch_high_level_row") and hasattr(L, "afx_batch_fetch_high_level_row")
    if with_row:
        rdesc, keep_names = b._row_desc(class_model, category_model, CLASS_NAMES, CATEGORY_NAMES, 0, 1, True, 0)
        row_capacity = int(L.afx_batch_high_level_row_capacity(b.h, ctypes.byref(rdesc)))
        row_text, keep_row = capi.pinned_array((max(1, row_capacity),), np.uint8)
        row = {"scalars": np.zeros((files, 15)), "begin": np.zeros((files, 9), dtype=np.int64), "length": np.zeros((files, 9), dtype=np.int32),
               "flags": np.zeros(files, dtype=np.int32), "non_finite": np.zeros(files, dtype=np.int32), "confidences": np.zeros((files, 2)),
               "status": np.zeros(files, dtype=np.int32)}
        rout = capi._RowOut(text=row_text.ctypes.data, text_capacity=row_capacity, **{k: a.ctypes.data for k, a in row.items()})
    times = {"fetch_high_level_text": [], "fetch_class_decision": [], "format_class_columns": [], "two_fetches_and_host": [], "fetch_high_level_row": []}
    host_bytes = 0
    for _ in range(10):
        b.run()
        b.sync()
        t0 = time.perf_counter()
        assert L.afx_batch_fetch_high_level_text(b.h, levels, ctypes.byref(tout)) == 0
        t1 = time.perf_counter()
        assert L.afx_batch_fetch_class_decision(b.h, ctypes.byref(desc), ctypes.byref(dout)) == 0
        t2 = time.perf_counter()
        host_bytes = H.host_format_class_columns(decision["class_signature"].ctypes.data, decision["class_strengths"].ctypes.data,
                                                 decision["classes"].ctypes.data, decision["category_signature"].ctypes.data,
                                                 decision["category_strengths"].ctypes.data, decision["categories"].ctypes.data, K,
                                                 name_bytes.ctypes.data, name_offset.ctypes.data, name_length.ctypes.data, files, 0,
                                                 host_text.ctypes.data)
        t3 = time.perf_counter()
        for name, ms in (("fetch_high_level_text", t1 - t0), ("fetch_class_decision", t2 - t1), ("format_class_columns", t3 - t2),
                         ("two_fetches_and_host", t3 - t0)):
            times[name].append(ms * 1e3)
        if with_row:                                 # alternating, so that both see the same machine
            b.run()
            b.sync()
            t0 = time.perf_counter()
            assert L.afx_batch_fetch_high_level_row(b.h, levels, ctypes.byref(rdesc), ctypes.byref(rout)) == 0
            times["fetch_high_level_row"].append((time.perf_counter() - t0) * 1e3)
    out = {"files": files, "seconds": seconds, "frames": b.total_frames, "build": afx.build_info(), "host_class_text_bytes": int(host_bytes)}
    for name, ms in times.items():
        if ms:
            out[name + "_ms"] = statistics.median(ms[3:])
    for name in ("two_fetches_and_host", "fetch_high_level_row"):
        if times[name]:
            out[name + "_min_ms"], out[name + "_max_ms"] = min(times[name][3:]), max(times[name][3:])
    if with_row:
        # the row's text is (a)'s: the class columns the host's bytes, the vector columns the text fetch's
        rb, rl = row["begin"], row["length"]
        joined = b"".join(row_text[rb[i, c]:rb[i, c] + rl[i, c]].tobytes() for i in range(files) for c in range(6))
        assert joined == host_text[:host_bytes].tobytes(), "the GPU's class columns differ from the host's"
        for i in range(files):
            for c in range(3):
                assert row_text[rb[i, 6 + c]:rb[i, 6 + c] + rl[i, 6 + c]].tobytes() == text[begin[i, c]:begin[i, c] + length[i, c]].tobytes()
        assert row["scalars"].tobytes() == scalars.tobytes() and row["flags"].tobytes() == decision["flags"].tobytes()
        out["row_text_bytes"] = int(rl.sum())
        out["row_downloaded_bytes"] = int(row_capacity + rb.nbytes + rl.nbytes + row["scalars"].nbytes + 4 * 8 * files)
        # the pool: the batch's rows over and over under distinct names, one transaction
        from afec_amd import hostlib
        index = np.arange(pool_rows) % files
        many = {"scalars": row["scalars"][index], "text": row_text, "begin": rb[index], "length": rl[index], "status": row["status"][index],
                "non_finite": row["non_finite"][index]}
        file_names = ["/samples/pack %04d/file %06d.wav" % (i // 100, i) for i in range(pool_rows)]
        props = [{"type": "wav", "size": 44 + 2 * n, "length": seconds, "sample_rate": 44100, "channels": 1, "bit_depth": 16}] * pool_rows
        with tempfile.TemporaryDirectory() as d:
            with hostlib.HighLevelPool(os.path.join(d, "high.db")) as pool:
                pool.insert_classifier("Classifiers", CLASS_NAMES)
                pool.insert_classifier("OneShot-Categories", CATEGORY_NAMES)
                t0 = time.perf_counter()
                failed = pool.insert_rows(file_names, np.arange(pool_rows), props, many)
                dt = time.perf_counter() - t0
            out["pool_rows"], out["pool_failed"], out["pool_rows_per_s"] = pool_rows, failed, pool_rows / dt
            out["pool_database_bytes"] = os.path.getsize(os.path.join(d, "high.db"))
    class_model.close()
    category_model.close()
    b.close()
    plan.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(sys.argv[1]), float(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 12500)
