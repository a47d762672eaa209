#!/usr/bin/env python3
"""What afx_batch_fetch_class_decision costs next to afx_batch_fetch_class_signature (class decision).

  class_decision_cost.py <files> <seconds>   one batch of <files> files of <seconds> s (LoadSample front end) and the
                                             reference's OneShot-vs-Loops bagging: prints one JSON line with the wall times of
                                             the fetches the loaded library has (medians of 7 after 3 warm-up rounds, each
                                             behind a batch synchronise) and the bytes each brings to the host

The library is the tree's, or the one AFX_LIBRARY names: run it once with a build of the parent commit (which has the
signature fetch only) and once with this tree's, in one visit, for the two numbers of DESIGN's section."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(files, seconds):
    import numpy as np
    import afec_amd as afx
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
    mask = afx.D_CLASSIFICATION_INPUTS | afx.D_AMPLITUDE_PEAK
    b, _ = plan.batch_from_raw([(pool[i % 8], 1) for i in range(files)], mask)
    fetches = {"fetch_class_signature": lambda: b.fetch_class_signature(model)}
    if hasattr(b, "fetch_class_decision"):
        fetches["fetch_class_decision"] = lambda: b.fetch_class_decision(class_model=model)
    b.run()
    times = {k: [] for k in fetches}
    results = {}
    for _ in range(10):
        for name, fetch in fetches.items():      # alternating, so that both see the same machine
            b.run()
            b.sync()
            t0 = time.perf_counter()
            results[name] = fetch()
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = {"files": files, "seconds": seconds, "frames": b.total_frames, "build": afx.build_info()}
    for name in fetches:
        out[name + "_ms"] = statistics.median(times[name][3:])
        arrays = results[name].values() if isinstance(results[name], dict) else results[name]
        out[name + "_bytes"] = int(sum(a.nbytes for a in arrays))
    model.close()
    b.close()
    plan.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(sys.argv[1]), float(sys.argv[2]))
