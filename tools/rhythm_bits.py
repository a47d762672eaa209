#!/usr/bin/env python3
"""Did the rhythm tracker's results move by a bit?  The digests of a fixed set of inputs, to compare between two builds.

usage: [AFX_LIBRARY=<libafx_hip.so of another build>] tools/rhythm_bits.py [--oracle-only]

Runs the batches below with the library AFX_LIBRARY names (default: the tree's) and prints, per file, the sha256 of the four
quantities of tests/test_gpu_rhythm_paths.bits (onset_functions, onsets, scalars, onset_statistics) and, last, one digest
over all of them.  Run it once per build, each in a fresh process, and diff the outputs.  Generators and helpers are those
of tests/test_gpu_rhythm_paths.py.  All files are 44.1 kHz; f32 where nothing else is said:

  a257, a256   the 257- and the 256-file batch of case (a): short and long onset path, every filler and empty file
  table        the eight files of case (c): long, empty, short, refused, one frame -> T <= 0, T == 1, fewer than four onsets
  nocap        8191 / 8192 / 8193 / 300 frames without the 20 s cap: the series staged in LDS and read from global memory,
               several chunks of the staged sums, a length that is no multiple of 256; nocap1: 8193 alone, no dynamic LDS
  zeros        300 frames of zeros: no variance, every key of the radix select equal, the valley walk on ties
  f64, raw     the double and the int16 files of case (b), one small batch each

Before any GPU run the oracle (tests/_oracle.py, CPU) says which stages the set reaches, and the tool stops if one is
missing: for each onset function a file with at least four onsets (the beat tracker runs) and one with fewer, a file with
window peaks, and a file whose final tempo is the duration heuristics' and one whose final tempo is its chain's."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import afec_amd as afx                                  # noqa: E402
from tests import test_gpu_rhythm_paths as paths        # noqa: E402

ZEROS = np.zeros(512 + 128 * (paths.SHORT_FRAMES - 1), dtype=np.float32)
ONE_FRAME = (0.25 * np.random.default_rng(78).uniform(-1, 1, 512)).astype(np.float32)


def named_f32():
    """(name, signal, analysed with the cap) of every f32 file of interest"""
    short = paths.click_track(paths.SHORT_FRAMES)
    files = [(name, x, True) for name, x in paths.interest_f32()]
    files += [(f"f32:{paths.SHORT_FRAMES}", short, True), ("f32:one", ONE_FRAME, True), ("f32:zeros", ZEROS, True)]
    return files + [(f"nocap:{t}", paths.click_track(t), False) for t in paths.LDS_LENGTHS + (paths.SHORT_FRAMES,)]


def properties():
    """which file shows which property, by the oracle's scalars -> the properties nobody shows"""
    shown = {}
    for name, x, cap in named_f32():
        s = paths.reference(name, x, cap=cap)["scalars"]
        chain = 1 if s[8] > s[2] else 0                 # the more confident function's chain (rhythm_final_kernel)
        has = [f"{fn} onset_count {'>= 4' if s[6 * t] >= 4 else '< 4'}" for t, fn in enumerate(("complex", "power"))]
        has += [f"{fn} peak count > 0" for t, fn in enumerate(("complex", "power")) if s[6 * t + 3] > 0]
        has.append("final tempo differs from its chain's" if s[12] != s[6 * chain + 1] else "final tempo is its chain's")
        for h in has:
            shown.setdefault(h, []).append(name)
        print(f"oracle {name}: " + "; ".join(has))
    wanted = [f"{fn} onset_count {c}" for fn in ("complex", "power") for c in (">= 4", "< 4")]
    wanted += ["complex peak count > 0", "power peak count > 0", "final tempo differs from its chain's", "final tempo is its chain's"]
    for w in wanted:
        print(f"property [{w}]: {', '.join(shown.get(w, [])) or 'MISSING'}")
    return [w for w in wanted if w not in shown]


def batches():
    """-> (tag, plan arguments, make(plan) -> fetched result, number of files)"""
    def plain(bufs):
        return lambda plan: paths.run(plan, bufs)

    def raw(pcms):
        def make(plan):
            b, _ = plan.batch_from_raw([(pcm, 1) for pcm in pcms], paths.MASK)
            try:
                b.run()
                return paths.fetch(b)
            finally:
                b.close()
        return make
    out = []
    for n in (paths.LONG_BATCH_FILES + 1, paths.LONG_BATCH_FILES):
        bufs, _ = paths.spread(paths.interest_f32(), n, np.float32)
        out.append((f"a{n}", {}, plain(bufs), n))
    a, b, c, d = (paths.click_track(t) for t in paths.TABLE_LONG_LENGTHS)
    table = [a, np.zeros(0, dtype=np.float32), paths.click_track(paths.SHORT_FRAMES), b,
             paths.click_track(paths.SHORT_FRAMES, dtype=np.float64), c, ONE_FRAME, d]
    out.append(("table", {}, plain(table), len(table)))
    nocap = [paths.click_track(t) for t in paths.LDS_LENGTHS + (paths.SHORT_FRAMES,)]
    out.append(("nocap", {"max_analysis_ms": 0}, plain(nocap), len(nocap)))
    out.append(("nocap1", {"max_analysis_ms": 0}, plain([nocap[2]]), 1))
    out.append(("zeros", {}, plain([ZEROS]), 1))
    out.append(("f64", {}, plain([x for _, x in paths.interest_f64()]), len(paths.interest_f64())))
    out.append(("raw", {}, raw([pcm for _, pcm in paths.interest_raw()]), len(paths.interest_raw())))
    return out


def main():
    missing = properties()
    if missing:
        print("the set does not show:", missing)
        return 2
    if "--oracle-only" in sys.argv[1:]:
        return 0
    print("library:", afx.library_path(), "|", afx.build_info())
    whole = hashlib.sha256()
    plans = {}
    for tag, plan_args, make, n_files in batches():
        key = tuple(sorted(plan_args.items()))
        if key not in plans:
            plans[key] = afx.Plan(**plan_args)
        r = make(plans[key])
        assert len(r["offsets"]) == n_files + 1, tag
        for i in range(n_files):
            digests = [hashlib.sha256(v).hexdigest() for v in paths.bits(r, i).values()]
            print(f"{tag}[{i}] frames={r['offsets'][i + 1] - r['offsets'][i]} " + " ".join(digests))
            whole.update("".join(digests).encode())
    for p in plans.values():
        p.close()
    print("all:", whole.hexdigest())
    return 0


if __name__ == "__main__":
    sys.exit(main())
