#!/usr/bin/env python3
"""tests/golden/highlevel.npz for tests/test_highlevel_ref_cpu.py: what the restatement of AnalyzeHighLevelDescriptors
(tests/_highlevel_ref.py) makes of the reference's own low-level series and peak / rms of its 75 fixture WAVs
(tests/golden/fixtures.npz), written once so that a later change of the restatement shows.  Data only.

fixtures.npz holds no rhythm tracker results; the BPM passes through a quantisation only, so every file gets a made-up
final tempo and confidence, stored next to the results.  Run from the repository root:
    python tests/golden/make_golden_highlevel.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import _highlevel_ref, _oracle  # noqa: E402


def fixture_series(z, i):
    """the SERIES of fixture file i from fixtures.npz (frames_i: the oracle record behind the magnitudes; neighbours_i)"""
    frames, neigh = z[f"frames_{i}"], z[f"neighbours_{i}"]
    first = _oracle.FIELDS["mag"][1]
    s = {}
    for k in _highlevel_ref.SERIES:
        if k in _oracle.FIELDS:
            a, b = _oracle.FIELDS[k]
            s[k] = frames[:, a - first:b - first] if b - a > 1 else frames[:, a - first]
        else:
            s[k] = neigh[:, sorted(_oracle.NEIGH_FIELDS.values()).index(_oracle.NEIGH_FIELDS[k])]
    return s


def made_up_tempo(i):
    return 60.0 + 1.37 * i, 0.01 * i


def main():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fixtures.npz"))
    out = {}
    for i in range(len(z["names"])):
        if f"frames_{i}" not in z:
            continue   # the file the reference refuses
        tempo, tempo_confidence = made_up_tempo(i)
        peak, rms = z[f"peakrms_{i}"]
        r = _highlevel_ref.high_level(fixture_series(z, i), tempo, tempo_confidence, peak, rms)
        out[f"tempo_{i}"] = np.array([tempo, tempo_confidence])
        for k in ("scalars", "signature", "pitch"):   # "peak" is the input series itself
            out[f"{k}_{i}"] = r[k]
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "highlevel.npz"), **out)
    print(f"wrote tests/golden/highlevel.npz: {sum(k.startswith('scalars_') for k in out)} files")


if __name__ == "__main__":
    main()
