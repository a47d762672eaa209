#!/usr/bin/env python3
"""tests/golden/classification.npz for tests/test_classification_ref_cpu.py: what the restatement of
TSampleClassificationDescriptors (tests/_classification_ref.py) makes of the reference's own low-level series of its fixture
WAVs (tests/golden/fixtures.npz), written once so that a later change of the restatement shows.  Data only.

fixtures.npz holds neither rhythm tracker results nor effective lengths; both pass through unchanged, so every file gets
made-up ones (made_up_scalars), stored next to the results.  Run from the repository root:
    python tests/golden/make_golden_classification.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import _classification_ref, _oracle  # noqa: E402


def fixture_series(z, i):
    """the SERIES of fixture file i from fixtures.npz (frames_i: the oracle record behind the magnitudes; neighbours_i)"""
    frames, neigh = z[f"frames_{i}"], z[f"neighbours_{i}"]
    first = _oracle.FIELDS["mag"][1]
    s = {}
    for k in _classification_ref.SERIES:
        if k in _oracle.FIELDS:
            a, b = _oracle.FIELDS[k]
            s[k] = frames[:, a - first:b - first] if b - a > 1 else frames[:, a - first]
        else:
            s[k] = neigh[:, sorted(_oracle.NEIGH_FIELDS.values()).index(_oracle.NEIGH_FIELDS[k])]
    return s


def made_up_scalars(i):
    """-> (the rhythm tracker's 14 scalars, effectve_length_12dB) of file i"""
    return np.array([0.03125 * i + 0.0078125 * k for k in range(14)]), 0.015625 * i


def main():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fixtures.npz"))
    out = {}
    for i in range(len(z["names"])):
        if f"frames_{i}" not in z:
            continue   # the file the reference refuses
        rhythm, length = made_up_scalars(i)
        values, _ = _classification_ref.classification_features(fixture_series(z, i), rhythm, length)
        out[f"features_{i}"] = values
        out[f"scalars_{i}"] = np.append(rhythm, length)
    out["silence"] = _classification_ref.silence_values()
    path = os.path.join(ROOT, "tests", "golden", "classification.npz")
    np.savez_compressed(path, **out)
    print(f"wrote tests/golden/classification.npz: {sum(k.startswith('features_') for k in out)} files, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
