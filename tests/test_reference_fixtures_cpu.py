"""The oracle against the reference's own objects on ALL of the reference's fixture WAVs (75 files under
Source/Crawler/XUnitTests/Resources/Kicks-vs-Snare-{Train,Test}: the folders UnitTests.cpp:152-423 crawls): their
images are under tests/golden/reference_wav/ (or tests/golden/wav/), and tests/golden/fixtures.npz
(tests/golden/make_golden_fixtures.py, from oracle/_ref/ref_driver) holds what LoadSample's converters, the per-frame
spectral loop and its neighbours of the reference made of each, and the oracle must agree -- LoadSample bit for bit,
the descriptors to 1e-6 (another FFT algorithm).  tests/golden/wav/ holds thirteen of these files with their expected
values for the GPU box.  CPU only."""
import hashlib
import os

import numpy as np

from tests import _oracle, _tol
from tests._oracle import FIELDS, NEIGH_FIELDS, Oracle
from tests._wav import parse_wav

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_every_fixture_of_the_reference():
    z = np.load(os.path.join(GOLD, "fixtures.npz"))
    names = [str(n) for n in z["names"]]
    spectral = FIELDS["mag"][1]
    neigh_cols = sorted(NEIGH_FIELDS.values())
    ora = Oracle()
    checked = frames = rejected = 0
    for i, name in enumerate(names):
        if f"stored_{i}" in z.files:
            image = open(os.path.join(GOLD, "wav", str(z[f"stored_{i}"])), "rb").read()
        else:
            image = open(os.path.join(GOLD, "reference_wav", name), "rb").read()
        try:
            channels, rate, bits, n, payload = parse_wav(image)
        except ValueError:
            rejected += 1                                   # "_Not A Wavefile.wav": UnitTests.cpp:338-350 expects exactly this one to fail
            continue
        assert rate == 44100 and bits in (16, 24), name
        data = np.frombuffer(payload, dtype=np.int16 if bits == 16 else np.uint8)
        peakrms, info_ref = z[f"peakrms_{i}"], z[f"info_{i}"]
        mono, info = _oracle.load_sample(data, channels)
        assert [info["data_offset"], info["silent_leading"], info["silent_trailing"], info["n_samples"]] == info_ref.tolist(), name
        assert hashlib.sha256(np.ascontiguousarray(mono, dtype=np.float64).tobytes()).digest() == z[f"mono_sha_{i}"].tobytes(), name
        assert np.float32(info["peak_value"]) == peakrms[0] and abs(info["rms_value"] - peakrms[1]) <= 1e-6 * peakrms[1], name
        want = z[f"frames_{i}"]                             # the record without the magnitude columns
        rec = ora.run(mono, cap=True)
        assert rec.shape[0] == want.shape[0], name
        for field, (a, b) in FIELDS.items():
            if field == "mag":
                continue
            rtol, atol = _tol.GPU_TOL[field]
            _tol.check(field, rec[:, a:b], want[:, a - spectral:b - spectral], min(rtol, 1e-6) if rtol else 0.0, atol, what=f"{name} oracle ")
        want_n = z[f"neighbours_{i}"]                       # the neighbours record's NEIGH_FIELDS columns, in column order
        nei = ora.run_neighbours(mono, cap=True)
        for field, col in NEIGH_FIELDS.items():
            rtol, atol = _tol.NEIGH_TOL[field]
            _tol.check(field, nei[:, col], want_n[:, neigh_cols.index(col)], rtol, atol, what=f"{name} oracle ")
        checked += 1
        frames += rec.shape[0]
    assert rejected == 1 and checked == len(names) - 1 and checked >= 70 and frames > 500
