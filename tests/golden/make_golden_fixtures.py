#!/usr/bin/env python3
"""Goldens of ALL of the reference's fixture WAVs (75 files under Source/Crawler/XUnitTests/Resources/Kicks-vs-Snare-
{Train,Test}: the folders UnitTests.cpp:152-423 crawls) for tests/test_reference_fixtures_cpu.py: each file's image and
what the reference's own objects (oracle/_ref/ref_driver, built by `make -C oracle ref`) make of it -- LoadSample's
converters (peak / rms, offsets and lengths, the normalised buffer as a sha256 of its doubles), the per-frame spectral
loop without the magnitude columns and its neighbours.  The images are copied to tests/golden/reference_wav/<the path
under Resources>, except those identical to one under tests/golden/wav/, which are recorded by that file's name.  Run in
the build container:
    python tests/golden/make_golden_fixtures.py <the reference checkout>
        -> tests/golden/fixtures.npz (the values) + tests/golden/reference_wav/ (the images)"""
import glob
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
WAV_DIR = os.path.join(ROOT, "tests", "golden", "wav")
IMAGE_DIR = os.path.join(ROOT, "tests", "golden", "reference_wav")
sys.path.insert(0, ROOT)

from tests import _oracle  # noqa: E402
from tests._wav import parse_wav  # noqa: E402


def main(reference):
    from tests.golden.make_golden import run_ref
    from tests.golden.make_golden_wav import run_ref_load
    if not os.path.exists(REF):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
    resources = os.path.join(reference, "Source", "Crawler", "XUnitTests", "Resources")
    files = sorted(glob.glob(os.path.join(resources, "**", "*.[wW][aA][vV]"), recursive=True))
    stored = {open(os.path.join(WAV_DIR, f), "rb").read(): f for f in os.listdir(WAV_DIR)}
    spectral = _oracle.FIELDS["mag"][1]
    neigh_cols = sorted(_oracle.NEIGH_FIELDS.values())
    out, names = {}, []
    for i, path in enumerate(files):
        names.append(os.path.relpath(path, resources))
        image = open(path, "rb").read()
        if image in stored:
            out[f"stored_{i}"] = np.array(stored[image])
        else:
            dst = os.path.join(IMAGE_DIR, names[-1])
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            with open(dst, "wb") as f:
                f.write(image)
        try:
            channels, rate, bits, n, payload = parse_wav(image)
        except ValueError:
            continue                                        # "_Not A Wavefile.wav": the test expects exactly this one to fail
        peakrms, info, mono = run_ref_load(payload, 0 if bits == 16 else 1, channels, n)
        out[f"peakrms_{i}"], out[f"info_{i}"] = peakrms, info
        out[f"mono_sha_{i}"] = np.frombuffer(hashlib.sha256(mono.tobytes()).digest(), dtype=np.uint8)
        out[f"frames_{i}"] = run_ref([mono], cap=1)[:, spectral:]
        out[f"neighbours_{i}"] = run_ref([mono], cap=1, mode="neighbours", record=_oracle.NEIGH_RECORD)[:, neigh_cols]
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "fixtures.npz"), **out)
    print(f"wrote tests/golden/fixtures.npz: {len(files)} files, {sum(k.startswith('stored_') for k in out)} of them as tests/golden/wav/ names, "
          f"the others under tests/golden/reference_wav/")


if __name__ == "__main__":
    main(sys.argv[1])
