#!/usr/bin/env python3
"""Goldens of the seeded cases tests/test_oracle.py and tests/test_oracle_resample.py hold against the reference's own
objects beyond the other goldens: three buffers through the per-frame spectral loop (oracle/_ref/ref_driver frames) and
60 random rates and lengths through the reference's libresample (ref_driver resample).  Inputs are seeded (the tests
regenerate them from the functions below), outputs are stored: the frames in full, the conversions in full for the short
ones and as (sha256, first / last 64 samples) for the long ones.  Run in the build container:
    python tests/golden/make_golden_spot.py      -> tests/golden/spot.npz"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
SHORT_OUTPUT = 10000     # conversions up to this many output samples are stored in full
sys.path.insert(0, ROOT)


def frames_buffers():
    rng = np.random.default_rng(7)
    return [rng.uniform(-1, 1, 2048 + 1024 * 5), 0.3 * rng.standard_normal(5000),
            np.sin(2 * np.pi * 3000 * np.arange(9000) / 44100) * np.linspace(1, 0, 9000)]


def resample_cases():
    """-> [(file rate, samples, the "16-bit float" buffer)]"""
    rng = np.random.default_rng(2026)
    out = []
    for _ in range(60):
        rate = int(rng.choice([8000, 11025, 16000, 22050, 32000, 48000, 88200, 96000, 176400, 192000])) if rng.random() < 0.5 else int(rng.integers(3000, 400000))
        n = int(rng.choice([1, 2, 3, 4039, 4040, 4041])) if rng.random() < 0.2 else int(np.exp(rng.uniform(np.log(5), np.log(60000))))
        out.append((rate, n, np.round(rng.uniform(-30000, 30000, n)).astype(np.float32)))
    return out


def run_ref_frames(bufs):
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "i"), os.path.join(d, "o")
        with open(fin, "wb") as f:
            f.write(struct.pack("<q", len(bufs)))
            for b in bufs:
                f.write(struct.pack("<q", b.size))
                f.write(b.astype(np.float64).tobytes())
        subprocess.check_call([REF, "frames", fin, fout, "0"])
        raw = open(fout, "rb").read()
    from tests import _oracle
    return np.frombuffer(raw[8:], dtype=np.float64).reshape(-1, _oracle.RECORD).copy()


def main():
    from tests.golden.make_golden_resample import run_ref_resample
    if not os.path.exists(REF):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
    out = {"frames": run_ref_frames(frames_buffers())}
    cases = []
    for k, (rate, n, x) in enumerate(resample_cases()):
        y, written, used = run_ref_resample(x, rate)
        cases.append((rate, n, y.size, written, used))
        if y.size <= SHORT_OUTPUT:
            out[f"resample_out_{k}"] = y
        else:
            out[f"resample_head_{k}"], out[f"resample_tail_{k}"] = y[:64], y[-64:]
            out[f"resample_sha_{k}"] = np.frombuffer(hashlib.sha256(y.tobytes()).digest(), dtype=np.uint8)
    out["resample_cases"] = np.array(cases, dtype=np.int64)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "spot.npz"), **out)
    print(f"wrote tests/golden/spot.npz: {out['frames'].shape[0]} frames, {len(cases)} conversions")


if __name__ == "__main__":
    sys.exit(main())
