"""Seams of the half-wave frame loop (afec_amd/csrc/afx_frames32.hip): what the hand-over of the overlap half from frame
to frame, the start of a chunk, the two halves of a wave and the two slots of finish_mfcc32 can get wrong.

A plan pinned to AFX_FRAME_KERNEL_HALFWAVE runs buffers of 1, 2, 3, 32, 33 and 65 frames (odd totals for the trailing
finish_mfcc32; neighbours of different lengths share a wave, one in each half) and a 70-frame buffer with five of its
own tails, once per class of the kernel: MFCC alone, the `star` set (statistics class) and AFX_D_ALL_LOW_LEVEL (full
class), each against the oracle at the bars and ceilings of tests/_tol.py.

The planner chooses the chunk length from the size of the batch (choose_chunk_frames: one frame per chunk for a batch
this small, 32 only from millions of frames), and with one frame per chunk nothing is ever handed over.  So every batch
here carries ballast -- eight buffers of 3 000 frames, not compared -- which makes the chunks three frames long: frames
at positions 0, 1 and 2 of a chunk, and a chunk seam every three frames.  The tests assert that the chunks have more
than one frame.

Position independence: the arithmetic of a frame does not depend on where the frame sits, so row f of a buffer x must
equal row 0 of the buffer x[1024 f:] of the same batch BIT FOR BIT (f = 1, 31, 32, 33, 69: handed-over and chunk-start
frames, both halves, both slots).  The parent of the commit that added this file meets that bit for bit as well."""
import numpy as np
import pytest

import afec_amd as afx
from tests import _tol
from tests._oracle import FIELDS, Oracle

pytestmark = pytest.mark.gpu

SEAM_FRAMES = (1, 2, 3, 32, 33, 65)
TAILS = (1, 31, 32, 33, 69)
STAR = (afx.D_MFCC | afx.D_SPECTRAL_RMS | afx.D_SPECTRAL_CENTROID | afx.D_SPECTRAL_SPREAD | afx.D_SPECTRAL_ROLLOFF |
        afx.D_SPECTRAL_FLATNESS)
MASKS = {"mfcc": afx.D_MFCC, "star": STAR, "all_low_level": afx.D_ALL_LOW_LEVEL}


def samples(frames):
    return 2048 + 1024 * (frames - 1)


@pytest.fixture(scope="module")
def buffers():
    """the buffers under test, then the ballast"""
    rng = np.random.default_rng(77)
    bufs = [rng.uniform(-1, 1, samples(n)).astype(np.float32) for n in SEAM_FRAMES]
    t = np.arange(samples(33))
    bufs[4] = (0.5 * np.sin(2 * np.pi * 440.0 * t / 44100) + 0.05 * rng.uniform(-1, 1, t.size)).astype(np.float32)   # tonal
    x = (rng.standard_normal(samples(70)) * np.exp(-np.arange(samples(70)) / 30000.0)).astype(np.float32)
    bufs.append(x)
    bufs += [x[1024 * f:].copy() for f in TAILS]
    block = rng.uniform(-1, 1, samples(3000)).astype(np.float32)
    return bufs, [block] * 8


@pytest.fixture(scope="module")
def oracle_rows(buffers):
    o = Oracle()
    return [o.run(b.astype(np.float64)) for b in buffers[0]]


@pytest.fixture(scope="module")
def results(buffers):
    """{mask name: (fetched fields, batch info)} of one batch per mask on a plan pinned to the half-wave kernel"""
    bufs, ballast = buffers
    plan = afx.Plan(max_analysis_ms=0, frame_kernel=afx.FRAME_KERNEL_HALFWAVE)
    out = {}
    try:
        for name, mask in MASKS.items():
            batch = plan.batch(bufs + ballast, mask)
            batch.run()
            batch.sync()
            out[name] = (batch.fetch(), batch.info())
            batch.close()
    finally:
        plan.close()
    return out


@pytest.mark.parametrize("name", list(MASKS))
def test_seam_buffers_match_the_oracle(results, oracle_rows, buffers, name):
    got, info = results[name]
    assert info["chunk_frames"] > 1, info     # frames are handed over inside a chunk
    off = got["frame_offset"]
    for i, ref in enumerate(oracle_rows):
        assert off[i + 1] - off[i] == ref.shape[0]
        for field, (a, b) in FIELDS.items():
            if field == "mag" or field not in got:
                continue
            _tol.check_gpu(field, got[field][off[i]:off[i + 1]].reshape(ref.shape[0], -1), ref[:, a:b], *_tol.GPU_TOL[field],
                           what=f"{name} buffer {i} ({ref.shape[0]} frames) ")


def test_mfcc_of_a_frame_does_not_depend_on_its_position(results):
    got, info = results["mfcc"]
    assert info["chunk_frames"] > 1, info
    off = got["frame_offset"]
    whole = len(SEAM_FRAMES)
    assert off[whole + 1] - off[whole] == 70
    for i, f in enumerate(TAILS):
        tail = whole + 1 + i
        assert off[tail + 1] - off[tail] == 70 - f
        row, first = got["mfcc"][off[whole] + f], got["mfcc"][off[tail]]
        print(f"frame {f}: max |difference| {np.max(np.abs(row - first)):.3e}")
        assert np.array_equal(row.view(np.uint64), first.view(np.uint64)), (f, row, first)
