"""The hop's way into the half-wave frame loop (afec_amd/csrc/afx_frames32.hip): every trip a wave moves the next frame's
new hop -- 4 KiB per half, from the chunk that half works on -- into its LDS plane by LDS-DMA, one trip ahead, and the
last frame of a chunk re-reads its own hop.  The image is [row][half][q]: every 1 KiB piece mixes both halves, so each lane
carries the address and the clamp of the half it fetches for, which is not the half it computes for.  What that addressing
can get wrong shows where the two halves of a wave differ: chunks of different length (the clamp on the frame index is
then active in one half only), an empty half, a half whose chunk starts off a 1 KiB boundary of the arena.

Batch shapes, one batch per class on a plan pinned to AFX_FRAME_KERNEL_HALFWAVE (MFCC class, statistics class `star`,
magnitude class AFX_D_ALL_LOW_LEVEL):
  * a one-frame buffer beside a 33-frame buffer: neighbours in the chunk table share a wave, one in each half;
  * buffers of exactly 32 and 64 frames;
  * 97 frames followed by a zero-length buffer;
  * a buffer whose length is 4 samples past its last frame, analysed with AFX_D_EFFECTIVE_LENGTH (the arena then keeps the
    whole buffer, rounded up to 4 samples): every buffer behind it starts at a sample offset that is a multiple of 4 floats
    and not of 256;
  * ballast (not compared) that makes the planner cut chunks of more than one frame, as tests/test_gpu_halfwave_seams.py
    explains, in a number that leaves the chunk count odd: the last wave has one empty half.

Each against the oracle at _tol.GPU_TOL, against the 64-lane kernel at the 1e-9 of tests/test_gpu_halfwave.py, and four
launches of one batch bit-equal to the first."""
import numpy as np
import pytest

import afec_amd as afx
from tests import _tol
from tests._oracle import FIELDS, Oracle

pytestmark = pytest.mark.gpu

STAR = (afx.D_MFCC | afx.D_SPECTRAL_RMS | afx.D_SPECTRAL_CENTROID | afx.D_SPECTRAL_SPREAD | afx.D_SPECTRAL_ROLLOFF |
        afx.D_SPECTRAL_FLATNESS)
MASKS = {"mfcc": afx.D_MFCC, "star": STAR, "all_low_level": afx.D_ALL_LOW_LEVEL}
FRAMES = (1, 33, 32, 64, 97, 0, 6, 5, 2)      # 0: a zero-length buffer; the 6-frame buffer carries 4 samples more
OFF_GRID = 6
BALLAST = 3000


def samples(frames):
    return 2048 + 1024 * (frames - 1) if frames > 0 else 0


@pytest.fixture(scope="module")
def buffers():
    rng = np.random.default_rng(1505)
    bufs = [rng.uniform(-1, 1, samples(n) + (4 if i == OFF_GRID else 0)).astype(np.float32) for i, n in enumerate(FRAMES)]
    t = np.arange(samples(33))
    bufs[1] = (0.5 * np.sin(2 * np.pi * 440.0 * t / 44100) + 0.05 * rng.uniform(-1, 1, t.size)).astype(np.float32)   # tonal
    block = rng.uniform(-1, 1, samples(BALLAST)).astype(np.float32)
    return bufs, [block] * 8


@pytest.fixture(scope="module")
def oracle_rows(buffers):
    o = Oracle()
    return [o.run(b.astype(np.float64)) if b.size >= 2048 else None for b in buffers[0]]


def run_batches(frame_kernel, bufs, launches):
    """{mask name: ([fetched fields after launch 1, after the last launch], batch info)}"""
    plan = afx.Plan(max_analysis_ms=0, frame_kernel=frame_kernel)
    out = {}
    try:
        for name, mask in MASKS.items():
            batch = plan.batch(bufs, mask | afx.D_EFFECTIVE_LENGTH)
            fetched = []
            for n in range(launches):
                batch.run()
                if n in (0, launches - 1):
                    batch.sync()
                    fetched.append({k: np.array(v, copy=True) for k, v in batch.fetch().items()})
            out[name] = (fetched, batch.info())
            batch.close()
    finally:
        plan.close()
    return out


@pytest.fixture(scope="module")
def halfwave(buffers):
    return run_batches(afx.FRAME_KERNEL_HALFWAVE, buffers[0] + buffers[1], 4)


@pytest.fixture(scope="module")
def lanes64(buffers):
    return run_batches(afx.FRAME_KERNEL_WAVE64, buffers[0] + buffers[1], 1)


@pytest.mark.parametrize("name", list(MASKS))
def test_the_batch_has_the_shapes_this_file_is_about(halfwave, name):
    info = halfwave[name][1]
    assert info["chunk_frames"] > 1, info          # the hop pointer advances inside a chunk, and is clamped at its end
    assert info["n_chunks"] % 2 == 1, info         # the last wave's second half is empty
    off = halfwave[name][0][0]["frame_offset"]
    assert [int(off[i + 1] - off[i]) for i in range(len(FRAMES))] == list(FRAMES)


@pytest.mark.parametrize("name", list(MASKS))
def test_against_the_oracle(halfwave, oracle_rows, name):
    got = halfwave[name][0][0]
    off = got["frame_offset"]
    for i, ref in enumerate(oracle_rows):
        if ref is None:
            assert off[i + 1] == off[i]
            continue
        assert off[i + 1] - off[i] == ref.shape[0]
        for field, (a, b) in FIELDS.items():
            if field == "mag" or field not in got:
                continue
            _tol.check_gpu(field, got[field][off[i]:off[i + 1]].reshape(ref.shape[0], -1), ref[:, a:b], *_tol.GPU_TOL[field],
                           what=f"{name} buffer {i} ({ref.shape[0]} frames) ")


@pytest.mark.parametrize("name", list(MASKS))
def test_against_the_64_lane_kernel(halfwave, lanes64, name):
    got, ref = halfwave[name][0][0], lanes64[name][0][0]
    assert got["frame_offset"].tolist() == ref["frame_offset"].tolist()
    rows = int(got["frame_offset"][len(FRAMES)])
    d = np.abs(got["mfcc"][:rows] - ref["mfcc"][:rows])
    print(f"{name}: max |half-wave - 64-lane| of the MFCC {d.max():.3e}")
    # two FFT factorisations of the same double arithmetic
    _tol.check("mfcc", got["mfcc"][:rows], ref["mfcc"][:rows], 1e-9, 1e-9, what="half-wave vs 64-lane ")


@pytest.mark.parametrize("name", list(MASKS))
def test_four_launches_of_one_batch_leave_the_same_bits(halfwave, name):
    first, last = halfwave[name][0]
    compared = [f for f in ("frame_offset", "buf_status", *FIELDS) if f in first]
    assert "mfcc" in compared
    for field in compared:
        assert first[field].tobytes() == last[field].tobytes(), field
