"""The partner fetch of the half-wave MFCC loop (afec_amd/csrc/afx_frames32.hip, stage U of class 0) on the GPU.

The untangle of bin k = 32 r + q pairs Z[k] with Z[1024 - k]: register v[31 - r] of lane 32 - q, for lanes 0 and 32 their
own v[(32 - r) & 31], for lane 16 its own v[31 - r].  Class 0 delivers the partner through the wave's plane in three
batches of four rows (tests/test_partner_plane_cpu.py has the map).  With a wrong partner |X[k]| is wrong by its own size,
and a tone at bin k makes that an O(1) error of the mel filter that holds the bin rather than one term of a noise sum: every
buffer here is three frames of 0.5 sin(2 pi k n / 2048) plus uniform noise at 0.05 (the mix of the tonal seam buffer of
tests/test_gpu_halfwave_seams.py), at the bins the lane map can get wrong:

    32 r, r = 1..11           lane 0 (and a constant 0.5 plus the noise for bin 0)
    32 r + 16, r = 0..11      lane 16, its own partner
    32 r + 1, 32 r + 31       lanes 1 and 31 (partners 31 and 1) of rows 0, 3 | 4, 7 | 8, 11: both sides of the two batch
                              boundaries and the ends of the untangled range

Neighbouring buffers -- the two halves of a wave -- carry different tones, one buffer has five frames (chunks of three
and two frames), and eight 3 000-frame buffers that are not compared make the chunks longer than one frame, as in the seams
test.  Every buffer is held to the oracle at the MFCC bars and ceiling of tests/_tol.py.

Premise (CPU, oracle alone): in the filter with the largest weight at bin k, the tone's term w[k] |X[k]| stands at least
20 dB (a factor of ten: the mel sums are sums of magnitudes) above the largest term w[j] |X[j]| of the filter's other bins
outside the window's main lobe (|j - k| > 2) -- its neighbours' noise floor.  The mel filters of the oracle end at bin 358
(filter 13 = bins 225..358): bins 368 = 32 * 11 + 16 and 383 = 32 * 11 + 31 belong to no filter, no MFCC depends on them,
and the premise cannot be stated for them; their buffers are run and compared like the others."""
import numpy as np
import pytest

import afec_amd as afx
from tests import _tol
from tests._oracle import FIELDS, Oracle

BATCH_EDGE_ROWS = (0, 3, 4, 7, 8, 11)
LANE0_BINS = [32 * r for r in range(1, 12)]
LANE16_BINS = [32 * r + 16 for r in range(12)]
EDGE_BINS = [32 * r + d for r in BATCH_EDGE_ROWS for d in (1, 31)]
NO_FILTER_BINS = (368, 383)
FRAMES = 3
ODD_TAIL_FRAMES = 5


def samples(frames):
    return 2048 + 1024 * (frames - 1)


def tone_bins():
    """bin of every tonal buffer, interleaved so that neighbours differ in lane as well as in bin"""
    groups = [list(LANE0_BINS), list(LANE16_BINS), list(EDGE_BINS)]
    order = []
    while any(groups):
        for g in groups:
            if g:
                order.append(g.pop(0))
    return order


@pytest.fixture(scope="module")
def buffers():
    """[(bin or None, signal)]: the constant buffer (bin 0), the tonal buffers, the five-frame buffer; then the ballast"""
    rng = np.random.default_rng(2048)

    def mix(k, frames):
        n = np.arange(samples(frames))
        return (0.5 * np.sin(2 * np.pi * k * n / 2048) + 0.05 * rng.uniform(-1, 1, n.size)).astype(np.float32)

    bufs = [(None, (0.5 + 0.05 * rng.uniform(-1, 1, samples(FRAMES))).astype(np.float32))]
    bufs += [(k, mix(k, FRAMES)) for k in tone_bins()]
    bufs.append((32 * 4 + 1, mix(32 * 4 + 1, ODD_TAIL_FRAMES)))
    block = rng.uniform(-1, 1, samples(3000)).astype(np.float32)
    return bufs, [block] * 8


@pytest.fixture(scope="module")
def oracle_rows(buffers):
    o = Oracle()
    return [o.run(x.astype(np.float64)) for _, x in buffers[0]], o.mel()


def test_neighbouring_buffers_carry_different_tones(buffers):
    bins = [k for k, _ in buffers[0]]
    assert sorted(k for k in bins[1:-1]) == sorted(LANE0_BINS + LANE16_BINS + EDGE_BINS)
    for a, b in zip(bins, bins[1:]):
        assert a != b and (a is None or b is None or (a & 31) != (b & 31)), (a, b)


def test_the_tone_stands_20_db_above_the_noise_floor_of_its_filter(buffers, oracle_rows):
    rows, mel = oracle_rows
    lo, hi = FIELDS["mag"]
    without = []
    for (k, _), ref in zip(buffers[0], rows):
        if k is None:
            continue
        if not mel[:, k].any():
            without.append(k)
            continue
        f = int(np.argmax(mel[:, k]))
        terms = ref[:, lo:hi] * mel[f]                       # [frame][bin]: the filter's terms
        floor = terms.copy()
        floor[:, max(k - 2, 0):k + 3] = 0.0
        with np.errstate(divide="ignore"):                    # bin 1: filter 0 has no bin outside the main lobe
            db = 20.0 * np.log10(terms[:, k] / floor.max(axis=1))
        print(f"bin {k:3d} (row {k >> 5}, lane {k & 31}): filter {f}, tone over the largest noise term {db.min():.1f} dB")
        assert db.min() >= 20.0, (k, f, db)
    assert sorted(set(without)) == list(NO_FILTER_BINS), without


@pytest.fixture(scope="module")
def result(buffers):
    bufs, ballast = buffers
    plan = afx.Plan(max_analysis_ms=0, frame_kernel=afx.FRAME_KERNEL_HALFWAVE)
    try:
        batch = plan.batch([x for _, x in bufs] + ballast, afx.D_MFCC)
        batch.run()
        batch.sync()
        out = (batch.fetch(), batch.info())
        batch.close()
    finally:
        plan.close()
    return out


@pytest.mark.gpu
def test_tonal_buffers_match_the_oracle(result, oracle_rows, buffers):
    got, info = result
    assert info["chunk_frames"] > 1, info     # the frame loop runs more than one trip per chunk
    rows, _ = oracle_rows
    off = got["frame_offset"]
    a, b = FIELDS["mfcc"]
    for i, ((k, _), ref) in enumerate(zip(buffers[0], rows)):
        assert off[i + 1] - off[i] == ref.shape[0] == (ODD_TAIL_FRAMES if i == len(rows) - 1 else FRAMES)
        _tol.check_gpu("mfcc", got["mfcc"][off[i]:off[i + 1]].reshape(ref.shape[0], -1), ref[:, a:b], *_tol.GPU_TOL["mfcc"],
                       what=f"buffer {i} (bin {k}) ")
