"""The inputs of tests/test_gpu_band_selection.py do what they are for, checked on the CPU oracle's magnitudes: the
tie design (tests/_bands_ref.py) puts classes of equal sort keys with distinguishable members on both cuts of every band,
with and without bins strictly beyond them, on either side of and across the sort-block boundaries of bands 11 and 13;
a selection by key alone is told apart from the right one; and the numpy reference the GPU test compares with is the
oracle's own arithmetic."""
import numpy as np
import pytest

from tests import _bands_ref as ref
from tests._oracle import FIELDS, Oracle

RTOL = 1e-11          # of the GPU comparison the inputs are for (tests/test_gpu_band_selection.py)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module", params=["f64", "f32"])
def records(request, oracle):
    """(dtype name, calibration misses, the oracle's records of TIE_BUFFERS, of the complexity edge buffers)"""
    dtype = np.float64 if request.param == "f64" else np.float32
    frame0 = lambda period: oracle.run(period)[0, :1024]
    ties, misses = [], []
    for design, frames in ref.TIE_BUFFERS:
        x, miss = ref.tie_design(design, frames, dtype, frame0)
        assert x.dtype == dtype and np.abs(x).max() < 1.0
        ties.append(oracle.run(x.astype(np.float64)))
        misses.append(miss)
    edges = [(name, oracle.run(x.astype(np.float64))) for name, x in ref.complexity_edge_buffers(dtype, frame0)]
    return request.param, misses, ties, edges


def test_calibration_reaches_the_targets(records):
    name, misses, _, _ = records
    # float64: the iteration's fixed point; float32: the input's rounding noise, under the 3e-7 to a bucket's edge
    assert max(misses) <= (1e-11 if name == "f64" else 2.5e-7), misses


def test_tie_design_meets_its_conditions(records):
    _, _, ties, _ = records
    seen, sides = ref.check_design_conditions([r[:, :1024] for r in ties], RTOL)
    assert len(sides) == 12


def test_tiled_frames_are_the_same_spectrum(records):
    _, _, ties, _ = records
    for r in ties:
        for f in range(2, r.shape[0], 2):
            assert np.array_equal(r[f, :1024].view(np.uint64), r[0, :1024].view(np.uint64))


def test_reference_is_the_oracles_arithmetic(records):
    _, _, ties, edges = records
    for what, r in [("tie buffer %d" % i, r) for i, r in enumerate(ties)] + edges:
        mag = r[:, :1024]
        a, b = FIELDS["sub_contrast"]
        want, got = r[:, a:b], ref.contrast(mag)
        ok = np.isfinite(want)
        assert np.array_equal(ok, np.isfinite(got)), what
        assert np.all(np.abs(got[ok] - want[ok]) <= 1e-13 * np.abs(want[ok])), (what, np.max(np.abs(got[ok] / want[ok] - 1)))
        sc, want_sc = ref.spectral_contrast(mag), r[:, FIELDS["spectral_contrast"][0]]
        ok = np.isfinite(want_sc)
        assert np.all(np.abs(sc[ok] - want_sc[ok]) <= 1e-13 * np.abs(want_sc[ok])), what
        a, b = FIELDS["sub_complexity"]
        assert np.array_equal(ref.complexity(mag), r[:, a:b]), what


def test_complexity_edges_are_edges(records):
    """the edge inputs put a counted maximum where they say: on the first / last bin of every band, on the seams"""
    _, _, _, edges = records
    by_name = dict(edges)
    for name in ("first bins", "last bins"):
        assert np.all(ref.complexity(by_name[name][:, :1024]) >= 1), name
    for name in ("seams 63 256 511", "seams 64 255 512", "seam pairs"):
        c = ref.complexity(by_name[name][:, :1024])
        assert np.all(c[:, [6, 11, 13]] >= 1), name
    quarter = by_name["quarter of the maximum"][0, :1024]
    for hi, lo in ((14, 20), (52, 62), (125, 150), (230, 300), (350, 420), (600, 640)):
        assert abs(quarter[lo] / quarter[hi] - 0.25) < 1e-8, (hi, lo)
    assert not np.any(ref.complexity(by_name["silence"][:, :1024]))


def test_census_and_key_only_selection_on_a_hand_made_band():
    """band 3 (bins 13..22, three bins per mean): 0.5 x 4 around the valley's cut with one bin below"""
    mag = np.zeros((1, 1024))
    mag[0, 1:752] = 1.0 + np.arange(751) * 1e-3                       # distinct keys everywhere else
    tie = 0.5 * (1.0 + np.array([2, 1, -1, -2]) * 2.0 ** -22)
    mag[0, 13:23] = [0.25, tie[0], tie[1], tie[2], tie[3], 0.7, 0.8, 0.9, 1.0, 1.1]
    assert len(set(ref.sort_key(tie).tolist())) == 1
    valley, peak = ref.tie_census(mag)[0][3]
    assert peak is None
    assert valley[:2] == (1, 4) and valley[3] == (14, 15, 16, 17) and abs(valley[2] - 4 * 2.0 ** -22) < 1e-9
    right = (0.25 + tie[2] + tie[3]) / 3
    wrong = (0.25 + tie[0] + tie[1]) / 3
    mean = mag[0, 13:23].sum() / 10
    assert ref.contrast(mag)[0, 3] == pytest.approx(-np.power(1.0 / right, 1.0 / np.log(mean)), rel=1e-14)
    assert ref.key_only_contrast(mag)[0, 3] == pytest.approx(-np.power(1.0 / wrong, 1.0 / np.log(mean)), rel=1e-14)
    assert abs(ref.key_only_contrast(mag)[0, 3] / ref.contrast(mag)[0, 3] - 1.0) > 1e-8
    assert ref.side_of_edge(11, (250, 255)) == "A" and ref.side_of_edge(11, (256,)) == "B" and ref.side_of_edge(13, (511, 512)) == "both"
