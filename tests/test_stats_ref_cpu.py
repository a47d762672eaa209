"""tests/_stats_ref.py without a GPU: the longdouble reference against the same formulas at 50 digits and against the
oracle's double restatement, the carrier buffers, and that the batch orders of tests/test_gpu_statistics_regimes.py
put every median path of stats_small_kernel to work under each mask they run with."""
import numpy as np
import pytest

import afec_amd as afx
from tests import _oracle, _stats_ref as sr

MASKS = {"amplitude_peak": afx.D_AMPLITUDE_PEAK | afx.D_STATISTICS,
         "mfcc + amplitude_peak": afx.D_MFCC | afx.D_AMPLITUDE_PEAK | afx.D_STATISTICS}


@pytest.fixture(scope="module")
def cases():
    return sr.cases()


def test_every_length_has_its_families(cases):
    got = {}
    for n, family, v in cases:
        assert v.dtype == np.float32 and v.shape == (n,) and np.all(v >= 0) and np.all(np.isfinite(v))
        got.setdefault(n, set()).add(family)
    assert sorted(got) == sorted(sr.LENGTHS + sr.EXTRA_LENGTHS)
    for n in sr.LENGTHS:
        assert got[n] == set(sr.FAMILIES if n <= 130 else sr.LONG_FAMILIES), n
        assert {"uniform", "ties", "constant", "with_zeros"} <= got[n]
    # the families are what they say
    by = {(n, f): v for n, f, v in cases}
    assert np.all(by[(33, "constant")] == np.float32(0.3)) and not by[(2049, "zeros")].any()
    assert set(np.unique(by[(130, "ties")])) == {0.25, 0.5, 0.75}
    assert by[(17, "first_only")].tolist() == [0.5] + [0.0] * 16 and by[(17, "last_only")].tolist() == [0.0] * 16 + [0.5]
    assert np.all(np.diff(by[(65, "ascending")]) >= 0) and np.all(np.diff(by[(65, "descending")]) <= 0)
    assert np.count_nonzero(by[(96, "with_zeros")] == 0) == 32 and np.count_nonzero(by[(2, "with_zeros")] == 0) == 1


def test_known_answers():
    got, how = sr.exact_statistics([1.0, 3.0])
    assert how == ("longdouble" if np.finfo(np.longdouble).nmant >= 63 else "oracle")
    want = [1, 3, 1, 2, np.sqrt(3.0), 1, 0.75, 0.1875]
    assert np.allclose(got[:8], want, rtol=1e-15, atol=0) and got[11] == 0 and got[12] == 0
    t = (np.array([1.0, 3.0]) - 0.75) / 0.1875
    assert np.allclose(got[8:11], [np.mean(t ** 3), np.mean(t ** 4) - 3, np.sqrt(3.0) / 2], rtol=1e-14, atol=0)
    assert sr.exact_statistics([])[0].tolist() == [0.0] * 13
    assert sr.exact_statistics([0.25])[0].tolist() == [0.25, 0.25, 0, 0.25] + [0.0] * 9
    # x = 0, 1, 2, 1: the two difference statistics start at n = 3; the lower median
    got = sr.exact_statistics([0.0, 1.0, 2.0, 1.0])[0]
    assert got[2] == 1.0 and got[11] == 1.0 and got[12] == 0.0 and got[6] == 2.0      # (1 + 4 + 3) / 4


def _calc_mp(v, mp):
    """TStatistics::Calc (oracle/afx_oracle.c:184-323) at mp's working precision"""
    x = [mp.mpf(float(t)) for t in v]
    n = len(x)
    o = [mp.mpf(0)] * 13
    if n == 0:
        return o
    if n == 1:
        o[0] = o[1] = o[3] = x[0]
        return o
    s = mp.fsum(x)
    mean = s / n
    gmean = mp.exp(mp.fsum(mp.log(abs(t) + mp.mpf(1e-20)) for t in x) / n)
    cen = mp.mpf(0) if s == 0 else mp.fsum(j * t for j, t in enumerate(x)) / s
    spr = mp.mpf(0) if s == 0 else mp.fsum((j - cen) ** 2 * t for j, t in enumerate(x)) / s
    o[0], o[1], o[2], o[3], o[4] = min(x), max(x), sorted(x)[(n - 1) // 2], mean, gmean
    o[5] = mp.fsum((t - mean) ** 2 for t in x) / n
    o[6], o[7] = cen, spr
    if abs(spr) > mp.mpf(float(np.float32(1e-12))):
        u = [(t - cen) / spr for t in x]
        o[8] = mp.fsum(t ** 3 for t in u) / n
        o[9] = mp.fsum(t ** 4 for t in u) / n - 3
    o[10] = mp.mpf(0) if mean == 0 else gmean / mean
    if n > 2:
        d = [abs(b - a) for a, b in zip(x, x[1:])]
        dmean = mp.fsum(d) / (n - 1)
        o[11] = dmean
        o[12] = mp.fsum((t - dmean) ** 2 for t in d) / (n - 1)
    return o


def test_reference_agrees_with_exact_arithmetic_and_with_the_oracle(cases):
    """longdouble within 1e-15 of the 50-digit value, the oracle (double, the reference's summation order) within 1e-12,
    1e-30 absolute for both; min, max and the median are elements of the series: equal."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp.clone()
    mp.dps = 50
    worst = {"longdouble": 0.0, "oracle": 0.0}
    for n, family, v in cases:
        exact = _calc_mp(v, mp)
        got, how = sr.exact_statistics(v)
        oracle = _oracle.calc_statistics(v.astype(np.float64), np.zeros(13))
        for name, values, rtol in ((how, got, 1e-15 if how == "longdouble" else 1e-12), ("oracle", oracle, 1e-12)):
            for k, stat in enumerate(afx.STAT_NAMES):
                if k < 3:
                    assert mp.mpf(float(values[k])) == exact[k], (name, n, family, stat, values[k], exact[k])
                    continue
                err = abs(mp.mpf(float(values[k])) - exact[k])
                assert err <= rtol * abs(exact[k]) + mp.mpf(1e-30), (name, n, family, stat, values[k], float(exact[k]), float(err))
                if exact[k] != 0:
                    worst[name] = max(worst[name], float(err / abs(exact[k])))
    print("worst relative error against 50 digits:", worst)


def test_carrier_holds_the_series_in_its_hops(cases):
    for n, family, v in cases:
        x = sr.carrier(v)
        assert x.dtype == np.float32
        if n == 0:
            assert x.size == 100 and not x.any()
            continue
        assert x.size == 2048 + 1024 * (n - 1)
        hops = x.reshape(-1, 1024)
        assert np.array_equal(hops[:n].__abs__().max(axis=1), v), (n, family)
        assert not hops[n:].any()                           # the tail beyond the last hop
        assert np.count_nonzero(x) == np.count_nonzero(v)


def test_reach_restates_the_dispatch_on_small_examples():
    r = sr.small_kernel_reach([16] * 64 + [17] + [0, 1, 129, 4000], 1)
    assert [r[b]["waves"] for b in sr.BRANCHES] == [1, 1, 0, 0]
    assert r["<=32"] == {"waves": 1, "distinct": 1, "distinct_with_idle": 1}
    assert r["<=16"] == {"waves": 1, "distinct": 1, "distinct_with_idle": 0}
    # stride 15: 64 lanes are four files and a bit; the longest of them decides for all
    r = sr.small_kernel_reach([2, 3, 4, 5, 128, 64, 64, 64, 64, 64, 64, 64, 64], 15)
    assert r[">64"] == {"waves": 2, "distinct": 5, "distinct_with_idle": 0}      # lanes 0..63 and 64..127 both hold file 4
    assert r["<=64"]["waves"] == 2 and r["<=64"]["distinct_with_idle"] == 1      # the last wave is partly behind the batch
    assert all(v["waves"] == 0 for v in sr.small_kernel_reach([0, 1, 129], 3).values())


@pytest.mark.parametrize("mask_name", sorted(MASKS))
def test_the_batches_reach_every_branch(cases, mask_name):
    stride = sr.record_stride(MASKS[mask_name])
    assert stride >= 1
    lengths = [n for n, _, _ in cases]
    order = sr.reach_order(lengths)
    assert sorted(order) == list(range(len(lengths))) and sorted(sr.shuffled_order(lengths)) == list(range(len(lengths)))
    reach = sr.small_kernel_reach([lengths[i] for i in order], stride)
    for branch in sr.BRANCHES:
        assert reach[branch]["waves"] >= 1, "at stride %d (%s) no wave of the branch-reaching order takes %s: %r" % (
            stride, mask_name, branch, reach)
    # the case the kernel's header describes: lanes of one wave with their own n each, and lanes with nothing to do
    assert max(r["distinct_with_idle"] for r in reach.values()) >= 3, (stride, reach)
    batches = sr.neighbour_batches(lengths)
    assert set(sr.NEIGHBOUR_REACH) | {"mixed"} | {"alone%d" % n for n in sr.ALONE_LONG_LENGTHS} == set(batches)
    for name, top in sr.NEIGHBOUR_REACH.items():
        got = sr.small_kernel_reach([lengths[i] for i in batches[name]], stride)
        assert got[top]["waves"] >= 1, "stride %d (%s): no wave of batch %s takes %s: %r" % (stride, mask_name, name, top, got)
        for branch in sr.BRANCHES[sr.BRANCHES.index(top) + 1:]:
            assert got[branch]["waves"] == 0, "stride %d (%s): batch %s reaches %s: %r" % (stride, mask_name, name, branch, got)
    for n in sr.SINGLE_FILE_LENGTHS + sr.ALONE_LONG_LENGTHS:
        assert [lengths[i] for i in batches["alone%d" % n]] == [n]
    for n in sr.SEAM_LENGTHS:      # the thresholds on a wave's largest n meet their own value, with every family
        assert [lengths[i] for i in batches["only%d" % n]] == [n] * len(sr.FAMILIES)
    # upto64 must not need the wave-per-series kernel at all (stats_small_kernel<false> alone)
    assert all(2 <= lengths[i] <= 64 for i in batches["upto64"]) and max(lengths[i] for i in batches["upto64"]) == 64
    assert max(lengths[i] for i in batches["upto128"]) == 128
