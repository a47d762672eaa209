"""Every length regime of afec_amd/csrc/afx_stats.hip on series that are CHOSEN, not whatever the frame kernels produce.

amplitude_peak carries the series (tests/_stats_ref.py: `carrier`): each test first asserts that the GPU's amplitude_peak
series equals the chosen values exactly -- an exact test of the amplitude path of both frame kernels on the side -- and only
then reads the statistics, so what they are held to (`exact_statistics`: TStatistics::Calc in longdouble) owes nothing to the
GPU.  The lengths cross every seam of the dispatch (n <= 1, the small kernel's networks for <= 16 / 32 / 64 frames and its
bisection up to 128, series_stats<4 | 8 | 16> up to 256 / 512 / 1024, the streamed path above), the families steer the
branches (ties at the median rank, constant, all zero, the spread cut, n = 2), and tests/test_stats_ref_cpu.py proves that
the batch orders used here put every median path of stats_small_kernel to work, with waves whose lanes hold several lengths.
The MFCC columns of the same batches (negative values) are checked as tests/test_gpu_statistics.py does, now at every seam.
Sums use that module's tolerances (1e-9 relative, 1e-12 absolute): on these inputs the longdouble reference is within
1.2e-16 of exact arithmetic and the oracle's double restatement within 4e-13 (tests/test_stats_ref_cpu.py), which leaves
three orders for another summation order over at most 2049 terms of one sign.  Measured: profiles/r14/statistics_regimes.txt.
"""
import ctypes

import numpy as np
import pytest

import afec_amd as afx
from tests import _oracle, _stats_ref as sr
from tests.test_gpu_statistics import ATOL, RTOL

pytestmark = pytest.mark.gpu

MASK_PEAK = afx.D_AMPLITUDE_PEAK | afx.D_STATISTICS              # stride 1: 64 files per wave of the small kernel
MASK_MFCC = afx.D_MFCC | afx.D_AMPLITUDE_PEAK | afx.D_STATISTICS  # stride 15: four files and a bit
KERNELS = {"wave64": afx.FRAME_KERNEL_WAVE64, "halfwave": afx.FRAME_KERNEL_HALFWAVE}
STAT = {name: k for k, name in enumerate(afx.STAT_NAMES)}


class Corpus:
    def __init__(self):
        self.cases = sr.cases()
        self.lengths = [n for n, _, _ in self.cases]
        self.bufs = [sr.carrier(v) for _, _, v in self.cases]
        self.want = [sr.exact_statistics(v)[0] for _, _, v in self.cases]


@pytest.fixture(scope="module")
def corpus():
    return Corpus()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(plan, corpus, order, mask):
    """one batch of the corpus' files in this order -> (series, statistics) as fetched"""
    b = plan.batch([corpus.bufs[i] for i in order], mask)
    stride = ctypes.c_int32()
    b.L.afx_batch_record_layout.argtypes = [ctypes.c_void_p] * 4
    assert b.L.afx_batch_record_layout(b.h, ctypes.byref(stride), None, None) == 0
    assert stride.value == sr.record_stride(mask)      # what the reach test of tests/test_stats_ref_cpu.py computed with
    b.run()
    series, stats = b.fetch(), b.fetch_statistics()
    b.close()
    off = series["frame_offset"]
    assert np.diff(off).tolist() == [corpus.lengths[i] for i in order]
    assert stats["stats_status"].tolist() == [0] * len(order)
    return series, stats


def regime(n):
    return "n<=1" if n < 2 else "small" if n <= 128 else "wave" if n <= 1024 else "streamed"


def check_chosen(corpus, order, series, stats, worst):
    off = series["frame_offset"]
    for p, i in enumerate(order):
        n, family, v = corpus.cases[i]
        tag = (n, family, "file %d of the batch" % p)
        # the precondition: the kernels reduced the chosen values
        assert np.array_equal(bits(series["amplitude_peak"][off[p]:off[p + 1]]), bits(v)), tag
        got, want = stats["amplitude_peak"][p], corpus.want[i]
        assert np.array_equal(bits(got[:3]), bits(want[:3])), (tag, "min / max / median", got[:3], want[:3])
        err = np.abs(got - want)
        for k in np.nonzero(want)[0]:
            key = (regime(n), afx.STAT_NAMES[k])
            worst[key] = max(worst.get(key, 0.0), err[k] / abs(want[k]))
        assert np.all(err <= RTOL * np.abs(want) + ATOL), (tag, got, want)
        # what is known exactly
        if n == 0:
            assert not got.any(), tag
        elif n == 1:
            assert np.array_equal(bits(got), bits([v[0], v[0], 0, v[0]] + [0] * 9)), (tag, got)
        else:
            named = {name: got[k] for name, k in STAT.items()}
            if family == "zeros":
                assert [named[s] for s in ("centroid", "spread", "skewness", "kurtosis", "flatness")] == [0] * 5, (tag, got)
            if family in ("first_only", "last_only"):
                assert named["centroid"] == (0 if family == "first_only" else n - 1), (tag, got)
                assert [named[s] for s in ("spread", "skewness", "kurtosis")] == [0] * 3, (tag, got)
            if n == 2:
                assert named["dmean"] == 0 and named["dvariance"] == 0, (tag, got)


def check_mfcc(order, series, stats):
    """the MFCC columns: all 13 against Calc of the GPU's own series, the median an element of it"""
    off = series["frame_offset"]
    for p in range(len(order)):
        for w in range(14):
            want = _oracle.calc_statistics(series["mfcc"][off[p]:off[p + 1], w], np.zeros(13))
            got = stats["mfcc"][p, w]
            assert got[2] == want[2], ("mfcc", p, w, "median", got[2], want[2])
            assert np.all(np.abs(got - want) <= RTOL * np.abs(want) + ATOL), ("mfcc", p, w, got, want)


@pytest.mark.parametrize("order_name", ["shuffled", "reaching"])
@pytest.mark.parametrize("mask_name,kernel", [("peak", "wave64"), ("mfcc", "wave64"), ("mfcc", "halfwave")])
def test_chosen_series_in_every_regime(corpus, mask_name, kernel, order_name):
    mask = MASK_PEAK if mask_name == "peak" else MASK_MFCC
    order = (sr.shuffled_order if order_name == "shuffled" else sr.reach_order)(corpus.lengths)
    plan = afx.Plan(max_analysis_ms=0, frame_kernel=KERNELS[kernel])
    series, stats = run(plan, corpus, order, mask)
    plan.close()
    worst = {}
    try:
        check_chosen(corpus, order, series, stats, worst)
    finally:
        for reg in ("small", "wave", "streamed"):
            print("worst relative error, %s, %s, %s, %-8s:" % (mask_name, kernel, order_name, reg),
                  " ".join("%s %.1e" % (s, worst[(reg, s)]) for s in afx.STAT_NAMES if (reg, s) in worst))
    if mask_name == "mfcc":
        check_mfcc(order, series, stats)


@pytest.mark.parametrize("mask_name", ["peak", "mfcc"])
def test_a_files_statistics_do_not_depend_on_its_neighbours(corpus, mask_name):
    """Bit for bit: a file of 42 frames beside one of 128 (stats_small_kernel<true>, its wave on the bisection path) and
    beside short ones (<false>, network_median<64>), alone, in a batch of everything, and among files of its own length
    only (16, 17, 32, 33, 64, 65: the wave's largest n sits on the threshold between two median paths) -- and three files
    of the wave-per-series kernel alone against the batch of everything.  The plan pins the frame kernel, as the
    crawler's does."""
    mask = MASK_PEAK if mask_name == "peak" else MASK_MFCC
    fields = ["amplitude_peak"] + (["mfcc"] if mask_name == "mfcc" else [])
    batches = sr.neighbour_batches(corpus.lengths)
    plan = afx.Plan(max_analysis_ms=0, frame_kernel=afx.FRAME_KERNEL_WAVE64)
    home = {}          # file -> {field: (series bytes, statistics bytes)} in the mixed batch
    compared = 0
    for name in ["mixed"] + sorted(k for k in batches if k != "mixed"):
        order = batches[name]
        series, stats = run(plan, corpus, order, mask)
        check_chosen(corpus, order, series, stats, {})     # every batch on its own against the reference, then each other
        off = series["frame_offset"]
        for p, i in enumerate(order):
            for f in fields:
                mine = (series[f][off[p]:off[p + 1]].tobytes(), stats[f][p].tobytes())
                if name == "mixed":
                    home.setdefault(i, {})[f] = mine
                    continue
                tag = (f, "file of %d frames (%s)" % corpus.cases[i][:2], "batch " + name)
                assert mine[0] == home[i][f][0], ("the SERIES differ between batches", tag)
                assert mine[1] == home[i][f][1], (tag, np.frombuffer(mine[1]).reshape(-1, 13), np.frombuffer(home[i][f][1]).reshape(-1, 13))
                compared += 1
    plan.close()
    small = sum(1 for n in corpus.lengths if 2 <= n <= 128)
    assert compared >= len(fields) * (small + len(sr.SINGLE_FILE_LENGTHS) + len(sr.ALONE_LONG_LENGTHS))


def test_running_a_batch_again_leaves_the_same_bytes(corpus):
    """the radix select's LDS histograms and the small kernel's tile are rebuilt by every run"""
    order = sr.shuffled_order(corpus.lengths)
    plan = afx.Plan(max_analysis_ms=0, frame_kernel=afx.FRAME_KERNEL_WAVE64)
    b = plan.batch([corpus.bufs[i] for i in order], MASK_MFCC)
    b.run()
    first = b.fetch_statistics()
    for _ in range(3):
        b.run()
    again = b.fetch_statistics()
    b.close()
    plan.close()
    assert sorted(first) == sorted(again)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k
