"""Chosen records for the two kernels above a run that read nothing but what the run left in device memory:
high_level_kernel (afec_amd/csrc/highlevel/afx_highlevel.hip) and classification_features_kernel
(afec_amd/csrc/classify/afx_classify.hip).  Every case is one file: the columns of its per-frame records, the 13
statistics of every column, the rhythm tracker's 14 scalars and a peak / rms pair -- what Batch.store_records writes over
a run's own results (tests/test_gpu_records_store.py), and what the restatements tests/_highlevel_ref.py and
tests/_classification_ref.py compute the expected answers from.

Exactness premise: unless a case says otherwise (`dyadic=False`, or a note in its builder), every value that enters one of
the kernel's sums is a multiple of 2^-10 with magnitude below 4 (integers up to 2^17 for the few cases that need a
frequency in Hz), so the sum over at most 4 200 frames is exact in any order of addition and the audible means are one
division of the same two numbers on the device and in the restatement.  A threshold value that is no such multiple
(0.8, 0.2 and their neighbours) stands alone among the audible frames: a sum of one term.

`reaches` names the conditions a case is built to reach (TARGETS lists them all); tests/test_records_cases_cpu.py reads
from the restatements' own intermediate values that it does.

Test helper only -- the product never imports it."""
import functools
import math

import numpy as np

from afec_amd import capi
from tests import _classification_ref as cf
from tests import _highlevel_ref as hl

WIDTHS = {name: width for name, width in capi.OUT_FIELDS if name != "magnitude"}
SERIES = list(capi.RECORD_SERIES)
NAN, INF = math.nan, math.inf
QUARTER = 11025.0
SUMMED = ["f0_confidence", "spectral_rolloff", "spectral_flatness", "auto_correlation", "spectral_flux", "spectral_contrast",
          "spectral_complexity", "spectral_inharmonicity"]          # what high_level_kernel adds up over the audible frames
TRACK_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 64, 65, 256, 257)
SIGNATURE_LENGTHS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 860, 4200)
CF_LENGTHS = (1, 44, 45, 64, 65, 128, 129, 256, 257, 512, 513)
MULTISET_LENGTHS = (1024, 1025, 1100, 4200)
TEMPI = (0.0, 0.24, 0.25, 119.75, 120.2499999, 89.9999, -0.3)
EPS32 = np.float32(1e-12)
LEVELS = {"1.0": np.float32(1.0), "eps": EPS32, "eps_up": np.nextafter(EPS32, np.float32(1.0)), "0": np.float32(0.0)}
USED_STAT_SLOTS = [slot for _, slot in cf.STATISTICS]
UNUSED_STAT_SLOTS = [s for s in range(13) if s not in USED_STAT_SLOTS]
USED_RHYTHM = [slot for _, slot in cf.RHYTHM_SCALARS]
UNUSED_RHYTHM = [0, 1, 3, 6, 7, 9]      # 12 and 13 are the high-level kernel's tempo and its confidence


def up(x):
    return float(np.nextafter(x, math.inf))


def down(x):
    return float(np.nextafter(x, -math.inf))


class Case:
    """one file.  columns: {series: [n] or [n][W]}, statistics: {series: [13] or [W][13]}, rhythm [14], levels (peak, rms)
    float32; non_finite: how many of the 1 680 classification features are not finite"""

    def __init__(self, name, n, seed):
        rng = np.random.default_rng(seed)
        self.name, self.n, self.reaches, self.dyadic, self.non_finite = name, n, [], True, 0
        self.columns, self.statistics = {}, {}
        for s in SERIES:
            w = WIDTHS[s]
            self.columns[s] = rng.integers(-4095, 4096, (n, w) if w > 1 else (n,)) / 1024.0
            self.statistics[s] = rng.integers(-4095, 4096, (w, 13) if w > 1 else (13,)) / 1024.0
        c = self.columns
        c["spectrum_bands"] = rng.integers(1, 17, (n, 28)) / 4.0          # 0.25 .. 4: the cubic stays well conditioned
        for s in ("spectral_flatness", "f0_confidence", "auto_correlation"):
            c[s] = rng.integers(0, 1025, n) / 1024.0
        c["spectral_rolloff"] = rng.integers(1, 4096, n) / 1024.0
        c["spectral_centroid"] = rng.integers(1, 4096, n) / 1024.0
        c["f0"] = np.zeros(n)                                             # no pitch anywhere until a builder says so
        c["amplitude_silence"] = np.zeros(n)                              # audible
        self.rhythm = rng.integers(0, 4096, 14) / 1024.0
        self.rhythm[12], self.rhythm[13] = 120.0, 0.5
        self.levels = (np.float32(0.5), np.float32(0.25))

    def reach(self, *targets):
        self.reaches += list(targets)
        return self

    def pitched(self, frames, confidence=0.875, others=0.0):
        """f0 / f0_confidence: {frame: Hz} confident with `confidence`, every other frame `others` and no pitch"""
        self.columns["f0_confidence"] = np.full(self.n, float(others))
        self.columns["f0"] = np.zeros(self.n)
        for p, hz in frames.items():
            self.columns["f0"][p], self.columns["f0_confidence"][p] = hz, confidence
        return self

    def silent(self, frames):
        self.columns["amplitude_silence"][list(frames)] = 1.0
        return self

    def series(self):
        return {k: self.columns[k] for k in hl.SERIES}


def _class_cases():
    out = []
    # one audible frame whose confidence IS the class threshold (a mean of one term), silent frames at the threshold and
    # one ulp above it with pitches that would move the median if the comparison were >=
    for tag, audible_conf, threshold, target in (("class_eq_0.8", 0.8, 0.8, "class:mean_eq_0.8"), ("class_below_0.8", down(0.8), 0.5, "class:mean_below_0.8"),
                                                 ("class_below_0.5", down(0.5), 0.2, "class:mean_below_0.5")):
        c = Case(tag, 3, len(out) + 100).silent([1, 2])
        c.columns["f0"] = np.array([440.0, 300.0, 200.0])
        c.columns["f0_confidence"] = np.array([audible_conf, threshold, up(threshold)])
        out.append(c.reach(target, f"confident:conf_eq_{threshold}", f"confident:conf_above_{threshold}"))
    out[0].reach("median:n_pitch_1")
    c = Case("class_half_from_quarters", 4, 104)
    c.columns["f0"] = np.array([100.0, 110.0, 120.0, 130.0])
    c.columns["f0_confidence"] = np.array([0.25, 0.75, 0.25, 0.75])
    out.append(c.reach("class:mean_eq_0.5"))
    c = Case("class_no_audible_frame", 6, 105).silent(range(6)).pitched({p: 220.0 + 13.0 * p for p in range(6)})
    out.append(c.reach("class:no_audible"))
    return out


def _confident_cases():
    c = Case("f0_edges", 5, 110).pitched({0: 20.0, 1: up(20.0), 2: QUARTER, 3: down(QUARTER), 4: NAN})
    out = [c.reach("confident:f0_nan", "median:n_pitch_2", "median:deviation_ge_6")]
    # each bound of f0 alone in its file, behind the look-ahead (frame 2 of 5), and one ulp inside it: on the bound the
    # file has no pitch at all -- base note -1, a track of zeros --, inside it one, so either comparison shows on the device
    for k, (tag, hz) in enumerate((("f0_eq_20", 20.0), ("f0_above_20", up(20.0)), ("f0_eq_quarter", QUARTER), ("f0_below_quarter", down(QUARTER)))):
        out.append(Case(tag + "_alone", 5, 111 + k).pitched({2: hz}).reach("confident:" + tag))
    return out


def _median_cases():
    out = []
    c = Case("median_no_pitch", 7, 120)
    c.columns["spectrum_bands"][:] = 0.0
    out.append(c.reach("median:n_pitch_0", "signature:zero_bands"))
    out.append(Case("median_three", 9, 121).pitched({2: 220.0, 5: 246.9375, 7: 233.125}, others=0.5).reach("median:n_pitch_3"))
    for tag, count, target in (("median_even_100", 100, "median:even_above_64"), ("median_odd_101", 101, "median:odd_above_64")):
        rng = np.random.default_rng(count)
        frames = rng.permutation(130)[:count]
        out.append(Case(tag, 130, 122 + count).pitched({int(p): 200.0 + 3.0 * k for k, p in enumerate(frames)}, others=0.5).reach(target))
    out.append(Case("median_all_equal", 70, 124).pitched({p: 330.0 for p in range(2, 68)}, others=0.75).reach("median:all_equal"))
    hz = [24.0 * 2 ** k for k in range(9)] + [10000.0]
    out.append(Case("median_every_exponent", 12, 125).pitched({p + 1: hz[(7 * p) % 10] for p in range(10)}).reach("median:every_exponent"))
    hz = [300.0, 200.0, 300.0, 400.0, 300.0, 250.0, 300.0, 350.0, 300.0]
    out.append(Case("median_duplicates", 20, 126).pitched({2 * p: v for p, v in enumerate(hz)}).reach("median:duplicates_both_sides"))
    c = Case("median_silent_frames_count", 5, 127).pitched({0: 100.0, 1: 110.0, 2: 400.0, 3: 410.0, 4: 420.0}).silent([2, 3, 4])
    out.append(c.reach("median:silent_confident_frames"))
    # the same 1 000 pitches, 0.5 Hz apart, in files on either side of the 1 024 keys the kernel keeps in LDS
    for n in MULTISET_LENGTHS:
        rng = np.random.default_rng(n)
        frames = rng.permutation(n)[:1000]
        values = rng.permutation(1000)
        c = Case(f"median_multiset_{n}", n, 128 + n).pitched({int(p): 100.0 + 0.5 * int(v) for p, v in zip(frames, values)})
        out.append(c.reach(f"median:multiset_{n}", *([f"signature:n{n}"] if n in SIGNATURE_LENGTHS else [])))
    return out


def _track_cases():
    out = []
    out.append(Case("track_n1", 1, 140).pitched({0: 440.0}).reach("track:n1"))
    for n in TRACK_LENGTHS[1:]:
        last = max(1, n // 4)
        for first, tag in ((last, "on_bound"), (last + 1, "behind_bound")):
            if first >= n:
                continue      # two frames: the bound is the last frame
            frames = {first: 440.0}
            if n - 1 > first:
                frames[n - 1] = 550.0
            out.append(Case(f"track_n{n}_{tag}", n, 141 + 2 * n + (first - last)).pitched(frames).reach(f"track:n{n}_{tag}"))
    out.append(Case("track_silent_in_look_ahead", 8, 150).pitched({1: 300.0, 2: 500.0}).silent([1]).reach("track:silent_in_look_ahead"))
    out.append(Case("track_0_and_200", 260, 151).pitched({0: 300.0, 200: 500.0}).reach("track:0_and_200"))
    out.append(Case("track_tile_edges", 130, 152).pitched({63: 300.0, 64: 400.0, 127: 500.0, 128: 600.0}).reach("track:63_64_127_128"))
    out.append(Case("track_last_frame_only", 100, 153).pitched({99: 440.0}).reach("track:last_frame_only"))
    return out


def _scalar_cases():
    out = []
    # (frequencies in Hz: integers, sums still exact)
    c = Case("clamps_high", 5, 160)
    c.columns.update(spectral_rolloff=np.full(5, 65536.0), spectral_centroid=np.full(5, 65536.0), spectral_flatness=np.full(5, 2.0),
                     auto_correlation=np.full(5, 0.75), f0_confidence=np.full(5, 0.75))
    c.levels = (LEVELS["1.0"], LEVELS["eps"])
    out.append(c.reach("clamp:brightness_above_1", "clamp:flatness_above_1", "clamp:noisiness_below_0", "clamp:harmonicity_above_1",
                       "clamp:auto_correlation_above_two_thirds", "level:1.0", "level:eps"))
    c = Case("clamps_low", 5, 161)
    c.columns.update(spectral_rolloff=np.full(5, 4.0), spectral_centroid=np.full(5, 131072.0), spectral_flatness=np.full(5, -1.0),
                     auto_correlation=np.full(5, -1.0), f0_confidence=np.full(5, 0.25))
    c.levels = (LEVELS["eps_up"], LEVELS["0"])
    out.append(c.reach("clamp:brightness_below_0", "clamp:centroid_above_100k", "clamp:rolloff_2_to_8", "clamp:flatness_below_0",
                       "clamp:noisiness_above_1", "clamp:harmonicity_below_0", "level:eps_up", "level:0"))
    c = Case("characteristics_inside", 6, 162)
    c.columns.update(spectral_rolloff=np.full(6, 3000.0), spectral_centroid=np.arange(6) * 500.0 + 2000.0, auto_correlation=np.full(6, 0.75),
                     f0_confidence=np.full(6, 0.25))
    out.append(c.reach("clamp:none"))
    for k, tempo in enumerate(TEMPI):
        c = Case(f"tempo_{tempo}", 2 + k, 170 + k)
        c.rhythm[12] = tempo
        c.rhythm[13] = [0.5, -0.0, 5e-324, 1.0 / 3.0, 1e300, -1.0 / 7.0, 2.0 ** -1022][k]
        out.append(c.reach(f"tempo:{tempo}"))
    return out


def _signature_cases():
    have = set(MULTISET_LENGTHS)
    return [Case(f"signature_n{n}", n, 180 + n).reach(f"signature:n{n}") for n in SIGNATURE_LENGTHS if n not in have]


def _classification_cases():
    """files on every seam of the time frames 0..43, 64, 128, 256, 512, with values that are no numbers where the kernel
    reads and where it does not; non_finite is counted by hand from SampleClassificationDescriptors' layout"""
    out = {n: Case(f"cf_n{n}", n, 200 + n).reach(f"cf:n{n}") for n in CF_LENGTHS}
    for c in out.values():
        c.dyadic = False
    # the seven used statistics of one series: one feature each
    c = out[1]
    c.statistics["spectral_flatness"][USED_STAT_SLOTS] = [NAN, INF, -INF, NAN, INF, -INF, NAN]
    c.non_finite = 7
    c.reach("cf:used_statistic_slots")
    # the six unused statistics of every series, and all 13 of the series the features do not name: none
    c = out[44]
    named = set(cf.SERIES) - {"spectrum_bands"}
    for s in SERIES:
        c.statistics[s][..., UNUSED_STAT_SLOTS if s in named else slice(None)] = NAN
    c.reach("cf:unused_statistic_slots")
    # row 44 of a file of 45 frames: time frame 44 is frame 64
    c = out[45]
    for s in SERIES:
        c.columns[s][44] = NAN
    c.reach("cf:unread_row_44")
    # rows the kernel reads
    c = out[64]
    c.columns["spectrum_bands"][0, 3] = NAN            # the merged band 2 of frame 0
    c.columns["spectral_flux"][43] = INF
    c.columns["amplitude_rms"][10] = -INF
    c.non_finite = 3
    c.reach("cf:nan_in_read_row", "cf:inf_in_read_row", "cf:neginf_in_read_row")
    c = out[65]
    c.columns["spectral_rms"][64] = NAN
    c.non_finite = 1
    c.reach("cf:nan_in_read_row")
    c = out[128]
    c.rhythm[USED_RHYTHM] = [NAN, INF, -INF, NAN, INF, -INF]
    c.non_finite = 6
    c.reach("cf:used_rhythm_scalars")
    c = out[129]
    for s in SERIES:
        c.columns[s][[44, 65]] = NAN
    c.rhythm[UNUSED_RHYTHM] = [NAN, INF, -INF, NAN, INF, -INF]
    c.reach("cf:unread_rows_44_65", "cf:unused_rhythm_scalars")
    # the mean of spectral_rms: its own feature and the 21 that pad the vector to a multiple of 48
    c = out[256]
    c.statistics["spectral_rms"][3] = NAN
    c.non_finite = 22
    c.reach("cf:padding")
    c = out[257]
    c.columns["spectral_contrast"][256] = INF
    c.non_finite = 1
    c.reach("cf:inf_in_read_row")
    c = out[512]
    for s in SERIES:
        c.columns[s][511] = NAN
    c.columns["amplitude_rms"][256] = -INF
    c.non_finite = 1
    c.reach("cf:neginf_in_read_row")
    c = out[513]
    c.columns["spectrum_bands"][512, 25:] = NAN         # 25 is the last band the signature merges; 26 and 27 are not read
    c.non_finite = 1
    c.reach("cf:nan_in_read_row")
    return list(out.values())


@functools.lru_cache(maxsize=None)
def cases():
    out = (_class_cases() + _confident_cases() + _median_cases() + _track_cases() + _scalar_cases() + _signature_cases() +
           _classification_cases())
    assert len({c.name for c in out}) == len(out)
    return out


def by_name(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected_high_level(name):
    """(ref.high_level of the case, its trace): computed once, shared, never changed"""
    c = by_name(name)
    trace = {}
    want = hl.high_level(c.series(), c.rhythm[12], c.rhythm[13], c.levels[0], c.levels[1], trace=trace)
    for a in list(want.values()) + [v for v in trace.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return want, trace


def case_statistics(c):
    return {k: c.statistics[k] for k in cf.SERIES}


def expected_features(c, effective_length_12db, silence):
    """ref.classification_features of the case (the effective length is the batch's own: store_records leaves it alone)"""
    series = {k: c.columns[k] for k in cf.SERIES}
    return cf.classification_features(series, c.rhythm, effective_length_12db, statistics=case_statistics(c), silence=silence)[0]


def _targets():
    t = ["class:mean_eq_0.8", "class:mean_below_0.8", "class:mean_eq_0.5", "class:mean_below_0.5", "class:no_audible"]
    t += [f"confident:conf_{side}_{thr}" for thr in hl.CLASS_THRESHOLDS for side in ("eq", "above")]
    t += ["confident:f0_eq_20", "confident:f0_above_20", "confident:f0_eq_quarter", "confident:f0_below_quarter", "confident:f0_nan"]
    t += [f"median:{k}" for k in ("n_pitch_0", "n_pitch_1", "n_pitch_2", "n_pitch_3", "even_above_64", "odd_above_64", "all_equal",
                                  "every_exponent", "duplicates_both_sides", "silent_confident_frames", "deviation_ge_6")]
    t += [f"median:multiset_{n}" for n in MULTISET_LENGTHS]
    t += ["track:n1"] + [f"track:n{n}_on_bound" for n in TRACK_LENGTHS[1:]] + [f"track:n{n}_behind_bound" for n in TRACK_LENGTHS[2:]]
    t += ["track:silent_in_look_ahead", "track:0_and_200", "track:63_64_127_128", "track:last_frame_only"]
    t += [f"clamp:{k}" for k in ("brightness_above_1", "brightness_below_0", "noisiness_above_1", "noisiness_below_0", "harmonicity_above_1",
                                 "harmonicity_below_0", "centroid_above_100k", "rolloff_2_to_8", "flatness_above_1", "flatness_below_0",
                                 "auto_correlation_above_two_thirds", "none")]
    t += [f"level:{k}" for k in LEVELS] + [f"tempo:{v}" for v in TEMPI]
    t += [f"signature:n{n}" for n in SIGNATURE_LENGTHS] + ["signature:zero_bands"]
    t += [f"cf:n{n}" for n in CF_LENGTHS]
    t += [f"cf:{k}" for k in ("nan_in_read_row", "inf_in_read_row", "neginf_in_read_row", "unread_row_44", "unread_rows_44_65",
                              "used_statistic_slots", "unused_statistic_slots", "used_rhythm_scalars", "unused_rhythm_scalars", "padding")]
    return t


TARGETS = _targets()
