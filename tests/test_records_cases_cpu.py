"""The chosen records of tests/_records_cases.py reach what they claim -- on the CPU, from the restatements alone
(tests/_highlevel_ref.py, tests/_classification_ref.py), before tests/test_gpu_records_store.py stores them on a device.

* exactness: for every case built on the dyadic premise, each sum the high-level kernel forms over the audible frames is
  the same number forwards, backwards and as math.fsum gives it, so the order of additions on the device cannot matter;
* reach: every condition of _records_cases.TARGETS is claimed by at least one case, and every claim is read back from the
  restatement's own intermediate values (high_level(trace=...)) or from the feature vector; a case that stops reaching its
  target fails here."""
import math

import numpy as np
import pytest

from tests import _classification_ref as cf
from tests import _highlevel_ref as hl
from tests import _records_cases as rc

S = {name: i for i, name in enumerate(hl.SCALARS)}
CASES = rc.cases()


def test_every_sum_of_a_dyadic_case_is_exact_in_any_order():
    checked = 0
    for c in CASES:
        if not c.dyadic:
            continue
        audible = c.columns["amplitude_silence"] == 0.0
        for name in rc.SUMMED:
            x = [float(v) for v in c.columns[name][audible]]
            forward = backward = 0.0
            for v in x:
                forward += v
            for v in reversed(x):
                backward += v
            assert forward == backward == math.fsum(x), (c.name, name)
            checked += 1
    assert checked >= 8 * 40


def test_every_target_is_claimed_and_no_case_claims_an_unknown_one():
    claimed = {t for c in CASES for t in c.reaches}
    assert claimed == set(rc.TARGETS), (sorted(set(rc.TARGETS) - claimed), sorted(claimed - set(rc.TARGETS)))
    assert all(c.reaches for c in CASES)
    lengths = {c.n for c in CASES}
    assert set(rc.SIGNATURE_LENGTHS) <= lengths and set(rc.CF_LENGTHS) <= lengths and set(rc.TRACK_LENGTHS) <= lengths


def frames_where(c, t, conf, confident):
    """frames whose f0 lies inside (20, quarter) and whose confidence is `conf`: all of them `confident` or not"""
    f0, fc = c.columns["f0"], c.columns["f0_confidence"]
    hit = [p for p in range(c.n) if fc[p] == conf and 20.0 < f0[p] < rc.QUARTER]
    return bool(hit) and all(bool(t["confident"][p]) == confident for p in hit)


def first_audible_confident(t):
    hit = np.nonzero(t["audible"] & t["confident"])[0]
    return int(hit[0]) if hit.size else -1


def reached(target, c, want, t):
    """does the restatement's run of case `c` show the condition `target`?"""
    kind, what = target.split(":", 1)
    sc, f0 = want["scalars"], c.columns["f0"]
    audible, confident = t["audible"], t["confident"]
    if kind == "class":
        one = int(audible.sum()) == 1
        if what == "mean_eq_0.8":
            return one and t["conf_mean"] == 0.8 and t["threshold"] == 0.8 and not confident[audible][0]
        if what == "mean_below_0.8":
            return one and t["conf_mean"] == rc.down(0.8) and t["threshold"] == 0.5
        if what == "mean_eq_0.5":
            return t["conf_mean"] == 0.5 and t["threshold"] == 0.5 and set(c.columns["f0_confidence"][audible]) == {0.25, 0.75}
        if what == "mean_below_0.5":
            return one and t["conf_mean"] == rc.down(0.5) and t["threshold"] == 0.2
        if what == "no_audible":
            return (not audible.any() and t["conf_mean"] == 0.0 and t["threshold"] == 0.2 and sc[S["base_note"]] > 0.0
                    and all(sc[S[k]] == 0.0 for k in ("brightness", "noisiness", "harmonicity", "base_note_confidence")))
    if kind == "confident":
        if what.startswith("conf_eq_"):
            thr = float(what[len("conf_eq_"):])
            return t["threshold"] == thr and frames_where(c, t, thr, False)
        if what.startswith("conf_above_"):
            thr = float(what[len("conf_above_"):])
            return t["threshold"] == thr and frames_where(c, t, rc.up(thr), True)
        high = c.columns["f0_confidence"] > t["threshold"]
        probe = {"f0_eq_20": (20.0, False), "f0_above_20": (rc.up(20.0), True), "f0_eq_quarter": (rc.QUARTER, False),
                 "f0_below_quarter": (rc.down(rc.QUARTER), True)}
        if what in probe:
            # the probed frame is audible, behind the look-ahead and the only one with a pitch: what the comparison decides
            # is the whole answer -- no pitch, base note -1 and a track of zeros, or one pitch, its note and a track from it on
            hz, is_confident = probe[what]
            hit = np.nonzero((f0 == hz) & high & audible)[0]
            if hit.size != 1 or np.count_nonzero(f0) != 1 or hit[0] <= t["look_ahead_last"] or bool(confident[hit[0]]) != is_confident:
                return False
            if not is_confident:
                return t["pitches"].size == 0 and sc[S["base_note"]] == -1.0 and np.all(t["pitch_hz"] == 0.0) and np.all(want["pitch"] == 0.0)
            return (t["pitches"].size == 1 and sc[S["base_note"]] == hl.freq_to_midi(hz) > 0.0 and np.all(t["pitch_hz"][:hit[0]] == 0.0)
                    and np.all(t["pitch_hz"][hit[0]:] == hz) and np.all(want["pitch"][hit[0]:] > 0.0))
        if what == "f0_nan":
            hit = np.nonzero(np.isnan(f0) & high)[0]
            return hit.size > 0 and not confident[hit].any() and np.all(np.isfinite(sc)) and np.all(np.isfinite(want["pitch"]))
    if kind == "median":
        pitches = np.sort(t["pitches"])
        k = pitches.size
        rank = (k - 1) // 2
        if what == "n_pitch_0":
            return k == 0 and sc[S["base_note"]] == -1.0 and sc[S["base_note_confidence"]] == 0.0
        if what == "n_pitch_1":
            return k == 1 and t["deviation"] == 0.0 and sc[S["base_note_confidence"]] == t["conf_mean"] > 0.0
        if what == "n_pitch_2":
            return k == 2 and t["median_hz"] == pitches[0] < pitches[1]
        if what == "n_pitch_3":
            return k == 3 and t["median_hz"] == pitches[1] and 0.0 < sc[S["base_note_confidence"]] < t["conf_mean"]
        if what == "even_above_64":
            return k > 64 and k % 2 == 0 and t["median_hz"] == pitches[rank] < pitches[rank + 1]
        if what == "odd_above_64":
            return k > 64 and k % 2 == 1 and t["median_hz"] == pitches[rank]
        if what == "all_equal":
            return k > 64 and pitches[0] == pitches[-1] == t["median_hz"] and t["deviation"] == 0.0
        if what == "every_exponent":
            return {math.frexp(v)[1] - 1 for v in pitches} == set(range(4, 14))
        if what == "duplicates_both_sides":
            return pitches[rank - 1] == pitches[rank] == pitches[rank + 1] and pitches[0] < pitches[rank] < pitches[-1]
        if what == "silent_confident_frames":
            heard = np.sort(f0[confident & audible])
            return heard.size > 0 and heard[(heard.size - 1) // 2] != t["median_hz"] == pitches[rank]
        if what == "deviation_ge_6":
            return t["deviation"] >= 6.0 and sc[S["base_note_confidence"]] == 0.0 and t["conf_mean"] > 0.0
        if what.startswith("multiset_"):
            return c.n == int(what[len("multiset_"):]) and k == 1000 and np.array_equal(pitches, 100.0 + 0.5 * np.arange(1000))
    if kind == "track":
        first, bound, hz = first_audible_confident(t), t["look_ahead_last"], t["pitch_hz"]
        if what == "n1":
            return c.n == 1 and bound == -1 and confident[0] and hz[0] == f0[0]
        if what.endswith("_on_bound") or what.endswith("_behind_bound"):
            n = int(what[1:what.index("_")])
            if what.endswith("_on_bound"):
                return c.n == n and first == bound == max(1, n // 4) and np.all(hz[:first + 1] == f0[first])
            return c.n == n and first == bound + 1 and np.all(hz[:first] == 0.0) and hz[first] == f0[first]
        if what == "silent_in_look_ahead":
            quiet = np.nonzero(confident & ~audible)[0]
            return quiet.size > 0 and quiet[0] < first <= bound and np.all(hz[:first + 1] == f0[first])
        if what == "0_and_200":
            return np.nonzero(confident)[0].tolist() == [0, 200] and np.all(hz[:200] == f0[0]) and np.all(hz[200:] == f0[200]) and c.n > 256
        if what == "63_64_127_128":
            return np.nonzero(confident & audible)[0].tolist() == [63, 64, 127, 128] and len(set(f0[[63, 64, 127, 128]])) == 4 and first > bound
        if what == "last_frame_only":
            return np.nonzero(confident & audible)[0].tolist() == [c.n - 1] and np.all(hz[:-1] == 0.0) and hz[-1] > 0.0
    if kind == "clamp":
        w = t["weights"]
        checks = {"brightness_above_1": lambda: w["brightness"] > 1.0 and sc[S["brightness"]] == 1.0,
                  "brightness_below_0": lambda: w["brightness"] < 0.0 and sc[S["brightness"]] == 0.0,
                  "noisiness_above_1": lambda: w["noisiness"] > 1.0 and sc[S["noisiness"]] == 1.0,
                  "noisiness_below_0": lambda: w["noisiness"] < 0.0 and sc[S["noisiness"]] == 0.0,
                  "harmonicity_above_1": lambda: w["harmonicity"] > 1.0 and sc[S["harmonicity"]] == 1.0,
                  "harmonicity_below_0": lambda: w["harmonicity"] < 0.0 and sc[S["harmonicity"]] == 0.0,
                  "centroid_above_100k": lambda: t["centroid_max"] > 100000.0 and hl.freq_to_midi(t["centroid_max"]) == 0.0,
                  "rolloff_2_to_8": lambda: 2.0 <= t["rolloff_mean"] <= 8.0 and hl.freq_to_midi(t["rolloff_mean"]) < 0.0,
                  "flatness_above_1": lambda: np.all(c.columns["spectral_flatness"][audible] > 1.0),
                  "flatness_below_0": lambda: np.all(c.columns["spectral_flatness"][audible] < 0.0),
                  "auto_correlation_above_two_thirds": lambda: 1.5 * t["auto_correlation_mean"] > 1.0,
                  "none": lambda: all(0.0 < w[k] < 1.0 and 0.0 < sc[S[k]] < 1.0 for k in ("brightness", "noisiness", "harmonicity"))}
        return bool(checks[what]())
    if kind == "level":
        v = rc.LEVELS[what]
        at = [i for i in (0, 1) if c.levels[i] == v and np.float32(c.levels[i]).tobytes() == v.tobytes()]
        # eps_up: 20 log10(1.0000001e-12) = -239.9999991, rounded to float
        db = {"1.0": lambda d: d == 0.0, "eps": lambda d: d == -200.0, "eps_up": lambda d: d == -240.0, "0": lambda d: d == -200.0}
        return bool(at) and all(db[what](sc[i]) for i in at)
    if kind == "tempo":
        v = float(what)
        return t["final_tempo"] == v and sc[S["bpm"]] == hl.quantize_nearest(v, 0.5) and \
            np.float64(sc[S["bpm_confidence"]]).tobytes() == np.float64(c.rhythm[13]).tobytes()
    if kind == "signature":
        if what == "zero_bands":
            return np.all(want["signature"] == 0.0) and not np.signbit(want["signature"]).any()
        bands = c.columns["spectrum_bands"]
        return c.n == int(what[1:]) and np.all(np.isin(bands * 4.0, np.arange(1, 17))) and np.all(np.isfinite(want["signature"]))
    raise AssertionError(f"no check for {target}")


@pytest.mark.parametrize("case", [c for c in CASES if any(not t.startswith("cf:") for t in c.reaches)], ids=lambda c: c.name)
def test_high_level_case_reaches_its_targets(case):
    want, trace = rc.expected_high_level(case.name)
    for target in case.reaches:
        if not target.startswith("cf:"):
            assert reached(target, case, want, trace), (case.name, target)
    # neighbours in rank differ by at least 2^-30 relative or not at all: a rank that is off by one is either the same
    # note or one far beyond the ceiling
    pitches = np.sort(trace["pitches"])
    if pitches.size > 1:
        steps = np.diff(pitches) / pitches[:-1]
        assert np.all((steps == 0.0) | (steps >= 2.0 ** -30)), case.name


def test_the_multiset_files_have_one_base_note():
    notes = {rc.expected_high_level(f"median_multiset_{n}")[0]["scalars"][S["base_note"]].tobytes() for n in rc.MULTISET_LENGTHS}
    assert len(notes) == 1
    want, trace = rc.expected_high_level("median_multiset_1024")
    assert trace["median_hz"] == 100.0 + 0.5 * 499 and want["scalars"][S["base_note"]] > 0.0


def test_tempi_cover_every_branch_of_the_quantiser():
    got = [hl.quantize_nearest(v, 0.5) for v in rc.TEMPI]
    assert got == [0.0, 0.0, 0.5, 120.0, 120.0, 90.0, -0.5]


@pytest.mark.parametrize("case", [c for c in CASES if any(t.startswith("cf:") for t in c.reaches)], ids=lambda c: c.name)
def test_classification_case_reaches_its_targets(case):
    silence = cf.silence_values()
    want = rc.expected_features(case, 0.25, silence)
    names = cf.feature_names()
    bad = [names[j] for j in np.nonzero(~np.isfinite(want))[0]]
    assert cf.non_finite(want) == len(bad) == case.non_finite, (case.name, bad)
    padded = [i for i, frame in enumerate(cf.TIME_SERIES) if frame >= case.n]
    for i, frame in enumerate(cf.TIME_SERIES):
        value = want[names.index(f"spectral_rms_t{i}")]
        if i in padded:
            assert value == silence[14]
        else:
            assert np.float64(value).tobytes() == np.float64(case.columns["spectral_rms"][frame]).tobytes()
    for target in case.reaches:
        what = target[3:]
        if what == f"n{case.n}":
            assert len(padded) == sum(1 for frame in cf.TIME_SERIES if frame >= case.n)
        elif what in ("nan_in_read_row", "inf_in_read_row", "neginf_in_read_row"):
            kind = {"nan_in_read_row": np.isnan, "inf_in_read_row": np.isposinf, "neginf_in_read_row": np.isneginf}[what]
            assert any(kind(want[j]) for j in range(want.size) if "_t" in names[j]), (case.name, target)
        elif what in ("unread_row_44", "unread_rows_44_65"):
            rows = [44] if what == "unread_row_44" else [44, 65]
            assert all(np.isnan(case.columns[s][r]).all() for s in rc.SERIES for r in rows) and case.non_finite == 0
        elif what == "used_statistic_slots":
            assert sorted(n for n in bad) == sorted(f"spectral_flatness_{stat}" for stat, _ in cf.STATISTICS)
        elif what == "unused_statistic_slots":
            assert case.non_finite == 0 and all(np.isnan(case.statistics[s][..., rc.UNUSED_STAT_SLOTS]).all() for s in rc.SERIES)
        elif what == "used_rhythm_scalars":
            assert sorted(bad) == sorted(name for name, _ in cf.RHYTHM_SCALARS)
        elif what == "unused_rhythm_scalars":
            assert case.non_finite == 0 and not np.isfinite(case.rhythm[rc.UNUSED_RHYTHM]).any()
        elif what == "padding":
            assert sorted(bad) == sorted(["spectral_rms_mean"] + [f"padding_{k}" for k in range(21)])
        else:
            raise AssertionError(f"no check for {target}")
