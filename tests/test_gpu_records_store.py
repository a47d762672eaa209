"""high_level_kernel (afec_amd/csrc/highlevel/afx_highlevel.hip) and classification_features_kernel
(afec_amd/csrc/classify/afx_classify.hip) on CHOSEN records: the cases of tests/_records_cases.py are written over the
results of a run with afx_batch_store_records, and the fetches above the run are held against the restatements
(tests/_highlevel_ref.py, tests/_classification_ref.py) of exactly the arrays that were stored.  What each case reaches is
asserted on the CPU (tests/test_records_cases_cpu.py).

The batches are made from zero PCM of 2 048 + 1 024 (n - 1) samples (n frames); their own results are overwritten.

What is compared how:
* bit for bit: the stored bytes through afx_batch_fetch_records / afx_batch_fetch_rhythm / afx_batch_fetch; `peak`; the BPM
  and its confidence; the audible means (the cases' sums are exact in any order, tests/_records_cases.py); which files have a
  base note and a base note confidence; where the pitch track changes and where it is zero; the copied classification
  features and the positions padded with the silence values; non_finite.  Values that are no numbers must be no numbers
  (NaN) or the same infinity at the same positions.
* through the device's log / pow (base note and its confidence, pitch, the three characteristics, the two levels, both
  signatures): BAR and ceiling() of tests/test_gpu_highlevel.py and CEILING of tests/test_gpu_classification.py, imported.
  There is no tie allowance: no file is left out."""
import numpy as np
import pytest

import afec_amd as afx
from tests import _classification_ref as cf
from tests import _highlevel_ref as hl
from tests import _records_cases as rc
from tests import test_gpu_classification as cfm
from tests import test_gpu_highlevel as hlm
from tests.test_gpu_high_level_text import check_text

pytestmark = pytest.mark.gpu

MASK = afx.D_HIGH_LEVEL_INPUTS | afx.D_CLASS_DECISION_INPUTS | afx.D_STATISTICS
S = hlm.S
WORST = {}
EXACT_MEANS = ("spectral_flatness", "spectral_flux", "spectral_complexity", "spectral_contrast", "spectral_inharmonicity", "pitch_confidence")
GROUPS = ([c for c in rc.cases() if c.n < 800], [c for c in rc.cases() if c.n >= 800])


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def zero_pcm(n):
    return np.zeros(2048 + 1024 * (n - 1), dtype=np.float32)


def pack(b, group):
    """the cases of `group` as afx_batch_store_records takes them: records [F][stride], statistics [n][stride][13], rhythm [n][14]"""
    lay = b.record_layout()
    records = np.zeros((b.total_frames, lay["stride"]))
    statistics = np.zeros((b.n_bufs, lay["stride"], afx.NUM_STATISTICS))
    rhythm = np.zeros((b.n_bufs, 14))
    row = 0
    for i, c in enumerate(group):
        for s in rc.SERIES:
            at, w = lay["offsets"][s], lay["widths"][s]
            if at >= 0:
                records[row:row + c.n, at:at + w] = c.columns[s].reshape(c.n, w)
                statistics[i, at:at + w] = c.statistics[s].reshape(w, afx.NUM_STATISTICS)
        rhythm[i] = c.rhythm
        row += c.n
    assert row == b.total_frames
    return records, statistics, rhythm


def same_or_both_nan(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


def hold(what, output, got, want):
    """hlm.hold with this module's own record of the worst error: a value the restatement does not make a number of must be
    the same on the device, every other one lies under the bars of tests/test_gpu_highlevel.py"""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    finite = np.isfinite(want)
    assert same_or_both_nan(got[~finite], want[~finite]), (what, output)
    e = hlm.error(got[finite], want[finite])
    WORST[output] = max(WORST.get(output, 0.0), e)
    print(f"HL-ERR {what} {output} {e:.3e}")
    assert e <= hlm.BAR, (what, output, e)
    assert e <= hlm.ceiling(output), (what, output, e, hlm.ceiling(output))


@pytest.fixture(scope="module")
def plan():
    p = afx.Plan(max_analysis_ms=0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def stored(plan):
    """every case stored over a run of zero PCM, two batches; per batch what every fetch then returns (made once, read only)"""
    out = []
    for group in GROUPS:
        b = plan.batch([zero_pcm(c.n) for c in group], MASK)
        b.run()
        records, statistics, rhythm = pack(b, group)
        b.store_records(records, statistics, rhythm)
        levels = [{"peak_value": float(c.levels[0]), "rms_value": float(c.levels[1])} for c in group]
        out.append({"group": group, "stored": (records, statistics, rhythm), "records": b.fetch_records(), "rhythm": b.fetch_rhythm(),
                    "unpacked": b.fetch(), "high": b.fetch_high_level(levels), "features": b.fetch_classification_features()})
        b.close()
    return out


def test_what_is_stored_is_what_every_fetch_reads(stored):
    for s in stored:
        records, statistics, rhythm = s["stored"]
        got = s["records"]
        assert np.diff(got["frame_offset"]).tolist() == [c.n for c in s["group"]] and np.all(got["buf_status"] == 0)
        assert np.array_equal(bits(got["records"]), bits(records)) and np.array_equal(bits(got["statistics"]), bits(statistics))
        assert np.array_equal(bits(s["rhythm"]["scalars"]), bits(rhythm))
        off = got["frame_offset"]
        for i, c in enumerate(s["group"]):
            for name in hl.SERIES + cf.SERIES:
                assert np.array_equal(bits(s["unpacked"][name][off[i]:off[i + 1]]), bits(c.columns[name])), (c.name, name)


def test_round_trip_partial_store_and_the_next_run(plan):
    group = [rc.by_name(k) for k in ("f0_edges", "cf_n45", "tempo_-0.3", "cf_n65")]
    b = plan.batch([zero_pcm(c.n) for c in group], MASK)
    with pytest.raises(afx.AfxError) as e:
        b.store_records(rhythm_scalars=np.zeros((4, 14)))
    assert e.value.status == -1 and "before afx_batch_run" in str(e.value)
    b.run()
    own, own_rhythm, own_high = b.fetch_records(), b.fetch_rhythm()["scalars"], b.fetch_high_level()
    records, statistics, rhythm = pack(b, group)
    records.view(np.uint64)[1, 2] = 0x7FF8000000012345          # NaNs with payloads, a signalling one among them
    records.view(np.uint64)[3, 0] = 0xFFF0000000000001
    statistics.view(np.uint64)[2, 5, 7] = 0x7FF4000000000000
    rhythm.view(np.uint64)[1, 3] = 0xFFFFFFFFFFFFFFFF
    b.store_records(records, statistics, rhythm)
    got = b.fetch_records()
    assert np.array_equal(bits(got["records"]), bits(records)) and np.array_equal(bits(got["statistics"]), bits(statistics))
    assert np.array_equal(bits(b.fetch_rhythm()["scalars"]), bits(rhythm))
    assert np.array_equal(got["frame_offset"], own["frame_offset"]) and np.array_equal(got["buf_status"], own["buf_status"])
    assert np.array_equal(bits(got["effective_length"]), bits(own["effective_length"]))
    lay = b.record_layout()
    unpacked = b.fetch()
    for name in hl.SERIES + cf.SERIES:
        at, w = lay["offsets"][name], lay["widths"][name]
        assert np.array_equal(bits(unpacked[name]).reshape(-1, w), bits(records[:, at:at + w])), name
    # records=None: the records stay, the other two change; nothing given: nothing changes
    b.store_records(None, statistics[::-1].copy(), rhythm + 1.0)
    b.store_records()
    got = b.fetch_records()
    assert np.array_equal(bits(got["records"]), bits(records)) and np.array_equal(bits(got["statistics"]), bits(statistics[::-1]))
    assert np.array_equal(bits(b.fetch_rhythm()["scalars"]), bits(rhythm + 1.0))
    # shape and dtype are checked against the layout
    for bad in (records[:-1], np.zeros(records.shape, dtype=np.float32), records.T, records[:, ::-1]):
        with pytest.raises(ValueError):
            b.store_records(bad)
    # the next run overwrites what was stored with the batch's own results, bit for bit
    b.run()
    again = b.fetch_records()
    for k in own:
        assert np.array_equal(own[k].view(np.uint8), again[k].view(np.uint8)), k
    assert np.array_equal(bits(b.fetch_rhythm()["scalars"]), bits(own_rhythm))
    high = b.fetch_high_level()
    for k in own_high:
        assert np.array_equal(own_high[k].view(np.uint8), high[k].view(np.uint8)), k
    b.close()
    # the parts a mask lacks are refused
    b = plan.batch([zero_pcm(2)], afx.D_MFCC | afx.D_AMPLITUDE_PEAK)
    b.run()
    stride = b.record_layout()["stride"]
    for kw in ({"statistics": np.zeros((1, stride, 13))}, {"rhythm_scalars": np.zeros((1, 14))}):
        with pytest.raises(afx.AfxError) as e:
            b.store_records(**kw)
        assert e.value.status == -1 and "was not in the batch mask" in str(e.value)
    b.store_records(np.full((2, stride), 0.375))
    assert np.all(b.fetch()["amplitude_peak"] == 0.375)
    b.close()


def test_high_level_of_every_case(stored):
    notes = {}
    for s in stored:
        off, high = s["records"]["frame_offset"], s["high"]
        assert np.all(high["status"] == 0)
        for i, c in enumerate(s["group"]):
            want, _ = rc.expected_high_level(c.name)
            rows = slice(off[i], off[i + 1])
            sc, sig, pitch, w = high["scalars"][i], high["signature"][i], high["pitch"][rows], want["scalars"]
            print("HL-CASE", c.name, " ".join(f"{k}={sc[S[k]]!r}" for k in ("base_note", "base_note_confidence", "pitch_confidence")))
            assert np.array_equal(bits(high["peak"][rows]), bits(c.columns["amplitude_peak"])), c.name
            # exact: the tempo and its confidence, the audible means (sums that are exact in any order)
            assert bits(sc[S["bpm"]]) == bits(w[S["bpm"]]) and bits(sc[S["bpm_confidence"]]) == bits(c.rhythm[13]), c.name
            for name in EXACT_MEANS:
                if np.isfinite(w[S[name]]):
                    assert bits(sc[S[name]]) == bits(w[S[name]]), (c.name, name, sc[S[name]], w[S[name]])
                else:      # a sum over a planted NaN or infinity: the same infinity, or a NaN (its payload is not the reference's)
                    assert same_or_both_nan(sc[S[name]], w[S[name]]), (c.name, name, sc[S[name]], w[S[name]])
            # exact: what the class and the comparisons against the thresholds decide
            assert (sc[S["base_note"]] == -1.0) == (w[S["base_note"]] == -1.0), c.name
            assert (sc[S["base_note_confidence"]] == 0.0) == (w[S["base_note_confidence"]] == 0.0), c.name
            assert np.array_equal(np.nonzero(np.diff(pitch))[0], np.nonzero(np.diff(want["pitch"]))[0]), c.name
            assert np.array_equal(pitch == 0.0, want["pitch"] == 0.0), c.name
            for name in ("brightness", "noisiness", "harmonicity"):
                if w[S[name]] in (0.0, 1.0):                       # a clamp: exactly the bound
                    assert sc[S[name]] == w[S[name]], (c.name, name)
            # through the device's log and pow
            hold(c.name, "pitch", pitch, want["pitch"])
            hold(c.name, "signature", sig, want["signature"])
            for name in ("peak_db", "rms_db", "base_note", "base_note_confidence", "brightness", "noisiness", "harmonicity"):
                hold(c.name, name, sc[S[name]], w[S[name]])
            if c.name.startswith("median_multiset_"):
                notes[c.n] = sc[S["base_note"]]
    # the same multiset of pitches, keys in LDS (1 024 frames) or read from the records: one base note
    assert sorted(notes) == list(rc.MULTISET_LENGTHS) and len({v.tobytes() for v in notes.values()}) == 1, notes
    print("HL-WORST " + " ".join(f"{k}={v:.3e}" for k, v in sorted(WORST.items())))


def test_classification_features_of_every_case(plan, stored):
    silence = plan.silence_features()
    worst = 0.0
    for s in stored:
        features, bad, status = s["features"]
        efflen = s["unpacked"]["effective_length"]
        assert np.all(status == 0)
        for i, c in enumerate(s["group"]):
            want, got = rc.expected_features(c, efflen[i][2], silence), features[i]
            copied = slice(cfm.SIGNATURE, None)
            assert np.array_equal(bits(got[copied]), bits(want[copied])), \
                (c.name, np.nonzero(bits(got[copied]) != bits(want[copied]))[0][:8] + cfm.SIGNATURE)
            padded = np.tile(np.array(cf.TIME_SERIES) >= c.n, 14)
            assert np.array_equal(bits(got[:cfm.SIGNATURE][padded]), bits(want[:cfm.SIGNATURE][padded])), c.name
            g, w = got[:cfm.SIGNATURE], want[:cfm.SIGNATURE]
            finite = np.isfinite(w)
            assert same_or_both_nan(g[~finite], w[~finite]), c.name
            e = cfm.signature_error(g[finite], w[finite])
            worst = max(worst, e)
            assert e <= cfm.CEILING < 1e-12, (c.name, e, cfm.CEILING)
            print(f"CF-CASE {c.name} non_finite={bad[i]} signature {e:.3e}")
            assert bad[i] == cf.non_finite(want) == c.non_finite, (c.name, bad[i], cf.non_finite(want), c.non_finite)
    assert sum(1 for s in stored for b in s["features"][1] if b > 0) >= 8
    print(f"CF-WORST signature={worst:.3e}")


def test_text_of_stored_records(plan):
    """amplitude_peak values that are no ordinary numbers, through the text fetch: held against the arrays the plain fetch
    returns from the same stored records"""
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 5e-324, 1e300])
    b = plan.batch([zero_pcm(special.size), zero_pcm(3)], afx.D_HIGH_LEVEL_INPUTS)
    b.run()
    records = b.fetch_records()["records"]
    records[:special.size, b.record_layout()["offsets"]["amplitude_peak"]] = special
    b.store_records(records)
    high, text = b.fetch_high_level(), b.fetch_high_level_text()
    assert np.array_equal(bits(high["peak"][:special.size]), bits(special))
    assert text["scalars"].tobytes() == high["scalars"].tobytes()
    check_text(text, high, b.fetch()["frame_offset"], "stored records")
    assert text["peak"][0] not in (b"[]", text["peak"][1])
    print("HLT-STORED", text["peak"][0])
    b.close()
