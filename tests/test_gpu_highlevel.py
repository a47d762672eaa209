"""afx_batch_fetch_high_level on the GPU (afec_amd/csrc/highlevel/afx_highlevel.hip) against the restatement of
AnalyzeHighLevelDescriptors (tests/_highlevel_ref.py; reference SampleAnalyser.cpp:1234-1606).

For every case the batch's OWN low-level records, rhythm scalars and load infos are fetched and fed to the restatement,
so the comparison isolates the new kernel from the parity bars of the low-level kernels.

PARITY UNPINNED: the reference's SampleAnalyser.cpp does not build here (Shark, LightGBM, CoreTypes), so the flow of
AnalyzeHighLevelDescriptors is not held against the reference's objects; the restatement's primitives and the fixture
files' inputs are (tests/test_highlevel_ref_cpu.py).

What is compared how:
* exact: status, the BPM (a multiple of 0.5) and its confidence, base note -1 / confidence 0 decisions, the frames where
  the pitch track changes value, NaN levels, `peak` equal to amplitude_peak bit for bit;
* everything else differs from the restatement only by the order of additions and the device's log / pow: BAR is the
  project's 1e-4 relative (README.md, Parity), CEILING the regression ceiling beside it.
* a file whose audible mean f0 confidence lies within TIE of 0.8 / 0.5 may fall into the other class on the device: it is
  reported and left out of the value comparison, at most 1 % of a test's files and none of the fixture set.

The error of a value is |got - want| / (|want| + 1e-9)."""
import os

import numpy as np
import pytest

import afec_amd as afx
from tests import _highlevel_ref as ref
from tests._wav import parse_wav

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
MASK = afx.D_HIGH_LEVEL_INPUTS
S = {name: i for i, name in enumerate(ref.SCALARS)}
BAR = 1e-4
TIE = 1e-9
# Regression ceilings: 10 x the worst error of each output over all tests of this module on the first clean run, measured
# against the restatement (never against a second GPU run), and never lower than 16 roundings of a double (3.6e-15: an
# output that came out exact on that run may still move by the last bits of a sum of ten terms).
# MEASURED: MI355X, 2026-10-16, build "afx abi=7 arch=gfx950 stamps=0 ablation=0 src=ab4b0936dd9ca55c" (the same figures as
# on the first clean run, build src=4706b31f494b4745, whose kernel file is this one).  The signature's
# worst value is a cubic that overshoots to about 1e-3 between a silent and a loud frame (cancellation of terms near 1).
MEASURED = {"base_note": 1.138e-16, "base_note_confidence": 1.850e-15, "brightness": 5.168e-16, "harmonicity": 2.342e-15,
            "noisiness": 2.550e-15, "peak_db": 0.0, "rms_db": 0.0, "pitch": 2.978e-16, "pitch_confidence": 2.503e-16,
            "signature": 4.396e-14, "spectral_complexity": 0.0, "spectral_contrast": 8.802e-16,
            "spectral_flatness": 1.916e-15, "spectral_flux": 1.332e-15, "spectral_inharmonicity": 0.0}
FLOOR = 16 * 2.0 ** -52
WORST = {}


def ceiling(output):
    return max(10.0 * MEASURED[output], FLOOR)


def error(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want) / (np.abs(want) + 1e-9)))


def hold(what, output, got, want):
    e = error(got, want)
    WORST[output] = max(WORST.get(output, 0.0), e)
    print(f"HL-ERR {what} {output} {e:.3e}")
    assert e <= BAR, (what, output, e)
    assert e <= ceiling(output), (what, output, e, ceiling(output))


def check_batch(b, levels, what, ties_allowed=None):
    """every file of batch `b` (it has run) against the restatement of its own low-level results; -> the fetch"""
    res, rh = b.fetch(), b.fetch_rhythm()
    hl = b.fetch_high_level(levels)
    off, status = res["frame_offset"], res["buf_status"]
    assert np.array_equal(hl["status"], status)
    assert np.array_equal(hl["peak"].view(np.uint64), res["amplitude_peak"].view(np.uint64))
    ties = 0
    for i in range(b.n_bufs):
        tag = f"{what}[{i}]"
        sl = slice(off[i], off[i + 1])
        series = {k: res[k][sl] for k in ref.SERIES}
        sc, sig, pitch = hl["scalars"][i], hl["signature"][i], hl["pitch"][sl]
        if status[i] != 0 or off[i + 1] == off[i]:
            assert np.all(sc == 0.0) and np.all(sig == 0.0), tag     # zeros (afx.h), whatever the levels are
            continue
        peak, rms = (levels[i]["peak_value"], levels[i]["rms_value"]) if levels is not None else (None, None)
        want = ref.high_level(series, rh["scalars"][i][12], rh["scalars"][i][13], peak, rms)
        w = want["scalars"]
        # decisions that do not depend on the class
        assert sc[S["bpm"]] == w[S["bpm"]] and sc[S["bpm"]] * 2.0 == np.round(sc[S["bpm"]] * 2.0), tag
        assert sc[S["bpm_confidence"]] == w[S["bpm_confidence"]], tag
        if levels is None:
            assert np.isnan(sc[S["peak_db"]]) and np.isnan(sc[S["rms_db"]]), tag
        else:
            hold(tag, "peak_db", sc[S["peak_db"]], w[S["peak_db"]])
            hold(tag, "rms_db", sc[S["rms_db"]], w[S["rms_db"]])
        hold(tag, "signature", sig, want["signature"])
        margin = ref.class_margin(series)
        print(f"HL-MARGIN {tag} {margin:.3e}")
        assert margin > TIE or ties_allowed != 0, (tag, margin)   # the cases of this module are chosen away from the thresholds
        if margin <= TIE:
            ties += 1
            print(f"HL-TIE {tag}: audible mean f0 confidence within {TIE} of a class threshold, values not compared")
            continue
        assert (sc[S["base_note"]] == -1.0) == (w[S["base_note"]] == -1.0), tag
        assert (sc[S["base_note_confidence"]] == 0.0) == (w[S["base_note_confidence"]] == 0.0), tag
        assert np.array_equal(np.nonzero(np.diff(pitch))[0], np.nonzero(np.diff(want["pitch"]))[0]), tag
        assert np.array_equal(pitch == 0.0, want["pitch"] == 0.0), tag
        hold(tag, "pitch", pitch, want["pitch"])
        for name in ref.SCALARS:
            if name not in ("peak_db", "rms_db", "bpm", "bpm_confidence"):
                hold(tag, name, sc[S[name]], w[S[name]])
    allowed = b.n_bufs // 100 if ties_allowed is None else ties_allowed
    assert ties <= allowed, (what, ties, allowed)
    print("HL-WORST " + " ".join(f"{k}={v:.3e}" for k, v in sorted(WORST.items())))
    return hl


def plan_for(kernel, **kw):
    return afx.Plan(frame_kernel=afx.FRAME_KERNEL_WAVE64 if kernel == "wave64" else afx.FRAME_KERNEL_HALFWAVE, **kw)


def fixture_raws():
    z = np.load(os.path.join(GOLD, "fixtures.npz"))
    raws = []
    for i, name in enumerate(str(n) for n in z["names"]):
        if f"stored_{i}" in z.files:
            image = open(os.path.join(GOLD, "wav", str(z[f"stored_{i}"])), "rb").read()
        else:
            image = open(os.path.join(GOLD, "reference_wav", name), "rb").read()
        try:
            channels, rate, bits, n, payload = parse_wav(image)
        except ValueError:
            continue   # the one file that is no wave file
        raws.append((np.frombuffer(payload, dtype=np.int16 if bits == 16 else np.uint8), channels))
    return raws


def synthetic(kind, frames, seed):
    """float32 PCM of exactly `frames` analysis frames: tonal / noisy / tone bursts between silent gaps"""
    n = 2048 + 1024 * (frames - 1)
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == "tonal":
        f = 180.0 + 40.0 * (seed % 7)
        x = 0.5 * np.sin(2 * np.pi * f * t / 44100.0) + 0.2 * np.sin(2 * np.pi * 2 * f * t / 44100.0) + 0.002 * rng.uniform(-1, 1, n)
    elif kind == "noisy":
        x = 0.4 * rng.uniform(-1, 1, n)
    else:
        x = 0.6 * np.sin(2 * np.pi * 261.6 * t / 44100.0) * ((t // 3072) % 3 != 1) + 0.05 * rng.uniform(-1, 1, n) * ((t // 5120) % 2 == 0)
    return x.astype(np.float32)


@pytest.mark.parametrize("kernel", ["wave64", "halfwave"])
def test_fixture_files_of_the_reference(kernel):
    raws = fixture_raws()
    assert len(raws) == 74
    plan = plan_for(kernel)
    b, infos = plan.batch_from_raw(raws, MASK)
    print("HL-INFO", kernel, b.info())
    b.run()
    hl = check_batch(b, infos, f"fixtures-{kernel}", ties_allowed=0)
    assert np.all(hl["status"] == 0) and np.all(np.isfinite(hl["scalars"]))
    b.close()
    plan.close()


def test_synthetic_files_of_the_golden_set():
    z = np.load(os.path.join(GOLD, "files.npz"))
    cases = sorted(k[len("raw_"):] for k in z.files if k.startswith("raw_"))
    assert len(cases) >= 4
    plan = afx.Plan()
    b, infos = plan.batch_from_raw([(z["raw_" + c], int(z["channels_" + c])) for c in cases], MASK)
    b.run()
    check_batch(b, infos, "files.npz", ties_allowed=0)
    b.close()
    plan.close()


@pytest.mark.parametrize("kernel", ["wave64", "halfwave"])
def test_synthetic_lengths(kernel):
    """tonal / noisy / silent-gapped files of 1, 2, 5, 63, 64, 65 and 860 frames (860: the 20 s cap's length), created
    from float PCM with afx_batch_create: no load infos, so the two levels are NaN and everything else is defined"""
    lengths = (1, 2, 5, 63, 64, 65, 860)
    bufs = [synthetic(kind, f, 11 * k + j) for k, kind in enumerate(("tonal", "noisy", "gapped")) for j, f in enumerate(lengths)]
    plan = plan_for(kernel)
    b = plan.batch(bufs, MASK)
    b.run()
    hl = check_batch(b, None, f"lengths-{kernel}", ties_allowed=0)
    assert np.diff(b.fetch()["frame_offset"]).tolist() == list(lengths) * 3
    assert np.all(np.isnan(hl["scalars"][:, :2])) and np.all(np.isfinite(hl["scalars"][:, 2:]))
    # the 20 s tonal file has a base note, and the pitch tracks are not all zero
    assert hl["scalars"][6, S["base_note"]] > 0.0 and np.any(hl["pitch"] > 0.0)
    # the same run with levels handed in: only the two dB scalars change
    levels = [{"peak_value": 0.03 * (i + 1), "rms_value": 0.01 * (i + 1)} for i in range(len(bufs))]
    hl2 = check_batch(b, levels, f"lengths-{kernel}-levels", ties_allowed=0)
    assert np.array_equal(hl["scalars"][:, 2:].view(np.uint64), hl2["scalars"][:, 2:].view(np.uint64))
    assert np.all(np.isfinite(hl2["scalars"][:, :2]))
    b.close()
    plan.close()


def test_series_longer_than_the_lds_stage_without_the_cap():
    """max_analysis_ms = 0: 1 100 and 4 200 frames -- the confident pitches no longer fit the kernel's 1 024 keys in LDS
    and the radix select reads them from the records; the median must still be the exact element"""
    plan = afx.Plan(max_analysis_ms=0)
    bufs = [synthetic("gapped", 1100, 5), synthetic("tonal", 4200, 3), synthetic("noisy", 40, 9)]
    b = plan.batch(bufs, MASK)
    b.run()
    hl = check_batch(b, None, "uncapped", ties_allowed=0)
    assert np.diff(b.fetch()["frame_offset"]).tolist() == [1100, 4200, 40]
    assert hl["scalars"][1, S["base_note"]] > 0.0
    b.close()
    plan.close()


def test_ragged_batch_with_an_empty_and_a_refused_buffer():
    rng = np.random.default_rng(21)
    a = synthetic("tonal", 30, 2)
    short = rng.uniform(-1, 1, 1000).astype(np.float32)            # fewer samples than one frame: no frames
    refused = rng.uniform(-1, 1, 2048 + 1024 * 4)                  # float64 among float32 buffers: AFX_ERR_BAD_BUFFER
    c = synthetic("gapped", 7, 4)
    plan = afx.Plan()
    b = plan.batch([a, short, refused, c, synthetic("noisy", 1, 6)], MASK)
    b.run()
    levels = [{"peak_value": 0.5, "rms_value": 0.1}] * 5
    hl = check_batch(b, levels, "ragged", ties_allowed=0)
    assert hl["status"].tolist() == [0, 0, -6, 0, 0]
    assert np.diff(b.fetch()["frame_offset"]).tolist() == [30, 0, 0, 7, 1]
    assert np.all(hl["scalars"][1:3] == 0.0) and np.all(hl["signature"][1:3] == 0.0)
    assert np.all(hl["scalars"][[0, 3, 4], S["peak_db"]] == hl["scalars"][0, S["peak_db"]]) and hl["scalars"][0, S["peak_db"]] < 0.0
    b.close()
    plan.close()


def test_repeated_and_partial_fetches_and_refusals():
    plan = afx.Plan()
    bufs = [synthetic("tonal", 20, 1), synthetic("gapped", 33, 2)]
    b = plan.batch(bufs, MASK)
    with pytest.raises(afx.AfxError) as ei:       # before the first run
        b.fetch_high_level()
    assert ei.value.status == -1
    b.run()
    one, two = b.fetch_high_level(), b.fetch_high_level()
    for k in one:
        assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), k     # bit for bit
    # NULL members of afx_high_out are skipped; the others are what the full fetch gave
    for want in (("scalars",), ("signature", "status"), ("pitch", "peak"), ()):
        part = b.fetch_high_level(want=want)
        assert sorted(part) == sorted(want)
        for k in want:
            assert np.array_equal(part[k].view(np.uint8), one[k].view(np.uint8)), k
    # a second run of the batch leaves the same results
    b.run()
    three = b.fetch_high_level()
    for k in one:
        assert np.array_equal(one[k].view(np.uint8), three[k].view(np.uint8)), k
    b.close()
    # a batch whose mask lacks one of the inputs
    for missing in (afx.D_RHYTHM, afx.D_SPECTRUM_BANDS, afx.D_F0, afx.D_AMPLITUDE_PEAK):
        b = plan.batch(bufs, MASK & ~missing)
        b.run()
        with pytest.raises(afx.AfxError) as ei:
            b.fetch_high_level()
        assert ei.value.status == -1
        b.close()
    # more series than needed are fine
    b = plan.batch(bufs, afx.D_ALL_PER_FRAME | afx.D_RHYTHM | afx.D_STATISTICS)
    b.run()
    more = b.fetch_high_level()
    assert more["pitch"].shape == one["pitch"].shape and np.all(np.isfinite(more["scalars"][:, 2:])) and np.all(more["status"] == 0)
    b.close()
    plan.close()
