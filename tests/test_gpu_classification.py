"""afx_batch_fetch_classification_features on the GPU (afec_amd/csrc/classify/afx_classify.hip) against the restatement of
TSampleClassificationDescriptors (tests/_classification_ref.py; reference SampleClassificationDescriptors.cpp:395-561).

Cases: the reference's 74 readable fixture WAVs and synthetic files through afx_batch_create_from_raw, synthetic files of
exactly 1, 2, 43, 44, 45, 65, 129, 257, 513 and 860 frames through afx_batch_create (LoadSample's padding leaves a whole
file 1 or an even number of frames, so the odd counts cannot come out of the front end), a refused buffer in each, an
empty batch; each with the mask AFX_D_CLASSIFICATION_INPUTS and with every per-frame series (another record stride).

For every case the batch's OWN records, statistics, rhythm scalars and effective lengths are fetched and fed to the
restatement, so the comparison isolates the new kernel from the parity bars of the kernels that wrote them.

PARITY UNPINNED: the reference's SampleClassificationDescriptors.cpp does not build here, so the flow is not held against
the reference's objects; the restatement's primitives and the fixture files' inputs are (tests/test_classification_ref_cpu.py).

What is compared how:
* the 1 008 gathered values (everything behind the signature) and the signature's padded positions: bit for bit;
* the signature's computed values differ from the restatement only by the device's pow against the host's: relative
  error |got - want| / |want| (0 where the two are equal), held under CEILING = 10 x the worst error measured over
  all tests of this module, which itself must lie below 1e-12 (three orders above a correctly rounded pow);
* non_finite equals the restatement's count and is 0 for every file of the set; status repeats buf_status."""
import numpy as np
import pytest

import afec_amd as afx
from tests import _classification_ref as ref
from tests.test_gpu_highlevel import fixture_raws

pytestmark = pytest.mark.gpu

MASK = afx.D_CLASSIFICATION_INPUTS
WIDE = afx.D_ALL_PER_FRAME | afx.D_STATISTICS | afx.D_EFFECTIVE_LENGTH | afx.D_RHYTHM   # another record stride
SIGNATURE = 14 * 48
LENGTHS = (1, 2, 43, 44, 45, 65, 129, 257, 513, 860)
# MEASURED: the worst relative error of a signature value against the restatement over all tests of this module
# (188 files), from the CF-WORST line: 2.2203333707193513e-16 -- one rounding of a double (2^-52 = 2.2204e-16).
# MI355X, 2026-10-16, on a build of this change that preceded the last edits of the host-side sources (the shared
# classify_time_frame of classify/afx_classify.h; the kernel's arithmetic is the same); that library reported
# "afx abi=7 arch=gfx950 stamps=0 ablation=0 src=251e894eedd1971f".  NOT re-measured on the final sources
# (src=81922fbf6634ebcb): no GPU run came through after them.
MEASURED_SIGNATURE = 2.2203333707193513e-16
CEILING = 10.0 * MEASURED_SIGNATURE
WORST = {"signature": 0.0}


def signature_error(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(got == want, 0.0, np.abs(got - want) / np.abs(want))
    return float(np.max(e)) if e.size else 0.0


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def check_batch(b, what):
    """every file of batch `b` (it has run) against the restatement of its own results; -> the fetch"""
    res, st, rh = b.fetch(), b.fetch_statistics(), b.fetch_rhythm()
    features, bad, status = b.fetch_classification_features()
    off = res["frame_offset"]
    assert features.shape == (b.n_bufs, 1680) and bad.shape == status.shape == (b.n_bufs,)
    assert np.array_equal(status, res["buf_status"])
    for i in range(b.n_bufs):
        tag = f"{what}[{i}]"
        if status[i] != 0 or off[i + 1] == off[i]:
            assert np.all(bits(features[i]) == 0) and bad[i] == 0, tag
            continue
        sl = slice(off[i], off[i + 1])
        series = {k: res[k][sl] for k in ref.SERIES}
        statistics = {k: st[k][i] for k in ref.SERIES}
        want, _ = ref.classification_features(series, rh["scalars"][i], res["effective_length"][i][2], statistics=statistics)
        got = features[i]
        frames = off[i + 1] - off[i]
        assert np.array_equal(bits(got[SIGNATURE:]), bits(want[SIGNATURE:])), \
            (tag, np.nonzero(bits(got[SIGNATURE:]) != bits(want[SIGNATURE:]))[0][:8] + SIGNATURE)
        padded = np.tile(np.array(ref.TIME_SERIES) >= frames, 14)
        assert np.array_equal(bits(got[:SIGNATURE][padded]), bits(want[:SIGNATURE][padded])), tag
        e = signature_error(got[:SIGNATURE], want[:SIGNATURE])
        WORST["signature"] = max(WORST["signature"], e)
        print(f"CF-ERR {tag} frames={frames} signature {e:.3e}")
        assert e < 1e-12, (tag, e)
        assert CEILING < 1e-12 and e <= CEILING, (tag, e, CEILING)
        assert bad[i] == ref.non_finite(want) == 0, (tag, bad[i])
    print(f"CF-WORST signature={WORST['signature']:.3e} build={afx.build_info()}")
    return features, bad, status


def synthetic(samples, seed):
    """a tone with a slow tremolo over noise, loud from the first to the last sample (nothing for LoadSample to trim)"""
    rng = np.random.default_rng(seed)
    t = np.arange(samples)
    f = 150.0 + 35.0 * (seed % 9)
    return 0.45 * np.sin(2 * np.pi * f * t / 44100.0) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t / 44100.0)) + 0.1 * rng.uniform(-1, 1, samples)


def synthetic_pcm(frames, seed):
    """float32 PCM of exactly `frames` analysis frames for afx_batch_create"""
    return synthetic(2048 + 1024 * (frames - 1), seed).astype(np.float32)


def synthetic_raw(frames, seed):
    """int16 mono PCM of 1 024 x `frames` samples for afx_batch_create_from_raw.  LoadSample pads a file so that it ends
    on an odd multiple of half a frame, so a whole file has 1 or an even number of frames (and the 20 s cap's 860): the
    LENGTHS come out as 1, 2, 42, 44, 44, 64, 128, 256, 512, 860 -- the odd counts are reached through afx_batch_create."""
    return np.round(20000 * synthetic(1024 * frames, seed)).astype(np.int16)


@pytest.mark.parametrize("mask", [MASK, WIDE], ids=["inputs", "wide"])
def test_fixture_files_of_the_reference(mask):
    raws = fixture_raws()
    assert len(raws) == 74
    plan = afx.Plan()
    b, _ = plan.batch_from_raw(raws, mask)
    b.run()
    features, bad, status = check_batch(b, f"fixtures-{mask:#x}")
    assert np.all(status == 0) and np.all(bad == 0) and np.all(np.isfinite(features))
    b.close()
    plan.close()


@pytest.mark.parametrize("source", ["pcm", "raw"])
@pytest.mark.parametrize("mask", [MASK, WIDE], ids=["inputs", "wide"])
def test_ragged_synthetic_lengths_with_a_refused_buffer(mask, source):
    """files of 1, 2, 43, 44, 45, 65, 129, 257, 513 and 860 frames (every boundary of sTimeSeries from both sides) and a
    refused buffer between them: with exactly these frame counts through afx_batch_create, and the same lengths through
    afx_batch_create_from_raw, whose LoadSample padding makes the odd counts even (synthetic_raw)"""
    plan = afx.Plan()
    if source == "pcm":
        bufs = [synthetic_pcm(f, k) for k, f in enumerate(LENGTHS)]
        bufs.insert(4, synthetic_pcm(3, 99).astype(np.float64))     # float64 among float32: refused (AFX_ERR_BAD_BUFFER)
        b = plan.batch(bufs, mask)
        expected = list(LENGTHS)
    else:
        raws = [(synthetic_raw(f, k), 1) for k, f in enumerate(LENGTHS)]
        raws.insert(4, (synthetic_raw(3, 99), 9))                   # nine channels: refused (AFX_ERR_BAD_BUFFER)
        b, _ = plan.batch_from_raw(raws, mask)
        oracle = ref._oracle.Oracle()
        expected = [oracle.num_frames(ref._oracle.load_sample(r, 1)[1]["n_samples"], cap=True) for r, _ in raws[:4] + raws[5:]]
        assert expected == [1, 2, 42, 44, 44, 64, 128, 256, 512, 860]
    b.run()
    features, bad, status = check_batch(b, f"lengths-{source}-{mask:#x}")
    counts = np.diff(b.fetch()["frame_offset"]).tolist()
    assert counts == expected[:4] + [0] + expected[4:]
    assert status.tolist() == [0] * 4 + [-6] + [0] * 6
    assert np.all(features[4] == 0.0) and bad[4] == 0
    # what the long files add: frames 64, 128, 256, 512 are real where the file has them, silence values where not
    names = afx.classification_feature_names()
    sil = plan.silence_features()
    for row, frames in zip([0, 1, 2, 3, 5, 6, 7, 8, 9, 10], expected):
        for i, frame in enumerate(ref.TIME_SERIES):
            # a frame of tone and noise has no flat spectrum: flatness 1 is the silence value
            assert (features[row][names.index(f"spectral_flatness_t{i}")] == sil[15]) == (frame >= frames), (row, i)
        assert (features[row][names.index("spectrum_signature_b3_t512")] > 0.0) == (frames > 512)
    b.close()
    plan.close()


def test_empty_batch():
    plan = afx.Plan()
    b, _ = plan.batch_from_raw([], MASK)
    b.run()
    features, bad, status = b.fetch_classification_features()
    assert features.shape == (0, 1680) and bad.size == 0 and status.size == 0
    b.close()
    plan.close()


def test_silence_features_are_the_analysis_of_one_frame_of_zeros():
    plan = afx.Plan()
    sil = plan.silence_features()
    assert sil.shape == (afx.NUM_CF_SILENCE,)
    assert np.array_equal(bits(sil), bits(ref.silence_values()))
    b = plan.batch([np.zeros(2048, dtype=np.float32)], MASK)
    b.run()
    res = b.fetch()
    assert res["frame_offset"].tolist() == [0, 1]
    own = np.concatenate([res["spectrum_bands"][0][:14]] + [np.atleast_1d(res[k][0]) for k in ref.SILENCE_SERIES])
    assert np.array_equal(bits(own), bits(sil)), (own, sil)
    # and they are what the fetch pads with: positions 1.. of this one-frame file
    features, bad, _ = b.fetch_classification_features()
    names = afx.classification_feature_names()
    for k, name in enumerate(ref.SILENCE_SERIES):
        a = names.index(f"{name}_t0")
        assert np.all(bits(features[0][a + 1:a + 48]) == bits(sil[14 + k])[0]), name
    for band in range(14):
        assert np.all(bits(features[0][48 * band + 1:48 * band + 48]) == bits(sil[band])[0]), band
    print("CF-ZEROS non_finite", int(bad[0]))
    b.close()
    plan.close()


def test_call_order_repeats_and_other_fetches():
    plan = afx.Plan()
    raws = [(synthetic_raw(20, 1), 1), (synthetic_raw(70, 2), 1)]
    b, infos = plan.batch_from_raw(raws, MASK | afx.D_HIGH_LEVEL_INPUTS)
    with pytest.raises(afx.AfxError) as ei:       # before the first run
        b.fetch_classification_features()
    assert ei.value.status == -1
    b.run()
    records_before, high_before = b.fetch(), b.fetch_high_level(infos)
    one, two = b.fetch_classification_features(), b.fetch_classification_features()
    for x, y in zip(one, two):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))              # bit for bit
    records_after, high_after = b.fetch(), b.fetch_high_level(infos)
    for k in records_before:
        assert np.array_equal(records_before[k].view(np.uint8), records_after[k].view(np.uint8)), k
    for k in high_before:
        assert np.array_equal(high_before[k].view(np.uint8), high_after[k].view(np.uint8)), k
    # afx_batch_fetch_records too: the raw records and statistics
    import ctypes
    stride = ctypes.c_int32()
    b.L.afx_batch_record_layout.argtypes = [ctypes.c_void_p] * 4
    b.L.afx_batch_record_layout(b.h, ctypes.byref(stride), None, None)
    b.L.afx_batch_fetch_records.argtypes = [ctypes.c_void_p] * 6
    raw = [np.zeros((b.total_frames, stride.value)) for _ in range(2)]
    assert b.L.afx_batch_fetch_records(b.h, raw[0].ctypes.data, None, None, None, None) == 0
    b.fetch_classification_features()
    assert b.L.afx_batch_fetch_records(b.h, raw[1].ctypes.data, None, None, None, None) == 0
    assert np.array_equal(raw[0].view(np.uint8), raw[1].view(np.uint8)) and np.any(raw[0] != 0.0)
    b.close()
    # a batch whose mask lacks one of the inputs
    for missing in (afx.D_RHYTHM, afx.D_STATISTICS, afx.D_EFFECTIVE_LENGTH, afx.D_MFCC, afx.D_AMPLITUDE_SILENCE):
        b, _ = plan.batch_from_raw(raws, MASK & ~missing)
        b.run()
        with pytest.raises(afx.AfxError) as ei:
            b.fetch_classification_features()
        assert ei.value.status == -1
        b.close()
    plan.close()
