"""Restatement of the model-free part of TSampleAnalyser::AnalyzeHighLevelDescriptors (the reference's
SampleAnalyser.cpp:1234-1606) in Python, written from the reference's text: serial sums in the reference's order, the
oracle's pinned primitives (tests/_oracle.py: mean, median, min, max, variance, lin_to_db) where one exists.

Test helper only -- the product never imports it.  PARITY UNPINNED: the reference's SampleAnalyser.cpp does not build
here (Shark, LightGBM, CoreTypes), so the flow below is not held against the reference's objects; its primitives and its
inputs (tests/golden/fixtures.npz) are."""
import math

import numpy as np

from tests import _oracle

SCALARS = ["peak_db", "rms_db", "base_note", "base_note_confidence", "bpm", "bpm_confidence", "brightness", "noisiness",
           "harmonicity", "spectral_flatness", "spectral_flux", "spectral_complexity", "spectral_contrast",
           "spectral_inharmonicity", "pitch_confidence"]
SERIES = ["amplitude_silence", "amplitude_peak", "f0", "f0_confidence", "auto_correlation", "spectral_rolloff",
          "spectral_centroid", "spectral_flatness", "spectral_flux", "spectral_complexity", "spectral_inharmonicity",
          "spectral_contrast", "spectrum_bands"]
SIGNATURE_FRAMES, SIGNATURE_BANDS = 64, 14
SPECTRUM_BANDS = [0, 1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25]   # sSpectrumBands, :1450-1453
CLASS_THRESHOLDS = (0.8, 0.5, 0.2)   # MHighPitchConfidenceValue, MMedium.., MLow.. (:64-66)


def freq_to_midi(freq):
    """aubio_freqtomidi (aubio mathutils.c:535-546, smpl_t = double)"""
    if freq < 2.0 or freq > 100000.0:
        return 0.0
    midi = freq / 6.875
    midi = math.log(midi) / 0.69314718055995
    midi *= 12.0
    midi -= 3.0
    return midi


def lin_to_db_float(value):
    """TAudioMath::LinToDb(float) (AudioMath.inl:38-53): the overload mPeakValue / mRmsValue select; it computes what the
    double overload (pinned: afx_oracle_lin_to_db) computes for the same value and rounds to float"""
    return float(np.float32(_oracle.stat("lin_to_db", float(np.float32(value)))))


def quantize_nearest(value, step):
    """TMath::Quantize(double&, Step, kRoundToNearest) (InlineMath.inl:625-636); d2i truncates"""
    value = value + step / 2.0 if value > 0.0 else value - step / 2.0
    return float(int(value / step)) * step


def interpolate_cubic(ym1, y0, y1, y2, pos):
    """SInterpolateCubic (:139-156)"""
    x = pos - math.floor(pos)
    xx = x * x
    xxx = xx * x
    a = -0.5 * xxx + xx - 0.5 * x
    b = 1.5 * xxx - 2.5 * xx + 1.0
    c = -1.5 * xxx + 2.0 * xx + 0.5 * x
    d = 0.5 * xxx - 0.5 * xx
    return a * ym1 + b * y0 + c * y1 + d * y2


def _mean(x):
    return _oracle.stat("mean", np.asarray(x, dtype=np.float64)) if len(x) else 0.0


def _mmin(a, b):
    return a if a < b else b


def _mmax(a, b):
    return a if a > b else b


def confidence_class(audible_confidence_mean):
    """the threshold of IsConfidentPitch (:1262-1277)"""
    if audible_confidence_mean >= CLASS_THRESHOLDS[0]:
        return CLASS_THRESHOLDS[0]
    if audible_confidence_mean >= CLASS_THRESHOLDS[1]:
        return CLASS_THRESHOLDS[1]
    return CLASS_THRESHOLDS[2]


def class_margin(series):
    """distance of the audible mean f0 confidence from the nearer class threshold (inf without audible frames: the mean
    is then the constant 0)"""
    audible = np.asarray(series["amplitude_silence"]) == 0.0
    if not audible.any():
        return math.inf
    m = _mean(np.asarray(series["f0_confidence"], dtype=np.float64)[audible])
    return min(abs(m - CLASS_THRESHOLDS[0]), abs(m - CLASS_THRESHOLDS[1]))


def high_level(series, final_tempo, final_tempo_confidence, peak_value=None, rms_value=None, sample_rate=44100, trace=None):
    """series: dict of the SERIES arrays of one file ([F] each, spectrum_bands [F][28]).
    -> dict: "scalars" [15] (SCALARS order), "signature" [64][14], "pitch" [F], "peak" [F].
    A file without frames yields zeros (the reference's resampling loop is undefined for it).
    trace: a dict that is filled with the intermediate values of the flow (what decided what) -- for tests that must
    know which branch a chosen input took (tests/test_records_cases_cpu.py); the result does not depend on it."""
    g = {k: np.asarray(series[k], dtype=np.float64) for k in SERIES}
    frames = g["f0"].size
    if frames == 0:
        return {"scalars": np.zeros(len(SCALARS)), "signature": np.zeros((SIGNATURE_FRAMES, SIGNATURE_BANDS)),
                "pitch": np.zeros(0), "peak": np.zeros(0)}
    audible = g["amplitude_silence"] == 0.0   # mSpectrumFrameIsAudible (:865-868)
    f0, conf = g["f0"], g["f0_confidence"]
    quarter = sample_rate // 4                # mSampleRate / 4, integers

    # ... BaseNote (:1234-1331)
    conf_mean = _mean(conf[audible])
    threshold = confidence_class(conf_mean)

    def is_confident(hz, c):
        return c > threshold and hz > 20 and hz < quarter

    confident = np.array([is_confident(f0[i], conf[i]) for i in range(frames)], dtype=bool)
    pitches = f0[confident]
    base_note = -1.0
    hz = deviation = math.nan
    if pitches.size:
        hz = _oracle.stat("median", pitches)
        if hz > 20 and hz < quarter:
            base_note = freq_to_midi(hz)
    if base_note > 0.0:
        offsets = np.array([abs(base_note - freq_to_midi(p)) for p in pitches])
        deviation = math.sqrt(_oracle.stat("variance", offsets, _oracle.stat("mean", offsets)))
        base_note_confidence = conf_mean * (1.0 - _mmin(1.0, deviation / 6.0))
    else:
        base_note_confidence = 0.0

    # ... Loudness (:1336-1339)
    peak_db = math.nan if peak_value is None else lin_to_db_float(peak_value)
    rms_db = math.nan if rms_value is None else lin_to_db_float(rms_value)

    # ... BPM (:1345-1349)
    bpm = quantize_nearest(float(final_tempo), 0.5)

    # ... Characteristics (:1354-1444)
    rolloff, centroid, flatness = g["spectral_rolloff"][audible], g["spectral_centroid"][audible], g["spectral_flatness"][audible]
    acorr = g["auto_correlation"][audible]
    brightness = noisiness = harmonicity = 0.0
    weights = {}
    if rolloff.size:
        w = freq_to_midi(_mean(rolloff)) / 128.0 * 0.7 + freq_to_midi(_oracle.stat("max", centroid)) / 128.0 * 0.3
        weights["brightness"] = w
        w = _mmax(0.0, _mmin(1.0, w))
        brightness = math.pow(w, 4.0)
        w = ((1.0 - _oracle.stat("min", flatness)) * 0.2 + (1.0 - _mean(flatness)) * 0.6 +
             (1.0 - _oracle.stat("max", flatness)) * 0.2)
        weights["noisiness"] = w
        w = _mmax(0.0, _mmin(1.0, w))
        noisiness = math.pow(w, 2.0)
        w = _mmin(1.0, 1.5 * _mean(acorr)) * 0.4 + _mmin(1.0, 2.0 * conf_mean) * 0.3 + _mean(flatness) * 0.3
        weights["harmonicity"] = w
        w = _mmax(0.0, _mmin(1.0, w))
        harmonicity = math.pow(w, 2.0)

    # ... Spectrum bands (:1450-1520)
    bands = g["spectrum_bands"].reshape(frames, -1)
    scaled = np.zeros((frames, SIGNATURE_BANDS))
    for f in range(frames):
        for b in range(SIGNATURE_BANDS):
            first = SPECTRUM_BANDS[b - 1] + 1 if b >= 1 else 0
            last = SPECTRUM_BANDS[b]
            merged = 0.0
            for sb in range(first, last + 1):
                merged += bands[f, sb]
            merged /= float(last - first + 1)
            scaled[f, b] = math.pow(merged * 1.25, 1.0 / 6.0)
    signature = np.zeros((SIGNATURE_FRAMES, SIGNATURE_BANDS))
    step = float(frames) / SIGNATURE_FRAMES
    pos = 0.0
    for i in range(SIGNATURE_FRAMES):
        ipos = int(pos)   # TMath::d2i
        im1, i0, i1, i2 = max(0, ipos - 1), ipos, min(frames - 1, ipos + 1), min(frames - 1, ipos + 2)
        for j in range(SIGNATURE_BANDS):
            signature[i, j] = interpolate_cubic(scaled[im1, j], scaled[i0, j], scaled[i1, j], scaled[i2, j], pos)
        pos += step

    # ... Spectral Features (:1529-1553)
    means = [_mean(g[k][audible]) for k in ("spectral_flatness", "spectral_flux", "spectral_complexity", "spectral_contrast",
                                            "spectral_inharmonicity")]

    # ... Pitch (:1557-1596)
    last_pitch = 0.0
    look_ahead_hit = -1
    if frames > 1:
        for i in range(max(1, frames // 4) + 1):
            if audible[i] and confident[i]:
                last_pitch = f0[i]
                look_ahead_hit = i
                break
    pitch = np.zeros(frames)
    pitch_hz = np.zeros(frames)
    for i in range(frames):
        if audible[i] and confident[i]:
            last_pitch = f0[i]
        pitch_hz[i] = last_pitch
        pitch[i] = freq_to_midi(last_pitch)

    if trace is not None:
        trace.update(frames=frames, audible=audible, conf_mean=conf_mean, threshold=threshold, confident=confident,
                     pitches=pitches, median_hz=hz, deviation=deviation if base_note > 0.0 else math.nan, weights=weights,
                     auto_correlation_mean=_mean(acorr), look_ahead_last=max(1, frames // 4) if frames > 1 else -1,
                     look_ahead_hit=look_ahead_hit, pitch_hz=pitch_hz, final_tempo=float(final_tempo),
                     rolloff_mean=_mean(rolloff), centroid_max=_oracle.stat("max", centroid) if centroid.size else math.nan)

    scalars = np.array([peak_db, rms_db, base_note, base_note_confidence, bpm, float(final_tempo_confidence), brightness,
                        noisiness, harmonicity] + means + [conf_mean])
    return {"scalars": scalars, "signature": signature, "pitch": pitch, "peak": g["amplitude_peak"].copy()}
