"""Restatement of TSampleClassificationDescriptors (the reference's SampleClassificationDescriptors.cpp:38-65, 395-561) in
Python, written from the reference's text: values and names are appended one by one in the reference's order, the merged
band is summed serially, statistics come from the oracle's pinned TStatistics::Calc (tests/_oracle.calc_statistics) unless
the caller hands in statistics of its own (the GPU test feeds the batch's).

Test helper only -- the product never imports it.  PARITY UNPINNED in the sense of DESIGN 2: the reference's
SampleClassificationDescriptors.cpp does not build here (CoreTypes, the analyser's model libraries), so the flow below is not
held against the reference's objects; its inputs (tests/golden/fixtures.npz) and its primitives (calc_statistics, the
oracle's frames of silence) are."""
import math

import numpy as np

from tests import _oracle

TIME_SERIES = list(range(44)) + [64, 128, 256, 512]                    # sTimeSeries (:38-42)
SPECTRUM_BANDS = [0, 1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25]    # sSpectrumBands (:62-65)
NUM_FEATURES = 1680
# (reference name, name of the series in this project's results) in the reference's order
SCALAR_SERIES = [("spectral_rms", "spectral_rms"), ("spectral_flatness", "spectral_flatness"), ("spectral_flux", "spectral_flux"),
                 ("spectral_contrast", "spectral_contrast"), ("spectral_complexity", "spectral_complexity"),
                 ("f0_confidence", "f0_confidence")]                    # :475-501
BAND_SERIES = [("spectral_rms_bands", "sub_rms"), ("spectral_flatness_bands", "sub_flatness"), ("spectral_flux_bands", "sub_flux"),
               ("spectral_complexity_bands", "sub_complexity"), ("spectral_contrast_bands", "sub_contrast"),
               ("cepstrum_bands", "mfcc")]                              # :506-513: complexity BEFORE contrast
SERIES = ["spectrum_bands", "amplitude_rms", "amplitude_silence"] + [k for _, k in SCALAR_SERIES + BAND_SERIES]
# sStatisticsNames (:111-141) and where each lies among the 13 of TStatistics::Calc (AFX_S_*)
STATISTICS = [("min", 0), ("max", 1), ("mean", 3), ("variance", 5), ("flatness", 10), ("dmean", 11), ("dvariance", 12)]
# :527-538, with the index into the rhythm tracker's 14 scalars (AFX_R_*)
RHYTHM_SCALARS = [("rhythm_complex_tempo_confidence", 2), ("rhythm_percussive_tempo_confidence", 8),
                  ("rhythm_complex_onset_contrast", 5), ("rhythm_percussive_onset_contrast", 11),
                  ("rhythm_complex_onset_strength", 4), ("rhythm_percussive_onset_strength", 10)]
# the order of afx_plan_get_silence_features behind the 14 bands
SILENCE_SERIES = ["spectral_rms", "spectral_flatness", "spectral_flux", "spectral_contrast", "spectral_complexity",
                  "f0_confidence", "amplitude_rms"]
NUM_SILENCE = 14 + len(SILENCE_SERIES)

_silence = None


def silence_values():
    """[21]: frequency_bands 0..13, then SILENCE_SERIES, of the LAST frame the oracle makes of 2 048 zeros -- what
    LoadSample (SA:646-701) turns the half second of zeros of SCreateSilenceSampleDescriptors (:326-360) into"""
    global _silence
    if _silence is None:
        o = _oracle.Oracle()
        zeros = np.zeros(2048)
        frame, neigh = o.run(zeros)[-1], o.run_neighbours(zeros)[-1]

        def value(name):
            if name in _oracle.FIELDS:
                return frame[_oracle.FIELDS[name][0]]
            return neigh[_oracle.NEIGH_FIELDS[name]]
        a = _oracle.FIELDS["spectrum_bands"][0]
        _silence = np.array(list(frame[a:a + 14]) + [value(k) for k in SILENCE_SERIES])
    return _silence.copy()


def statistics_of(series):
    """{series: [13] or [W][13]}: TStatistics::Calc of every column of SERIES"""
    out = {}
    for k in SERIES:
        x = np.asarray(series[k], dtype=np.float64)
        out[k] = _oracle.calc_statistics(x) if x.ndim == 1 else np.stack([_oracle.calc_statistics(x[:, c]) for c in range(x.shape[1])])
    return out


def classification_features(series, rhythm, effective_length_12db, statistics=None, silence=None):
    """series: dict of the SERIES arrays of one file ([F] each; spectrum_bands [F][28], the band series [F][14]);
    rhythm: the rhythm tracker's 14 scalars; statistics: as statistics_of() gives them (None: computed here).
    -> (values [1680], names [1680]); the reference throws where a value is not finite, this returns it."""
    g = {k: np.asarray(series[k], dtype=np.float64) for k in SERIES}
    frames = g["spectral_rms"].shape[0]
    bands = g["spectrum_bands"].reshape(frames, -1)
    st = statistics_of(g) if statistics is None else statistics
    sil = silence_values() if silence is None else np.asarray(silence, dtype=np.float64)
    values, names = [], []

    def add(name, value):
        names.append(name)
        values.append(float(value))

    def add_time_frames(name, x, no_value):        # SAddDescriptorSpectrumTimeFrames (:73-102): the INDEX in the name
        for i, frame in enumerate(TIME_SERIES):
            add(f"{name}_t{i}", x[frame] if frame < frames else no_value)

    def add_statistics(name, s):                   # SAddDescriptorSpectrumStatistics (:106-164)
        for stat, slot in STATISTICS:
            add(f"{name}_{stat}", s[slot])

    def add_band_statistics(name, s):              # SAddDescriptorBandStatistics (:206-268): band outer
        for band in range(s.shape[0]):
            for stat, slot in STATISTICS:
                add(f"{name}_{stat}_b{band}", s[band][slot])

    # ... sharpened, condensed spectrum bands (:432-469): the frame NUMBER in the name
    for b in range(len(SPECTRUM_BANDS)):
        for frame in TIME_SERIES:
            name = f"spectrum_signature_b{b}_t{frame}"
            if frame < frames:
                first = SPECTRUM_BANDS[b - 1] + 1 if b - 1 >= 0 else 0
                last = SPECTRUM_BANDS[b]
                merged = 0.0
                for sb in range(first, last + 1):
                    merged += bands[frame, sb]
                merged /= float(last - first + 1)
                add(name, math.pow(merged * 1.25, 1.0 / 6.0))
            else:
                add(name, sil[b])                  # mSpectrumBands.mValues.Last()[b]: band b of the 28 (:466)
    # ... spectrum time series vectors (:475-491), their statistics (:496-501)
    for i, (name, key) in enumerate(SCALAR_SERIES):
        add_time_frames(name, g[key], sil[14 + SILENCE_SERIES.index(key)])
    for name, key in SCALAR_SERIES:
        add_statistics(name, st[key])
    # ... band statistics (:506-513)
    for name, key in BAND_SERIES:
        add_band_statistics(name, np.asarray(st[key]))
    # ... amplitude, rhythm and length (:519-538)
    add_time_frames("amplitude_rms", g["amplitude_rms"], sil[14 + SILENCE_SERIES.index("amplitude_rms")])
    add_statistics("amplitude_rms", st["amplitude_rms"])
    add_statistics("amplitude_silence", st["amplitude_silence"])
    for name, slot in RHYTHM_SCALARS:
        add(name, rhythm[slot])
    add("effectve_length_12dB", effective_length_12db)
    # ... pad to sTimeSeriesLength width (:543-553)
    k = 0
    while len(values) % len(TIME_SERIES) != 0:
        add(f"padding_{k}", st["spectral_rms"][3])
        k += 1
    return np.array(values), names


def feature_names():
    zeros = {k: np.zeros((1, 28 if k == "spectrum_bands" else 14)) if k in ("spectrum_bands",) + tuple(b for _, b in BAND_SERIES)
             else np.zeros(1) for k in SERIES}
    return classification_features(zeros, np.zeros(14), 0.0, silence=np.zeros(NUM_SILENCE))[1]


def non_finite(values):
    return int(np.sum(~np.isfinite(values)))
