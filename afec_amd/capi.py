"""ctypes binding of include/afx.h (libafx_hip.so).

The library is the only compute path: if it is missing or fails to load this module raises --
there is no Python or CPU fallback.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# AFX_LIBRARY selects an alternative build of the same library (kernel tuning experiments)
_LIB_PATH = os.environ.get("AFX_LIBRARY") or os.path.join(_HERE, "lib", "libafx_hip.so")

D_MFCC = 1 << 0
D_SPECTRAL_RMS = 1 << 1
D_SPECTRAL_CENTROID = 1 << 2
D_SPECTRAL_SPREAD = 1 << 3
D_SPECTRAL_SKEWNESS = 1 << 4
D_SPECTRAL_KURTOSIS = 1 << 5
D_SPECTRAL_ROLLOFF = 1 << 6
D_SPECTRAL_FLATNESS = 1 << 7
D_SPECTRAL_FLUX = 1 << 8
D_SPECTRUM_BANDS = 1 << 9
D_BAND_FEATURES = 1 << 10
D_AMPLITUDE_PEAK = 1 << 11
D_AMPLITUDE_RMS = 1 << 12
D_MAGNITUDE = 1 << 13
D_STATISTICS = 1 << 14
# neighbours of the spectral set
D_AMPLITUDE_SILENCE = 1 << 15
D_AMPLITUDE_ENVELOPE = 1 << 16
D_SPECTRAL_COMPLEXITY = 1 << 17
D_AUTO_CORRELATION = 1 << 18
D_F0 = 1 << 19
D_SPECTRAL_INHARMONICITY = 1 << 20
D_TRISTIMULUS = 1 << 21
D_EFFECTIVE_LENGTH = 1 << 22   # per buffer: [n_bufs][3]
D_RHYTHM = 1 << 23             # per buffer: the 512/128 rhythm tracker (fetch_rhythm)
RHYTHM_SCALARS = [f"rhythm_{k}_{n}" for k in ("complex", "percussive")
                  for n in ("onset_count", "tempo", "tempo_confidence", "onset_frequency_mean", "onset_strength",
                            "onset_contrast")] + ["rhythm_final_tempo", "rhythm_final_tempo_confidence"]
NUM_STATISTICS = 13
STAT_NAMES = ["min", "max", "median", "mean", "gmean", "variance", "centroid", "spread", "skewness",
              "kurtosis", "flatness", "dmean", "dvariance"]
D_C2 = D_MFCC
D_SPECTRAL_STATS = 0x1FE
D_ALL_LOW_LEVEL = 0x1FFF
D_NEIGHBOURS = 0x3F8000
D_ALL_PER_FRAME = D_ALL_LOW_LEVEL | D_NEIGHBOURS
# afx_batch_fetch_high_level: the bits a batch's mask must hold, the scalars' order (AFX_HL_*), the signature's shape
D_HIGH_LEVEL_INPUTS = (D_AMPLITUDE_SILENCE | D_AMPLITUDE_PEAK | D_F0 | D_AUTO_CORRELATION | D_SPECTRAL_ROLLOFF |
                       D_SPECTRAL_CENTROID | D_SPECTRAL_FLATNESS | D_SPECTRAL_FLUX | D_SPECTRAL_COMPLEXITY |
                       D_SPECTRAL_INHARMONICITY | D_BAND_FEATURES | D_SPECTRUM_BANDS | D_RHYTHM)
HL_SCALARS = ["peak_db", "rms_db", "base_note", "base_note_confidence", "bpm", "bpm_confidence", "brightness", "noisiness",
              "harmonicity", "spectral_flatness", "spectral_flux", "spectral_complexity", "spectral_contrast",
              "spectral_inharmonicity", "pitch_confidence"]
(HL_PEAK_DB, HL_RMS_DB, HL_BASE_NOTE, HL_BASE_NOTE_CONFIDENCE, HL_BPM, HL_BPM_CONFIDENCE, HL_BRIGHTNESS, HL_NOISINESS,
 HL_HARMONICITY, HL_SPECTRAL_FLATNESS, HL_SPECTRAL_FLUX, HL_SPECTRAL_COMPLEXITY, HL_SPECTRAL_CONTRAST,
 HL_SPECTRAL_INHARMONICITY, HL_PITCH_CONFIDENCE) = range(15)
NUM_HL_SCALARS = len(HL_SCALARS)
HL_SIGNATURE_FRAMES, HL_SIGNATURE_BANDS = 64, 14
# afx_batch_fetch_classification_features: the bits a batch's mask must hold, the vector's shape
D_CLASSIFICATION_INPUTS = (D_MFCC | D_SPECTRAL_RMS | D_SPECTRAL_FLATNESS | D_SPECTRAL_FLUX | D_SPECTRUM_BANDS |
                           D_BAND_FEATURES | D_AMPLITUDE_RMS | D_AMPLITUDE_SILENCE | D_SPECTRAL_COMPLEXITY | D_F0 |
                           D_STATISTICS | D_EFFECTIVE_LENGTH | D_RHYTHM)
CF_TIME_FRAMES, NUM_CLASSIFICATION_FEATURES, NUM_CF_SILENCE = 48, 1680, 21
# afx_batch_fetch_class_decision: the mask's bits, afx_decision_out.flags, the scalars afx_decide reads per file
D_CLASS_DECISION_INPUTS = D_CLASSIFICATION_INPUTS | D_AMPLITUDE_PEAK
DECISION_IS_ONESHOT, DECISION_IS_LOOP, DECISION_OVERRIDDEN = 1, 2, 4
# afx_batch_fetch_high_level_text: the columns that come back as text (AFX_HLT_*)
HLT_COLUMNS = ["spectrum_signature", "pitch", "peak"]
# afx_batch_fetch_high_level_row: the nine text columns of the reference's high-level table, in its order (AFX_HLR_*)
HLR_COLUMNS = ["class_signature", "classes", "class_strengths", "category_signature", "categories", "category_strengths",
               "spectrum_signature", "pitch", "peak"]
DECISION_SCALARS = ["effectve_length_24dB", "rhythm_percussive_onset_count", "rhythm_percussive_tempo_confidence",
                    "rhythm_complex_tempo_confidence", "spectral_flux_mean"]
PRECISION_F64, PRECISION_F32 = 0, 1
PCM_F32, PCM_F64 = 0, 1
FRAME_KERNEL_AUTO, FRAME_KERNEL_WAVE64, FRAME_KERNEL_HALFWAVE = 0, 1, 2   # afx_plan_desc.frame_kernel
PLAN_NO_SIDE_STREAM = 1                                                   # afx_plan_desc.flags

# every symbol include/afx.h declares (tests check the library exports exactly these)
EXPORTS = [
    "afx_status_str", "afx_last_error", "afx_build_info", "afx_plan_create", "afx_plan_destroy",
    "afx_plan_get_window", "afx_plan_get_mel_table", "afx_plan_get_bin_range", "afx_num_frames",
    "afx_extract_batch", "afx_batch_create", "afx_batch_total_frames", "afx_batch_run",
    "afx_batch_sync", "afx_batch_run_timed", "afx_batch_fetch", "afx_batch_fetch_statistics", "afx_batch_destroy",
    "afx_algorithmic_bytes_per_frame", "afx_batch_create_from_raw", "afx_batch_fetch_samples",
    "afx_host_alloc", "afx_host_free", "afx_batch_record_layout", "afx_batch_fetch_records", "afx_batch_store_records",
    "afx_batch_set_file_info", "afx_batch_rhythm_frames", "afx_batch_fetch_rhythm", "afx_batch_fetch_onset_functions",
    "afx_plan_set_blocking_wait", "afx_batch_get_info", "afx_plan_probe_device", "afx_device_count",
    "afx_batch_fetch_high_level",
    "afx_batch_fetch_classification_features", "afx_classification_feature_name", "afx_plan_get_silence_features",
    "afx_model_create_from_lightgbm", "afx_model_destroy", "afx_model_get_info", "afx_batch_fetch_class_signature",
    "afx_model_evaluate_features", "afx_batch_fetch_class_decision", "afx_decide",
    "afx_batch_high_level_text_capacity", "afx_batch_fetch_high_level_text", "afx_format_json_g9",
    "afx_batch_high_level_row_capacity", "afx_batch_fetch_high_level_row", "afx_format_class_json",
    "afx_flac_probe", "afx_flac_build_index",
    "afx_batch_create_from_device", "afx_batch_export_device", "afx_batch_export_statistics_device",
    "afx_batch_export_frame_counts_device",
    "afx_batch_create_from_raw_device", "afx_batch_export_samples_device", "afx_batch_export_sample_counts_device",
    "afx_batch_export_file_results_device",
]
RAW_I16, RAW_I24, RAW_F32, RAW_I32, RAW_F64 = 0, 1, 2, 3, 4
RAW_I16_BE, RAW_I24_BE, RAW_F32_BE, RAW_I32_BE, RAW_F64_BE = 5, 6, 7, 8, 9   # the same with Motorola byte order (AIFF)
RAW_FLAC = 10   # a FLAC stream, decoded on the GPU: afx_raw.data points at an afx_flac_stream (Plan.batch_from_raw takes the image)
_RAW_BYTES = {RAW_I16: 2, RAW_I24: 3, RAW_F32: 4, RAW_I32: 4, RAW_F64: 8,
              RAW_I16_BE: 2, RAW_I24_BE: 3, RAW_F32_BE: 4, RAW_I32_BE: 4, RAW_F64_BE: 8}

# the series of a record in afx_batch_record_layout's order (AFX_NUM_SERIES)
RECORD_SERIES = ["mfcc", "spectral_rms", "spectral_centroid", "spectral_spread", "spectral_skewness", "spectral_kurtosis",
                 "spectral_rolloff", "spectral_flatness", "spectral_flux", "spectrum_bands", "amplitude_peak", "amplitude_rms",
                 "sub_rms", "sub_flatness", "sub_flux", "sub_complexity", "sub_contrast", "spectral_contrast", "amplitude_silence",
                 "amplitude_envelope", "spectral_complexity", "auto_correlation", "f0", "f0_confidence", "failsafe_f0",
                 "spectral_inharmonicity", "tristimulus1", "tristimulus2", "tristimulus3"]

# afx_out fields: name -> width per frame, in declaration order
OUT_FIELDS = [
    ("mfcc", 14), ("spectral_rms", 1), ("spectral_centroid", 1), ("spectral_spread", 1),
    ("spectral_skewness", 1), ("spectral_kurtosis", 1), ("spectral_rolloff", 1),
    ("spectral_flatness", 1), ("spectral_flux", 1), ("spectrum_bands", 28), ("sub_rms", 14),
    ("sub_flatness", 14), ("sub_flux", 14), ("sub_complexity", 14), ("sub_contrast", 14),
    ("spectral_contrast", 1), ("amplitude_peak", 1), ("amplitude_rms", 1), ("magnitude", 1024),
    ("amplitude_silence", 1), ("amplitude_envelope", 1), ("spectral_complexity", 1), ("auto_correlation", 1),
    ("f0", 1), ("f0_confidence", 1), ("failsafe_f0", 1), ("spectral_inharmonicity", 1),
    ("tristimulus1", 1), ("tristimulus2", 1), ("tristimulus3", 1),
]
FIELD_MASK = {
    "mfcc": D_MFCC, "spectral_rms": D_SPECTRAL_RMS, "spectral_centroid": D_SPECTRAL_CENTROID,
    "spectral_spread": D_SPECTRAL_SPREAD, "spectral_skewness": D_SPECTRAL_SKEWNESS,
    "spectral_kurtosis": D_SPECTRAL_KURTOSIS, "spectral_rolloff": D_SPECTRAL_ROLLOFF,
    "spectral_flatness": D_SPECTRAL_FLATNESS, "spectral_flux": D_SPECTRAL_FLUX,
    "spectrum_bands": D_SPECTRUM_BANDS, "sub_rms": D_BAND_FEATURES, "sub_flatness": D_BAND_FEATURES,
    "sub_flux": D_BAND_FEATURES, "sub_complexity": D_BAND_FEATURES, "sub_contrast": D_BAND_FEATURES,
    "spectral_contrast": D_BAND_FEATURES, "amplitude_peak": D_AMPLITUDE_PEAK,
    "amplitude_rms": D_AMPLITUDE_RMS, "magnitude": D_MAGNITUDE,
    "amplitude_silence": D_AMPLITUDE_SILENCE, "amplitude_envelope": D_AMPLITUDE_ENVELOPE,
    "spectral_complexity": D_SPECTRAL_COMPLEXITY, "auto_correlation": D_AUTO_CORRELATION,
    "f0": D_F0, "f0_confidence": D_F0, "failsafe_f0": D_F0,
    "spectral_inharmonicity": D_SPECTRAL_INHARMONICITY,
    "tristimulus1": D_TRISTIMULUS, "tristimulus2": D_TRISTIMULUS, "tristimulus3": D_TRISTIMULUS,
}


class AfxError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"afx status {status}: {text}")
        self.status = status


class _PlanDesc(ctypes.Structure):
    _fields_ = [("sample_rate", ctypes.c_int32), ("fft_size", ctypes.c_int32),
                ("hop_size", ctypes.c_int32), ("device", ctypes.c_int32),
                ("precision", ctypes.c_int32), ("max_analysis_ms", ctypes.c_int32),
                ("frame_kernel", ctypes.c_int32), ("flags", ctypes.c_int32)]


class _BatchInfo(ctypes.Structure):
    _fields_ = [("frame_kernel", ctypes.c_int32), ("feature_class", ctypes.c_int32), ("pcm_kind", ctypes.c_int32),
                ("chunk_frames", ctypes.c_int32), ("n_chunks", ctypes.c_int32), ("grid_blocks", ctypes.c_int32),
                ("arena_bytes", ctypes.c_int64)]


class _Buf(ctypes.Structure):
    _fields_ = [("pcm", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("n_samples", ctypes.c_int64)]


class _Out(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n, _ in OUT_FIELDS] + [
        ("effective_length", ctypes.c_void_p), ("frame_offset", ctypes.c_void_p), ("buf_status", ctypes.c_void_p)]


class _Raw(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("format", ctypes.c_int32), ("channels", ctypes.c_int32),
                ("sample_rate", ctypes.c_int32), ("reserved", ctypes.c_int32), ("n_frames", ctypes.c_int64)]


class _FlacFrame(ctypes.Structure):   # afx_flac_frame
    _fields_ = [("byte_off", ctypes.c_int64), ("first_sample", ctypes.c_int64)]


class _FlacStream(ctypes.Structure):   # afx_flac_stream
    _fields_ = [("frames", ctypes.c_void_p), ("frames_bytes", ctypes.c_int64), ("index", ctypes.c_void_p), ("n_index", ctypes.c_int32),
                ("bits_per_sample", ctypes.c_int32), ("stream_channels", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class _FlacInfo(ctypes.Structure):   # afx_flac_info
    _fields_ = [("sample_rate", ctypes.c_int32), ("channels", ctypes.c_int32), ("bits_per_sample", ctypes.c_int32),
                ("min_blocksize", ctypes.c_int32), ("max_blocksize", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("total_samples", ctypes.c_int64), ("first_frame_off", ctypes.c_int64)]


class _LoadInfo(ctypes.Structure):
    _fields_ = [("peak_value", ctypes.c_float), ("rms_value", ctypes.c_float), ("data_offset", ctypes.c_int32),
                ("silent_leading", ctypes.c_int32), ("silent_trailing", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("n_samples", ctypes.c_int64)]


class _HighOut(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("scalars", "signature", "pitch", "peak", "status")]


class _HighTextOut(ctypes.Structure):
    _fields_ = [("scalars", ctypes.c_void_p), ("text", ctypes.c_void_p), ("text_capacity", ctypes.c_int64), ("begin", ctypes.c_void_p),
                ("length", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class _DecisionDesc(ctypes.Structure):
    _fields_ = [("class_model", ctypes.c_void_p), ("loop_class", ctypes.c_int32), ("oneshot_class", ctypes.c_int32),
                ("use_heuristics", ctypes.c_int32), ("category_model", ctypes.c_void_p), ("category_none_class", ctypes.c_int32)]


_DECISION_OUT = ("class_signature", "class_strengths", "classes", "category_signature", "category_strengths", "categories",
                 "confidences", "flags", "non_finite")


class _DecisionOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in _DECISION_OUT]


class _DecisionIn(ctypes.Structure):
    _fields_ = [("n_files", ctypes.c_int32), ("n_categories", ctypes.c_int32), ("class_signature", ctypes.c_void_p),
                ("category_signature", ctypes.c_void_p), ("peaks", ctypes.c_void_p), ("frame_offset", ctypes.c_void_p),
                ("scalars", ctypes.c_void_p), ("non_finite", ctypes.c_void_p), ("loop_class", ctypes.c_int32),
                ("oneshot_class", ctypes.c_int32), ("use_heuristics", ctypes.c_int32), ("category_none_class", ctypes.c_int32)]


class _Name(ctypes.Structure):
    _fields_ = [("text", ctypes.c_char_p), ("length", ctypes.c_int32)]


class _RowDesc(ctypes.Structure):
    _fields_ = [("decision", _DecisionDesc), ("class_names", ctypes.POINTER(_Name)), ("n_class_names", ctypes.c_int32),
                ("n_category_names", ctypes.c_int32), ("category_names", ctypes.POINTER(_Name))]


class _RowOut(ctypes.Structure):
    _fields_ = [("scalars", ctypes.c_void_p), ("text", ctypes.c_void_p), ("text_capacity", ctypes.c_int64), ("begin", ctypes.c_void_p),
                ("length", ctypes.c_void_p), ("flags", ctypes.c_void_p), ("non_finite", ctypes.c_void_p), ("confidences", ctypes.c_void_p),
                ("status", ctypes.c_void_p)]


class _ClassJsonIn(ctypes.Structure):
    _fields_ = [("n_files", ctypes.c_int32), ("n_categories", ctypes.c_int32), ("class_signature", ctypes.c_void_p),
                ("class_strengths", ctypes.c_void_p), ("classes", ctypes.c_void_p), ("category_signature", ctypes.c_void_p),
                ("category_strengths", ctypes.c_void_p), ("categories", ctypes.c_void_p), ("class_names", ctypes.POINTER(_Name)),
                ("category_names", ctypes.POINTER(_Name))]


class _StatsOut(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n, _ in OUT_FIELDS if n != "magnitude"] + [("stats_status", ctypes.c_void_p)]


def build_info():
    """afx_build_info() of the loaded library: "afx abi=N arch=gfx950 stamps=0 ablation=0 src=<hash of its sources>"."""
    return load_library().afx_build_info().decode()


def library_path():
    return _LIB_PATH


def device_count():
    """afx_device_count(): HIP devices this process can use (0 without a GPU)."""
    L = load_library()
    L.afx_device_count.restype = ctypes.c_int
    return int(L.afx_device_count())


def build_library(force=False):
    """Compile libafx_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    args = ["make", "-C", src_dir]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return _LIB_PATH


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH) and "AFX_LIBRARY" not in os.environ:
        try:
            build_library()      # hipcc is part of the image, on the GPU box as well
        except Exception as e:   # noqa: BLE001
            raise ImportError(f"{_LIB_PATH} is missing and could not be built ({e}); the HIP extension is "
                              "the only compute path, there is no fallback") from e
    if not os.path.exists(_LIB_PATH):
        raise ImportError(f"{_LIB_PATH} is missing (the HIP extension is the only compute path; there is no fallback)")
    L = ctypes.CDLL(_LIB_PATH)
    vp, i32, i64, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32
    L.afx_status_str.restype = ctypes.c_char_p
    L.afx_status_str.argtypes = [ctypes.c_int]
    L.afx_last_error.restype = ctypes.c_char_p
    L.afx_build_info.restype = ctypes.c_char_p
    L.afx_plan_create.argtypes = [ctypes.POINTER(_PlanDesc), ctypes.POINTER(vp)]
    L.afx_plan_destroy.argtypes = [vp]
    L.afx_plan_destroy.restype = None
    L.afx_plan_get_window.argtypes = [vp, vp]
    L.afx_plan_get_mel_table.argtypes = [vp, vp]
    L.afx_plan_get_bin_range.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.afx_num_frames.restype = i64
    L.afx_num_frames.argtypes = [vp, i64]
    L.afx_extract_batch.argtypes = [vp, ctypes.POINTER(_Buf), i32, u32, ctypes.POINTER(_Out)]
    L.afx_batch_create.argtypes = [vp, ctypes.POINTER(_Buf), i32, u32, ctypes.POINTER(vp)]
    L.afx_batch_total_frames.restype = i64
    L.afx_batch_total_frames.argtypes = [vp]
    L.afx_batch_run.argtypes = [vp]
    L.afx_batch_sync.argtypes = [vp]
    L.afx_batch_run_timed.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_float)]
    L.afx_batch_fetch.argtypes = [vp, ctypes.POINTER(_Out)]
    L.afx_batch_fetch_statistics.argtypes = [vp, ctypes.POINTER(_StatsOut)]
    L.afx_batch_destroy.argtypes = [vp]
    L.afx_batch_destroy.restype = None
    L.afx_batch_create_from_raw.argtypes = [vp, ctypes.POINTER(_Raw), i32, u32, ctypes.POINTER(vp), ctypes.POINTER(_LoadInfo)]
    L.afx_batch_fetch_samples.argtypes = [vp, i32, vp, i64]
    L.afx_flac_probe.argtypes = [vp, i64, ctypes.POINTER(_FlacInfo)]
    L.afx_flac_build_index.argtypes = [vp, i64, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i64)]
    L.afx_host_alloc.restype = vp
    L.afx_host_alloc.argtypes = [i64]
    L.afx_host_free.argtypes = [vp]
    L.afx_host_free.restype = None
    L.afx_batch_record_layout.argtypes = [vp, ctypes.POINTER(i32), vp, vp]
    L.afx_batch_fetch_records.argtypes = [vp, vp, vp, vp, vp, vp]
    L.afx_batch_store_records.argtypes = [vp, vp, vp, vp]
    L.afx_batch_set_file_info.argtypes = [vp, vp]
    L.afx_batch_rhythm_frames.restype = i64
    L.afx_batch_rhythm_frames.argtypes = [vp, vp]
    L.afx_batch_fetch_rhythm.argtypes = [vp, vp, vp, vp]
    L.afx_batch_get_info.argtypes = [vp, ctypes.POINTER(_BatchInfo)]
    L.afx_batch_fetch_onset_functions.argtypes = [vp, vp]
    L.afx_algorithmic_bytes_per_frame.restype = i64
    L.afx_algorithmic_bytes_per_frame.argtypes = [vp, u32, i32]
    L.afx_batch_fetch_high_level.argtypes = [vp, ctypes.POINTER(_LoadInfo), ctypes.POINTER(_HighOut)]
    L.afx_batch_fetch_classification_features.argtypes = [vp, vp, vp, vp]
    L.afx_classification_feature_name.argtypes = [i32, ctypes.c_char_p, i32]
    L.afx_plan_get_silence_features.argtypes = [vp, vp]
    L.afx_model_create_from_lightgbm.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), i32, vp, vp, vp,
                                                 i32, ctypes.c_double, ctypes.POINTER(vp)]
    L.afx_model_destroy.argtypes = [vp]
    L.afx_model_destroy.restype = None
    L.afx_model_get_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), vp]
    L.afx_batch_fetch_class_signature.argtypes = [vp, vp, vp, vp, vp]
    L.afx_model_evaluate_features.argtypes = [vp, vp, i32, vp, vp, vp]
    L.afx_batch_fetch_class_decision.argtypes = [vp, ctypes.POINTER(_DecisionDesc), ctypes.POINTER(_DecisionOut)]
    L.afx_decide.argtypes = [vp, ctypes.POINTER(_DecisionIn), ctypes.POINTER(_DecisionOut)]
    L.afx_batch_high_level_text_capacity.restype = i64
    L.afx_batch_high_level_text_capacity.argtypes = [vp]
    L.afx_batch_fetch_high_level_text.argtypes = [vp, ctypes.POINTER(_LoadInfo), ctypes.POINTER(_HighTextOut)]
    L.afx_format_json_g9.argtypes = [vp, vp, i64, vp, vp, i32, vp, i64, vp, vp]
    L.afx_batch_high_level_row_capacity.restype = i64
    L.afx_batch_high_level_row_capacity.argtypes = [vp, ctypes.POINTER(_RowDesc)]
    L.afx_batch_fetch_high_level_row.argtypes = [vp, ctypes.POINTER(_LoadInfo), ctypes.POINTER(_RowDesc), ctypes.POINTER(_RowOut)]
    L.afx_format_class_json.argtypes = [vp, ctypes.POINTER(_ClassJsonIn), vp, i64, vp, vp]
    _lib = L
    return L


def classification_feature_names():
    """the 1 680 names of afx_batch_fetch_classification_features' columns (afx_classification_feature_name; no device)"""
    L = load_library()
    buf = ctypes.create_string_buffer(64)
    names = []
    for i in range(NUM_CLASSIFICATION_FEATURES):
        n = L.afx_classification_feature_name(i, buf, len(buf))
        if n < 0:
            _check(L, n)
        names.append(buf.value.decode())
    return names


def _decision_out(n, with_classes, k):
    """the arrays of an afx_decision_out for n files (one spare row for n = 0) -> (struct, dict of [n]-row views)"""
    rows = max(1, n)
    arrays = {"confidences": np.zeros((rows, 2)), "flags": np.zeros(rows, dtype=np.int32), "non_finite": np.zeros(rows, dtype=np.int32)}
    if with_classes:
        arrays.update(class_signature=np.zeros((rows, 2), dtype=np.float32), class_strengths=np.zeros((rows, 2)),
                      classes=np.full((rows, 2), -1, dtype=np.int32))
    if k:
        arrays.update(category_signature=np.zeros((rows, k), dtype=np.float32), category_strengths=np.zeros((rows, k)),
                      categories=np.full((rows, k), -1, dtype=np.int32))
    out = _DecisionOut()
    for name, a in arrays.items():
        setattr(out, name, a.ctypes.data)
    return out, {name: arrays[name][:n] for name in _DECISION_OUT if name in arrays}


def decide(plan, peaks, frame_offset, scalars, class_signature=None, category_signature=None, non_finite=None, loop_class=0,
           oneshot_class=1, use_heuristics=True, category_none_class=-1):
    """afx_decide: the class decision's kernel (SampleAnalyser.cpp:1097-1231) on inputs of the caller's, no batch: peaks
    [frame_offset[-1]] (every file's amplitude_peak frames), frame_offset [n + 1], scalars [n][5] (DECISION_SCALARS order),
    class_signature [n][2] and / or category_signature [n][K] -> dict as Batch.fetch_class_decision's"""
    frame_offset = np.ascontiguousarray(frame_offset, dtype=np.int64).reshape(-1)
    n = frame_offset.size - 1
    peaks = np.ascontiguousarray(peaks, dtype=np.float64).reshape(-1)
    scalars = np.ascontiguousarray(scalars, dtype=np.float64).reshape(-1, len(DECISION_SCALARS))
    if n < 0 or scalars.shape[0] != n or (n and peaks.size != frame_offset[-1]):
        raise ValueError("frame_offset holds n + 1 offsets into peaks, scalars one row per file")
    d = _DecisionIn(n_files=n, peaks=peaks.ctypes.data, frame_offset=frame_offset.ctypes.data, scalars=scalars.ctypes.data,
                    loop_class=loop_class, oneshot_class=oneshot_class, use_heuristics=int(bool(use_heuristics)),
                    category_none_class=category_none_class)
    k = 0
    if class_signature is not None:
        class_signature = np.ascontiguousarray(class_signature, dtype=np.float32).reshape(n, 2)
        d.class_signature = class_signature.ctypes.data
    if category_signature is not None:
        category_signature = np.ascontiguousarray(category_signature, dtype=np.float32)
        if category_signature.ndim != 2 or category_signature.shape[0] != n:
            raise ValueError("category_signature holds one row of K weights per file")
        k = d.n_categories = category_signature.shape[1]
        d.category_signature = category_signature.ctypes.data
    if non_finite is not None:
        non_finite = np.ascontiguousarray(non_finite, dtype=np.int32).reshape(n)
        d.non_finite = non_finite.ctypes.data
    out, res = _decision_out(n, class_signature is not None, k)
    _check(plan.L, plan.L.afx_decide(plan.h, ctypes.byref(d), ctypes.byref(out)))
    return res


def json_g9_capacity(count, inner=0):
    """the bytes afx_format_json_g9 wants for a column of `count` values: 2 + 17 values + 2 rows"""
    return 2 + 17 * count + (2 * (count // inner) if inner else 0)


def format_json_g9(plan, columns):
    """afx_format_json_g9: the text kernel of Batch.fetch_high_level_text on doubles of the caller's, no batch.  columns: a
    list of 1-D arrays (written as "[a,b,c]") and 2-D arrays ([rows][W], written as "[[a,b],[c,d]]") -> list of bytes, every
    number as snprintf("%.9g") writes it (NaN, INF, -INF for the values that are no numbers)"""
    arrays = [np.ascontiguousarray(c, dtype=np.float64) for c in columns]
    if any(a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] == 0) for a in arrays):
        raise ValueError("a column is a 1-D array or a 2-D array of rows that are not empty")
    inner = np.array([a.shape[1] if a.ndim == 2 else 0 for a in arrays] + [0], dtype=np.int32)
    offset = np.concatenate([[0], np.cumsum([a.size for a in arrays])]).astype(np.int64)
    return format_json_g9_raw(plan, np.concatenate([a.reshape(-1) for a in arrays] + [np.zeros(0)]), offset, inner[:len(arrays)])["texts"]


def format_json_g9_raw(plan, values, column_offset, inner, text_capacity=None):
    """afx_format_json_g9 with the arrays as the C call takes them (the checks are the library's) -> dict: "texts" (list of
    bytes), "begin" int64 [n], "length" int32 [n], "capacity" (the bytes of text asked for)"""
    values = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    column_offset = np.ascontiguousarray(column_offset, dtype=np.int64).reshape(-1)
    inner = np.ascontiguousarray(inner, dtype=np.int32).reshape(-1)
    n = inner.size
    if column_offset.size != n + 1:
        raise ValueError("column_offset holds one offset more than there are columns")
    if text_capacity is None:
        text_capacity = sum(json_g9_capacity(max(0, int(column_offset[c + 1] - column_offset[c])), max(0, int(inner[c]))) for c in range(n))
    text = np.zeros(max(1, text_capacity), dtype=np.uint8)
    begin, length = np.zeros(max(1, n), dtype=np.int64), np.zeros(max(1, n), dtype=np.int32)
    _check(plan.L, plan.L.afx_format_json_g9(plan.h, values.ctypes.data, values.size, column_offset.ctypes.data, inner.ctypes.data, n,
                                             text.ctypes.data, text_capacity, begin.ctypes.data, length.ctypes.data))
    return {"texts": [text[begin[c]:begin[c] + length[c]].tobytes() for c in range(n)], "begin": begin[:n], "length": length[:n],
            "capacity": text_capacity}


def _names(names):
    """a list of str / bytes -> (ctypes array of afx_name or None, what keeps its bytes alive)"""
    if not names:
        return None, []
    raw = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in names]
    arr = (_Name * len(raw))()
    for i, r in enumerate(raw):
        arr[i].text, arr[i].length = r, len(r)
    return arr, raw


def names_slot_bytes(names):
    """the bytes of a column of names that holds every one of them once: 2 + the sum of length + 3"""
    return 2 + sum(len(s.encode("utf-8") if isinstance(s, str) else s) + 3 for s in names or [])


def class_json_file_bytes(class_names, category_names):
    """the bytes of one file's six class slots in afx_format_class_json's text: they lie one behind the other, file after file"""
    return (2 * json_g9_capacity(len(class_names or [])) + names_slot_bytes(class_names)
            + 2 * json_g9_capacity(len(category_names or [])) + names_slot_bytes(category_names))


def format_class_json(plan, class_signature=None, class_strengths=None, classes=None, class_names=None, category_signature=None,
                      category_strengths=None, categories=None, category_names=None, n_files=None, text=None):
    """afx_format_class_json: the class columns' text kernel of Batch.fetch_high_level_row on arrays of the caller's, no batch.
    The class arrays are [n][2] (float32 signature, float64 strengths, int32 picks, -1 padded), the category arrays [n][K];
    either triple may be left out (its columns are "[]").  -> dict: "texts" [n][6] bytes (HLR_COLUMNS[:6] order), "text",
    "begin" int64 [n][6], "length" int32 [n][6], "capacity".  text: a uint8 array to fill in place of a new one."""
    d = _ClassJsonIn()
    keep = []
    n = n_files

    def take(a, dtype, width):
        nonlocal n
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.ndim != 2 or (width is not None and a.shape[1] != width) or (n is not None and a.shape[0] != n):
            raise ValueError("the arrays hold one row per file, 2 wide for the classes and K for the categories")
        n = a.shape[0]
        keep.append(a)
        return a.ctypes.data

    d.class_signature, d.class_strengths, d.classes = take(class_signature, np.float32, 2), take(class_strengths, np.float64, 2), take(classes, np.int32, 2)
    k = None
    for name, a, dtype in (("category_signature", category_signature, np.float32), ("category_strengths", category_strengths, np.float64),
                           ("categories", categories, np.int32)):
        setattr(d, name, take(a, dtype, k))
        if a is not None:
            k = keep[-1].shape[1]
    d.n_files, d.n_categories = n or 0, k or 0
    d.class_names, raw0 = _names(class_names)
    d.category_names, raw1 = _names(category_names)
    capacity = (n or 0) * class_json_file_bytes(class_names if d.classes else None, category_names if d.categories else None)
    if text is None:
        text = np.zeros(max(1, capacity), dtype=np.uint8)
    rows = max(1, n or 0)
    begin, length = np.zeros((rows, 6), dtype=np.int64), np.zeros((rows, 6), dtype=np.int32)
    _check(plan.L, plan.L.afx_format_class_json(plan.h, ctypes.byref(d), text.ctypes.data, text.size, begin.ctypes.data, length.ctypes.data))
    n = n or 0
    return {"texts": [[text[begin[i, c]:begin[i, c] + length[i, c]].tobytes() for c in range(6)] for i in range(n)], "text": text,
            "begin": begin[:n], "length": length[:n], "capacity": capacity}


def pinned_array(shape, dtype):
    """numpy array in page-locked host memory (afx_host_alloc); keep the returned owner alive."""
    L = load_library()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = L.afx_host_alloc(max(n, 1))
    if not p:
        raise MemoryError("afx_host_alloc failed")

    class _Owner:
        def __del__(self, p=p, L=L):
            L.afx_host_free(p)

    buf = (ctypes.c_char * max(n, 1)).from_address(p)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    return arr, _Owner()


def _check(L, st):
    if st != 0:
        raise AfxError(st, (L.afx_status_str(st) or b"").decode() + ": " + (L.afx_last_error() or b"").decode())


def _pack_bufs(bufs):
    """list of 1-D float32/float64 arrays -> (ctypes array of afx_buf, keep-alive list)."""
    keep = []
    arr = (_Buf * max(1, len(bufs)))()
    for i, b in enumerate(bufs):
        b = np.asarray(b)
        if b.dtype == np.float32:
            dt = PCM_F32
        elif b.dtype == np.float64:
            dt = PCM_F64
        else:
            raise TypeError("PCM buffers must be float32 or float64")
        b = np.ascontiguousarray(b.reshape(-1))
        keep.append(b)
        arr[i].pcm = b.ctypes.data if b.size else None
        arr[i].dtype = dt
        arr[i].n_samples = b.size
    return arr, keep


def _alloc_out(mask, total_frames, n_bufs):
    out = _Out()
    res = {}
    for name, width in OUT_FIELDS:
        if mask & FIELD_MASK[name]:
            a = np.zeros((total_frames, width) if width > 1 else (total_frames,), dtype=np.float64)
            res[name] = a
            setattr(out, name, a.ctypes.data if a.size else None)
    if mask & D_EFFECTIVE_LENGTH:
        el = np.zeros((max(1, n_bufs), 3), dtype=np.float64)
        out.effective_length = el.ctypes.data
        res["effective_length"] = el[:n_bufs]
    fo = np.zeros(n_bufs + 1, dtype=np.int64)
    bs = np.zeros(max(1, n_bufs), dtype=np.int32)
    out.frame_offset = fo.ctypes.data
    out.buf_status = bs.ctypes.data
    res["frame_offset"] = fo
    res["buf_status"] = bs[:n_bufs]
    return out, res


class Plan:
    """afx_plan: the analogue of constructing TSampleAnalyser(44100, 2048, 1024)."""

    def __init__(self, sample_rate=44100, fft_size=2048, hop_size=1024, device=0,
                 precision=PRECISION_F64, max_analysis_ms=20000, frame_kernel=FRAME_KERNEL_AUTO, flags=0):
        self.L = load_library()
        d = _PlanDesc(sample_rate, fft_size, hop_size, device, precision, max_analysis_ms, frame_kernel, flags)
        h = ctypes.c_void_p()
        _check(self.L, self.L.afx_plan_create(ctypes.byref(d), ctypes.byref(h)))
        self.h = h
        self.fft_size, self.hop_size, self.precision = fft_size, hop_size, precision

    def close(self):
        if getattr(self, "h", None):
            self.L.afx_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def window(self):
        a = np.zeros(self.fft_size)
        _check(self.L, self.L.afx_plan_get_window(self.h, a.ctypes.data))
        return a

    def mel_table(self):
        a = np.zeros((14, self.fft_size // 2))
        _check(self.L, self.L.afx_plan_get_mel_table(self.h, a.ctypes.data))
        return a

    def bin_range(self):
        f, c = ctypes.c_int32(), ctypes.c_int32()
        _check(self.L, self.L.afx_plan_get_bin_range(self.h, ctypes.byref(f), ctypes.byref(c)))
        return f.value, c.value

    def silence_features(self):
        """afx_plan_get_silence_features: [21] what a time position without a frame is filled with (frequency_bands 0..13,
        spectral_rms, _flatness, _flux, _contrast, _complexity, f0_confidence, amplitude_rms of one frame of zeros)"""
        a = np.zeros(NUM_CF_SILENCE)
        _check(self.L, self.L.afx_plan_get_silence_features(self.h, a.ctypes.data))
        return a

    def num_frames(self, n_samples):
        return int(self.L.afx_num_frames(self.h, int(n_samples)))

    def bytes_per_frame(self, mask, pcm_dtype=PCM_F32):
        return int(self.L.afx_algorithmic_bytes_per_frame(self.h, mask, pcm_dtype))

    def extract(self, bufs, mask=D_ALL_LOW_LEVEL):
        """One-shot afx_extract_batch on host buffers; returns dict of numpy arrays."""
        arr, keep = _pack_bufs(bufs)
        total = sum(self.num_frames(b.size) for b in keep)
        out, res = _alloc_out(mask, total, len(keep))
        _check(self.L, self.L.afx_extract_batch(self.h, arr, len(keep), mask, ctypes.byref(out)))
        del keep
        return res

    def batch(self, bufs, mask=D_ALL_LOW_LEVEL):
        return Batch(self, bufs, mask)

    def batch_from_raw(self, raws, mask=D_ALL_LOW_LEVEL):
        """raws: list of (array, channels[, sample_rate]), or (FLAC image, None, None, RAW_FLAC);
        array dtype int16 / int32 / float32 / float64 (interleaved,
        shape [frames*channels] or [frames, channels]) or uint8 of packed 24-bit little-endian samples; files at another
        sample_rate than the plan's are converted on the GPU (SampleAnalyser.cpp:563-607).
        Returns (Batch, list of load-info dicts): the LoadSample front end on the GPU."""
        n = len(raws)
        arr = (_Raw * max(1, n))()
        keep = []
        for i, item in enumerate(raws):
            if len(item) > 3 and item[3] is not None and int(item[3]) == RAW_FLAC:
                # (FLAC image, channels or None, sample_rate or None, RAW_FLAC): indexed here on the host, decoded on the GPU;
                # an image the indexer refuses goes on as a buffer the library refuses (status in buf_status)
                # (or a ready _FlacStream, channels, sample_rate, RAW_FLAC, n_frames: the caller's own descriptor and memory)
                if isinstance(item[0], _FlacStream):
                    stream, holds, channels, rate, frames = item[0], item[0], int(item[1]), int(item[2]), int(item[4])
                else:
                    stream, holds, channels, rate, frames = flac_stream(item[0], self.L)
                keep.append(holds)
                arr[i].data = ctypes.addressof(stream) if stream is not None else None
                arr[i].format, arr[i].channels, arr[i].sample_rate, arr[i].n_frames = RAW_FLAC, channels, rate, frames
                continue
            data, channels = item[0], int(item[1])
            rate = int(item[2]) if len(item) > 2 else 0
            data = np.ascontiguousarray(np.asarray(data).reshape(-1))
            if len(item) > 3 and item[3] is not None:
                # (array, channels, sample_rate, RAW_* code): the array's bytes as they are, in the stated format --
                # how the big-endian formats are handed over (a NumPy dtype does not say "AIFF payload")
                fmt = int(item[3])
                data = data.view(np.uint8)
                frames = data.size // (_RAW_BYTES.get(fmt, 1) * max(channels, 1))
            elif data.dtype == np.int16:
                fmt, frames = RAW_I16, data.size // max(channels, 1)
            elif data.dtype == np.float32:
                fmt, frames = RAW_F32, data.size // max(channels, 1)
            elif data.dtype == np.uint8:
                fmt, frames = RAW_I24, data.size // (3 * max(channels, 1))
            elif data.dtype == np.int32:
                fmt, frames = RAW_I32, data.size // max(channels, 1)
            elif data.dtype == np.float64:
                fmt, frames = RAW_F64, data.size // max(channels, 1)
            else:
                raise TypeError("raw PCM must be int16, int32, float32, float64 or uint8 (packed int24)")
            keep.append(data)
            arr[i].data = data.ctypes.data if data.size else None
            arr[i].format, arr[i].channels, arr[i].sample_rate, arr[i].n_frames = fmt, channels, rate, frames
        info = (_LoadInfo * max(1, n))()
        h = ctypes.c_void_p()
        _check(self.L, self.L.afx_batch_create_from_raw(self.h, arr, n, mask, ctypes.byref(h), info))
        b = Batch.__new__(Batch)
        b.plan, b.L, b.mask, b.n_bufs, b.h = self, self.L, mask, n, h
        b.total_frames = int(self.L.afx_batch_total_frames(h))
        infos = [{k: getattr(info[i], k) for k, _ in _LoadInfo._fields_ if k != "reserved"} for i in range(n)]
        return b, infos


def flac_probe(image, L=None):
    """afx_flac_probe on a FLAC image (bytes or uint8 array) -> (status, dict of STREAMINFO's facts and first_frame_off)"""
    L = L or load_library()
    image = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray)) else image).view(np.uint8)
    info = _FlacInfo()
    st = L.afx_flac_probe(image.ctypes.data if image.size else None, image.size, ctypes.byref(info))
    return st, {k: int(getattr(info, k)) for k, _ in _FlacInfo._fields_ if k != "reserved"}


def flac_build_index(image, L=None):
    """afx_flac_build_index -> (status, int64 [frames + 1, 2] of (byte offset from the first frame, first sample), total samples)"""
    L = L or load_library()
    image = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray)) else image).view(np.uint8)
    n, total = ctypes.c_int32(), ctypes.c_int64()
    src = image.ctypes.data if image.size else None
    st = L.afx_flac_build_index(src, image.size, None, 0, ctypes.byref(n), ctypes.byref(total))
    if st != -4:                                          # AFX_ERR_OUT_OF_MEMORY: the count, now with room
        return st, np.zeros((0, 2), dtype=np.int64), 0
    index = np.zeros((n.value + 1, 2), dtype=np.int64)
    st = L.afx_flac_build_index(src, image.size, index.ctypes.data, n.value + 1, ctypes.byref(n), ctypes.byref(total))
    return st, index, total.value


def flac_stream(image, L=None, index=None):
    """the afx_flac_stream of an image for afx_raw.data -> (_FlacStream or None, what must stay alive, afx_raw.channels,
    sample_rate, n_frames).  `index`: the caller's own instead of the indexer's."""
    st, info = flac_probe(image, L)
    if st == 0 and index is None:
        st, index, total = flac_build_index(image, L)
    if st != 0:
        return None, None, 1, 0, 0
    image = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray)) else image).view(np.uint8)
    index = np.ascontiguousarray(index, dtype=np.int64)
    frames = image[info["first_frame_off"]:info["first_frame_off"] + int(index[-1, 0])]
    s = _FlacStream(frames.ctypes.data, frames.size, index.ctypes.data, len(index) - 1, info["bits_per_sample"], info["channels"], 0)
    return s, (s, image, frames, index), min(info["channels"], 2), info["sample_rate"], int(index[-1, 1])


class Model:
    """afx_model: a bagging of LightGBM models on the plan's device, with the normalisation and the outlier limits of the
    reference's model file (afx_model_create_from_lightgbm).  texts: the models' LightGBM v3 texts (str or bytes); scale,
    offset, limits: [1680] each; the early stop's defaults are LightGBM's, which the reference evaluates with."""

    def __init__(self, plan, texts, scale, offset, limits, early_stop_freq=10, early_stop_margin=10.0):
        self.L = plan.L
        raw = [t.encode() if isinstance(t, str) else bytes(t) for t in texts]
        n = len(raw)
        ptrs = (ctypes.c_char_p * max(1, n))(*raw)
        lens = (ctypes.c_size_t * max(1, n))(*[len(t) for t in raw])
        vectors = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (scale, offset, limits)]
        if any(v.size != NUM_CLASSIFICATION_FEATURES for v in vectors):
            raise ValueError("scale, offset and limits hold NUM_CLASSIFICATION_FEATURES values each")
        h = ctypes.c_void_p()
        _check(self.L, self.L.afx_model_create_from_lightgbm(plan.h, ptrs, lens, n, vectors[0].ctypes.data, vectors[1].ctypes.data,
                                                             vectors[2].ctypes.data, int(early_stop_freq), float(early_stop_margin),
                                                             ctypes.byref(h)))
        self.h = h
        k, m = ctypes.c_int32(), ctypes.c_int32()
        _check(self.L, self.L.afx_model_get_info(h, ctypes.byref(k), ctypes.byref(m), None))
        self.n_classes, self.n_models = k.value, m.value
        trees = np.zeros(self.n_models, dtype=np.int32)
        _check(self.L, self.L.afx_model_get_info(h, None, None, trees.ctypes.data))
        self.trees_per_model = trees.tolist()

    def evaluate_features(self, features):
        """afx_model_evaluate_features: the models on feature vectors of the caller's, [n][1680] ->
        (signature float32 [n][n_classes], iterations_used [n][n_models], non_finite [n])"""
        features = np.ascontiguousarray(features, dtype=np.float64).reshape(-1, NUM_CLASSIFICATION_FEATURES)
        n = features.shape[0]
        signature = np.zeros((max(1, n), self.n_classes), dtype=np.float32)
        used = np.zeros((max(1, n), self.n_models), dtype=np.int32)
        non_finite = np.zeros(max(1, n), dtype=np.int32)
        _check(self.L, self.L.afx_model_evaluate_features(self.h, features.ctypes.data, n, signature.ctypes.data, used.ctypes.data,
                                                          non_finite.ctypes.data))
        return signature[:n], used[:n], non_finite[:n]

    def close(self):
        if getattr(self, "h", None):
            self.L.afx_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """afx_batch: PCM resident in HBM, re-runnable."""

    def __init__(self, plan, bufs, mask):
        self.plan, self.L, self.mask = plan, plan.L, mask
        arr, keep = _pack_bufs(bufs)
        self.n_bufs = len(keep)
        h = ctypes.c_void_p()
        _check(self.L, self.L.afx_batch_create(plan.h, arr, self.n_bufs, mask, ctypes.byref(h)))
        self.h = h
        self.total_frames = int(self.L.afx_batch_total_frames(h))

    def run(self):
        _check(self.L, self.L.afx_batch_run(self.h))

    def info(self):
        """afx_batch_get_info: which STFT kernel the batch launches, its chunking, the PCM kept in HBM."""
        i = _BatchInfo()
        _check(self.L, self.L.afx_batch_get_info(self.h, ctypes.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in _BatchInfo._fields_}

    def sync(self):
        _check(self.L, self.L.afx_batch_sync(self.h))

    def run_timed(self, steps):
        """steps launches bracketed by HIP events on the batch stream -> elapsed ms."""
        ms = ctypes.c_float()
        _check(self.L, self.L.afx_batch_run_timed(self.h, steps, ctypes.byref(ms)))
        return ms.value

    def fetch(self):
        out, res = _alloc_out(self.mask, self.total_frames, self.n_bufs)
        _check(self.L, self.L.afx_batch_fetch(self.h, ctypes.byref(out)))
        return res

    def fetch_samples(self, buf, n):
        a = np.zeros(n, dtype=np.float64)
        _check(self.L, self.L.afx_batch_fetch_samples(self.h, buf, a.ctypes.data, n))
        return a

    def fetch_statistics(self):
        """dict name -> [n_bufs, W, 13] (W squeezed for scalar series) + "stats_status"."""
        out = _StatsOut()
        res = {}
        for name, width in OUT_FIELDS:
            if name == "magnitude" or not (self.mask & FIELD_MASK[name]):
                continue
            a = np.zeros((self.n_bufs, width, NUM_STATISTICS) if width > 1 else (self.n_bufs, NUM_STATISTICS))
            res[name] = a
            setattr(out, name, a.ctypes.data if a.size else None)
        st = np.zeros(max(1, self.n_bufs), dtype=np.int32)
        out.stats_status = st.ctypes.data
        _check(self.L, self.L.afx_batch_fetch_statistics(self.h, ctypes.byref(out)))
        res["stats_status"] = st[:self.n_bufs]
        return res

    def record_layout(self):
        """afx_batch_record_layout -> dict: "stride" (doubles per record), "offsets" {series: first column, -1 when the
        series is not in the mask} and "widths" {series: columns}, RECORD_SERIES order"""
        stride = ctypes.c_int32()
        offsets, widths = np.zeros(len(RECORD_SERIES), dtype=np.int32), np.zeros(len(RECORD_SERIES), dtype=np.int32)
        _check(self.L, self.L.afx_batch_record_layout(self.h, ctypes.byref(stride), offsets.ctypes.data, widths.ctypes.data))
        return {"stride": stride.value, "offsets": dict(zip(RECORD_SERIES, offsets.tolist())),
                "widths": dict(zip(RECORD_SERIES, widths.tolist()))}

    def fetch_records(self, statistics=None):
        """afx_batch_fetch_records: the raw records as the kernels leave them -> dict: "records" [F][stride],
        "frame_offset" [n_bufs + 1], "buf_status" [n_bufs], with AFX_D_STATISTICS in the mask (statistics=False leaves them
        out) "statistics" [n_bufs][stride][13], with AFX_D_EFFECTIVE_LENGTH "effective_length" [n_bufs][3]"""
        n, stride = self.n_bufs, self.record_layout()["stride"]
        if statistics is None:
            statistics = bool(self.mask & D_STATISTICS)
        res = {"records": np.zeros((self.total_frames, stride)), "frame_offset": np.zeros(n + 1, dtype=np.int64),
               "buf_status": np.zeros(max(1, n), dtype=np.int32)}
        if statistics:
            res["statistics"] = np.zeros((n, stride, NUM_STATISTICS))
        if self.mask & D_EFFECTIVE_LENGTH:
            res["effective_length"] = np.zeros((max(1, n), 3))

        def ptr(k):
            return res[k].ctypes.data if k in res and res[k].size else None
        _check(self.L, self.L.afx_batch_fetch_records(self.h, ptr("records"), ptr("statistics"), ptr("frame_offset"), ptr("buf_status"),
                                                      ptr("effective_length")))
        res["buf_status"] = res["buf_status"][:n]
        if "effective_length" in res:
            res["effective_length"] = res["effective_length"][:n]
        return res

    def store_records(self, records=None, statistics=None, rhythm_scalars=None):
        """afx_batch_store_records: overwrite what the last run left in device memory -- records [F][stride], statistics
        [n_bufs][stride][13], rhythm_scalars [n_bufs][14] (RHYTHM_SCALARS order), float64 and C-contiguous, each optional --
        so that every later fetch of the batch reads these values; the next run() overwrites them."""
        stride = self.record_layout()["stride"]
        shapes = {"records": (self.total_frames, stride), "statistics": (self.n_bufs, stride, NUM_STATISTICS),
                  "rhythm_scalars": (self.n_bufs, len(RHYTHM_SCALARS))}
        given = {"records": records, "statistics": statistics, "rhythm_scalars": rhythm_scalars}
        ptrs = []
        for name, a in given.items():
            if a is None:
                ptrs.append(None)
                continue
            if not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.shape != shapes[name] or not a.flags["C_CONTIGUOUS"]:
                raise ValueError(f"{name} must be a C-contiguous float64 array of shape {shapes[name]}")
            ptrs.append(a.ctypes.data if a.size else None)
        _check(self.L, self.L.afx_batch_store_records(self.h, *ptrs))

    def set_file_info(self, info):
        """info: per buffer (original_sample_rate, data_offset, original_samples) -- what TSampleData carries besides
        the samples; the rhythm tracker's duration heuristics use it (SampleAnalyser.cpp:1001-1004)."""
        a = np.zeros(max(1, self.n_bufs), dtype=[("rate", np.int32), ("offset", np.int32), ("samples", np.int64)])
        for i, (rate, offset, samples) in enumerate(info):
            a[i] = (rate, offset, samples)
        _check(self.L, self.L.afx_batch_set_file_info(self.h, a.ctypes.data))

    def rhythm_frames(self):
        off = np.zeros(self.n_bufs + 1, dtype=np.int64)
        self.L.afx_batch_rhythm_frames(self.h, off.ctypes.data)
        return off

    def fetch_rhythm(self, statistics=False, onset_functions=False):
        """dict: "offsets" [n_bufs+1], "onsets" [T][2] (complex, percussive), "scalars" [n_bufs][14] (RHYTHM_SCALARS
        order), optionally "onset_statistics" [n_bufs][2][13] and "onset_functions" float32 [T][2]."""
        off = self.rhythm_frames()
        rows = int(off[-1])
        res = {"offsets": off, "onsets": np.zeros((rows, 2)), "scalars": np.zeros((self.n_bufs, len(RHYTHM_SCALARS)))}
        st = np.zeros((self.n_bufs, 2, NUM_STATISTICS)) if statistics else None
        _check(self.L, self.L.afx_batch_fetch_rhythm(self.h, res["onsets"].ctypes.data if rows else None,
                                                     res["scalars"].ctypes.data if self.n_bufs else None,
                                                     st.ctypes.data if statistics and self.n_bufs else None))
        if statistics:
            res["onset_statistics"] = st
        if onset_functions:
            odf = np.zeros((max(rows, 1), 2), dtype=np.float32)
            _check(self.L, self.L.afx_batch_fetch_onset_functions(self.h, odf.ctypes.data))
            res["onset_functions"] = odf[:rows]
        return res

    def fetch_high_level(self, levels=None, want=("scalars", "signature", "pitch", "peak", "status")):
        """afx_batch_fetch_high_level: the model-free high-level descriptors of every buffer (SampleAnalyser.cpp:1234-1606).
        levels: the load-info dicts Plan.batch_from_raw returned (their peak_value / rms_value become peak_db / rms_db;
        None: the two are NaN).  dict: "scalars" [n_bufs][15] (HL_SCALARS order), "signature" [n_bufs][64][14], "pitch" [F],
        "peak" [F], "status" [n_bufs]; `want` names the members to fetch (the others are passed as NULL)."""
        n = self.n_bufs
        res = {"scalars": np.zeros((n, NUM_HL_SCALARS)), "signature": np.zeros((n, HL_SIGNATURE_FRAMES, HL_SIGNATURE_BANDS)),
               "pitch": np.zeros(self.total_frames), "peak": np.zeros(self.total_frames), "status": np.zeros(n, dtype=np.int32)}
        res = {k: v for k, v in res.items() if k in want}
        out = _HighOut()
        for k, v in res.items():
            setattr(out, k, v.ctypes.data if v.size else None)
        info = None
        if levels is not None:
            if len(levels) != n:
                raise ValueError("levels must hold one load info per buffer")
            info = (_LoadInfo * max(1, n))()
            for i, d in enumerate(levels):
                info[i].peak_value, info[i].rms_value = d["peak_value"], d["rms_value"]
        _check(self.L, self.L.afx_batch_fetch_high_level(self.h, info, ctypes.byref(out)))
        return res

    def high_level_text_capacity(self):
        """afx_batch_high_level_text_capacity: the bytes of text fetch_high_level_text may need for this batch"""
        return int(self.L.afx_batch_high_level_text_capacity(self.h))

    def fetch_high_level_text(self, levels=None, text=None):
        """afx_batch_fetch_high_level_text: the scalars of fetch_high_level and, in place of its three arrays, their text as
        the reference's database stores it (JSON, every number as "%.9g").  dict: "scalars" [n_bufs][15], "status" [n_bufs],
        "text" uint8 [capacity], "begin" int64 [n_bufs][3], "length" int32 [n_bufs][3] (HLT_COLUMNS order), and per column
        name a list of n_bufs bytes objects.  text: a uint8 array to fill (page-locked memory, say) in place of a new one."""
        n = self.n_bufs
        capacity = self.high_level_text_capacity()
        if text is None:
            text = np.zeros(max(1, capacity), dtype=np.uint8)
        res = {"scalars": np.zeros((n, NUM_HL_SCALARS)), "status": np.zeros(n, dtype=np.int32), "text": text,
               "begin": np.zeros((n, len(HLT_COLUMNS)), dtype=np.int64), "length": np.zeros((n, len(HLT_COLUMNS)), dtype=np.int32)}
        out = _HighTextOut(text_capacity=text.size)
        for k in ("scalars", "status", "text", "begin", "length"):
            setattr(out, k, res[k].ctypes.data if res[k].size else None)
        info = None
        if levels is not None:
            if len(levels) != n:
                raise ValueError("levels must hold one load info per buffer")
            info = (_LoadInfo * max(1, n))()
            for i, d in enumerate(levels):
                info[i].peak_value, info[i].rms_value = d["peak_value"], d["rms_value"]
        _check(self.L, self.L.afx_batch_fetch_high_level_text(self.h, info, ctypes.byref(out)))
        for c, name in enumerate(HLT_COLUMNS):
            res[name] = [text[res["begin"][i, c]:res["begin"][i, c] + res["length"][i, c]].tobytes() for i in range(n)]
        return res

    def _row_desc(self, class_model, category_model, class_names, category_names, loop_class, oneshot_class, use_heuristics,
                  category_none_class):
        d = _RowDesc()
        d.decision = _DecisionDesc(class_model=class_model.h if class_model else None, loop_class=loop_class, oneshot_class=oneshot_class,
                                   use_heuristics=int(bool(use_heuristics)), category_model=category_model.h if category_model else None,
                                   category_none_class=category_none_class)
        d.class_names, raw0 = _names(class_names)
        d.category_names, raw1 = _names(category_names)
        d.n_class_names, d.n_category_names = len(raw0), len(raw1)
        return d, (raw0, raw1)

    def high_level_row_capacity(self, class_names=None, category_names=None):
        """afx_batch_high_level_row_capacity: the bytes of text fetch_high_level_row may need for this batch with these names"""
        d, keep = self._row_desc(None, None, class_names, category_names, 0, 1, True, -1)
        return int(self.L.afx_batch_high_level_row_capacity(self.h, ctypes.byref(d)))

    def fetch_high_level_row(self, levels=None, class_model=None, category_model=None, class_names=None, category_names=None,
                             loop_class=0, oneshot_class=1, use_heuristics=True, category_none_class=-1, text=None):
        """afx_batch_fetch_high_level_row: everything the reference's high-level database stores for every buffer, out of one
        fetch: "scalars" [n][15], the nine text columns as "text" uint8 [capacity] with "begin" int64 [n][9] and "length"
        int32 [n][9] (HLR_COLUMNS order) and per column name a list of n bytes objects, and the class decision's "flags" [n],
        "non_finite" [n], "confidences" [n][2], "status" [n].  class_names / category_names: the models' class names (str or
        bytes), none without the model.  text: a uint8 array to fill (page-locked memory, say) in place of a new one."""
        n = self.n_bufs
        d, keep = self._row_desc(class_model, category_model, class_names, category_names, loop_class, oneshot_class, use_heuristics,
                                 category_none_class)
        if text is None:
            text = np.zeros(max(1, int(self.L.afx_batch_high_level_row_capacity(self.h, ctypes.byref(d)))), dtype=np.uint8)
        res = {"scalars": np.zeros((n, NUM_HL_SCALARS)), "text": text, "begin": np.zeros((n, len(HLR_COLUMNS)), dtype=np.int64),
               "length": np.zeros((n, len(HLR_COLUMNS)), dtype=np.int32), "flags": np.zeros(n, dtype=np.int32),
               "non_finite": np.zeros(n, dtype=np.int32), "confidences": np.zeros((n, 2)), "status": np.zeros(n, dtype=np.int32)}
        out = _RowOut(text_capacity=text.size)
        for name, a in res.items():
            setattr(out, name, a.ctypes.data if a.size else None)
        info = None
        if levels is not None:
            if len(levels) != n:
                raise ValueError("levels must hold one load info per buffer")
            info = (_LoadInfo * max(1, n))()
            for i, lv in enumerate(levels):
                info[i].peak_value, info[i].rms_value = lv["peak_value"], lv["rms_value"]
        _check(self.L, self.L.afx_batch_fetch_high_level_row(self.h, info, ctypes.byref(d), ctypes.byref(out)))
        for c, name in enumerate(HLR_COLUMNS):
            res[name] = [text[res["begin"][i, c]:res["begin"][i, c] + res["length"][i, c]].tobytes() for i in range(n)]
        return res

    def fetch_classification_features(self):
        """afx_batch_fetch_classification_features: the reference's model input of every buffer
        (SampleClassificationDescriptors.cpp:395-561) -> (features [n_bufs][1680], non_finite [n_bufs], status [n_bufs]);
        classification_feature_names() names the columns."""
        n = self.n_bufs
        features = np.zeros((max(1, n), NUM_CLASSIFICATION_FEATURES))   # one spare row: the C call wants a pointer for n = 0 too
        non_finite, status = np.zeros(max(1, n), dtype=np.int32), np.zeros(max(1, n), dtype=np.int32)
        _check(self.L, self.L.afx_batch_fetch_classification_features(self.h, features.ctypes.data, non_finite.ctypes.data,
                                                                      status.ctypes.data))
        return features[:n], non_finite[:n], status[:n]

    def fetch_class_signature(self, model):
        """afx_batch_fetch_class_signature: the reference's class signature of every buffer (SampleAnalyser.cpp:1075-1231)
        -> (signature float32 [n_bufs][n_classes], iterations_used [n_bufs][n_models], non_finite [n_bufs])"""
        n = self.n_bufs
        signature = np.zeros((max(1, n), model.n_classes), dtype=np.float32)
        used = np.zeros((max(1, n), model.n_models), dtype=np.int32)
        non_finite = np.zeros(max(1, n), dtype=np.int32)
        _check(self.L, self.L.afx_batch_fetch_class_signature(self.h, model.h, signature.ctypes.data, used.ctypes.data,
                                                              non_finite.ctypes.data))
        return signature[:n], used[:n], non_finite[:n]

    def fetch_class_decision(self, class_model=None, category_model=None, loop_class=0, oneshot_class=1, use_heuristics=True,
                             category_none_class=-1):
        """afx_batch_fetch_class_decision: what the reference makes of the signatures of every buffer
        (SampleAnalyser.cpp:1097-1231) -> dict: "confidences" [n][2] (IsOneShot, IsLoop; -1: not evaluated), "flags" [n]
        (DECISION_*), "non_finite" [n]; with a class model "class_signature" float32 [n][2], "class_strengths" [n][2],
        "classes" int32 [n][2] (picked indices in pick order, -1 padded); with a category model of K classes
        "category_signature" [n][K], "category_strengths" [n][K], "categories" [n][K]"""
        d = _DecisionDesc(class_model=class_model.h if class_model else None, loop_class=loop_class, oneshot_class=oneshot_class,
                          use_heuristics=int(bool(use_heuristics)), category_model=category_model.h if category_model else None,
                          category_none_class=category_none_class)
        out, res = _decision_out(self.n_bufs, class_model is not None, category_model.n_classes if category_model else 0)
        _check(self.L, self.L.afx_batch_fetch_class_decision(self.h, ctypes.byref(d), ctypes.byref(out)))
        return res

    def close(self):
        if getattr(self, "h", None):
            self.L.afx_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
