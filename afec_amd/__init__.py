"""afec_amd -- MI355X-native low-level audio feature extraction (the AFEC crawler's per-frame
spectral hot path as HIP kernels behind the C-ABI of include/afx.h).

Python here is test/bench plumbing over the C-ABI (ctypes); the product is
afec_amd/lib/libafx_hip.so and the C++ host layer in afec_amd/host/.
"""
from .capi import (  # noqa: F401
    AfxError, Batch, Model, Plan, build_info, decide, format_json_g9, format_class_json, HLR_COLUMNS, build_library, device_count, library_path, load_library,
    D_MFCC, D_SPECTRAL_RMS, D_SPECTRAL_CENTROID, D_SPECTRAL_SPREAD, D_SPECTRAL_SKEWNESS,
    D_SPECTRAL_KURTOSIS, D_SPECTRAL_ROLLOFF, D_SPECTRAL_FLATNESS, D_SPECTRAL_FLUX,
    D_SPECTRUM_BANDS, D_BAND_FEATURES, D_AMPLITUDE_PEAK, D_AMPLITUDE_RMS, D_MAGNITUDE, D_STATISTICS, NUM_STATISTICS, STAT_NAMES,
    D_AMPLITUDE_SILENCE, D_AMPLITUDE_ENVELOPE, D_SPECTRAL_COMPLEXITY, D_AUTO_CORRELATION, D_F0,
    D_SPECTRAL_INHARMONICITY, D_TRISTIMULUS, D_EFFECTIVE_LENGTH, D_RHYTHM, RHYTHM_SCALARS, D_NEIGHBOURS, D_ALL_PER_FRAME,
    D_C2, D_SPECTRAL_STATS, D_ALL_LOW_LEVEL, PRECISION_F64, PRECISION_F32, PCM_F32, PCM_F64,
    FRAME_KERNEL_AUTO, FRAME_KERNEL_WAVE64, FRAME_KERNEL_HALFWAVE, PLAN_NO_SIDE_STREAM,
    D_HIGH_LEVEL_INPUTS, HL_SCALARS, NUM_HL_SCALARS, HL_SIGNATURE_FRAMES, HL_SIGNATURE_BANDS,
    D_CLASSIFICATION_INPUTS, CF_TIME_FRAMES, NUM_CLASSIFICATION_FEATURES, NUM_CF_SILENCE, classification_feature_names,
    D_CLASS_DECISION_INPUTS, DECISION_IS_ONESHOT, DECISION_IS_LOOP, DECISION_OVERRIDDEN, DECISION_SCALARS,
)
from .device import (  # noqa: F401
    DeviceArray, Stream, create_batch_from_device, export, export_into, export_statistics, features, frame_counts,
    EXPORT_PACKED, EXPORT_PADDED, SERIES, SERIES_MAGNITUDE,
    create_batch_from_raw_device, export_samples, sample_counts, RAW_INTERLEAVED, RAW_PLANAR,
    file_results, file_results_into, embedding, FILE_KINDS,
)
