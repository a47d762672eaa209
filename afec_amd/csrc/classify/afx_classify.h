// afec_amd/csrc/classify/afx_classify.h -- the classification features' kernel (afx_classify.hip) and its launcher, shared
// with the entry points of afx_classification.cpp and afx_class_decision.cpp.  Kept apart from afx_internal.h for the reason
// highlevel/afx_highlevel.h gives; a device mock implements this launcher too.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../afx_internal.h"

namespace afx {

constexpr int kClassifyTimeFrames = 48;   // AFX_CF_TIME_FRAMES: sTimeSeries = 0..43, 64, 128, 256, 512
constexpr int kClassifyBands = 14;        // sSpectrumBands = 0, 1, 3, .. 25: the merge of the high-level signature
constexpr int kClassifyFeatures = 1680;   // AFX_NUM_CLASSIFICATION_FEATURES = 35 x 48
constexpr int kClassifySilence = 21;      // AFX_NUM_CF_SILENCE

// Where each section of the vector starts (SampleClassificationDescriptors.cpp:430-553)
constexpr int kClassifySeriesAt = kClassifyBands * kClassifyTimeFrames;           //  672: six scalar series x 48 frames
constexpr int kClassifySeriesStatsAt = kClassifySeriesAt + 6 * kClassifyTimeFrames;   //  960: their seven statistics
constexpr int kClassifyBandStatsAt = kClassifySeriesStatsAt + 6 * 7;              // 1002: six band series x 14 bands x 7
constexpr int kClassifyAmplitudeAt = kClassifyBandStatsAt + 6 * kNumSub * 7;      // 1590: amplitude_rms x 48 frames
constexpr int kClassifyAmplitudeStatsAt = kClassifyAmplitudeAt + kClassifyTimeFrames;   // 1638: amplitude_rms, amplitude_silence x 7
constexpr int kClassifyScalarsAt = kClassifyAmplitudeStatsAt + 2 * 7;             // 1652: six rhythm scalars, effectve_length_12dB
constexpr int kClassifyPaddingAt = kClassifyScalarsAt + 7;                        // 1659: 21 x the spectral_rms mean
static_assert(kClassifyFeatures - kClassifyPaddingAt == 21 && kClassifyFeatures % kClassifyTimeFrames == 0, "35 x 48");

// sTimeSeries[i] (:38-42): the frame of time position i
__host__ __device__ inline int classify_time_frame(int i) { return (i < 44) ? i : 64 << (i - 44); }

// What a frame the file does not have is filled with: the descriptors of one frame of 2 048 zeros, which is what the
// reference's half second of silence (SCreateSilenceSampleDescriptors, :326-360) becomes in LoadSample.  frequency_bands
// 0..13 (the signature's band b takes band b of the 28, :466), then spectral_rms, spectral_flatness, spectral_flux,
// spectral_contrast, spectral_complexity, f0_confidence, amplitude_rms.
constexpr double kClassifySilenceValues[kClassifySilence] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
                                                             0.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0};

struct ClassifyArgs {
  const double* rec;            // [F][lay.stride]: the per-frame records of the batch's last run
  RecordLayout lay;             // every series of AFX_D_CLASSIFICATION_INPUTS is selected
  const int64_t* frame_offset;  // [n_bufs + 1], device
  const double* stats;          // [n_bufs][lay.stride][13]: the statistics of every record column
  const double* rt_scalars;     // [n_bufs][14]: the rhythm tracker's scalars
  const double* efflen12;       // [n_bufs]: effectve_length_12dB in seconds, as afx_batch_fetch hands it out
  const int32_t* status;        // [n_bufs]: buf_status (a buffer with another status than 0 yields zeros)
  int32_t n_bufs;
  double* features;             // [n_bufs][kClassifyFeatures]
  int32_t* non_finite;          // [n_bufs]: how many of a buffer's features are NaN or infinite
};
// one wave per buffer, on `stream`
hipError_t launch_classification_features(const ClassifyArgs& a, hipStream_t stream);

}  // namespace afx
