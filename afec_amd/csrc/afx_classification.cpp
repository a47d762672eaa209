// afec_amd/csrc/afx_classification.cpp -- afx_batch_fetch_classification_features: TSampleClassificationDescriptors
// (SampleClassificationDescriptors.cpp:395-561), the 1 680 values per file the reference's models read, for every buffer
// of a batch that has run.  One kernel launch (classify/afx_classify.hip) on the batch's stream over what the run left in
// device memory, one device-to-host transfer of its result block.  As everywhere on the host side (afx_host.h), nothing
// here computes a feature: the effective lengths go up as afx_batch_fetch hands them out, the block comes back.
// Beside it what a caller needs to read the block: the features' names and the values a missing frame is filled with.

#include <cstdio>
#include <cstring>

#include "afx_host.h"
#include "classify/afx_classify.h"

using namespace afx::host;

namespace {

const char* const kStatNames[7] = {"min", "max", "mean", "variance", "flatness", "dmean", "dvariance"};
const char* const kSeriesNames[6] = {"spectral_rms", "spectral_flatness", "spectral_flux", "spectral_contrast",
                                     "spectral_complexity", "f0_confidence"};
const char* const kBandSeriesNames[6] = {"spectral_rms_bands", "spectral_flatness_bands", "spectral_flux_bands",
                                         "spectral_complexity_bands", "spectral_contrast_bands", "cepstrum_bands"};
const char* const kScalarNames[7] = {"rhythm_complex_tempo_confidence", "rhythm_percussive_tempo_confidence",
                                     "rhythm_complex_onset_contrast", "rhythm_percussive_onset_contrast",
                                     "rhythm_complex_onset_strength", "rhythm_percussive_onset_strength",
                                     "effectve_length_12dB"};

// the name of feature j as the reference's kExtractFeatureNames pass builds it; the sections are those of the kernel
int feature_name(int j, char* dst, size_t cap) {
  using namespace afx;
  if (j < kClassifySeriesAt)   // the frame NUMBER here (:439), the index everywhere else (:99)
    return std::snprintf(dst, cap, "spectrum_signature_b%d_t%d", j / kClassifyTimeFrames, classify_time_frame(j % kClassifyTimeFrames));
  if (j < kClassifySeriesStatsAt) {
    const int q = j - kClassifySeriesAt;
    return std::snprintf(dst, cap, "%s_t%d", kSeriesNames[q / kClassifyTimeFrames], q % kClassifyTimeFrames);
  }
  if (j < kClassifyBandStatsAt) {
    const int q = j - kClassifySeriesStatsAt;
    return std::snprintf(dst, cap, "%s_%s", kSeriesNames[q / 7], kStatNames[q % 7]);
  }
  if (j < kClassifyAmplitudeAt) {
    const int q = j - kClassifyBandStatsAt, r = q % (kNumSub * 7);
    return std::snprintf(dst, cap, "%s_%s_b%d", kBandSeriesNames[q / (kNumSub * 7)], kStatNames[r % 7], r / 7);
  }
  if (j < kClassifyAmplitudeStatsAt) return std::snprintf(dst, cap, "amplitude_rms_t%d", j - kClassifyAmplitudeAt);
  if (j < kClassifyScalarsAt) {
    const int q = j - kClassifyAmplitudeStatsAt;
    return std::snprintf(dst, cap, "%s_%s", (q / 7) ? "amplitude_silence" : "amplitude_rms", kStatNames[q % 7]);
  }
  if (j < kClassifyPaddingAt) return std::snprintf(dst, cap, "%s", kScalarNames[j - kClassifyScalarsAt]);
  return std::snprintf(dst, cap, "padding_%d", j - kClassifyPaddingAt);
}

}  // namespace

extern "C" {

int afx_classification_feature_name(int32_t index, char* dst, int32_t capacity) {
  if (!dst || index < 0 || index >= afx::kClassifyFeatures || capacity <= 0) return fail(AFX_ERR_INVALID_ARG, "bad argument");
  char name[64];
  const int len = feature_name(index, name, sizeof(name));
  if (len < 0 || len >= (int)sizeof(name) || len >= capacity) return fail(AFX_ERR_INVALID_ARG, "capacity too small for the name");
  std::memcpy(dst, name, (size_t)len + 1);
  return len;
}

int afx_plan_get_silence_features(const afx_plan* plan, double* out) {
  if (!plan || !out) return fail(AFX_ERR_INVALID_ARG, "null argument");
  std::memcpy(out, afx::kClassifySilenceValues, sizeof(afx::kClassifySilenceValues));
  return AFX_OK;
}

int afx_batch_fetch_classification_features(afx_batch* b, double* features, int32_t* non_finite, int32_t* status) {
  if (!b || !features) return fail(AFX_ERR_INVALID_ARG, "null argument");
  // a batch keeps AFX_D_STATISTICS apart from its mask: the statistics' device block stands for the bit
  constexpr uint32_t kSeriesBits = AFX_D_CLASSIFICATION_INPUTS & ~(uint32_t)AFX_D_STATISTICS;
  if ((b->mask & kSeriesBits) != kSeriesBits || (b->n_bufs > 0 && !b->d_stats))
    return fail(AFX_ERR_INVALID_ARG, "the batch mask lacks an input of the classification features (AFX_D_CLASSIFICATION_INPUTS)");
  if (!b->ran) return fail(AFX_ERR_INVALID_ARG, "afx_batch_fetch_classification_features before afx_batch_run");
  const size_t n = (size_t)b->n_bufs;
  if (n == 0) return AFX_OK;
  HIP_TRY(hipSetDevice(b->plan->desc.device));

  // the block: the features and the counts (what comes back), behind them the effective lengths and the buffers' status
  // (what goes up)
  const size_t n_features = n * afx::kClassifyFeatures, n_counts = (n + 1) & ~(size_t)1;
  const size_t out_bytes = n_features * sizeof(double) + n_counts * sizeof(int32_t);
  const size_t in_bytes = n * sizeof(double) + n * sizeof(int32_t);
  HIP_TRY(ws_reserve(b->plan, b->ws->high, out_bytes + in_bytes));
  HIP_TRY(ws_result_pin_reserve(b->ws, out_bytes + in_bytes));
  char* const d_block = (char*)b->ws->high.p;
  char* const block = (char*)b->ws->h_high;

  HIP_TRY(hipStreamSynchronize(b->stream));   // the run's effective-length kernel has written d_efflen
  {
    std::vector<double> seconds(n * 3);
    const int st = effective_length_seconds(b, seconds.data());
    if (st != AFX_OK) return st;
    double* const up = (double*)(block + out_bytes);
    for (size_t i = 0; i < n; ++i) up[i] = seconds[i * 3 + 2];
    std::memcpy(up + n, b->buf_status.data(), n * sizeof(int32_t));
  }
  afx::ClassifyArgs a{};
  a.rec = b->d_rec;
  a.lay = b->lay;
  a.frame_offset = b->d_frame_offset;
  a.stats = b->d_stats;
  a.rt_scalars = b->d_rt_scalars;
  a.efflen12 = (const double*)(d_block + out_bytes);
  a.status = (const int32_t*)(a.efflen12 + n);
  a.n_bufs = b->n_bufs;
  a.features = (double*)d_block;
  a.non_finite = (int32_t*)(a.features + n_features);

  HIP_TRY(hipMemcpyAsync(d_block + out_bytes, block + out_bytes, in_bytes, hipMemcpyHostToDevice, b->stream));
  HIP_TRY(afx::launch_classification_features(a, b->stream));
  {
    const Download item{block, d_block, out_bytes};
    HIP_TRY(download_through_plan(b, &item, 1));   // waits for the batch's stream first, then for the transfer
  }
  std::memcpy(features, block, n_features * sizeof(double));
  if (non_finite) std::memcpy(non_finite, block + n_features * sizeof(double), n * sizeof(int32_t));
  if (status) std::memcpy(status, b->buf_status.data(), n * sizeof(int32_t));
  return AFX_OK;
}

}  // extern "C"
