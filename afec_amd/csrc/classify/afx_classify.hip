// afec_amd/csrc/classify/afx_classify.hip -- the feature vector of a file that the reference's classification models are
// trained and evaluated on, TSampleClassificationDescriptors (SampleClassificationDescriptors.cpp:395-561), from what a batch
// holds in device memory after afx_batch_run: its per-frame records, the 13 statistics of every record column, the rhythm
// tracker's scalars, and the effective length the host formed.  Nothing here touches audio samples.
//
// A gather: of the 1 680 values only the signature's 672 are computed (a merge of one or two bands and a pow), the others
// are copies.  One wave per file; lane = output index in strides of 64, so a wave's store covers 512 contiguous bytes of the
// file's row.  Where a value comes from is a closed form of its index (the section starts of afx_classify.h), so no table
// goes up with a launch.  The sections' starts are no multiples of 64: the lanes of a wave diverge where two sections meet,
// six times in 27 rounds.  Reads: at most 48 rows of the file's records (frames 0..43 and 64, 128, 256, 512 where the
// file has them) and the seven used of every column's 13 statistics; both were written by the run's kernels just before
// and are short enough to come from the caches.

#include <hip/hip_runtime.h>

#include "afx_classify.h"
#include "../afx_device.h"

namespace afx {
namespace {

constexpr int kWaves = 4;   // files per workgroup (the waves share nothing but the launch)

// the t-th of min, max, mean, variance, flatness, dmean, dvariance (:127-141) among the 13 of TStatistics::Calc
// (AFX_S_*: 0, 1, 3, 5, 10, 11, 12)
__device__ __forceinline__ int stat_slot(int t) { return (t < 2) ? t : (t < 4) ? 2 * t - 1 : t + 6; }

__device__ __forceinline__ int pick6(int s, int c0, int c1, int c2, int c3, int c4, int c5) {
  return (s == 0) ? c0 : (s == 1) ? c1 : (s == 2) ? c2 : (s == 3) ? c3 : (s == 4) ? c4 : c5;
}

// one band of the signature (:445-461): the mean of the source bands first..last, a little overscaled, compressed.
// A copy of highlevel/afx_highlevel.hip's function of this name: that file's kernel is pinned to its recorded resources
// and results, so the two lines are not worth a header both would have to include.
__device__ __forceinline__ double merged_band(const double* bands, int first, int last) {
  double v = 0.0;
  for (int sb = first; sb <= last; ++sb) v += bands[sb];
  v /= (double)(last - first + 1);
  return pow(v * 1.25, 1.0 / 6.0);
}

__device__ __forceinline__ bool not_finite(double v) {
  return ((unsigned long long)__double_as_longlong(v) & 0x7FF0000000000000ull) == 0x7FF0000000000000ull;
}

__global__ __launch_bounds__(64 * kWaves) void classification_features_kernel(ClassifyArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int file = (int)blockIdx.x * kWaves + wave;
  if (file >= a.n_bufs) return;
  const RecordLayout& lay = a.lay;
  const int64_t stride = lay.stride;
  const int64_t row0 = a.frame_offset[file];
  const int n = (int)(a.frame_offset[file + 1] - row0);
  double* out = a.features + (int64_t)file * kClassifyFeatures;
  if (n <= 0 || a.status[file] != 0) {
    // no frames (an empty or a refused buffer): zeros, as the high-level fetch answers
    for (int j = lane; j < kClassifyFeatures; j += 64) out[j] = 0.0;
    if (lane == 0) a.non_finite[file] = 0;
    return;
  }
  const double* rec = a.rec + row0 * stride;
  const double* stats = a.stats + (int64_t)file * stride * 13;
  const double* rhythm = a.rt_scalars + (int64_t)file * 14;

  int bad = 0;
  for (int j = lane; j < kClassifyFeatures; j += 64) {
    double v;
    if (j < kClassifySeriesAt) {
      // spectrum_signature_b<b>_t<frame> (:432-469), band outer, time inner
      const int b = j / kClassifyTimeFrames;
      const int frame = classify_time_frame(j - b * kClassifyTimeFrames);
      if (frame < n) {
        // sSpectrumBands = 0, 1, 3, 5, .. 25: a band ends there and starts behind the one before
        const double* bands = rec + (int64_t)frame * stride + lay.bands;
        v = merged_band(bands, (b < 2) ? b : 2 * b - 2, (b < 2) ? b : 2 * b - 1);
      } else {
        v = kClassifySilenceValues[b];
      }
    } else if (j < kClassifySeriesStatsAt) {
      // <series>_t<i> of the six scalar series (:475-491)
      const int q = j - kClassifySeriesAt;
      const int s = q / kClassifyTimeFrames;
      const int frame = classify_time_frame(q - s * kClassifyTimeFrames);
      const int col = pick6(s, lay.srms, lay.flatness, lay.flux, lay.contrast, lay.complexity, lay.f0_conf);
      v = (frame < n) ? rec[(int64_t)frame * stride + col] : kClassifySilenceValues[kClassifyBands + s];
    } else if (j < kClassifyBandStatsAt) {
      // <series>_<stat> of the same six (:496-501)
      const int q = j - kClassifySeriesStatsAt;
      const int s = q / 7;
      const int col = pick6(s, lay.srms, lay.flatness, lay.flux, lay.contrast, lay.complexity, lay.f0_conf);
      v = stats[col * 13 + stat_slot(q - s * 7)];
    } else if (j < kClassifyAmplitudeAt) {
      // <series>_<stat>_b<band> of the six band series, complexity before contrast (:506-513); band outer, statistic inner
      const int q = j - kClassifyBandStatsAt;
      const int s = q / (kNumSub * 7);
      const int r = q - s * (kNumSub * 7);
      const int band = r / 7;
      const int col = pick6(s, lay.sub_rms, lay.sub_flat, lay.sub_flux, lay.sub_cplx, lay.sub_contrast, lay.mfcc) + band;
      v = stats[col * 13 + stat_slot(r - band * 7)];
    } else if (j < kClassifyAmplitudeStatsAt) {
      // amplitude_rms_t<i> (:519-520)
      const int frame = classify_time_frame(j - kClassifyAmplitudeAt);
      v = (frame < n) ? rec[(int64_t)frame * stride + lay.amp_rms] : kClassifySilenceValues[kClassifySilence - 1];
    } else if (j < kClassifyScalarsAt) {
      // amplitude_rms_<stat>, then amplitude_silence_<stat> (:521-524)
      const int q = j - kClassifyAmplitudeStatsAt;
      const int s = q / 7;
      v = stats[(s ? lay.silence : lay.amp_rms) * 13 + stat_slot(q - s * 7)];
    } else if (j < kClassifyPaddingAt) {
      // complex, percussive tempo confidence (AFX_R_* 2, 8), onset contrast (5, 11), onset strength (4, 10), then
      // effectve_length_12dB (:527-538)
      const int q = j - kClassifyScalarsAt;
      const int slot = ((q & 1) ? 6 : 0) + ((q < 2) ? 2 : (q < 4) ? 5 : 4);
      v = (q == 6) ? a.efflen12[file] : rhythm[slot];
    } else {
      v = stats[lay.srms * 13 + 3];   // padding_<k>: the spectral_rms mean (:543-553)
    }
    out[j] = v;
    bad += not_finite(v) ? 1 : 0;
  }
  bad = wave_sum_i(bad);
  if (lane == 0) a.non_finite[file] = bad;
}

}  // namespace

hipError_t launch_classification_features(const ClassifyArgs& a, hipStream_t stream) {
  if (a.n_bufs <= 0) return hipSuccess;
  const int blocks = (a.n_bufs + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(classification_features_kernel, dim3(blocks), dim3(64 * kWaves), 0, stream, a);
  return hipGetLastError();
}

}  // namespace afx
