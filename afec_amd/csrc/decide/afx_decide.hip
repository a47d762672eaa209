// afec_amd/csrc/decide/afx_decide.hip -- what the reference makes of a file's class signature (AnalyzeHighLevelDescriptors,
// SampleAnalyser.cpp:1097-1231): the relative strengths (TClassificationTools::CategoryStrengths, ClassificationTools.cpp:7-39),
// the two heuristics that may override the model (TClassificationHeuristics::IsOneShot / IsLoop,
// ClassificationHeuristics.cpp:12-149; MUseClassificationHeuristics, SampleAnalyser.cpp:72), the picked classes
// (PickAllStrongCategories, ClassificationTools.cpp:46-128), and the same for the categories' model, gated by the classes.
// Everything it reads lies in device memory after afx_batch_run and the signature kernel; a few dozen bytes per file come down.
//
// One wave per file, four files per workgroup (the waves share nothing but the launch).  The hot part is IsOneShot's
// correlation of the peak envelope with a fade-out: the first and the last frame above -24 dB (a wave minimum and maximum:
// what the reference's two scans from the ends find), then the five sums of TStatistics::Correlation
// (Statistics.cpp:604-638) over the frames between them, lane = frame in strides of 64, reduced over the wave -- so the
// sums are formed in another order than the reference's serial loop and agree to rounding, not to the bit.  Everything
// behind the sums is the same scalar arithmetic in every lane: strengths and picks of at most 64 classes, read from LDS.
//
// Every loop is bounded by the file's frame count or the class count; no loop waits for a comparison to succeed, so a NaN
// peak (it compares false: a silent frame) or a NaN signature cannot keep a wave from returning.  std::min, std::max and
// MMin are spelled out as the comparisons the reference compiles to: which operand a NaN leaves is part of the result.
//
// What bounds it: one strided pass over at most a few hundred doubles per file (860 at the default analysis limit) with a
// pow per frame, five reductions, then dependent scalar code: latency, as the models' kernel before it.

#include <hip/hip_runtime.h>

#include "afx_decide.h"
#include "../afx_device.h"

// products are rounded before they are added, as the reference's build rounds them
#pragma clang fp contract(off)

namespace afx {
namespace {

constexpr int kWaves = 4;   // files per workgroup
constexpr int kFlagOneShot = 1, kFlagLoop = 2, kFlagOverridden = 4;
constexpr double kMinDefaultWeight = 0.2, kMinFallbackWeight = 0.01;   // SA:1156-1157, :1211-1212

__device__ __forceinline__ double std_min(double a, double b) { return (b < a) ? b : a; }
__device__ __forceinline__ double std_max(double a, double b) { return (a < b) ? b : a; }
__device__ __forceinline__ double m_min(double a, double b) { return (a < b) ? a : b; }   // MMin, InlineMath.inl:22-25

// CategoryStrengths with MinWeight 0 (ClassificationTools.cpp:7-39): the float weights widened to double (mClassSignature is
// a TList<double> assigned from floats), the sum in index order in every lane, lane c's strength into s[c]
__device__ __forceinline__ void relative_strengths(const float* w, int n, double* s, int lane) {
  double sum = 0.0;
  for (int c = 0; c < n; ++c) {
    const double v = (double)w[c];
    if (v >= 0.0) sum += v;
  }
  if (lane < n) {
    const double v = (double)w[lane];
    s[lane] = (v >= 0.0 && sum > 0.0) ? v / sum : 0.0;
  }
  wave_lds_fence();
}

// PickAllStrongCategories (ClassificationTools.cpp:46-128) on indices: the same serial code in every lane over the
// strengths s[0..n) in LDS.  order[0..count) receives the picks in pick order (every lane writes the same values, so a
// lane reads back what it wrote); returns count, *picked the set as a mask.
__device__ __forceinline__ int pick_strong(const double* s, int n, int none, int* order, unsigned long long* picked_out) {
  unsigned long long picked = 0;
  int count = 0;
  for (int i = 0; i < n; ++i) {   // :58-80
    double best = 0.0;
    int best_at = -1;
    for (int j = 0; j < n; ++j) {
      const double w = s[j];
      if (w > kMinDefaultWeight && w >= best && !((picked >> j) & 1ull)) {   // >=: the later index wins a tie
        best = w;
        best_at = j;
      }
    }
    if (best_at < 0) break;
    picked |= 1ull << best_at;
    order[count++] = best_at;
  }
  if (count == 0 && n > 0) {      // :83-90: std::max_element, the first maximum
    int at = 0;
    for (int j = 1; j < n; ++j)
      if (s[at] < s[j]) at = j;
    if (s[at] > kMinFallbackWeight) {
      picked = 1ull << at;
      order[count++] = at;
    }
  }
  if (count > 0 && order[0] == none) {   // :101-106: a leading "None" empties the list
    count = 0;
    picked = 0;
  }
  int kept = 0;                          // :108-116: secondary "None"s leave it
  for (int i = 0; i < count; ++i) {
    const int c = order[i];
    if (c == none) picked &= ~(1ull << c);
    else order[kept++] = c;
  }
  *picked_out = picked;
  return kept;
}

__global__ __launch_bounds__(64 * kWaves) void class_decision_kernel(DecideArgs a) {
  __shared__ double s_strength[kWaves][kDecideMaxCategories];
  __shared__ int s_order[kWaves][kDecideMaxCategories];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int file = (int)blockIdx.x * kWaves + wave;
  if (file >= a.n_files) return;
  double* const s = s_strength[wave];
  int* const order = s_order[wave];
  const int n_cat = a.category_signature ? a.n_categories : 0;
  double* const class_strengths = a.class_strengths + (int64_t)file * kDecideClasses;
  int32_t* const classes = a.classes + (int64_t)file * kDecideClasses;
  double* const category_strengths = a.category_strengths + (int64_t)file * n_cat;
  int32_t* const categories = a.categories + (int64_t)file * n_cat;
  double* const confidences = a.confidences + (int64_t)file * 2;

  const int64_t row0 = a.frame_offset[file];
  const int n = (int)(a.frame_offset[file + 1] - row0);
  const int bad = a.non_finite_in ? a.non_finite_in[file] : 0;
  if (lane == 0) a.non_finite[file] = bad;
  if (n <= 0 || (a.status && a.status[file] != 0) || bad != 0) {
    // no frames, a refused buffer, or features the reference would have failed the file for
    if (lane < kDecideClasses) {
      class_strengths[lane] = 0.0;
      classes[lane] = -1;
      confidences[lane] = -1.0;
    }
    if (lane < n_cat) {
      category_strengths[lane] = 0.0;
      categories[lane] = -1;
    }
    if (lane == 0) a.flags[file] = 0;
    return;
  }

  // ---- classes (SA:1081-1169) ----
  int flags = 0;
  double oneshot_confidence = -1.0, loop_confidence = -1.0;   // SA:1118-1119
  bool loop_only = false;                                      // the picked classes hold "Loop" and no "OneShot"
  if (a.class_signature) {
    relative_strengths(a.class_signature + (int64_t)file * kDecideClasses, kDecideClasses, s, lane);
    if (a.use_heuristics) {
      const double length = a.efflen24.at(file);
      const double onsets = a.onset_count.at(file);
      bool is_oneshot, is_loop = false;
      // IsOneShot (ClassificationHeuristics.cpp:12-98)
      if (length < 0.5) {
        oneshot_confidence = 0.85;
        is_oneshot = true;
      } else if (length < 1.0 && onsets <= 2.0) {
        oneshot_confidence = 0.75;
        is_oneshot = true;
      } else {
        const double length_confidence = pow(1.0 - (std_min(4.0, std_max(0.0, length - 1.0)) / 4.0), 0.5);
        // the envelope without its silent ends (:51-76).  The leading scan stops at the first frame above the floor, the
        // trailing one at the last frame above it or, "f > SilentLeadingFrames", one behind the leading scan's: that frame
        // is above the floor itself, so the envelope is first..last, and empty when no frame is above the floor
        const double* const peak = a.peak + row0 * a.peak_stride;
        int first = n, last = -1;
        for (int f = lane; f < n; f += 64) {
          if (peak[(int64_t)f * a.peak_stride] > a.silence_floor) {
            first = min(first, f);
            last = max(last, f);
          }
        }
        first = wave_min_i(first);
        last = wave_max_i(last);
        const int m = (last < 0) ? 0 : last - first + 1;
        // TStatistics::Correlation(FadeOut, Envelope, m) (Statistics.cpp:604-638); FadeOut[i] = pow(1 - i / (m - 1), 4):
        // with m == 1 that is pow(0 / 0, 4), a NaN, which the test on denom2 below turns into a correlation of 0
        double correlation = 0.0;
        if (m > 0) {
          double ss1 = 0.0, ss2 = 0.0, ss11 = 0.0, ss12 = 0.0, ss22 = 0.0;
          const double last_index = (double)(m - 1);
          for (int i = lane; i < m; i += 64) {
            const double x = pow(1.0 - (double)i / last_index, 4.0);
            const double y = peak[(int64_t)(first + i) * a.peak_stride];
            ss12 = ss12 + x * y;
            ss1 = ss1 + x;
            ss11 = ss11 + x * x;
            ss2 = ss2 + y;
            ss22 = ss22 + y * y;
          }
          ss12 = wave_sum(ss12);
          ss1 = wave_sum(ss1);
          ss11 = wave_sum(ss11);
          ss2 = wave_sum(ss2);
          ss22 = wave_sum(ss22);
          const double length_m = (double)m;
          ss1 = ss1 / length_m;
          ss2 = ss2 / length_m;
          const double denom2 = (ss11 - ss1 * ss1 * length_m) * (ss22 - ss2 * ss2 * length_m);
          const double num = ss12 - (ss1 * ss2 * length_m);
          constexpr double kEpsilon = 1e-12f;   // MEpsilon: a float literal widened to double
          if (fabs(denom2) > kEpsilon) correlation = num / sqrt(denom2);
        }
        const double envelope_confidence = std_min(1.0, fabs(correlation));   // a fade-in counts as well (:90)
        oneshot_confidence = length_confidence * 0.3 + envelope_confidence * 0.7;
        is_oneshot = oneshot_confidence > 0.7;
      }
      // IsLoop (:102-149), only when IsOneShot said no (SA:1135)
      if (!is_oneshot) {
        if (onsets < 8.0 || a.flux_mean.at(file) > 0.9) {
          loop_confidence = 0.0;
        } else {
          const double length_confidence = pow(std_max(0.0, std_min(4.0, length - 1.0) / 4.0), 0.5);
          const double percussive = a.percussive_confidence.at(file);
          double rhythm_confidence = 0.0;
          if (percussive > 0.25 && a.complex_confidence.at(file) > 0.25) rhythm_confidence = std_min(1.0, percussive * 2.0);
          loop_confidence = length_confidence * 0.3 + rhythm_confidence * 0.7;
          is_loop = loop_confidence > 0.7;
        }
      }
      // the override (SA:1121-1148): not renormalised.  Every lane holds the same values; lane 0 stores them
      const double loop_strength = s[a.loop_class], oneshot_strength = s[a.oneshot_class];
      wave_lds_fence();
      if (is_oneshot) {
        flags |= kFlagOneShot;
        if (loop_strength > oneshot_strength) {
          flags |= kFlagOverridden;
          if (lane == 0) {
            s[a.loop_class] = m_min(oneshot_confidence / 2.0, loop_strength);
            s[a.oneshot_class] = oneshot_confidence;
          }
        }
      } else if (is_loop) {
        flags |= kFlagLoop;
        if (loop_strength < oneshot_strength) {
          flags |= kFlagOverridden;
          if (lane == 0) {
            s[a.loop_class] = loop_confidence;
            s[a.oneshot_class] = m_min(loop_confidence / 2.0, oneshot_strength);
          }
        }
      }
      wave_lds_fence();
    }
    unsigned long long picked;
    const int count = pick_strong(s, kDecideClasses, -1, order, &picked);
    if (lane < kDecideClasses) {
      class_strengths[lane] = ((picked >> lane) & 1ull) ? s[lane] : 0.0;   // :119-125
      classes[lane] = (lane < count) ? order[lane] : -1;
    }
    loop_only = count > 0 && !((picked >> a.oneshot_class) & 1ull);
    wave_lds_fence();
  } else if (lane < kDecideClasses) {
    class_strengths[lane] = 0.0;
    classes[lane] = -1;
  }
  if (lane == 0) {
    confidences[0] = oneshot_confidence;
    confidences[1] = loop_confidence;
    a.flags[file] = flags;
  }

  // ---- categories (SA:1176-1231): for files whose classes are empty or hold "OneShot" ----
  if (n_cat > 0) {
    if (loop_only) {
      if (lane < n_cat) {
        category_strengths[lane] = 0.0;
        categories[lane] = -1;
      }
    } else {
      relative_strengths(a.category_signature + (int64_t)file * n_cat, n_cat, s, lane);
      unsigned long long picked;
      const int count = pick_strong(s, n_cat, a.none_category, order, &picked);
      if (lane < n_cat) {
        category_strengths[lane] = ((picked >> lane) & 1ull) ? s[lane] : 0.0;
        categories[lane] = (lane < count) ? order[lane] : -1;
      }
    }
  }
}

}  // namespace

hipError_t launch_class_decision(const DecideArgs& a, hipStream_t stream) {
  if (a.n_files <= 0) return hipSuccess;
  const int blocks = (a.n_files + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(class_decision_kernel, dim3(blocks), dim3(64 * kWaves), 0, stream, a);
  return hipGetLastError();
}

}  // namespace afx
