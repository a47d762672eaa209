// afec_amd/csrc/gbdt/afx_gbdt.hip -- the class signature of a file (SampleAnalyser.cpp:1075-1231): its 1 680 classification
// features, normalised and clipped (ClassificationTestDataItem.cpp:36-41), through a bagging of LightGBM models
// (Models/GBDT.cpp:326-373, Models/Bagging.h:192-217), from the feature block classification_features_kernel left in device
// memory.  Nothing comes down but the answer: n_classes floats per file.
//
// One wave per file, four files per workgroup (the waves share nothing but the launch).  The wave puts its normalised
// features into LDS (13 440 B), then walks model after model in periods of early_stop_freq iterations: the period's
// freq x n_classes trees are spread over the lanes, 64 at a time, each lane walking one tree (features from LDS, nodes
// from global memory: a model is a few hundred KB that every wave of the launch reads, so it comes from L2), the leaf
// values go to LDS, and lane k adds those of class k IN ITERATION ORDER -- the raw scores are the sums GBDT::PredictRaw
// (gbdt_prediction.cpp:13-32) forms one tree after the other, bit for bit.  The margin test behind a full period
// (prediction_early_stop.cpp:25-52) reads the scores from LDS in every lane, so the decision to stop is the same in all.
// Then ConvertOutput (softmax or a sigmoid per class), the cast to float and the float sum over the models in model order.
//
// What bounds it: the walks are dependent loads (node -> feature -> child), a handful per tree; with the reference's model
// (3 leaves: two levels) a period is 20 trees on 20 lanes, so latency, not bandwidth or arithmetic.

#include <hip/hip_runtime.h>

#include "afx_gbdt.h"
#include "../afx_device.h"

namespace afx {
namespace {

constexpr int kWaves = 4;   // files per workgroup

__device__ __forceinline__ bool not_finite(double v) {
  return ((unsigned long long)__double_as_longlong(v) & 0x7FF0000000000000ull) == 0x7FF0000000000000ull;
}

// Tree::Predict (tree.h:590-603): GetLeaf's walk (:690-702) with NumericalDecision (:328-346), then the leaf's value
__device__ __forceinline__ double tree_output(const GbdtModel& m, int tree, const double* x) {
  const int leaf0 = m.leaf_first[tree];
  if (m.num_leaves[tree] <= 1) return m.leaf_value[leaf0];
  const int node0 = m.node_first[tree];
  constexpr double kZeroThreshold = 1e-35f;   // meta.h:54: a float literal widened to double
  int node = 0;
  while (node >= 0) {
    const int g = node0 + node;
    double v = x[m.split_feature[g]];
    const int d = m.decision_type[g];
    const int missing = (d >> 2) & 3;   // MissingType: 0 none, 1 zero, 2 NaN
    if (v != v && missing != 2) v = 0.0;
    const bool is_default = (missing == 1 && v >= -kZeroThreshold && v <= kZeroThreshold) || (missing == 2 && v != v);
    const bool left = is_default ? (d & 2) != 0 : v <= m.threshold[g];
    node = left ? m.left_child[g] : m.right_child[g];
  }
  return m.leaf_value[leaf0 + ~node];
}

__global__ __launch_bounds__(64 * kWaves) void class_signature_kernel(GbdtArgs a) {
  __shared__ double s_x[kWaves][kGbdtFeatures];
  __shared__ double s_leaf[kWaves][64];
  __shared__ double s_raw[kWaves][kGbdtMaxClasses];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int file = (int)blockIdx.x * kWaves + wave;
  if (file >= a.n_bufs) return;
  const GbdtModel& m = a.model;
  const int n_classes = m.n_classes, n_models = m.n_models;
  float* const signature = a.signature + (int64_t)file * n_classes;
  int32_t* const used_out = a.iterations_used + (int64_t)file * n_models;
  double* const x = s_x[wave];
  double* const leaf = s_leaf[wave];
  double* const raws = s_raw[wave];

  // x = clamp(features * A + b, -L, L), the product rounded before the sum as shark's two passes round it; the count of
  // values that are NaN or infinite as classification_features_kernel takes it
  const bool empty = a.frame_offset[file + 1] - a.frame_offset[file] <= 0 || a.status[file] != 0;
  int bad = 0;
  if (!empty) {
    const double* f = a.features + (int64_t)file * kGbdtFeatures;
    for (int j = lane; j < kGbdtFeatures; j += 64) {
      const double v = f[j];
      bad += not_finite(v) ? 1 : 0;
      const double hi = m.limits[j], lo = -hi;
      double y = mul_rn(v, m.scale[j]) + m.offset[j];
      y = (hi < y) ? hi : y;    // std::min(max, y)
      y = (lo < y) ? y : lo;    // std::max(min, y)
      x[j] = y;
    }
    bad = wave_sum_i(bad);
  }
  if (empty || bad != 0) {
    // no frames, a refused buffer, or a feature the reference would have failed the file for: zeros and the count
    if (lane < n_classes) signature[lane] = 0.0f;
    if (lane < n_models) used_out[lane] = 0;
    if (lane == 0) a.non_finite[file] = bad;
    return;
  }
  wave_lds_fence();

  const int freq = m.early_stop_freq;
  float mean = 0.0f;   // lane k: class k
  for (int mi = 0; mi < n_models; ++mi) {
    const int tree0 = m.tree_first[mi];
    const int iterations = (m.tree_first[mi + 1] - tree0) / n_classes;
    double raw = 0.0;    // lane k: the raw score of class k
    int used = iterations;
    for (int it0 = 0; it0 < iterations;) {
      const int count = min(freq, iterations - it0);   // the iterations of this period
      const int trees = count * n_classes;
      const int first = tree0 + it0 * n_classes;
      for (int base = 0; base < trees; base += 64) {
        const int chunk = min(64, trees - base);
        if (lane < chunk) leaf[lane] = tree_output(m, first + base + lane, x);
        wave_lds_fence();
        if (lane < n_classes) {
          // tree j of the period belongs to class j % n_classes: the first of this class in the chunk, then every n_classes-th
          for (int j = (lane - base % n_classes + n_classes) % n_classes; j < chunk; j += n_classes) raw += leaf[j];
        }
        wave_lds_fence();
      }
      it0 += count;
      if (count == freq) {
        // CreateMulticlass' callback: the two largest of the raw scores, the same computation in every lane
        if (lane < n_classes) raws[lane] = raw;
        wave_lds_fence();
        double top = raws[0], second = raws[1];
        if (second > top) { const double t = top; top = second; second = t; }
        for (int k = 2; k < n_classes; ++k) {
          const double v = raws[k];
          if (v > top) { second = top; top = v; } else if (v > second) { second = v; }
        }
        wave_lds_fence();
        if (top - second > m.early_stop_margin) {
          used = it0;
          break;
        }
      }
    }

    // ConvertOutput (multiclass_objective.hpp:132-134, :239-243; Common::Softmax, common.h:545-558), then (float)
    double out;
    if (m.objective[mi] == kGbdtSoftmax) {
      if (lane < n_classes) raws[lane] = raw;
      wave_lds_fence();
      double wmax = raws[0];
      for (int k = 1; k < n_classes; ++k) wmax = (wmax < raws[k]) ? raws[k] : wmax;
      double wsum = 0.0;
      for (int k = 0; k < n_classes; ++k) wsum += exp(raws[k] - wmax);
      wave_lds_fence();
      out = exp(raw - wmax) / wsum;
    } else {
      out = 1.0 / (1.0 + exp(-m.sigmoid[mi] * raw));
    }
    mean += (float)out;   // Bagging.h:206-210: float sums in model order
    if (lane == 0) used_out[mi] = used;
  }
  if (lane < n_classes) signature[lane] = mean / (float)n_models;
  if (lane == 0) a.non_finite[file] = 0;
}

}  // namespace

hipError_t launch_class_signature(const GbdtArgs& a, hipStream_t stream) {
  if (a.n_bufs <= 0) return hipSuccess;
  const int blocks = (a.n_bufs + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(class_signature_kernel, dim3(blocks), dim3(64 * kWaves), 0, stream, a);
  return hipGetLastError();
}

}  // namespace afx
