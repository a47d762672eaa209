// afec_amd/csrc/afx_decision_block.h -- what the fetches that end in a class decision share, host only: the decision's
// blocks (afx_block.h), its checks and the launches behind the feature kernel.  afx_batch_fetch_class_decision
// (afx_class_decision.cpp) brings the decision block back; afx_batch_fetch_high_level_row (afx_high_level_row.cpp) leaves it
// on the device for the text kernel.
#pragma once

#include <cmath>

#include "afx_block.h"
#include "afx_model.h"
#include "decide/afx_decide.h"
#include "gbdt/afx_gbdt.h"

namespace afx {
namespace host {

// one launch of the models' kernel: `n` vectors at `features` of a block at `base`, its three results at the offsets given
inline afx::GbdtArgs gbdt_args(const afx_model* model, char* base, size_t features, const int64_t* frame_offset, size_t status, int32_t n,
                        size_t signature, size_t iterations_used, size_t non_finite) {
  afx::GbdtArgs g{};
  g.model = model->dev;
  g.features = at<double>(base, features);
  g.frame_offset = frame_offset;
  g.status = at<int32_t>(base, status);
  g.n_bufs = n;
  g.signature = at<float>(base, signature);
  g.iterations_used = at<int32_t>(base, iterations_used);
  g.non_finite = at<int32_t>(base, non_finite);
  return g;
}

// What class_signature_kernel writes for one bagging: what a signature fetch brings back (afx_class_decision.cpp) and the
// export of the per-file results leaves on the device (afx_device_file_io.cpp).
struct SignatureBlock {
  size_t n, n_classes, n_models, signature, iterations_used, non_finite, end;
  SignatureBlock(Layout& l, size_t n_vectors, const afx::GbdtModel& m) : n(n_vectors), n_classes((size_t)m.n_classes), n_models((size_t)m.n_models) {
    signature = l.take<float>(n * n_classes);
    iterations_used = l.take<int32_t>(n * n_models);
    non_finite = l.take<int32_t>(n);
    end = l.bytes();
  }
  void hand_out(const char* host, float* out_signature, int32_t* out_iterations_used, int32_t* out_non_finite) const {
    std::memcpy(out_signature, host + signature, n * n_classes * sizeof(float));
    if (out_iterations_used) std::memcpy(out_iterations_used, host + iterations_used, n * n_models * sizeof(int32_t));
    if (out_non_finite) std::memcpy(out_non_finite, host + non_finite, n * sizeof(int32_t));
  }
};

// What afx_decision_out names: the two signatures (a model that is not there has an array of no length), which the decision
// kernel reads, then what it writes.
struct DecisionBlock {
  size_t n, k, signature[2], class_strengths, confidences, category_strengths, classes, categories, flags, non_finite, end;
  bool with_classes;
  DecisionBlock(Layout& l, size_t n_files, bool has_class_model, size_t n_categories) : n(n_files), k(n_categories), with_classes(has_class_model) {
    signature[0] = l.take<float>(with_classes ? n * 2 : 0);
    signature[1] = l.take<float>(n * k);
    class_strengths = l.take<double>(n * 2);
    confidences = l.take<double>(n * 2);
    category_strengths = l.take<double>(n * k);
    classes = l.take<int32_t>(n * 2);
    categories = l.take<int32_t>(n * k);
    flags = l.take<int32_t>(n);
    non_finite = l.take<int32_t>(n);
    end = l.bytes();
  }
  void point(afx::DecideArgs* a, char* base) const {
    a->class_signature = with_classes ? at<float>(base, signature[0]) : nullptr;
    a->category_signature = k ? at<float>(base, signature[1]) : nullptr;
    a->class_strengths = at<double>(base, class_strengths);
    a->confidences = at<double>(base, confidences);
    a->category_strengths = at<double>(base, category_strengths);
    a->classes = at<int32_t>(base, classes);
    a->categories = at<int32_t>(base, categories);
    a->flags = at<int32_t>(base, flags);
    a->non_finite = at<int32_t>(base, non_finite);
  }
  void hand_out(const char* host, afx_decision_out* out) const {
    // without a class model the reference's lists are empty: nothing is written for them
    if (out->class_signature && with_classes) std::memcpy(out->class_signature, host + signature[0], n * 2 * sizeof(float));
    if (out->class_strengths && with_classes) std::memcpy(out->class_strengths, host + class_strengths, n * 2 * sizeof(double));
    if (out->classes && with_classes) std::memcpy(out->classes, host + classes, n * 2 * sizeof(int32_t));
    if (out->category_signature && k) std::memcpy(out->category_signature, host + signature[1], n * k * sizeof(float));
    if (out->category_strengths && k) std::memcpy(out->category_strengths, host + category_strengths, n * k * sizeof(double));
    if (out->categories && k) std::memcpy(out->categories, host + categories, n * k * sizeof(int32_t));
    if (out->confidences) std::memcpy(out->confidences, host + confidences, n * 2 * sizeof(double));
    if (out->flags) std::memcpy(out->flags, host + flags, n * sizeof(int32_t));
    if (out->non_finite) std::memcpy(out->non_finite, host + non_finite, n * sizeof(int32_t));
  }
};

// Between the feature block and the decision block of a batch's class decision: what the models' kernel writes and only the
// decision kernel reads, for the class model [0] and the category model [1].  It stays on the device.
struct DecisionScratch {
  size_t iterations_used[2], non_finite[2];
  DecisionScratch(Layout& l, size_t n, const afx_model* const models[2]) {
    for (int m = 0; m < 2; ++m) iterations_used[m] = l.take<int32_t>(models[m] ? n * (size_t)models[m]->dev.n_models : 0);
    for (int m = 0; m < 2; ++m) non_finite[m] = l.take<int32_t>(n);
  }
};

// the indices a decision names: AFX_OK or why not
inline int check_decision_indices(int loop_class, int oneshot_class, int none_class, int n_categories) {
  if (loop_class < 0 || loop_class > 1 || oneshot_class < 0 || oneshot_class > 1 || loop_class == oneshot_class)
    return fail(AFX_ERR_INVALID_ARG, "loop_class and oneshot_class are 0 and 1 in either order");
  if (none_class < -1 || none_class >= n_categories) return fail(AFX_ERR_INVALID_ARG, "category_none_class names no class of the category model");
  return AFX_OK;
}

// what a decision is told, the same from a batch and from the caller's arrays; the blocks point the rest
inline afx::DecideArgs decide_args(int32_t n_files, size_t n_categories, int loop_class, int oneshot_class, int use_heuristics, int none_class) {
  afx::DecideArgs a{};
  a.n_categories = (int32_t)n_categories;
  a.loop_class = loop_class;
  a.oneshot_class = oneshot_class;
  a.use_heuristics = use_heuristics != 0;
  a.none_category = none_class;
  a.silence_floor = std::exp(-24.0 * (std::log(10.0) / 20.0));   // DbToLin(-24), AudioMath.inl:108-123
  a.n_files = n_files;
  return a;
}

// the checks of afx_batch_fetch_class_decision on its description (both models NULL is the caller's to judge); *k: the
// category model's classes, 0 without one
inline int check_decision_desc(const afx_batch* b, const afx_decision_desc* desc, size_t* k) {
  const afx_model* const models[2] = {desc->class_model, desc->category_model};
  for (const afx_model* m : models)
    if (m && m->plan->desc.device != b->plan->desc.device) return fail(AFX_ERR_INVALID_ARG, "a model lives on another device than the batch");
  if (models[0] && models[0]->dev.n_classes != afx::kDecideClasses)
    return fail(AFX_ERR_UNSUPPORTED, "the class model has to have the two classes \"Loop\" and \"OneShot\"");
  *k = models[1] ? (size_t)models[1]->dev.n_classes : 0;
  AFX_TRY(check_decision_indices(desc->loop_class, desc->oneshot_class, desc->category_none_class, (int)*k));
  if (!(b->mask & AFX_D_AMPLITUDE_PEAK)) return fail(AFX_ERR_INVALID_ARG, "the batch mask lacks AFX_D_AMPLITUDE_PEAK (AFX_D_CLASS_DECISION_INPUTS)");
  return AFX_OK;
}

// behind the feature kernel on the batch's stream: the models' kernel once per model given, then the decision kernel, over
// the three blocks of a result block at rb.dev; nothing is downloaded
inline int enqueue_class_decision(afx_batch* b, const afx_decision_desc* desc, const FeatureBlock& fb, const DecisionScratch& scratch,
                                  const DecisionBlock& db, const ResultBlock& rb) {
  const afx_model* const models[2] = {desc->class_model, desc->category_model};
  for (int m = 0; m < 2; ++m) {
    if (!models[m]) continue;
    const afx::GbdtArgs g = gbdt_args(models[m], rb.dev, fb.features, b->d_frame_offset, fb.status, b->n_bufs, db.signature[m],
                                      scratch.iterations_used[m], scratch.non_finite[m]);
    HIP_TRY(afx::launch_class_signature(g, b->stream));
  }
  afx::DecideArgs a = decide_args(b->n_bufs, db.k, desc->loop_class, desc->oneshot_class, desc->use_heuristics, desc->category_none_class);
  a.peak = b->d_rec + b->lay.amp_peak;
  a.peak_stride = b->lay.stride;
  a.frame_offset = b->d_frame_offset;
  a.efflen24 = {at<double>(rb.dev, fb.efflen24), 1};
  a.onset_count = {b->d_rt_scalars + AFX_R_PERCUSSIVE_ONSET_COUNT, AFX_NUM_RHYTHM_SCALARS};
  a.percussive_confidence = {b->d_rt_scalars + AFX_R_PERCUSSIVE_TEMPO_CONFIDENCE, AFX_NUM_RHYTHM_SCALARS};
  a.complex_confidence = {b->d_rt_scalars + AFX_R_COMPLEX_TEMPO_CONFIDENCE, AFX_NUM_RHYTHM_SCALARS};
  a.flux_mean = {b->d_stats + (size_t)b->lay.flux * AFX_NUM_STATISTICS + AFX_S_MEAN, (int64_t)b->lay.stride * AFX_NUM_STATISTICS};
  a.status = at<int32_t>(rb.dev, fb.status);
  // the same features: the same count from either model's kernel
  a.non_finite_in = at<int32_t>(rb.dev, scratch.non_finite[models[0] ? 0 : 1]);
  db.point(&a, rb.dev);
  HIP_TRY(afx::launch_class_decision(a, b->stream));
  return AFX_OK;
}

}  // namespace host
}  // namespace afx
