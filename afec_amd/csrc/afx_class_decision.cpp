// afec_amd/csrc/afx_class_decision.cpp -- the fetches that evaluate the reference's models on the classification features.
// afx_batch_fetch_class_signature shares the feature fetch's launch (launch_features, afx_classification.cpp): the same
// kernel into the same block, the models' kernel (gbdt/afx_gbdt.hip) behind it on the same stream, and only that kernel's
// few bytes per file come back (SampleAnalyser.cpp:1075-1231).  afx_batch_fetch_class_decision goes one kernel further
// (decide/afx_decide.hip): what the reference makes of the signatures -- strengths, heuristics, classes, categories
// (SampleAnalyser.cpp:1097-1231).  afx_model_evaluate_features and afx_decide run the same two kernels on inputs the caller
// holds, in a device block of their own.  Every entry point reads: check, layout, arguments, launch, one download, hand out.

#include <cstring>

#include "afx_decision_block.h"

using namespace afx::host;

namespace {

// What goes up for afx_decide in front of its decision block.
struct DecideInputs {
  size_t n, frames, peaks, scalars, frame_offset, non_finite;
  DecideInputs(Layout& l, const afx_decision_in* in) : n((size_t)in->n_files), frames((size_t)in->frame_offset[in->n_files]) {
    peaks = l.take<double>(frames);
    scalars = l.take<double>(n * AFX_NUM_DECISION_SCALARS);
    frame_offset = l.take<int64_t>(n + 1);
    non_finite = l.take<int32_t>(n);
  }
  void fill(char* host, const afx_decision_in* in) const {   // `host` starts out as zeros: a count that is not given is 0
    if (frames) std::memcpy(host + peaks, in->peaks, frames * sizeof(double));
    std::memcpy(host + scalars, in->scalars, n * AFX_NUM_DECISION_SCALARS * sizeof(double));
    std::memcpy(host + frame_offset, in->frame_offset, (n + 1) * sizeof(int64_t));
    if (in->non_finite) std::memcpy(host + non_finite, in->non_finite, n * sizeof(int32_t));
  }
  void point(afx::DecideArgs* a, char* base) const {
    const double* const s = at<double>(base, scalars);
    a->peak = at<double>(base, peaks);
    a->peak_stride = 1;
    a->frame_offset = at<int64_t>(base, frame_offset);
    a->efflen24 = {s + AFX_DS_EFFECTIVE_LENGTH_24DB, AFX_NUM_DECISION_SCALARS};
    a->onset_count = {s + AFX_DS_PERCUSSIVE_ONSET_COUNT, AFX_NUM_DECISION_SCALARS};
    a->percussive_confidence = {s + AFX_DS_PERCUSSIVE_TEMPO_CONFIDENCE, AFX_NUM_DECISION_SCALARS};
    a->complex_confidence = {s + AFX_DS_COMPLEX_TEMPO_CONFIDENCE, AFX_NUM_DECISION_SCALARS};
    a->flux_mean = {s + AFX_DS_SPECTRAL_FLUX_MEAN, AFX_NUM_DECISION_SCALARS};
    a->status = nullptr;
    a->non_finite_in = at<int32_t>(base, non_finite);
  }
};

}  // namespace

extern "C" {

int afx_batch_fetch_class_signature(afx_batch* b, const afx_model* model, float* signature, int32_t* iterations_used, int32_t* nonfinite) {
  if (!b || !model || !signature) return fail(AFX_ERR_INVALID_ARG, "null argument");
  if (model->plan->desc.device != b->plan->desc.device) return fail(AFX_ERR_INVALID_ARG, "the model lives on another device than the batch");
  Layout layout;
  const FeatureBlock fb(layout, (size_t)b->n_bufs);
  const SignatureBlock sb(layout, (size_t)b->n_bufs, model->dev);
  ResultBlock rb;
  const int st = launch_features(b, "afx_batch_fetch_class_signature", layout, fb, &rb);
  if (st != AFX_OK || rb.n == 0) return st;
  const afx::GbdtArgs g = gbdt_args(model, rb.dev, fb.features, b->d_frame_offset, fb.status, b->n_bufs, sb.signature, sb.iterations_used, sb.non_finite);
  HIP_TRY(afx::launch_class_signature(g, b->stream));
  HIP_TRY(download_result(b, rb, sb.signature, sb.end));
  sb.hand_out(rb.host, signature, iterations_used, nonfinite);
  return AFX_OK;
}

int afx_model_evaluate_features(const afx_model* model, const double* features, int32_t n_vectors, float* signature,
                                int32_t* iterations_used, int32_t* nonfinite) {
  if (!model || n_vectors < 0 || (n_vectors > 0 && (!features || !signature))) return fail(AFX_ERR_INVALID_ARG, "bad argument");
  if (n_vectors == 0) return AFX_OK;
  HIP_TRY(hipSetDevice(model->plan->desc.device));
  // one block of its own (this is not the crawl's path: no batch, no workspace): a frame table that gives every vector one
  // frame and a status of zeros, what the kernel writes, and last the vectors, which go up from the caller's own array
  const size_t n = (size_t)n_vectors;
  Layout layout;
  const size_t frame_offset = layout.take<int64_t>(n + 1), status = layout.take<int32_t>(n);
  const SignatureBlock sb(layout, n, model->dev);
  const size_t vectors = layout.take<double>(n * afx::kGbdtFeatures);
  std::vector<char> host(vectors, 0);
  for (size_t i = 0; i <= n; ++i) at<int64_t>(host.data(), frame_offset)[i] = (int64_t)i;
  DeviceBlock dev;
  AFX_TRY(dev.allocate(layout.bytes(), "device memory for the feature vectors"));
  const afx::GbdtArgs g = gbdt_args(model, dev.get(), vectors, at<int64_t>(dev.get(), frame_offset), status, n_vectors, sb.signature,
                                    sb.iterations_used, sb.non_finite);
  HIP_TRY(hipMemcpy(dev.get() + vectors, features, layout.bytes() - vectors, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dev.get(), host.data(), sb.signature, hipMemcpyHostToDevice));
  HIP_TRY(afx::launch_class_signature(g, nullptr));
  HIP_TRY(hipMemcpy(host.data() + sb.signature, dev.get() + sb.signature, sb.end - sb.signature, hipMemcpyDeviceToHost));   // waits for the kernel
  sb.hand_out(host.data(), signature, iterations_used, nonfinite);
  return AFX_OK;
}

int afx_batch_fetch_class_decision(afx_batch* b, const afx_decision_desc* desc, afx_decision_out* out) {
  if (!b || !desc || !out) return fail(AFX_ERR_INVALID_ARG, "null argument");
  const afx_model* const models[2] = {desc->class_model, desc->category_model};
  if (!models[0] && !models[1]) return fail(AFX_ERR_INVALID_ARG, "neither a class model nor a category model");
  size_t k = 0;
  AFX_TRY(check_decision_desc(b, desc, &k));
  Layout layout;
  const FeatureBlock fb(layout, (size_t)b->n_bufs);
  const DecisionScratch scratch(layout, (size_t)b->n_bufs, models);
  const DecisionBlock db(layout, (size_t)b->n_bufs, models[0] != nullptr, k);
  ResultBlock rb;
  const int st = launch_features(b, "afx_batch_fetch_class_decision", layout, fb, &rb);
  if (st != AFX_OK || rb.n == 0) return st;
  AFX_TRY(enqueue_class_decision(b, desc, fb, scratch, db, rb));
  HIP_TRY(download_result(b, rb, db.signature[0], db.end));
  db.hand_out(rb.host, out);
  return AFX_OK;
}

int afx_decide(const afx_plan* plan, const afx_decision_in* in, afx_decision_out* out) {
  if (!plan || !in || !out || in->n_files < 0) return fail(AFX_ERR_INVALID_ARG, "bad argument");
  const bool with_classes = in->class_signature != nullptr, with_categories = in->category_signature != nullptr;
  if (!with_classes && !with_categories) return fail(AFX_ERR_INVALID_ARG, "neither a class signature nor a category signature");
  if (with_categories && (in->n_categories < 2 || in->n_categories > afx::kDecideMaxCategories))
    return fail(AFX_ERR_INVALID_ARG, "n_categories outside 2..64");
  const size_t n = (size_t)in->n_files, k = with_categories ? (size_t)in->n_categories : 0;
  AFX_TRY(check_decision_indices(in->loop_class, in->oneshot_class, in->category_none_class, (int)k));
  if (n == 0) return AFX_OK;
  if (!in->frame_offset || !in->scalars) return fail(AFX_ERR_INVALID_ARG, "null argument");
  // the kernel follows these offsets into the peaks: they start at 0 and never step back
  if (in->frame_offset[0] != 0) return fail(AFX_ERR_INVALID_ARG, "frame_offset[0] is not 0");
  for (size_t i = 0; i < n; ++i)
    if (in->frame_offset[i + 1] < in->frame_offset[i]) return fail(AFX_ERR_INVALID_ARG, "frame_offset steps back");
  if (in->frame_offset[n] > 0 && !in->peaks) return fail(AFX_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(plan->desc.device));
  // one block of its own (this is not the crawl's path: no batch, no workspace): what goes up -- the inputs and the decision
  // block's signatures -- then what the kernel writes
  Layout layout;
  const DecideInputs inputs(layout, in);
  const DecisionBlock db(layout, n, with_classes, k);
  std::vector<char> host(layout.bytes(), 0);
  inputs.fill(host.data(), in);
  if (with_classes) std::memcpy(host.data() + db.signature[0], in->class_signature, n * 2 * sizeof(float));
  if (with_categories) std::memcpy(host.data() + db.signature[1], in->category_signature, n * k * sizeof(float));
  DeviceBlock dev;
  AFX_TRY(dev.allocate(layout.bytes(), "device memory for the decision's inputs"));
  afx::DecideArgs a = decide_args(in->n_files, k, in->loop_class, in->oneshot_class, in->use_heuristics, in->category_none_class);
  inputs.point(&a, dev.get());
  db.point(&a, dev.get());
  HIP_TRY(hipMemcpy(dev.get(), host.data(), db.class_strengths, hipMemcpyHostToDevice));
  HIP_TRY(afx::launch_class_decision(a, nullptr));
  HIP_TRY(hipMemcpy(host.data() + db.class_strengths, dev.get() + db.class_strengths, db.end - db.class_strengths, hipMemcpyDeviceToHost));   // waits for the kernel
  db.hand_out(host.data(), out);   // the signatures as they went in
  return AFX_OK;
}

}  // extern "C"
