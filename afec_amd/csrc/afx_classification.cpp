// afec_amd/csrc/afx_classification.cpp -- afx_batch_fetch_classification_features: TSampleClassificationDescriptors
// (SampleClassificationDescriptors.cpp:395-561), the 1 680 values per file the reference's models read, for every buffer
// of a batch that has run.  One kernel launch (classify/afx_classify.hip) on the batch's stream over what the run left in
// device memory, one device-to-host transfer of its result block.  As everywhere on the host side (afx_host.h), nothing
// here computes a feature: the effective lengths go up as afx_batch_fetch hands them out, the block comes back.
// Beside it what a caller needs to read the block: the features' names and the values a missing frame is filled with.
// afx_batch_fetch_class_signature shares the launch (launch_features): the same kernel into the same block, the models'
// kernel (gbdt/afx_gbdt.hip) behind it on the same stream, and only that kernel's few bytes per file come back
// (SampleAnalyser.cpp:1075-1231).  afx_batch_fetch_class_decision goes one kernel further (decide/afx_decide.hip): what the
// reference makes of the signatures -- strengths, heuristics, classes, categories (SampleAnalyser.cpp:1097-1231) -- and
// afx_decide runs that kernel on inputs the caller holds.

#include <cmath>
#include <cstdio>
#include <cstring>

#include "afx_host.h"
#include "afx_model.h"
#include "classify/afx_classify.h"
#include "decide/afx_decide.h"
#include "gbdt/afx_gbdt.h"

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

// The feature block of one fetch in the workspace's result buffers (device and page-locked host, same layout): the features
// and the counts (what classification_features_kernel writes), behind them the effective lengths and the buffers' status
// (what goes up: effectve_length_12dB for the features, effectve_length_24dB for the class decision's heuristics), behind
// them `tail_bytes` for what the caller's own kernels write.
struct FeatureBlock {
  size_t n = 0, n_features = 0;
  size_t out_bytes = 0;     // features + counts
  size_t tail_at = 0;       // where the caller's part starts (a multiple of 8)
  char* d_block = nullptr;
  char* block = nullptr;
  const double* d_efflen24 = nullptr;   // [n], seconds
  afx::ClassifyArgs args{};
};

// Checks the batch, uploads the kernel's small inputs and launches it into the block, all on the batch's stream; nothing
// is downloaded and nothing waited for behind the launch.  fb->n == 0: an empty batch, nothing launched.
int launch_features(afx_batch* b, const char* who, size_t tail_bytes, FeatureBlock* fb) {
  // a batch keeps AFX_D_STATISTICS apart from its mask: the statistics' device block stands for the bit
  constexpr uint32_t kSeriesBits = AFX_D_CLASSIFICATION_INPUTS & ~(uint32_t)AFX_D_STATISTICS;
  if ((b->mask & kSeriesBits) != kSeriesBits || (b->n_bufs > 0 && !b->d_stats))
    return fail(AFX_ERR_INVALID_ARG, "the batch mask lacks an input of the classification features (AFX_D_CLASSIFICATION_INPUTS)");
  if (!b->ran) return fail(AFX_ERR_INVALID_ARG, std::string(who) + " before afx_batch_run");
  const size_t n = (size_t)b->n_bufs;
  if (n == 0) return AFX_OK;
  HIP_TRY(hipSetDevice(b->plan->desc.device));

  const size_t n_features = n * afx::kClassifyFeatures, n_counts = (n + 1) & ~(size_t)1;
  const size_t out_bytes = n_features * sizeof(double) + n_counts * sizeof(int32_t);
  const size_t in_bytes = 2 * n * sizeof(double) + n * sizeof(int32_t);
  const size_t tail_at = (out_bytes + in_bytes + 7) & ~(size_t)7;
  HIP_TRY(ws_reserve(b->plan, b->ws->high, tail_at + tail_bytes));
  HIP_TRY(ws_result_pin_reserve(b->ws, tail_at + tail_bytes));
  char* const d_block = (char*)b->ws->high.p;
  char* const block = (char*)b->ws->h_high;

  HIP_TRY(hipStreamSynchronize(b->stream));   // the run's effective-length kernel has written d_efflen
  {
    std::vector<double> seconds(n * 3);
    const int st = effective_length_seconds(b, seconds.data());
    if (st != AFX_OK) return st;
    double* const up = (double*)(block + out_bytes);
    for (size_t i = 0; i < n; ++i) {
      up[i] = seconds[i * 3 + 2];
      up[n + i] = seconds[i * 3 + 1];
    }
    std::memcpy(up + 2 * n, b->buf_status.data(), n * sizeof(int32_t));
  }
  afx::ClassifyArgs& a = fb->args;
  a = afx::ClassifyArgs{};
  a.rec = b->d_rec;
  a.lay = b->lay;
  a.frame_offset = b->d_frame_offset;
  a.stats = b->d_stats;
  a.rt_scalars = b->d_rt_scalars;
  a.efflen12 = (const double*)(d_block + out_bytes);
  a.status = (const int32_t*)(a.efflen12 + 2 * n);
  a.n_bufs = b->n_bufs;
  a.features = (double*)d_block;
  a.non_finite = (int32_t*)(a.features + n_features);

  HIP_TRY(hipMemcpyAsync(d_block + out_bytes, block + out_bytes, in_bytes, hipMemcpyHostToDevice, b->stream));
  HIP_TRY(afx::launch_classification_features(a, b->stream));
  fb->n = n;
  fb->n_features = n_features;
  fb->out_bytes = out_bytes;
  fb->tail_at = tail_at;
  fb->d_block = d_block;
  fb->block = block;
  fb->d_efflen24 = a.efflen12 + n;
  return AFX_OK;
}


// ---- the class decision ----

size_t round8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

// Where the decision kernel's results lie in one block, in the order of their alignment: what afx_decision_out names but
// the signatures.  The same layout on the device and on the host.
struct DecisionBlock {
  size_t class_strengths, confidences, category_strengths, classes, categories, flags, non_finite, bytes;
  DecisionBlock(size_t n, size_t k) {
    class_strengths = 0;
    confidences = class_strengths + n * 2 * sizeof(double);
    category_strengths = confidences + n * 2 * sizeof(double);
    classes = category_strengths + n * k * sizeof(double);
    categories = classes + n * 2 * sizeof(int32_t);
    flags = categories + n * k * sizeof(int32_t);
    non_finite = flags + n * sizeof(int32_t);
    bytes = round8(non_finite + n * sizeof(int32_t));
  }
  void point(afx::DecideArgs* a, char* d) const {
    a->class_strengths = (double*)(d + class_strengths);
    a->confidences = (double*)(d + confidences);
    a->category_strengths = (double*)(d + category_strengths);
    a->classes = (int32_t*)(d + classes);
    a->categories = (int32_t*)(d + categories);
    a->flags = (int32_t*)(d + flags);
    a->non_finite = (int32_t*)(d + non_finite);
  }
  void hand_out(const char* h, size_t n, size_t k, bool with_classes, afx_decision_out* out) const {
    // without a class model the reference's lists are empty: nothing is written for them
    if (out->class_strengths && with_classes) std::memcpy(out->class_strengths, h + class_strengths, n * 2 * sizeof(double));
    if (out->classes && with_classes) std::memcpy(out->classes, h + classes, n * 2 * sizeof(int32_t));
    if (out->category_strengths && k) std::memcpy(out->category_strengths, h + category_strengths, n * k * sizeof(double));
    if (out->categories && k) std::memcpy(out->categories, h + categories, n * k * sizeof(int32_t));
    if (out->confidences) std::memcpy(out->confidences, h + confidences, n * 2 * sizeof(double));
    if (out->flags) std::memcpy(out->flags, h + flags, n * sizeof(int32_t));
    if (out->non_finite) std::memcpy(out->non_finite, h + non_finite, n * sizeof(int32_t));
  }
};

// the indices a decision names: AFX_OK or why not
int check_decision_indices(int loop_class, int oneshot_class, int none_class, int n_categories) {
  if (loop_class < 0 || loop_class > 1 || oneshot_class < 0 || oneshot_class > 1 || loop_class == oneshot_class)
    return fail(AFX_ERR_INVALID_ARG, "loop_class and oneshot_class are 0 and 1 in either order");
  if (none_class < -1 || none_class >= n_categories) return fail(AFX_ERR_INVALID_ARG, "category_none_class names no class of the category model");
  return AFX_OK;
}

double silence_floor_24db() { return std::exp(-24.0 * (std::log(10.0) / 20.0)); }   // DbToLin(-24), AudioMath.inl:108-123

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
  FeatureBlock fb;
  const int st = launch_features(b, "afx_batch_fetch_classification_features", 0, &fb);
  if (st != AFX_OK || fb.n == 0) return st;
  {
    const Download item{fb.block, fb.d_block, fb.out_bytes};
    HIP_TRY(download_through_plan(b, &item, 1));   // waits for the batch's stream first, then for the transfer
  }
  std::memcpy(features, fb.block, fb.n_features * sizeof(double));
  if (non_finite) std::memcpy(non_finite, fb.block + fb.n_features * sizeof(double), fb.n * sizeof(int32_t));
  if (status) std::memcpy(status, b->buf_status.data(), fb.n * sizeof(int32_t));
  return AFX_OK;
}

int afx_batch_fetch_class_signature(afx_batch* b, const afx_model* model, float* signature, int32_t* iterations_used, int32_t* nonfinite) {
  if (!b || !model || !signature) return fail(AFX_ERR_INVALID_ARG, "null argument");
  if (model->plan->desc.device != b->plan->desc.device) return fail(AFX_ERR_INVALID_ARG, "the model lives on another device than the batch");
  // behind the feature block: the signatures, the iterations used, the counts (what comes back)
  const size_t n = (size_t)b->n_bufs, n_classes = (size_t)model->dev.n_classes, n_models = (size_t)model->dev.n_models;
  const size_t sig_bytes = (n * n_classes * sizeof(float) + 7) & ~(size_t)7;
  const size_t tail_bytes = sig_bytes + (n * n_models + n) * sizeof(int32_t);
  FeatureBlock fb;
  const int st = launch_features(b, "afx_batch_fetch_class_signature", tail_bytes, &fb);
  if (st != AFX_OK || fb.n == 0) return st;
  afx::GbdtArgs g{};
  g.model = model->dev;
  g.features = fb.args.features;
  g.frame_offset = b->d_frame_offset;
  g.status = fb.args.status;
  g.n_bufs = b->n_bufs;
  g.signature = (float*)(fb.d_block + fb.tail_at);
  g.iterations_used = (int32_t*)(fb.d_block + fb.tail_at + sig_bytes);
  g.non_finite = g.iterations_used + n * n_models;
  HIP_TRY(afx::launch_class_signature(g, b->stream));
  char* const tail = fb.block + fb.tail_at;
  {
    const Download item{tail, fb.d_block + fb.tail_at, tail_bytes};
    HIP_TRY(download_through_plan(b, &item, 1));
  }
  std::memcpy(signature, tail, n * n_classes * sizeof(float));
  if (iterations_used) std::memcpy(iterations_used, tail + sig_bytes, n * n_models * sizeof(int32_t));
  if (nonfinite) std::memcpy(nonfinite, tail + sig_bytes + n * n_models * sizeof(int32_t), n * sizeof(int32_t));
  return AFX_OK;
}

int afx_model_evaluate_features(const afx_model* model, const double* features, int32_t n_vectors, float* signature,
                                int32_t* iterations_used, int32_t* nonfinite) {
  if (!model || n_vectors < 0 || (n_vectors > 0 && (!features || !signature))) return fail(AFX_ERR_INVALID_ARG, "bad argument");
  if (n_vectors == 0) return AFX_OK;
  HIP_TRY(hipSetDevice(model->plan->desc.device));
  // one block of its own (this is not the crawl's path: no batch, no workspace): the vectors, a frame table that gives
  // every vector one frame, a status of zeros; behind them what the kernel writes
  const size_t n = (size_t)n_vectors, n_classes = (size_t)model->dev.n_classes, n_models = (size_t)model->dev.n_models;
  const size_t feature_bytes = n * afx::kGbdtFeatures * sizeof(double), offset_bytes = (n + 1) * sizeof(int64_t);
  const size_t status_bytes = (n * sizeof(int32_t) + 7) & ~(size_t)7;
  const size_t sig_bytes = (n * n_classes * sizeof(float) + 7) & ~(size_t)7;
  const size_t in_bytes = feature_bytes + offset_bytes + status_bytes;
  const size_t out_bytes = sig_bytes + (n * n_models + n) * sizeof(int32_t);
  std::vector<char> host(offset_bytes + status_bytes + out_bytes, 0);
  for (size_t i = 0; i <= n; ++i) ((int64_t*)host.data())[i] = (int64_t)i;
  char* d_block = nullptr;
  {
    const hipError_t e = hipMalloc((void**)&d_block, in_bytes + out_bytes);
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      return fail(AFX_ERR_OUT_OF_MEMORY, "device memory for the feature vectors");
    }
    HIP_TRY(e);
  }
  afx::GbdtArgs g{};
  g.model = model->dev;
  g.features = (const double*)d_block;
  g.frame_offset = (const int64_t*)(d_block + feature_bytes);
  g.status = (const int32_t*)(d_block + feature_bytes + offset_bytes);
  g.n_bufs = n_vectors;
  g.signature = (float*)(d_block + in_bytes);
  g.iterations_used = (int32_t*)(d_block + in_bytes + sig_bytes);
  g.non_finite = g.iterations_used + n * n_models;
  hipError_t e = hipMemcpy(d_block, features, feature_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_block + feature_bytes, host.data(), offset_bytes + status_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = afx::launch_class_signature(g, nullptr);
  char* const out = host.data() + offset_bytes + status_bytes;
  if (e == hipSuccess) e = hipMemcpy(out, d_block + in_bytes, out_bytes, hipMemcpyDeviceToHost);   // waits for the kernel
  (void)hipFree(d_block);
  HIP_TRY(e);
  std::memcpy(signature, out, n * n_classes * sizeof(float));
  if (iterations_used) std::memcpy(iterations_used, out + sig_bytes, n * n_models * sizeof(int32_t));
  if (nonfinite) std::memcpy(nonfinite, out + sig_bytes + n * n_models * sizeof(int32_t), n * sizeof(int32_t));
  return AFX_OK;
}

int afx_batch_fetch_class_decision(afx_batch* b, const afx_decision_desc* desc, afx_decision_out* out) {
  if (!b || !desc || !out) return fail(AFX_ERR_INVALID_ARG, "null argument");
  const afx_model* const cm = desc->class_model;
  const afx_model* const gm = desc->category_model;
  if (!cm && !gm) return fail(AFX_ERR_INVALID_ARG, "neither a class model nor a category model");
  for (const afx_model* m : {cm, gm})
    if (m && m->plan->desc.device != b->plan->desc.device) return fail(AFX_ERR_INVALID_ARG, "a model lives on another device than the batch");
  if (cm && cm->dev.n_classes != afx::kDecideClasses)
    return fail(AFX_ERR_UNSUPPORTED, "the class model has to have the two classes \"Loop\" and \"OneShot\"");
  const size_t k = gm ? (size_t)gm->dev.n_classes : 0;
  {
    const int st = check_decision_indices(desc->loop_class, desc->oneshot_class, desc->category_none_class, (int)k);
    if (st != AFX_OK) return st;
  }
  if (!(b->mask & AFX_D_AMPLITUDE_PEAK)) return fail(AFX_ERR_INVALID_ARG, "the batch mask lacks AFX_D_AMPLITUDE_PEAK (AFX_D_CLASS_DECISION_INPUTS)");

  // behind the feature block: what the models' kernel writes and only the decision kernel reads (iterations used, counts),
  // then what comes back: the signatures and the decision's block
  const size_t n = (size_t)b->n_bufs;
  const size_t class_models = cm ? (size_t)cm->dev.n_models : 0, category_models = gm ? (size_t)gm->dev.n_models : 0;
  const size_t scratch_bytes = round8((n * (class_models + category_models) + 2 * n) * sizeof(int32_t));
  const size_t class_sig_bytes = round8(cm ? n * 2 * sizeof(float) : 0), category_sig_bytes = round8(n * k * sizeof(float));
  const DecisionBlock db(n, k);
  const size_t back_bytes = class_sig_bytes + category_sig_bytes + db.bytes;
  FeatureBlock fb;
  const int st = launch_features(b, "afx_batch_fetch_class_decision", scratch_bytes + back_bytes, &fb);
  if (st != AFX_OK || fb.n == 0) return st;
  char* const d_scratch = fb.d_block + fb.tail_at;
  char* const d_back = d_scratch + scratch_bytes;
  int32_t* const d_class_used = (int32_t*)d_scratch;
  int32_t* const d_category_used = d_class_used + n * class_models;
  int32_t* const d_class_bad = d_category_used + n * category_models;
  int32_t* const d_category_bad = d_class_bad + n;
  float* const d_class_sig = (float*)d_back;
  float* const d_category_sig = (float*)(d_back + class_sig_bytes);

  afx::GbdtArgs g{};
  g.features = fb.args.features;
  g.frame_offset = b->d_frame_offset;
  g.status = fb.args.status;
  g.n_bufs = b->n_bufs;
  if (cm) {
    g.model = cm->dev;
    g.signature = d_class_sig;
    g.iterations_used = d_class_used;
    g.non_finite = d_class_bad;
    HIP_TRY(afx::launch_class_signature(g, b->stream));
  }
  if (gm) {
    g.model = gm->dev;
    g.signature = d_category_sig;
    g.iterations_used = d_category_used;
    g.non_finite = d_category_bad;
    HIP_TRY(afx::launch_class_signature(g, b->stream));
  }

  afx::DecideArgs a{};
  a.class_signature = cm ? d_class_sig : nullptr;
  a.category_signature = gm ? d_category_sig : nullptr;
  a.n_categories = (int32_t)k;
  a.loop_class = desc->loop_class;
  a.oneshot_class = desc->oneshot_class;
  a.use_heuristics = desc->use_heuristics != 0;
  a.none_category = desc->category_none_class;
  a.peak = b->d_rec + b->lay.amp_peak;
  a.peak_stride = b->lay.stride;
  a.frame_offset = b->d_frame_offset;
  a.efflen24 = {fb.d_efflen24, 1};
  a.onset_count = {b->d_rt_scalars + AFX_R_PERCUSSIVE_ONSET_COUNT, 14};
  a.percussive_confidence = {b->d_rt_scalars + AFX_R_PERCUSSIVE_TEMPO_CONFIDENCE, 14};
  a.complex_confidence = {b->d_rt_scalars + AFX_R_COMPLEX_TEMPO_CONFIDENCE, 14};
  a.flux_mean = {b->d_stats + (size_t)b->lay.flux * 13 + AFX_S_MEAN, (int64_t)b->lay.stride * 13};
  a.status = fb.args.status;
  a.non_finite_in = cm ? d_class_bad : d_category_bad;   // the same features: the same count from either model's kernel
  a.silence_floor = silence_floor_24db();
  a.n_files = b->n_bufs;
  db.point(&a, d_back + class_sig_bytes + category_sig_bytes);
  HIP_TRY(afx::launch_class_decision(a, b->stream));

  char* const back = fb.block + fb.tail_at + scratch_bytes;
  {
    const Download item{back, d_back, back_bytes};
    HIP_TRY(download_through_plan(b, &item, 1));
  }
  if (out->class_signature && cm) std::memcpy(out->class_signature, back, n * 2 * sizeof(float));
  if (out->category_signature && gm) std::memcpy(out->category_signature, back + class_sig_bytes, n * k * sizeof(float));
  db.hand_out(back + class_sig_bytes + category_sig_bytes, n, k, cm != nullptr, out);
  return AFX_OK;
}

int afx_decide(const afx_plan* plan, const afx_decision_in* in, afx_decision_out* out) {
  if (!plan || !in || !out || in->n_files < 0) return fail(AFX_ERR_INVALID_ARG, "bad argument");
  const bool with_classes = in->class_signature != nullptr, with_categories = in->category_signature != nullptr;
  if (!with_classes && !with_categories) return fail(AFX_ERR_INVALID_ARG, "neither a class signature nor a category signature");
  if (with_categories && (in->n_categories < 2 || in->n_categories > afx::kDecideMaxCategories))
    return fail(AFX_ERR_INVALID_ARG, "n_categories outside 2..64");
  const size_t n = (size_t)in->n_files, k = with_categories ? (size_t)in->n_categories : 0;
  {
    const int st = check_decision_indices(in->loop_class, in->oneshot_class, in->category_none_class, (int)k);
    if (st != AFX_OK) return st;
  }
  if (n == 0) return AFX_OK;
  if (!in->frame_offset || !in->scalars) return fail(AFX_ERR_INVALID_ARG, "null argument");
  // the kernel follows these offsets into the peaks: they start at 0 and never step back
  if (in->frame_offset[0] != 0) return fail(AFX_ERR_INVALID_ARG, "frame_offset[0] is not 0");
  for (size_t i = 0; i < n; ++i)
    if (in->frame_offset[i + 1] < in->frame_offset[i]) return fail(AFX_ERR_INVALID_ARG, "frame_offset steps back");
  const size_t frames = (size_t)in->frame_offset[n];
  if (frames > 0 && !in->peaks) return fail(AFX_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(plan->desc.device));

  // one block of its own (this is not the crawl's path: no batch, no workspace): what goes up, then what the kernel writes
  const size_t peaks_at = 0, scalars_at = peaks_at + frames * sizeof(double), offsets_at = scalars_at + n * AFX_NUM_DECISION_SCALARS * sizeof(double);
  const size_t class_sig_at = offsets_at + (n + 1) * sizeof(int64_t), category_sig_at = class_sig_at + round8(n * 2 * sizeof(float));
  const size_t bad_at = category_sig_at + round8(n * k * sizeof(float));
  const size_t in_bytes = bad_at + round8(n * sizeof(int32_t));
  const DecisionBlock db(n, k);
  std::vector<char> host(in_bytes + db.bytes, 0);
  if (frames) std::memcpy(host.data() + peaks_at, in->peaks, frames * sizeof(double));
  std::memcpy(host.data() + scalars_at, in->scalars, n * AFX_NUM_DECISION_SCALARS * sizeof(double));
  std::memcpy(host.data() + offsets_at, in->frame_offset, (n + 1) * sizeof(int64_t));
  if (with_classes) std::memcpy(host.data() + class_sig_at, in->class_signature, n * 2 * sizeof(float));
  if (with_categories) std::memcpy(host.data() + category_sig_at, in->category_signature, n * k * sizeof(float));
  if (in->non_finite) std::memcpy(host.data() + bad_at, in->non_finite, n * sizeof(int32_t));
  char* d_block = nullptr;
  {
    const hipError_t e = hipMalloc((void**)&d_block, in_bytes + db.bytes);
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      return fail(AFX_ERR_OUT_OF_MEMORY, "device memory for the decision's inputs");
    }
    HIP_TRY(e);
  }
  const double* const d_scalars = (const double*)(d_block + scalars_at);
  afx::DecideArgs a{};
  a.class_signature = with_classes ? (const float*)(d_block + class_sig_at) : nullptr;
  a.category_signature = with_categories ? (const float*)(d_block + category_sig_at) : nullptr;
  a.n_categories = (int32_t)k;
  a.loop_class = in->loop_class;
  a.oneshot_class = in->oneshot_class;
  a.use_heuristics = in->use_heuristics != 0;
  a.none_category = in->category_none_class;
  a.peak = (const double*)(d_block + peaks_at);
  a.peak_stride = 1;
  a.frame_offset = (const int64_t*)(d_block + offsets_at);
  a.efflen24 = {d_scalars + AFX_DS_EFFECTIVE_LENGTH_24DB, AFX_NUM_DECISION_SCALARS};
  a.onset_count = {d_scalars + AFX_DS_PERCUSSIVE_ONSET_COUNT, AFX_NUM_DECISION_SCALARS};
  a.percussive_confidence = {d_scalars + AFX_DS_PERCUSSIVE_TEMPO_CONFIDENCE, AFX_NUM_DECISION_SCALARS};
  a.complex_confidence = {d_scalars + AFX_DS_COMPLEX_TEMPO_CONFIDENCE, AFX_NUM_DECISION_SCALARS};
  a.flux_mean = {d_scalars + AFX_DS_SPECTRAL_FLUX_MEAN, AFX_NUM_DECISION_SCALARS};
  a.status = nullptr;
  a.non_finite_in = (const int32_t*)(d_block + bad_at);
  a.silence_floor = silence_floor_24db();
  a.n_files = in->n_files;
  db.point(&a, d_block + in_bytes);
  hipError_t e = hipMemcpy(d_block, host.data(), in_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = afx::launch_class_decision(a, nullptr);
  if (e == hipSuccess) e = hipMemcpy(host.data() + in_bytes, d_block + in_bytes, db.bytes, hipMemcpyDeviceToHost);   // waits for the kernel
  (void)hipFree(d_block);
  HIP_TRY(e);
  if (out->class_signature && with_classes) std::memcpy(out->class_signature, in->class_signature, n * 2 * sizeof(float));
  if (out->category_signature && with_categories) std::memcpy(out->category_signature, in->category_signature, n * k * sizeof(float));
  db.hand_out(host.data() + in_bytes, n, k, with_classes, out);
  return AFX_OK;
}

}  // extern "C"
