// afec_amd/csrc/afx_device_file_io.cpp -- the per-file results into device memory of the caller's:
// afx_batch_export_file_results_device.  What afx_batch_fetch_high_level, afx_batch_fetch_classification_features and
// afx_batch_fetch_class_signature bring back to the host stays on the device: the kernels of those fetches, launched through
// the halves they share (enqueue_high_level, enqueue_features, the models' launch), write into ONE reservation of the batch's
// result block whose layout holds their blocks behind one another, and one launch of devio/afx_devio_file.hip scatters the
// block into the caller's destinations.  Everything is decided by devio/afx_devio_file_plan.h before anything is enqueued;
// here the runtime is asked what the caller's pointers are, and the record is enqueued.  This is the only translation unit
// that names launch_devio_file_export: the mock builds that list their host files by name link without it.

#include <vector>

#include "afx_decision_block.h"
#include "devio/afx_devio_file.h"
#include "devio/afx_devio_file_plan.h"

using namespace afx::host;

extern "C" {

int afx_batch_export_file_results_device(afx_batch* b, const afx_load_info* levels, const afx_model* model, const afx_file_device_out* outs,
                                         int32_t n_outs, int32_t layout, int64_t max_frames, double pad_value, void* consumer_stream) {
  if (!b) return fail(AFX_ERR_INVALID_ARG, "null batch");
  FileExportShape shape;
  shape.ran = b->ran;
  shape.n_bufs = b->n_bufs;
  shape.frame_offset = b->frame_offset.data();
  shape.has_high_level_inputs = has_high_level_inputs(b);
  shape.lacks_high_level = kLacksHighLevelInputs;
  shape.has_feature_inputs = has_feature_inputs(b);
  shape.lacks_features = kLacksFeatureInputs;
  shape.has_model = model != nullptr;
  shape.n_classes = model ? model->dev.n_classes : 0;
  FileExportPlan p = plan_file_export(shape, outs, n_outs, layout, max_frames, pad_value);
  if (p.status != AFX_OK) return fail(p.status, p.why);
  bool with_model = false;
  for (int32_t what : p.what) with_model = with_model || file_kind_needs_model(what);
  if (with_model && model->plan->desc.device != b->plan->desc.device)
    return fail(AFX_ERR_INVALID_ARG, "the model lives on another device than the batch");
  if (b->n_bufs == 0 || n_outs == 0) return AFX_OK;
  HIP_TRY(hipSetDevice(b->plan->desc.device));
  {
    std::vector<DevioAlloc> allocs(p.extent_bytes.size());
    for (size_t k = 0; k < p.extent_bytes.size(); ++k)
      if (p.extent_bytes[k] > 0) allocs[k] = devio_ask_runtime(outs[k].dst);
    const int k = file_extents_ok(outs, p.extent_bytes, allocs.data(), b->plan->desc.device);
    if (k >= 0)
      return fail(AFX_ERR_INVALID_ARG, "destination " + std::to_string(k) + " (" + file_kind_name(outs[k].what) +
                                           "): its extent does not lie inside one device allocation on the plan's device");
  }

  // one layout for the blocks of the fetches whose kernels the destinations need (a block that is not needed has no length)
  const size_t n = (size_t)b->n_bufs;
  Layout lay;
  const HighBlock hb(lay, p.needs_high_level ? n : 0, p.needs_high_level ? (size_t)b->total_frames : 0);
  const FeatureBlock fb(lay, p.needs_features ? n : 0);
  const SignatureBlock sb(lay, p.needs_signature ? n : 0, p.needs_signature ? model->dev : afx::GbdtModel{});
  ResultBlock rb;
  AFX_TRY(reserve_result_block(b, true, "", "afx_batch_export_file_results_device", lay, &rb));
  rb.uploaded = b->ws->ev_copy;

  // the features' launch waits for the batch's stream and reads the effective lengths on the host: first, while nothing of
  // this call is on the stream; from then on the host only enqueues
  if (p.needs_features) AFX_TRY(enqueue_features(b, fb, rb));
  if (p.needs_signature) {
    const afx::GbdtArgs g = gbdt_args(model, rb.dev, fb.features, b->d_frame_offset, fb.status, b->n_bufs, sb.signature, sb.iterations_used, sb.non_finite);
    HIP_TRY(afx::launch_class_signature(g, b->stream));
  }
  if (p.needs_high_level) AFX_TRY(enqueue_high_level(b, levels, hb, rb));
  // The halves above copy their small inputs (levels, effective lengths, statuses) out of rb.host on the stream, and this
  // call may return before the stream has run: the next fetch of the batch would write rb.host again.  So the host waits
  // here for the event recorded directly behind the last of those copies -- not for the kernels behind it.
  if (p.needs_features || (p.needs_high_level && levels)) HIP_TRY(wait_for_event(b->ws, rb.uploaded));

  afx::DevioFileArgs& a = p.args;
  a.frame_offset = b->d_frame_offset;
  if (model) { a.scale = model->dev.scale; a.offset = model->dev.offset; a.limits = model->dev.limits; }
  const size_t source[AFX_NUM_FILE_KINDS] = {hb.scalars, hb.signature, hb.pitch, hb.peak, fb.features, fb.features, sb.signature, fb.non_finite};
  for (size_t k = 0; k < p.what.size(); ++k) a.outs[k].src = rb.dev + source[p.what[k]];
  HIP_TRY(afx::launch_devio_file_export(a, b->stream));
  return devio_hand_over(b, consumer_stream);
}

}  // extern "C"
