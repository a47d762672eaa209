// afec_amd/csrc/afx_high_level.cpp -- afx_batch_fetch_high_level: the model-free part of
// TSampleAnalyser::AnalyzeHighLevelDescriptors (SampleAnalyser.cpp:1234-1606) for every buffer of a batch that has run.
// One kernel launch (highlevel/afx_highlevel.hip) on the batch's stream over what the run left in device memory, one
// device-to-host transfer of its result block.  As everywhere on the host side (afx_host.h), nothing here computes a
// descriptor: the caller's peak / rms pairs go up as they are, the block comes back and is handed out by rows.
// launch_high_level_block is the launch this fetch shares with afx_batch_fetch_high_level_text (afx_high_level_text.cpp),
// which leaves the block's arrays on the device and brings their text back.

#include <cstring>

#include "afx_block.h"
#include "highlevel/afx_highlevel.h"

using namespace afx::host;

namespace afx {
namespace host {

bool has_high_level_inputs(const afx_batch* b) { return (b->mask & AFX_D_HIGH_LEVEL_INPUTS) == AFX_D_HIGH_LEVEL_INPUTS; }
const char* const kLacksHighLevelInputs = "the batch mask lacks a series the high-level descriptors read (AFX_D_HIGH_LEVEL_INPUTS)";

int enqueue_high_level(afx_batch* b, const afx_load_info* levels, const HighBlock& hb, const ResultBlock& rb) {
  afx::HighArgs a{};
  a.rec = b->d_rec;
  a.lay = b->lay;
  a.frame_offset = b->d_frame_offset;
  a.rt_scalars = b->d_rt_scalars;
  a.n_bufs = b->n_bufs;
  a.sample_rate = b->plan->desc.sample_rate;
  hb.point(&a, rb.dev, levels != nullptr);

  if (levels) {
    float* const pairs = at<float>(rb.host, hb.levels);
    for (size_t i = 0; i < rb.n; ++i) {
      pairs[2 * i] = levels[i].peak_value;
      pairs[2 * i + 1] = levels[i].rms_value;
    }
    HIP_TRY(hipMemcpyAsync(rb.dev + hb.levels, pairs, rb.n * 2 * sizeof(float), hipMemcpyHostToDevice, b->stream));
    if (rb.uploaded) HIP_TRY(hipEventRecord(rb.uploaded, b->stream));
  }
  HIP_TRY(afx::launch_high_level(a, b->stream));
  return AFX_OK;
}

int launch_high_level_block(afx_batch* b, const char* who, const afx_load_info* levels, const Layout& layout, const HighBlock& hb, ResultBlock* rb) {
  const int st = reserve_result_block(b, has_high_level_inputs(b), kLacksHighLevelInputs, who, layout, rb);
  if (st != AFX_OK || rb->n == 0) return st;
  return enqueue_high_level(b, levels, hb, *rb);
}

}  // namespace host
}  // namespace afx

extern "C" {

int afx_batch_fetch_high_level(afx_batch* b, const afx_load_info* levels, afx_high_out* out) {
  if (!b || !out) return fail(AFX_ERR_INVALID_ARG, "null argument");
  Layout layout;
  const HighBlock hb(layout, (size_t)b->n_bufs, (size_t)b->total_frames);
  ResultBlock rb;
  const int st = launch_high_level_block(b, "afx_batch_fetch_high_level", levels, layout, hb, &rb);
  if (st != AFX_OK || rb.n == 0) return st;
  HIP_TRY(download_result(b, rb, hb.scalars, hb.levels));
  hb.hand_out(rb.host, out);
  if (out->status) std::memcpy(out->status, b->buf_status.data(), rb.n * sizeof(int32_t));
  return AFX_OK;
}

}  // extern "C"
