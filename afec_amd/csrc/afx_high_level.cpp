// afec_amd/csrc/afx_high_level.cpp -- afx_batch_fetch_high_level: the model-free part of
// TSampleAnalyser::AnalyzeHighLevelDescriptors (SampleAnalyser.cpp:1234-1606) for every buffer of a batch that has run.
// One kernel launch (highlevel/afx_highlevel.hip) on the batch's stream over what the run left in device memory, one
// device-to-host transfer of its result block.  As everywhere on the host side (afx_host.h), nothing here computes a
// descriptor: the caller's peak / rms pairs go up as they are, the block comes back and is handed out by rows.

#include <cstring>

#include "afx_block.h"
#include "highlevel/afx_highlevel.h"

using namespace afx::host;

namespace {

// The high-level block: what high_level_kernel writes and the fetch brings back (scalars, signature, pitch, peak), behind
// it the caller's peak / rms pairs on their way up.
struct HighBlock {
  size_t n, frames, scalars, signature, pitch, peak, levels;
  HighBlock(Layout& l, size_t n_bufs, size_t total_frames) : n(n_bufs), frames(total_frames) {
    scalars = l.take<double>(n * afx::kHighScalars);
    signature = l.take<double>(n * afx::kHighSignatureFrames * afx::kHighSignatureBands);
    pitch = l.take<double>(frames);
    peak = l.take<double>(frames);
    levels = l.take<float>(n * 2);
  }
  void point(afx::HighArgs* a, char* base, bool with_levels) const {
    a->scalars = at<double>(base, scalars);
    a->signature = at<double>(base, signature);
    a->pitch = at<double>(base, pitch);
    a->peak = at<double>(base, peak);
    a->levels = with_levels ? at<float>(base, levels) : nullptr;
  }
  void hand_out(const char* host, afx_high_out* out) const {
    if (out->scalars) std::memcpy(out->scalars, host + scalars, n * afx::kHighScalars * sizeof(double));
    if (out->signature) std::memcpy(out->signature, host + signature, n * afx::kHighSignatureFrames * afx::kHighSignatureBands * sizeof(double));
    if (out->pitch && frames) std::memcpy(out->pitch, host + pitch, frames * sizeof(double));
    if (out->peak && frames) std::memcpy(out->peak, host + peak, frames * sizeof(double));
  }
};

}  // namespace

extern "C" {

int afx_batch_fetch_high_level(afx_batch* b, const afx_load_info* levels, afx_high_out* out) {
  if (!b || !out) return fail(AFX_ERR_INVALID_ARG, "null argument");
  Layout layout;
  const HighBlock hb(layout, (size_t)b->n_bufs, (size_t)b->total_frames);
  ResultBlock rb;
  const int st = reserve_result_block(b, (b->mask & AFX_D_HIGH_LEVEL_INPUTS) == AFX_D_HIGH_LEVEL_INPUTS,
                                      "the batch mask lacks a series the high-level descriptors read (AFX_D_HIGH_LEVEL_INPUTS)",
                                      "afx_batch_fetch_high_level", layout, &rb);
  if (st != AFX_OK || rb.n == 0) return st;

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
  }
  HIP_TRY(afx::launch_high_level(a, b->stream));
  HIP_TRY(download_result(b, rb, hb.scalars, hb.levels));
  hb.hand_out(rb.host, out);
  if (out->status) std::memcpy(out->status, b->buf_status.data(), rb.n * sizeof(int32_t));
  return AFX_OK;
}

}  // extern "C"
