// afec_amd/csrc/afx_high_level.cpp -- afx_batch_fetch_high_level: the model-free part of
// TSampleAnalyser::AnalyzeHighLevelDescriptors (SampleAnalyser.cpp:1234-1606) for every buffer of a batch that has run.
// One kernel launch (highlevel/afx_highlevel.hip) on the batch's stream over what the run left in device memory, one
// device-to-host transfer of its result block.  As everywhere on the host side (afx_host.h), nothing here computes a
// descriptor: the caller's peak / rms pairs go up as they are, the block comes back and is handed out by rows.

#include <cstring>

#include "afx_host.h"
#include "highlevel/afx_highlevel.h"

using namespace afx::host;

extern "C" {

int afx_batch_fetch_high_level(afx_batch* b, const afx_load_info* levels, afx_high_out* out) {
  if (!b || !out) return fail(AFX_ERR_INVALID_ARG, "null argument");
  if ((b->mask & AFX_D_HIGH_LEVEL_INPUTS) != AFX_D_HIGH_LEVEL_INPUTS)
    return fail(AFX_ERR_INVALID_ARG, "the batch mask lacks a series the high-level descriptors read (AFX_D_HIGH_LEVEL_INPUTS)");
  if (!b->ran) return fail(AFX_ERR_INVALID_ARG, "afx_batch_fetch_high_level before afx_batch_run");
  const size_t n = (size_t)b->n_bufs, frames = (size_t)b->total_frames;
  if (n == 0) return AFX_OK;
  HIP_TRY(hipSetDevice(b->plan->desc.device));

  // the result block: scalars, signature, pitch, peak (doubles), and behind them the uploaded peak / rms pairs (floats)
  const size_t n_scalars = n * afx::kHighScalars, n_signature = n * afx::kHighSignatureFrames * afx::kHighSignatureBands;
  const size_t doubles = n_scalars + n_signature + 2 * frames;
  const size_t block_bytes = doubles * sizeof(double), level_bytes = n * 2 * sizeof(float);
  HIP_TRY(ws_reserve(b->plan, b->ws->high, block_bytes + level_bytes));
  HIP_TRY(ws_result_pin_reserve(b->ws, block_bytes + level_bytes));
  double* const d_block = (double*)b->ws->high.p;
  float* const d_levels = (float*)(d_block + doubles);

  double* const block = (double*)b->ws->h_high;
  float* const pairs = (float*)(block + doubles);
  if (levels) {
    for (size_t i = 0; i < n; ++i) {
      pairs[2 * i] = levels[i].peak_value;
      pairs[2 * i + 1] = levels[i].rms_value;
    }
  }
  afx::HighArgs a{};
  a.rec = b->d_rec;
  a.lay = b->lay;
  a.frame_offset = b->d_frame_offset;
  a.rt_scalars = b->d_rt_scalars;
  a.levels = levels ? d_levels : nullptr;
  a.n_bufs = b->n_bufs;
  a.sample_rate = b->plan->desc.sample_rate;
  a.scalars = d_block;
  a.signature = a.scalars + n_scalars;
  a.pitch = a.signature + n_signature;
  a.peak = a.pitch + frames;

  if (levels) HIP_TRY(hipMemcpyAsync(d_levels, pairs, level_bytes, hipMemcpyHostToDevice, b->stream));
  HIP_TRY(afx::launch_high_level(a, b->stream));
  {
    const Download item{block, d_block, block_bytes};
    HIP_TRY(download_through_plan(b, &item, 1));   // waits for the batch's stream first, then for the transfer
  }

  const double* src = block;
  if (out->scalars) std::memcpy(out->scalars, src, n_scalars * sizeof(double));
  src += n_scalars;
  if (out->signature) std::memcpy(out->signature, src, n_signature * sizeof(double));
  src += n_signature;
  if (out->pitch && frames) std::memcpy(out->pitch, src, frames * sizeof(double));
  src += frames;
  if (out->peak && frames) std::memcpy(out->peak, src, frames * sizeof(double));
  if (out->status) std::memcpy(out->status, b->buf_status.data(), n * sizeof(int32_t));
  return AFX_OK;
}

}  // extern "C"
