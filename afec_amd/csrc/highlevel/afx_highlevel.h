// afec_amd/csrc/highlevel/afx_highlevel.h -- the high-level descriptors' kernel (afx_highlevel.hip) and its launcher, shared
// with the entry point afx_batch_fetch_high_level (afx_high_level.cpp).  Kept apart from afx_internal.h, which the run's
// translation units include and this fetch's need not reach; a device mock implements that header's launchers and the
// four of the fetches above a run (this one, classify/, gbdt/, decide/), as tests/sanitize/mock_kernels.cpp does.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../afx_internal.h"

namespace afx {

constexpr int kHighScalars = 15;          // AFX_NUM_HL_SCALARS, in the order of the AFX_HL_* indices
constexpr int kHighSignatureFrames = 64;  // kNumberOfHighLevelSpectrumBandFrames
constexpr int kHighSignatureBands = 14;   // kNumberOfHighLevelSpectrumBands

struct HighArgs {
  const double* rec;            // [F][lay.stride]: the per-frame records of the batch's last run
  RecordLayout lay;             // every series of AFX_D_HIGH_LEVEL_INPUTS is selected
  const int64_t* frame_offset;  // [n_bufs + 1], device
  const int32_t* status;        // [n_bufs], device: buf_status (a buffer with another status than 0 yields zeros)
  const double* rt_scalars;     // [n_bufs][14]: the rhythm tracker's scalars (final tempo and its confidence)
  const float* levels;          // [n_bufs][2]: TSampleData::mPeakValue, mRmsValue; nullptr: the two dB scalars are NaN
  int32_t n_bufs;
  int32_t sample_rate;
  double* scalars;              // [n_bufs][kHighScalars]
  double* signature;            // [n_bufs][64][14]
  double* pitch;                // [F]
  double* peak;                 // [F]
};
// one wave per buffer, on `stream`
hipError_t launch_high_level(const HighArgs& a, hipStream_t stream);

}  // namespace afx
