// afec_amd/csrc/flac/afx_flac.h -- the FLAC decode kernels (afx_flac.hip) and their launcher, shared with
// afx_batch_create.cpp.  Kept apart from afx_internal.h for the reason highlevel/afx_highlevel.h gives.  The device mock
// does NOT implement this launcher: afx_batch_create.cpp refers to it weakly, and the plan of the raw arena
// (afx_raw_plan.h) refuses an AFX_RAW_FLAC buffer where it is absent.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "afx_flac_decode.h"

namespace afx {

constexpr int kFlacWalkThreads = 64;      // one lane per FLAC frame: serial, divergent work -- one wave per workgroup spreads it
constexpr int kFlacRestoreThreads = 64;   // one lane per kept subframe
constexpr int kFlacOutputThreads = 256;   // one lane per sample frame; a workgroup takes a tile of 256 of one file

// One FLAC file of a batch: where its pieces lie in the raw arena (byte offsets, each a multiple of 16).  The index is
// the caller's, checked on the host before it goes up (afx_raw_plan.h, flac_descriptor_ok: offsets and samples strictly rising, frames
// of at most kMaxFrameBytes and kMaxBlocksize, the sentinel equal to frames_bytes / n_samples), so every address the
// kernels form from it lies inside the file's own slots.
struct FlacFile {
  int64_t out_off;      // the decoded, interleaved native PCM: the file's raw_off
  int64_t bytes_off;    // the frames as they lie in the file
  int64_t index_off;    // afx_flac_frame[n_index + 1]
  int64_t work_off;     // int32[n_samples x stream_channels]: frame k's subframe c at (first_sample x channels + c x blocksize)
  int64_t sub_off;      // flac::Subframe[n_index x stream_channels]
  int64_t assign_off;   // int32[n_index]: the frames' channel assignments
  int64_t n_samples;
  int32_t n_index;
  int32_t bits;             // 8, 16 or 24
  int32_t stream_channels;  // 1..8; the first min(2, .) are kept
  int32_t frame_first;      // host-made prefix of n_index over the batch's FLAC files
  int32_t tile_first;       // host-made prefix of ceil(n_samples / kFlacOutputThreads)
  int32_t pad;
};
static_assert(sizeof(FlacFile) == 80, "table layout");

inline int64_t flac_output_tiles(int64_t n_samples) { return (n_samples + kFlacOutputThreads - 1) / kFlacOutputThreads; }

// decodes files[0 .. n_files) on `stream`: bit walk (n_frames lanes), restore (2 x n_frames lanes), output (n_tiles
// workgroups).  status[i] is ORed with 1 << flac::kFrame* for every failed frame of file i; the caller has zeroed it.
hipError_t launch_flac_decode(unsigned char* raw, const FlacFile* files, int n_files, int64_t n_frames, int64_t n_tiles,
                              int32_t* status, hipStream_t stream);

}  // namespace afx
