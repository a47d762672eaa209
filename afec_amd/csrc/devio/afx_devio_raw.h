// afec_amd/csrc/devio/afx_devio_raw.h -- LoadSample on device-resident audio: the tables and launchers of
// afx_devio_raw.hip, shared with afx_device_io.cpp and the planning of afx_devio_raw_plan.h.  None of the files the device
// mock builds refers to these launchers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace afx {

// ---- input: the caller's raw PCM in device memory into the raw arena, one launch per batch ----
// What one workgroup moves: kDevioRawTileFrames sample frames of one buffer.  A multiple of 16, so that a tile's bytes
// (frames x channels x 2, 3, 4 or 8) are a multiple of 16 for every format: every slot of the raw arena starts on a
// 16-byte boundary (afx_raw_plan.h), hence every tile's arena side does.
constexpr int kDevioRawThreads = 256;
constexpr int kDevioRawTileFrames = 2048;
static_assert(kDevioRawTileFrames % 16 == 0, "a tile's arena side starts on a 16-byte boundary");

// One accepted buffer of a batch (one RawPlan::Piece).  The caller's side is only sample-aligned (packed int24: any byte).
struct DevioRawBuf {
  const void* src;        // the caller's device pointer: interleaved frames, or the first plane
  int64_t dst_off;        // byte offset of the buffer's slot in the raw arena (a multiple of 16)
  int64_t n_frames;
  int64_t plane_stride;   // planar: SAMPLES between the starts of consecutive planes (0 when interleaved)
  int32_t tile_first;     // the buffer's first tile of the launch (host-made prefix over ceil(n_frames / kDevioRawTileFrames))
  int32_t channels;
  int32_t bps;            // bytes per sample: 2, 3, 4 or 8
  int32_t planar;
};
static_assert(sizeof(DevioRawBuf) == 48, "table layout");

inline int64_t devio_raw_tiles(int64_t n_frames) { return (n_frames + kDevioRawTileFrames - 1) / kDevioRawTileFrames; }

// Moves bufs[0 .. n_bufs) into `arena`, one workgroup per tile, on `stream`: exactly n_frames x channels x bps bytes from
// each slot's start.  Of the caller's memory it reads the buffers' ranges and, of interleaved buffers, the whole aligned
// 16-byte granules those ranges touch.  n_tiles is the sum of devio_raw_tiles() over the buffers.
// elementwise != 0: interleaved buffers that are not aligned like their slots go element by element instead of through
// the realigning path (tools/devio_raw_cost.py compares the two; the product passes 0).
hipError_t launch_devio_raw_gather(unsigned char* arena, const DevioRawBuf* bufs, int n_bufs, int64_t n_tiles, int elementwise,
                                   hipStream_t stream);

// ---- output: the analysed samples of every file into the caller's device memory, one launch per call ----
constexpr int kDevioSampleTile = 4096;   // elements of one row a workgroup writes (samples and padding alike)

struct DevioSamplesArgs {
  const void* pcm;       // the batch's arena
  const int64_t* rows;   // device, [3][n_bufs]: arena_off (samples, a multiple of 4), used, the bits of FinalScaling
  void* dst;
  int64_t buf_stride;    // elements between rows, >= every used[i]
  double pad_value;
  int32_t n_bufs;
  int32_t pcm_kind;      // afx::kPcm*
  int32_t f32;           // 1: the destination holds floats
  int32_t tiles_per_row; // ceil(buf_stride / kDevioSampleTile)
};
// grid = n_bufs x tiles_per_row
hipError_t launch_devio_samples(const DevioSamplesArgs& a, hipStream_t stream);
hipError_t launch_devio_sample_counts(const int64_t* rows, int n_bufs, int64_t* counts, hipStream_t stream);

}  // namespace afx
