// afec_amd/csrc/devio/afx_devio.h -- device-resident input and output: the tables and launchers of
// afx_devio.hip, shared with afx_device_io.cpp and the planning of afx_devio_plan.h.  Kept apart from afx_internal.h for
// the reason highlevel/afx_highlevel.h gives.  None of the files the device mock builds refers to these launchers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace afx {

// ---- input: the caller's device buffers into the PCM arena, one launch per batch ----
// What one workgroup copies: 256 threads x 16 samples (float: four 16-byte vectors a thread, double: eight).
constexpr int kDevioThreads = 256;
constexpr int kDevioTileSamples = 4096;

// One accepted buffer of a batch.  The arena side starts on a 16-byte boundary (afx_batch_plan.cpp: place_buffers), the
// caller's side only on an element boundary (a slice of a tensor).
struct DevioBuf {
  const void* src;      // the caller's device pointer
  int64_t dst_off;      // first sample of the buffer in the arena (a multiple of 4)
  int64_t n;            // samples to copy: the analysed prefix, exactly what the host path's transfer moves
  int32_t tile_first;   // the buffer's first tile of the launch (host-made prefix over ceil(n / kDevioTileSamples))
  int32_t pad;
};
static_assert(sizeof(DevioBuf) == 32, "table layout");

inline int64_t devio_tiles(int64_t n) { return (n + kDevioTileSamples - 1) / kDevioTileSamples; }

// copies bufs[0 .. n_bufs) into `arena` (elements of elem_bytes = 4 or 8), one workgroup per tile, on `stream`; n_tiles is
// the sum of devio_tiles() over the buffers (what tile_first was made from)
hipError_t launch_devio_gather(void* arena, const DevioBuf* bufs, int n_bufs, int64_t n_tiles, int elem_bytes, hipStream_t stream);

// ---- output: chosen series of the records into the caller's device memory, one launch per call ----
constexpr int kDevioMaxOuts = 30;      // AFX_NUM_SERIES + the magnitudes
constexpr int kDevioRows = 16;         // record rows (or padding rows) a workgroup handles
constexpr int kDevioMaxStride = 134;   // widest record: every series of afx_host.h's kFields

struct DevioSeries {
  void* dst;
  int64_t row_stride;   // elements between consecutive frames
  int64_t buf_stride;   // padded layout: elements between files (0 when packed)
  int32_t col;          // first column of the series in a record row (0 for the magnitudes)
  int32_t width;
  int32_t f32;          // 1: the destination holds floats
  int32_t from_mag;     // 1: rows of mag [F][1024] instead of rec [F][stride]
};
struct DevioExportArgs {
  const double* rec;            // [F][stride]
  const double* mag;            // [F][1024]
  const int64_t* frame_offset;  // [n_bufs + 1], device; padded layout only
  int64_t frames;               // F
  int64_t max_frames;           // padded layout: rows of a file's slot (0 when packed)
  int64_t pad_rows;             // padded layout: n_bufs * max_frames - F
  double pad_value;
  int32_t stride, n_bufs, n_outs, padded;
  uint32_t data_tiles;          // ceil(F / kDevioRows); the padding rows' tiles follow
  DevioSeries outs[kDevioMaxOuts];
};
// grid = data_tiles + ceil(pad_rows / kDevioRows)
hipError_t launch_devio_export(const DevioExportArgs& a, hipStream_t stream);

struct DevioStatsArgs {
  const double* stats;   // [n_bufs][stride][13]
  int32_t stride, n_bufs, n_outs;
  DevioSeries outs[kDevioMaxOuts];   // dst [n_bufs][width][13]; the strides are unused
};
hipError_t launch_devio_export_stats(const DevioStatsArgs& a, hipStream_t stream);
hipError_t launch_devio_frame_counts(const int64_t* frame_offset, int n_bufs, int64_t* counts, hipStream_t stream);

}  // namespace afx
