// afec_amd/csrc/devio/afx_devio_file.h -- the per-file results into device memory of the caller's: the table
// and launcher of afx_devio_file.hip, shared with afx_device_file_io.cpp and the planning of afx_devio_file_plan.h.  Kept
// apart from afx_internal.h for the reason highlevel/afx_highlevel.h gives.  None of the files the device mock builds
// refers to this launcher.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace afx {

constexpr int kDevioFileThreads = 256;
constexpr int kDevioFileMaxOuts = 16;     // AFX_FILE_MAX_OUTS: every kind as float and as double
constexpr int kDevioFileTileRows = 1024;  // frames (or padding rows) of the tracks one workgroup handles: four a lane

// how a destination's source is read
enum : int32_t {
  kFileSrcF64 = 0,         // doubles, [n_bufs][width]: the scalars, the spectrum signature, the features
  kFileSrcNormalised = 1,  // the features, each clamp(mul_rn(v, scale[j]) + offset[j], -limits[j], limits[j])
  kFileSrcF32 = 2,         // floats, [n_bufs][width]: the class signature
  kFileSrcI32 = 3,         // int32, [n_bufs]: the non-finite counts, into an int32 destination
  kFileSrcTrack = 4        // doubles, [F]: pitch and peak, one element a frame
};

struct DevioFileOut {
  void* dst;
  const void* src;      // the result block's array: the enqueuing side's to set
  int64_t row_stride;   // elements between files (tracks: between frames)
  int64_t buf_stride;   // padded tracks: elements between files (0 otherwise)
  int32_t width;        // elements of a row
  int32_t source;       // kFileSrc*
  int32_t f32;          // 1: the destination holds floats
  int32_t pad;
};
static_assert(sizeof(DevioFileOut) == 48, "table layout");

struct DevioFileArgs {
  const int64_t* frame_offset;                  // [n_bufs + 1], device: the batch's own copy
  const double *scale, *offset, *limits;        // [width of the features], device: the model's (kFileSrcNormalised only)
  int64_t frames;                               // F
  int64_t max_frames;                           // padded tracks: rows of a file's slot (0 when packed)
  int64_t pad_rows;                             // padded tracks: n_bufs * max_frames - F
  double pad_value;
  int32_t n_bufs, n_outs, padded, pad;
  uint32_t file_groups;                         // n_bufs where a per-file kind is among the destinations, else 0
  uint32_t data_tiles;                          // ceil(F / kDevioFileTileRows) where a track is, else 0; the padding rows' tiles follow
  DevioFileOut outs[kDevioFileMaxOuts];
};
// grid = file_groups + data_tiles + ceil(pad_rows / kDevioFileTileRows); nothing to do: nothing launched
hipError_t launch_devio_file_export(const DevioFileArgs& a, hipStream_t stream);

}  // namespace afx
