// afec_amd/csrc/devio/afx_devio_file.hip -- the per-file results into device memory of the caller's.  One
// kernel, one launch per call, a pure memory mover but for the features' normalisation:
//
//   devio_file_export_kernel   workgroups [0, file_groups): one file each, every per-file destination's row of it, the
//                              lanes striding along the row (two elements a lane where the source row starts on a 16-byte
//                              boundary and the destination row on one of its own two elements, element by element otherwise);
//                              the workgroups behind them: kDevioFileTileRows frames of the tracks each, then the padding
//                              rows of the padded layout, mapped as devio_export_kernel maps them
//
// Every address is formed from a table the host has checked against the extents of the allocations involved
// (afx_devio_file_plan.h); nothing here reads or writes beyond what those checks cover.

#include <hip/hip_runtime.h>

#include "../afx_internal.h"
#include "../afx_device.h"
#include "afx_devio_file.h"

namespace afx {
namespace {

// what class_signature_kernel makes of feature j before it walks the trees (gbdt/afx_gbdt.hip): the product rounded on
// its own, the same two comparisons in the same order
__device__ __forceinline__ double normalised(double v, double scale, double offset, double limit) {
  const double hi = limit, lo = -limit;
  double y = mul_rn(v, scale) + offset;
  y = (hi < y) ? hi : y;    // std::min(max, y)
  y = (lo < y) ? y : lo;    // std::max(min, y)
  return y;
}

__device__ __forceinline__ bool aligned(const void* p, unsigned bytes) { return (((uintptr_t)p) & (bytes - 1)) == 0; }

// One row of doubles at `src` into the destination's row at element `at`.  Two elements a lane and round: one 16-byte load,
// one 16-byte store of doubles or one 8-byte store of floats (a wave's stores are still back to back; four elements a lane
// for a float4 would keep sixteen doubles of the normalisation's operands in flight and cost the eighth wave of a SIMD).
__device__ __forceinline__ void copy_row(const DevioFileArgs& a, const DevioFileOut& o, const double* __restrict__ src, int64_t at, int t) {
  const bool norm = o.source == kFileSrcNormalised;
  const int w = o.width;
  float* const dst32 = reinterpret_cast<float*>(o.dst) + at;
  double* const dst64 = reinterpret_cast<double*>(o.dst) + at;
  int done = 0;
  if (aligned(src, 16) && (o.f32 ? aligned(dst32, 8) : aligned(dst64, 16)) &&
      (!norm || (aligned(a.scale, 16) && aligned(a.offset, 16) && aligned(a.limits, 16)))) {
    const int vectors = w >> 1;
    for (int v = t; v < vectors; v += kDevioFileThreads) {
      double2 x = reinterpret_cast<const double2*>(src)[v];
      if (norm) {
        const double2 s = reinterpret_cast<const double2*>(a.scale)[v], b = reinterpret_cast<const double2*>(a.offset)[v],
                      l = reinterpret_cast<const double2*>(a.limits)[v];
        x.x = normalised(x.x, s.x, b.x, l.x);
        x.y = normalised(x.y, s.y, b.y, l.y);
      }
      if (o.f32) reinterpret_cast<float2*>(dst32)[v] = make_float2((float)x.x, (float)x.y);   // round to nearest even
      else reinterpret_cast<double2*>(dst64)[v] = x;
    }
    done = vectors << 1;
  }
  // a row that starts between the boundaries, and the element behind the last whole vector: element by element
  for (int j = done + t; j < w; j += kDevioFileThreads) {
    double v = src[j];
    if (norm) v = normalised(v, a.scale[j], a.offset[j], a.limits[j]);
    if (o.f32) dst32[j] = (float)v;
    else dst64[j] = v;
  }
}

__device__ __forceinline__ void store_track(const DevioFileOut& o, int64_t at, double v) {
  if (o.f32) reinterpret_cast<float*>(o.dst)[at] = (float)v;   // round to nearest even
  else reinterpret_cast<double*>(o.dst)[at] = v;
}

__global__ __launch_bounds__(kDevioFileThreads) void devio_file_export_kernel(const DevioFileArgs a) {
  const int t = (int)threadIdx.x;
  if (blockIdx.x < a.file_groups) {
    const int64_t file = blockIdx.x;
    for (int k = 0; k < a.n_outs; ++k) {
      const DevioFileOut& o = a.outs[k];
      const int64_t at = file * o.row_stride;
      if (o.source == kFileSrcF64 || o.source == kFileSrcNormalised) {
        copy_row(a, o, reinterpret_cast<const double*>(o.src) + file * o.width, at, t);
      } else if (o.source == kFileSrcF32) {   // at most 64 floats: element by element, widened exactly
        const float* src = reinterpret_cast<const float*>(o.src) + file * o.width;
        for (int j = t; j < o.width; j += kDevioFileThreads) {
          if (o.f32) reinterpret_cast<float*>(o.dst)[at + j] = src[j];
          else reinterpret_cast<double*>(o.dst)[at + j] = (double)src[j];
        }
      } else if (o.source == kFileSrcI32) {
        if (t == 0) reinterpret_cast<int32_t*>(o.dst)[at] = reinterpret_cast<const int32_t*>(o.src)[file];
      }
    }
    return;
  }
  // the tracks: a tile of frames, or of padding rows
  const uint32_t tile = blockIdx.x - a.file_groups;
  const bool pad_tile = tile >= a.data_tiles;
  const int64_t row0 = (int64_t)(pad_tile ? tile - a.data_tiles : tile) * kDevioFileTileRows;
  const int64_t rows_left = (pad_tile ? a.pad_rows : a.frames) - row0;
  const int rows = (int)(rows_left < kDevioFileTileRows ? rows_left : kDevioFileTileRows);
  for (int i = t; i < rows; i += kDevioFileThreads) {
    const int64_t r = row0 + i;
    int64_t buf = 0, local = r;
    if (a.padded) {
      // data rows: the last file whose first frame is not behind r (of files without frames in front of it, the last one:
      // the one that holds r).  Padding rows: the same search over the files' first padding rows, b * max_frames - first frame.
      int lo = 0, hi = a.n_bufs - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int64_t key = pad_tile ? (int64_t)mid * a.max_frames - a.frame_offset[mid] : a.frame_offset[mid];
        if (key <= r) lo = mid; else hi = mid - 1;
      }
      const int64_t f0 = a.frame_offset[lo], f1 = a.frame_offset[lo + 1];
      buf = lo;
      local = pad_tile ? (f1 - f0) + (r - ((int64_t)lo * a.max_frames - f0)) : r - f0;
    }
    for (int k = 0; k < a.n_outs; ++k) {
      const DevioFileOut& o = a.outs[k];
      if (o.source != kFileSrcTrack) continue;
      store_track(o, buf * o.buf_stride + local * o.row_stride, pad_tile ? a.pad_value : reinterpret_cast<const double*>(o.src)[r]);
    }
  }
}

}  // namespace

hipError_t launch_devio_file_export(const DevioFileArgs& a, hipStream_t stream) {
  const int64_t pad_tiles = (a.pad_rows + kDevioFileTileRows - 1) / kDevioFileTileRows;
  const int64_t grid = (int64_t)a.file_groups + (int64_t)a.data_tiles + pad_tiles;
  if (a.n_outs <= 0 || a.n_bufs <= 0 || grid <= 0) return hipSuccess;
  if (a.n_outs > kDevioFileMaxOuts || grid > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(devio_file_export_kernel, dim3((unsigned)grid), dim3(kDevioFileThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace afx
