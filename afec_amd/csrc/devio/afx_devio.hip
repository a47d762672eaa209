// afec_amd/csrc/devio/afx_devio.hip -- device-resident input and output.  Pure memory movers:
//
//   devio_gather_kernel   the caller's device buffers into the PCM arena, one workgroup per tile of kDevioTileSamples
//                         samples of one buffer: exactly the bytes the host path's transfers write
//   devio_export_kernel   kDevioRows record rows per workgroup, staged once through LDS (one coalesced read of the rows),
//                         then every requested series scattered to its destination, as double or float; the padding rows
//                         of the padded layout are further workgroups of the same launch
//   devio_stats_kernel    the per-file statistics of chosen series, one workgroup per file
//   devio_counts_kernel   frames per file
//
// Every address is formed from tables the host has checked against the extents of the allocations involved
// (afx_devio_plan.h); nothing here reads or writes beyond what those checks cover.

#include <hip/hip_runtime.h>

#include "afx_devio.h"

namespace afx {
namespace {

// the last buffer whose first tile is not behind `tile` (every buffer of the table has at least one tile)
__device__ __forceinline__ int buf_of_tile(const DevioBuf* __restrict__ bufs, int n_bufs, int tile) {
  int lo = 0, hi = n_bufs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (bufs[mid].tile_first <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kDevioThreads) void devio_gather_kernel(unsigned char* __restrict__ arena, const DevioBuf* __restrict__ bufs,
                                                                     int n_bufs, int wide) {
  const int tile = (int)blockIdx.x;
  const DevioBuf& f = bufs[buf_of_tile(bufs, n_bufs, tile)];
  const int64_t first = (int64_t)(tile - f.tile_first) * kDevioTileSamples;
  const int64_t left = f.n - first;
  if (left <= 0) return;
  const int count = (int)(left < kDevioTileSamples ? left : kDevioTileSamples);
  const int shift = wide ? 3 : 2;
  const unsigned char* src = (const unsigned char*)f.src + (first << shift);
  unsigned char* dst = arena + ((f.dst_off + first) << shift);   // a multiple of 16: dst_off is one of 4 samples, a tile of 4 096
  int done = 0;
  if (((uintptr_t)src & 15) == 0) {
    // aligned alike: 16-byte vectors, a workgroup's accesses back to back
    const int vectors = count >> (4 - shift);
    for (int v = (int)threadIdx.x; v < vectors; v += kDevioThreads)
      reinterpret_cast<uint4*>(dst)[v] = reinterpret_cast<const uint4*>(src)[v];
    done = vectors << (4 - shift);
  }
  // a slice that starts between 16-byte boundaries, and the samples behind the last whole vector: element by element
  if (wide)
    for (int i = done + (int)threadIdx.x; i < count; i += kDevioThreads)
      reinterpret_cast<uint64_t*>(dst)[i] = reinterpret_cast<const uint64_t*>(src)[i];
  else
    for (int i = done + (int)threadIdx.x; i < count; i += kDevioThreads)
      reinterpret_cast<uint32_t*>(dst)[i] = reinterpret_cast<const uint32_t*>(src)[i];
}

__device__ __forceinline__ void store_as(const DevioSeries& o, int64_t at, double v) {
  if (o.f32) reinterpret_cast<float*>(o.dst)[at] = (float)v;   // round to nearest even
  else reinterpret_cast<double*>(o.dst)[at] = v;
}

__global__ __launch_bounds__(kDevioThreads) void devio_export_kernel(const DevioExportArgs a) {
  __shared__ double s_rec[kDevioRows * kDevioMaxStride];
  __shared__ int64_t s_buf[kDevioRows];     // the row's file (0 when packed)
  __shared__ int64_t s_local[kDevioRows];   // the row within its file's slot (the batch-wide row when packed)
  const int t = (int)threadIdx.x;
  const bool pad_tile = blockIdx.x >= a.data_tiles;
  const int64_t row0 = (int64_t)(pad_tile ? blockIdx.x - a.data_tiles : blockIdx.x) * kDevioRows;
  const int64_t rows_left = (pad_tile ? a.pad_rows : a.frames) - row0;
  const int rows = (int)(rows_left < kDevioRows ? rows_left : kDevioRows);
  if (t < rows) {
    const int64_t r = row0 + t;
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
    s_buf[t] = buf;
    s_local[t] = local;
  }
  if (!pad_tile && a.stride > 0) {
    // the rows of this tile lie one behind the other: rows x stride doubles from a 16-byte boundary (16 rows of 8 bytes)
    const int n = rows * a.stride;
    const double* src = a.rec + row0 * a.stride;
    for (int e = t; e < (n >> 1); e += kDevioThreads)
      reinterpret_cast<double2*>(s_rec)[e] = reinterpret_cast<const double2*>(src)[e];
    if ((n & 1) && t == 0) s_rec[n - 1] = src[n - 1];
  }
  __syncthreads();
  const int r16 = t >> 4, c16 = t & 15;   // 16 lanes to a row: a 14-wide series keeps 14 of them busy
  for (int k = 0; k < a.n_outs; ++k) {
    const DevioSeries& o = a.outs[k];
    if (o.from_mag) {
      for (int idx = t; idx < rows * 1024; idx += kDevioThreads) {
        const int r = idx >> 10, c = idx & 1023;
        const double v = pad_tile ? a.pad_value : a.mag[(row0 + r) * 1024 + c];
        store_as(o, s_buf[r] * o.buf_stride + s_local[r] * o.row_stride + c, v);
      }
    } else if (r16 < rows) {
      const int64_t at = s_buf[r16] * o.buf_stride + s_local[r16] * o.row_stride;
      for (int c = c16; c < o.width; c += 16)
        store_as(o, at + c, pad_tile ? a.pad_value : s_rec[r16 * a.stride + o.col + c]);
    }
  }
}

__global__ __launch_bounds__(kDevioThreads) void devio_stats_kernel(const DevioStatsArgs a) {
  const int64_t i = blockIdx.x;
  for (int k = 0; k < a.n_outs; ++k) {
    const DevioSeries& o = a.outs[k];
    const int n = o.width * 13;
    const double* src = a.stats + (i * a.stride + o.col) * 13;
    for (int idx = (int)threadIdx.x; idx < n; idx += kDevioThreads) store_as(o, i * n + idx, src[idx]);
  }
}

__global__ __launch_bounds__(kDevioThreads) void devio_counts_kernel(const int64_t* __restrict__ frame_offset, int n_bufs, int64_t* __restrict__ counts) {
  const int i = (int)blockIdx.x * kDevioThreads + (int)threadIdx.x;
  if (i < n_bufs) counts[i] = frame_offset[i + 1] - frame_offset[i];
}

}  // namespace

hipError_t launch_devio_gather(void* arena, const DevioBuf* bufs, int n_bufs, int64_t n_tiles, int elem_bytes, hipStream_t stream) {
  if (n_bufs <= 0 || n_tiles <= 0) return hipSuccess;
  if (n_tiles > 0x7FFFFFFF || (elem_bytes != 4 && elem_bytes != 8)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(devio_gather_kernel, dim3((unsigned)n_tiles), dim3(kDevioThreads), 0, stream, (unsigned char*)arena, bufs, n_bufs,
                     elem_bytes == 8 ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_devio_export(const DevioExportArgs& a, hipStream_t stream) {
  const int64_t pad_tiles = (a.pad_rows + kDevioRows - 1) / kDevioRows;
  const int64_t grid = (int64_t)a.data_tiles + pad_tiles;
  if (a.n_outs <= 0 || grid <= 0) return hipSuccess;
  if (a.n_outs > kDevioMaxOuts || a.stride > kDevioMaxStride || grid > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(devio_export_kernel, dim3((unsigned)grid), dim3(kDevioThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_devio_export_stats(const DevioStatsArgs& a, hipStream_t stream) {
  if (a.n_outs <= 0 || a.n_bufs <= 0) return hipSuccess;
  if (a.n_outs > kDevioMaxOuts) return hipErrorInvalidValue;
  hipLaunchKernelGGL(devio_stats_kernel, dim3((unsigned)a.n_bufs), dim3(kDevioThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_devio_frame_counts(const int64_t* frame_offset, int n_bufs, int64_t* counts, hipStream_t stream) {
  if (n_bufs <= 0) return hipSuccess;
  hipLaunchKernelGGL(devio_counts_kernel, dim3((unsigned)((n_bufs + kDevioThreads - 1) / kDevioThreads)), dim3(kDevioThreads), 0, stream,
                     frame_offset, n_bufs, counts);
  return hipGetLastError();
}

}  // namespace afx
