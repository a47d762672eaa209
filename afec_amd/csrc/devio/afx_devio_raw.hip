// afec_amd/csrc/devio/afx_devio_raw.hip -- LoadSample on device-resident audio.  Pure memory movers:
//
//   devio_raw_gather_kernel     the caller's raw PCM in device memory into the raw arena, one workgroup per tile of
//                               kDevioRawTileFrames sample frames of one buffer: exactly the bytes the host path's
//                               transfers write (afx_batch_create.cpp: upload_pieces).  Interleaved buffers are a byte
//                               copy, in 16-byte vectors whatever the source's alignment; planar buffers are interleaved
//                               on their way, consecutive lanes taking consecutive frames
//   devio_samples_kernel        the analysed samples of every file as rows of the caller's device memory, double or float,
//                               the padding behind them in the same launch
//   devio_sample_counts_kernel  samples per file
//
// Every address is formed from tables the host has checked against the extents of the allocations involved
// (afx_devio_raw_plan.h).  Of the caller's memory the gather reads the checked ranges and, for interleaved buffers, the
// whole aligned 16-byte granules those ranges touch (they cannot leave the ranges' pages); nothing else.

#include <hip/hip_runtime.h>

#include "../afx_internal.h"
#include "afx_devio_raw.h"

namespace afx {
namespace {

// the last buffer whose first tile is not behind `tile` (every buffer of the table has at least one tile)
__device__ __forceinline__ int raw_buf_of_tile(const DevioRawBuf* __restrict__ bufs, int n_bufs, int tile) {
  int lo = 0, hi = n_bufs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (bufs[mid].tile_first <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// 16 bytes from byte 4 * Q + r of the 32 bytes {lo, hi} (r = 0..3): what lies at an address 4 * Q + r bytes behind a
// 16-byte boundary, from the two aligned granules around it
template <int Q>
__device__ __forceinline__ uint4 realigned(const uint4 lo, const uint4 hi, unsigned r) {
  const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return make_uint4(__builtin_amdgcn_alignbyte(w[Q + 1], w[Q], r), __builtin_amdgcn_alignbyte(w[Q + 2], w[Q + 1], r),
                    __builtin_amdgcn_alignbyte(w[Q + 3], w[Q + 2], r), __builtin_amdgcn_alignbyte(w[Q + 4], w[Q + 3], r));
}

// vectors 16-byte vectors to dst (aligned) from src_aligned + 4 * Q + r bytes: vector v is made of the granules v and
// v + 1, and its last byte lies in granule v + 1 (4 * Q + r >= 1), so both are granules the copied range touches
template <int Q>
__device__ __forceinline__ void copy_realigned(uint4* __restrict__ dst, const uint4* __restrict__ src_aligned, int vectors, unsigned r) {
  for (int v = (int)threadIdx.x; v < vectors; v += kDevioRawThreads) dst[v] = realigned<Q>(src_aligned[v], src_aligned[v + 1], r);
}

template <typename E>
__device__ __forceinline__ int copy_elements(unsigned char* __restrict__ dst, const unsigned char* __restrict__ src, int bytes) {
  const int n = bytes / (int)sizeof(E);
  for (int i = (int)threadIdx.x; i < n; i += kDevioRawThreads) reinterpret_cast<E*>(dst)[i] = reinterpret_cast<const E*>(src)[i];
  return n * (int)sizeof(E);
}

// frames [first, first + count) of a planar buffer: lane i takes frame first + i, reads its sample of every plane (a wave
// reads 64 consecutive samples of a plane) and writes the frame (a wave's frames lie one behind the other)
template <typename E>
__device__ __forceinline__ void interleave(unsigned char* __restrict__ slot, const DevioRawBuf& f, int64_t first, int count) {
  const E* __restrict__ src = reinterpret_cast<const E*>(f.src);
  E* __restrict__ dst = reinterpret_cast<E*>(slot);
  for (int i = (int)threadIdx.x; i < count; i += kDevioRawThreads) {
    const int64_t frame = first + i;
    for (int c = 0; c < f.channels; ++c) dst[frame * f.channels + c] = src[(int64_t)c * f.plane_stride + frame];
  }
}
struct Packed24 { unsigned char b[3]; };
static_assert(sizeof(Packed24) == 3 && alignof(Packed24) == 1, "packed int24");

__global__ __launch_bounds__(kDevioRawThreads) void devio_raw_gather_kernel(unsigned char* __restrict__ arena, const DevioRawBuf* __restrict__ bufs,
                                                                           int n_bufs, int elementwise) {
  const int tile = (int)blockIdx.x;
  const DevioRawBuf& f = bufs[raw_buf_of_tile(bufs, n_bufs, tile)];
  const int64_t first = (int64_t)(tile - f.tile_first) * kDevioRawTileFrames;
  const int64_t left = f.n_frames - first;
  if (left <= 0) return;
  const int count = (int)(left < kDevioRawTileFrames ? left : kDevioRawTileFrames);
  unsigned char* slot = arena + f.dst_off;
  if (f.planar) {
    switch (f.bps) {
      case 2: interleave<uint16_t>(slot, f, first, count); break;
      case 3: interleave<Packed24>(slot, f, first, count); break;
      case 4: interleave<uint32_t>(slot, f, first, count); break;
      default: interleave<uint64_t>(slot, f, first, count); break;
    }
    return;
  }
  // interleaved: bytes [first, first + count) x frame bytes of the buffer; the slot's side is a multiple of 16 (the slot is,
  // and a tile's bytes are: kDevioRawTileFrames is a multiple of 16)
  const int frame_bytes = f.channels * f.bps;
  const int bytes = count * frame_bytes;   // at most 2 048 x 64
  const unsigned char* src = (const unsigned char*)f.src + first * frame_bytes;
  unsigned char* dst = slot + first * frame_bytes;
  const unsigned m = (unsigned)((uintptr_t)src & 15);
  const int vectors = bytes >> 4;
  int done = vectors << 4;
  if (m == 0) {
    // aligned alike: 16-byte vectors, a workgroup's accesses back to back
    for (int v = (int)threadIdx.x; v < vectors; v += kDevioRawThreads)
      reinterpret_cast<uint4*>(dst)[v] = reinterpret_cast<const uint4*>(src)[v];
  } else if (!elementwise) {
    // a slice that starts between 16-byte boundaries (of a decoder's output: the common case): aligned source granules,
    // shifted into place, 16-byte stores
    const uint4* src_aligned = reinterpret_cast<const uint4*>(src - m);
    const unsigned r = m & 3;
    switch (m >> 2) {
      case 0: copy_realigned<0>(reinterpret_cast<uint4*>(dst), src_aligned, vectors, r); break;
      case 1: copy_realigned<1>(reinterpret_cast<uint4*>(dst), src_aligned, vectors, r); break;
      case 2: copy_realigned<2>(reinterpret_cast<uint4*>(dst), src_aligned, vectors, r); break;
      default: copy_realigned<3>(reinterpret_cast<uint4*>(dst), src_aligned, vectors, r); break;
    }
  } else {
    // the obvious form, kept for the comparison: the widest element the source's alignment allows
    done = (m & 1) ? 0 : (m & 2) ? copy_elements<uint16_t>(dst, src, bytes) : (m & 4) ? copy_elements<uint32_t>(dst, src, bytes)
                                                                                 : copy_elements<uint64_t>(dst, src, bytes);
  }
  // the bytes behind the last whole vector (a buffer's last tile only), byte by byte
  for (int i = done + (int)threadIdx.x; i < bytes; i += kDevioRawThreads) dst[i] = src[i];
}

// sample `at` of the arena as the kernels form it: (double)x * FinalScaling behind the LoadSample front end
__device__ __forceinline__ double scaled(float x, int kind, double scale) {
  return kind == kPcmScaledF32 ? (double)x * scale : (double)x;
}

__global__ __launch_bounds__(kDevioRawThreads) void devio_samples_kernel(const DevioSamplesArgs a) {
  const int file = (int)(blockIdx.x / (unsigned)a.tiles_per_row), tile = (int)(blockIdx.x % (unsigned)a.tiles_per_row);
  const int64_t off = a.rows[file], used = a.rows[a.n_bufs + file];
  const double scale = __longlong_as_double(a.rows[2 * (int64_t)a.n_bufs + file]);
  const int64_t e0 = (int64_t)tile * kDevioSampleTile;
  const int64_t left = a.buf_stride - e0;
  const int count = (int)(left < kDevioSampleTile ? left : kDevioSampleTile);
  const int64_t row = (int64_t)file * a.buf_stride + e0;   // first element of the tile in the destination
  const int kind = a.pcm_kind;
  const float* __restrict__ pf = reinterpret_cast<const float*>(a.pcm) + off;
  const double* __restrict__ pd = reinterpret_cast<const double*>(a.pcm) + off;
  const double pad = a.pad_value;
  auto value = [&](int64_t e) { return e < used ? (kind == kPcmF64 ? pd[e] : scaled(pf[e], kind, scale)) : pad; };
  int done = 0;
  if (a.f32) {
    float* __restrict__ dst = reinterpret_cast<float*>(a.dst) + row;
    if (((uintptr_t)dst & 15) == 0) {
      // the row starts on a 16-byte boundary, a tile is 16 KiB: four floats a store; the arena side is 16-byte aligned too
      const int vectors = count >> 2;
      for (int v = (int)threadIdx.x; v < vectors; v += kDevioRawThreads) {
        const int64_t e = e0 + 4 * (int64_t)v;
        float4 o;
        if (e + 4 <= used && kind != kPcmF64) {
          const float4 x = reinterpret_cast<const float4*>(pf)[e >> 2];
          o = make_float4((float)scaled(x.x, kind, scale), (float)scaled(x.y, kind, scale), (float)scaled(x.z, kind, scale),
                          (float)scaled(x.w, kind, scale));
        } else {
          o = make_float4((float)value(e), (float)value(e + 1), (float)value(e + 2), (float)value(e + 3));
        }
        reinterpret_cast<float4*>(dst)[v] = o;
      }
      done = vectors << 2;
    }
    for (int i = done + (int)threadIdx.x; i < count; i += kDevioRawThreads) dst[i] = (float)value(e0 + i);   // round to nearest even
  } else {
    double* __restrict__ dst = reinterpret_cast<double*>(a.dst) + row;
    if (((uintptr_t)dst & 15) == 0) {
      const int vectors = count >> 1;
      for (int v = (int)threadIdx.x; v < vectors; v += kDevioRawThreads) {
        const int64_t e = e0 + 2 * (int64_t)v;
        double2 o;
        if (e + 2 <= used && kind == kPcmF64) o = reinterpret_cast<const double2*>(pd)[e >> 1];
        else o = make_double2(value(e), value(e + 1));
        reinterpret_cast<double2*>(dst)[v] = o;
      }
      done = vectors << 1;
    }
    for (int i = done + (int)threadIdx.x; i < count; i += kDevioRawThreads) dst[i] = value(e0 + i);
  }
}

__global__ __launch_bounds__(kDevioRawThreads) void devio_sample_counts_kernel(const int64_t* __restrict__ rows, int n_bufs, int64_t* __restrict__ counts) {
  const int i = (int)blockIdx.x * kDevioRawThreads + (int)threadIdx.x;
  if (i < n_bufs) counts[i] = rows[n_bufs + i];
}

}  // namespace

hipError_t launch_devio_raw_gather(unsigned char* arena, const DevioRawBuf* bufs, int n_bufs, int64_t n_tiles, int elementwise,
                                   hipStream_t stream) {
  if (n_bufs <= 0 || n_tiles <= 0) return hipSuccess;
  if (n_tiles > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(devio_raw_gather_kernel, dim3((unsigned)n_tiles), dim3(kDevioRawThreads), 0, stream, arena, bufs, n_bufs, elementwise);
  return hipGetLastError();
}

hipError_t launch_devio_samples(const DevioSamplesArgs& a, hipStream_t stream) {
  const int64_t grid = (int64_t)a.n_bufs * a.tiles_per_row;
  if (grid <= 0) return hipSuccess;
  if (grid > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(devio_samples_kernel, dim3((unsigned)grid), dim3(kDevioRawThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_devio_sample_counts(const int64_t* rows, int n_bufs, int64_t* counts, hipStream_t stream) {
  if (n_bufs <= 0) return hipSuccess;
  hipLaunchKernelGGL(devio_sample_counts_kernel, dim3((unsigned)((n_bufs + kDevioRawThreads - 1) / kDevioRawThreads)), dim3(kDevioRawThreads), 0,
                     stream, rows, n_bufs, counts);
  return hipGetLastError();
}

}  // namespace afx
