// afec_amd/csrc/rawpcm/afx_rawpcm.hip -- big-endian PCM made native, in place in the raw arena.
//
// An AIFF's sample data goes to the device as it lies in the file (afec_amd/host/AifFile.h); its samples have the
// semantics of the native formats (afx.h: AFX_RAW_*_BE) with the bytes of each in Motorola order.  raw_native_kernel
// turns them round before the conversion and LoadSample kernels run, which therefore see only formats they know.
//
//   one launch per batch; one workgroup of 256 threads per 12 288-byte tile of a file's padded slot; the tile's file by
//   binary search in the host-made prefix (RawNativeFile::tile_first)
//   2 / 4 / 8-byte samples: a thread takes three 16-byte vectors 4 KiB apart (coalesced), through the padded end
//   packed 24-bit: a thread takes one 48-byte unit (16 samples) and exchanges byte 0 and byte 2 of each; the slot's
//   padded length is a multiple of 16, not of 48, so the last unit of a file has one or two vectors only
//   a thread reads all of its vectors before it writes any; no vector belongs to two threads
//
// One read and one write of the payload: bound by memory traffic.

#include <hip/hip_runtime.h>

#include "afx_rawpcm.h"

namespace afx {
namespace {

// v_perm_b32: byte i of the result is byte sel[i] of {hi : lo} (0..3 = lo, 4..7 = hi)
__device__ __forceinline__ unsigned perm(unsigned hi, unsigned lo, unsigned sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

__device__ __forceinline__ unsigned swap16x2(unsigned w) { return perm(w, w, 0x02030001u); }

// twelve bytes = four packed 24-bit samples: b2 b1 b0 b5 | b4 b3 b8 b7 | b6 b11 b10 b9
__device__ __forceinline__ void swap24x4(unsigned& w0, unsigned& w1, unsigned& w2) {
  const unsigned o0 = perm(w1, w0, 0x05000102u);
  const unsigned t = perm(w0, w2, 0x00000007u);    // b3, b8
  const unsigned o1 = perm(w1, t, 0x07010004u);
  const unsigned o2 = perm(w2, w1, 0x05060702u);
  w0 = o0; w1 = o1; w2 = o2;
}

__global__ __launch_bounds__(kRawNativeThreads) void raw_native_kernel(unsigned char* raw, const RawNativeFile* __restrict__ files, int n_files) {
  const int tile = (int)blockIdx.x;
  int lo = 0, hi = n_files - 1;   // the last file whose first tile is not behind this one
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (files[mid].tile_first <= tile) lo = mid; else hi = mid - 1;
  }
  const RawNativeFile f = files[lo];
  const int64_t n_vec = (f.bytes + 15) >> 4;                                   // the slot's 16-byte vectors
  const int64_t v0 = (int64_t)(tile - f.tile_first) * (kRawNativeTileBytes / 16);
  uint4* slot = reinterpret_cast<uint4*>(raw + f.raw_off);
  const int tid = (int)threadIdx.x;

  int64_t at[3];
  uint4 w[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    at[j] = v0 + (f.kind == 3 ? tid * 3 + j : j * kRawNativeThreads + tid);
    w[j] = (at[j] < n_vec) ? slot[at[j]] : make_uint4(0u, 0u, 0u, 0u);
  }
  if (f.kind == 3) {
    swap24x4(w[0].x, w[0].y, w[0].z);
    swap24x4(w[0].w, w[1].x, w[1].y);
    swap24x4(w[1].z, w[1].w, w[2].x);
    swap24x4(w[2].y, w[2].z, w[2].w);
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (f.kind == 2) {
        w[j] = make_uint4(swap16x2(w[j].x), swap16x2(w[j].y), swap16x2(w[j].z), swap16x2(w[j].w));
      } else if (f.kind == 4) {
        w[j] = make_uint4(__builtin_bswap32(w[j].x), __builtin_bswap32(w[j].y), __builtin_bswap32(w[j].z), __builtin_bswap32(w[j].w));
      } else {
        w[j] = make_uint4(__builtin_bswap32(w[j].y), __builtin_bswap32(w[j].x), __builtin_bswap32(w[j].w), __builtin_bswap32(w[j].z));
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (at[j] < n_vec) slot[at[j]] = w[j];
}

}  // namespace

hipError_t launch_raw_native(unsigned char* raw, const RawNativeFile* files, int n_files, int64_t n_tiles, hipStream_t stream) {
  if (n_files <= 0 || n_tiles <= 0) return hipSuccess;
  if (n_tiles > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(raw_native_kernel, dim3((unsigned)n_tiles), dim3(kRawNativeThreads), 0, stream, raw, files, n_files);
  return hipGetLastError();
}

}  // namespace afx
