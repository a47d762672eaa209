// afec_amd/csrc/flac/afx_flac.hip -- FLAC frames decoded in the raw arena.
//
// A FLAC goes to the device as it lies in the file, with the host's frame index (flac/afx_flac_index.cpp).  Entropy
// decoding is serial inside one frame and nowhere else: frames carry their own header, Rice state and CRC-16.  Three
// launches per batch, each sized from the index:
//
//   flac_walk_kernel     one lane per frame: CRC-16, header, subframe headers, warm-ups, coefficients, Rice / raw residuals
//                        -> int32 work area + one flac::Subframe per subframe + the frame's channel assignment
//   flac_restore_kernel  one lane per kept subframe (the first two channels): CONSTANT / VERBATIM / FIXED / LPC in place
//   flac_output_kernel   one lane per sample frame: stereo decorrelation undone, interleaved, narrowed to the native
//                        format at the file's raw_off
//
// The three bodies are the functions of afx_flac_decode.h, which g++ compiles too; the kernels find their frame, call
// them and record a failure.  A failed frame marks its subframes kSubSkip, so the restore never acts on a record the
// walk did not finish, and sets its file's status; the host fails that file.  The work area and the records are not
// cleared between batches: nothing reads an element that this batch's walk has not written or marked.

#include <hip/hip_runtime.h>

#include "afx.h"
#include "afx_flac.h"

namespace afx {
namespace {

// the last file whose prefix (frame_first or tile_first) is not behind `at`
template <int32_t FlacFile::*Prefix>
__device__ __forceinline__ int file_of(const FlacFile* __restrict__ files, int n_files, int at) {
  int lo = 0, hi = n_files - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (files[mid].*Prefix <= at) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kFlacWalkThreads) void flac_walk_kernel(unsigned char* raw, const FlacFile* __restrict__ files, int n_files,
                                                                     int n_frames, int32_t* status) {
  const int g = (int)blockIdx.x * kFlacWalkThreads + (int)threadIdx.x;
  if (g >= n_frames) return;
  const int fi = file_of<&FlacFile::frame_first>(files, n_files, g);
  const FlacFile& f = files[fi];
  const int k = g - f.frame_first;
  if (k >= f.n_index) return;
  const afx_flac_frame* index = reinterpret_cast<const afx_flac_frame*>(raw + f.index_off);
  const afx_flac_frame here = index[k], next = index[k + 1];
  const int32_t blocksize = (int32_t)(next.first_sample - here.first_sample);
  int32_t* work = reinterpret_cast<int32_t*>(raw + f.work_off) + here.first_sample * f.stream_channels;
  flac::Subframe* sub = reinterpret_cast<flac::Subframe*>(raw + f.sub_off) + (int64_t)k * f.stream_channels;
  int32_t assignment = 0;
  const int32_t st = flac::walk_frame(raw + f.bytes_off + here.byte_off, next.byte_off - here.byte_off, blocksize, f.stream_channels,
                                      f.bits, work, sub, &assignment);
  if (st != flac::kFrameOk) {
    for (int c = 0; c < f.stream_channels; ++c) sub[c].kind = flac::kSubSkip;
    assignment = 0;
    atomicOr(&status[fi], 1 << st);
  }
  reinterpret_cast<int32_t*>(raw + f.assign_off)[k] = assignment;
}

__global__ __launch_bounds__(kFlacRestoreThreads) void flac_restore_kernel(unsigned char* raw, const FlacFile* __restrict__ files, int n_files,
                                                                           int n_frames) {
  const int g = (int)blockIdx.x * kFlacRestoreThreads + (int)threadIdx.x;
  const int frame = g >> 1, c = g & 1;
  if (frame >= n_frames) return;
  const FlacFile& f = files[file_of<&FlacFile::frame_first>(files, n_files, frame)];
  const int k = frame - f.frame_first;
  if (k >= f.n_index || c >= f.stream_channels) return;
  const afx_flac_frame* index = reinterpret_cast<const afx_flac_frame*>(raw + f.index_off);
  const int64_t first = index[k].first_sample;
  const int32_t blocksize = (int32_t)(index[k + 1].first_sample - first);
  int32_t* data = reinterpret_cast<int32_t*>(raw + f.work_off) + first * f.stream_channels + (int64_t)c * blocksize;
  const flac::Subframe* sub = reinterpret_cast<const flac::Subframe*>(raw + f.sub_off) + (int64_t)k * f.stream_channels + c;
  flac::restore_subframe(*sub, data, blocksize);
}

__global__ __launch_bounds__(kFlacOutputThreads) void flac_output_kernel(unsigned char* raw, const FlacFile* __restrict__ files, int n_files) {
  const int tile = (int)blockIdx.x;
  const FlacFile& f = files[file_of<&FlacFile::tile_first>(files, n_files, tile)];
  const int64_t n = (int64_t)(tile - f.tile_first) * kFlacOutputThreads + (int)threadIdx.x;
  if (n >= f.n_samples) return;
  const afx_flac_frame* index = reinterpret_cast<const afx_flac_frame*>(raw + f.index_off);
  int lo = 0, hi = f.n_index - 1;   // the frame that holds sample n
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (index[mid].first_sample <= n) lo = mid; else hi = mid - 1;
  }
  const int64_t first = index[lo].first_sample;
  const int32_t blocksize = (int32_t)(index[lo + 1].first_sample - first);
  const int32_t* data = reinterpret_cast<const int32_t*>(raw + f.work_off) + first * f.stream_channels + (n - first);
  const int kept = f.stream_channels < 2 ? 1 : 2;
  const int width = f.bits == 24 ? 3 : 2;
  unsigned char* dst = raw + f.out_off + n * (kept * width);
  if (kept == 1) {
    flac::store_native(dst, data[0], f.bits);
  } else {
    int32_t left, right;
    flac::undo_assignment(reinterpret_cast<const int32_t*>(raw + f.assign_off)[lo], data[0], data[blocksize], &left, &right);
    flac::store_native(dst, left, f.bits);
    flac::store_native(dst + width, right, f.bits);
  }
}

}  // namespace

hipError_t launch_flac_decode(unsigned char* raw, const FlacFile* files, int n_files, int64_t n_frames, int64_t n_tiles,
                              int32_t* status, hipStream_t stream) {
  if (n_files <= 0 || n_frames <= 0 || n_tiles <= 0) return hipSuccess;
  if (n_frames > 0x3FFFFFFF || n_tiles > 0x7FFFFFFF) return hipErrorInvalidValue;
  const unsigned walk_blocks = (unsigned)((n_frames + kFlacWalkThreads - 1) / kFlacWalkThreads);
  const unsigned restore_blocks = (unsigned)((2 * n_frames + kFlacRestoreThreads - 1) / kFlacRestoreThreads);
  hipLaunchKernelGGL(flac_walk_kernel, dim3(walk_blocks), dim3(kFlacWalkThreads), 0, stream, raw, files, n_files, (int)n_frames, status);
  hipLaunchKernelGGL(flac_restore_kernel, dim3(restore_blocks), dim3(kFlacRestoreThreads), 0, stream, raw, files, n_files, (int)n_frames);
  hipLaunchKernelGGL(flac_output_kernel, dim3((unsigned)n_tiles), dim3(kFlacOutputThreads), 0, stream, raw, files, n_files);
  return hipGetLastError();
}

}  // namespace afx
