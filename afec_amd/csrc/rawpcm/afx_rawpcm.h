// afec_amd/csrc/rawpcm/afx_rawpcm.h -- the byte-order kernel (afx_rawpcm.hip) and its launcher, shared with
// afx_batch_create.cpp.  Kept apart from afx_internal.h for the reason highlevel/afx_highlevel.h gives.  The device mock
// does NOT implement this launcher: afx_batch_create.cpp refers to it weakly, and the plan of the raw arena
// (afx_raw_plan.h) refuses a big-endian buffer where it is absent.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace afx {

// What one workgroup rewrites: 256 threads x 48 bytes.  48 is the unit of packed 24-bit samples (16 samples, three
// 16-byte vectors); for 2-, 4- and 8-byte samples a thread takes three 16-byte vectors a wavefront's width apart.
constexpr int kRawNativeThreads = 256;
constexpr int kRawNativeTileBytes = kRawNativeThreads * 48;   // 12 288

// One big-endian file of a batch.  Its slot in the raw arena starts on a 16-byte boundary and is padded to one
// (afx_raw_plan.h: plan_raw_arena), so whole 16-byte vectors are read and written up to (bytes + 15) & ~15 and never beyond.
struct RawNativeFile {
  int64_t raw_off;      // byte offset of the payload in the raw arena, a multiple of 16
  int64_t bytes;        // payload bytes (frames x channels x bytes per sample)
  int32_t kind;         // bytes per sample: 2, 3, 4 or 8
  int32_t tile_first;   // the file's first tile of the launch (host-made prefix over ceil(padded bytes / tile))
};
static_assert(sizeof(RawNativeFile) == 24, "table layout");

inline int64_t raw_native_tiles(int64_t bytes) {
  const int64_t padded = (bytes + 15) & ~(int64_t)15;
  return (padded + kRawNativeTileBytes - 1) / kRawNativeTileBytes;
}

// rewrites the payload of files[0 .. n_files) in place into the native byte order, one workgroup per tile, on `stream`;
// n_tiles is the sum of raw_native_tiles() over the files (what tile_first was made from)
hipError_t launch_raw_native(unsigned char* raw, const RawNativeFile* files, int n_files, int64_t n_tiles, hipStream_t stream);

}  // namespace afx
