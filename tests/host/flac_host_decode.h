// tests/host/flac_host_decode.h -- the three kernels of afec_amd/csrc/flac/afx_flac.hip as host loops around the SAME
// functions (afx_flac_decode.h), over buffers of exactly the sizes the device slots have, so that a sanitizer sees every
// byte the GPU code would touch outside them.  Shared by tests/host/flac_decode_main.cpp (the CPU decode test) and
// tests/sanitize/flac_decode_main.cpp (ASan + UBSan).
#pragma once

#include <cstdint>
#include <cstring>
#include <memory>

#include "afx.h"
#include "../../afec_amd/csrc/flac/afx_flac_decode.h"

namespace flac_host {

struct Decoded {
  std::unique_ptr<uint8_t[]> pcm;   // the native PCM of the first two channels, as it lies at the file's raw_off
  int64_t pcm_bytes = 0;
  int32_t status = 0;               // OR of 1 << afx::flac::kFrame* over the frames
  int32_t kept = 0, width = 0;
};

// frames[0 .. frames_bytes) and index[0 .. n_index] as afx_flac_stream names them; false when the host refuses the index
inline bool decode(const uint8_t* frames, int64_t frames_bytes, const afx_flac_frame* index, int32_t n_index, int64_t n_samples,
                   int32_t bits, int32_t channels, Decoded* out, bool isolate_frames = false) {
  namespace fl = afx::flac;
  if (!fl::index_ok(index, n_index, frames_bytes, n_samples) || channels < 1 || channels > 8 || (bits != 8 && bits != 16 && bits != 24)) return false;
  out->kept = channels < 2 ? 1 : 2;
  out->width = bits == 24 ? 3 : 2;
  out->pcm_bytes = n_samples * out->kept * out->width;
  out->pcm.reset(new uint8_t[(size_t)out->pcm_bytes]);
  std::memset(out->pcm.get(), 0xA5, (size_t)out->pcm_bytes);
  std::unique_ptr<int32_t[]> work(new int32_t[(size_t)(n_samples * channels)]);
  std::unique_ptr<fl::Subframe[]> sub(new fl::Subframe[(size_t)n_index * channels]);
  std::unique_ptr<int32_t[]> assign(new int32_t[(size_t)n_index]);
  for (int64_t i = 0; i < n_samples * channels; ++i) work[i] = 0x5A5A5A5A;   // the arena is never cleared: stale, but initialised
  for (int32_t k = 0; k < n_index; ++k) {   // flac_walk_kernel
    const int32_t blocksize = (int32_t)(index[k + 1].first_sample - index[k].first_sample);
    fl::Subframe* s = sub.get() + (int64_t)k * channels;
    int32_t assignment = 0;
    // isolate_frames: the frame's bytes in an allocation of their own, so that a read past the frame (not only past the
    // stream) is a sanitizer finding
    const int64_t frame_len = index[k + 1].byte_off - index[k].byte_off;
    std::unique_ptr<uint8_t[]> alone;
    const uint8_t* frame = frames + index[k].byte_off;
    if (isolate_frames) {
      alone.reset(new uint8_t[(size_t)frame_len]);
      std::memcpy(alone.get(), frame, (size_t)frame_len);
      frame = alone.get();
    }
    const int32_t st = fl::walk_frame(frame, frame_len, blocksize, channels, bits,
                                      work.get() + index[k].first_sample * channels, s, &assignment);
    if (st != fl::kFrameOk) {
      for (int c = 0; c < channels; ++c) s[c].kind = fl::kSubSkip;
      assignment = 0;
      out->status |= 1 << st;
    }
    assign[k] = assignment;
  }
  for (int32_t k = 0; k < n_index; ++k)     // flac_restore_kernel
    for (int c = 0; c < out->kept; ++c) {
      const int32_t blocksize = (int32_t)(index[k + 1].first_sample - index[k].first_sample);
      fl::restore_subframe(sub[(int64_t)k * channels + c], work.get() + index[k].first_sample * channels + (int64_t)c * blocksize, blocksize);
    }
  for (int32_t k = 0; k < n_index; ++k) {   // flac_output_kernel
    const int64_t first = index[k].first_sample;
    const int32_t blocksize = (int32_t)(index[k + 1].first_sample - first);
    for (int32_t i = 0; i < blocksize; ++i) {
      const int32_t* data = work.get() + first * channels + i;
      uint8_t* dst = out->pcm.get() + (first + i) * (out->kept * out->width);
      if (out->kept == 1) {
        fl::store_native(dst, data[0], bits);
      } else {
        int32_t left, right;
        fl::undo_assignment(assign[k], data[0], data[blocksize], &left, &right);
        fl::store_native(dst, left, bits);
        fl::store_native(dst + out->width, right, bits);
      }
    }
  }
  return true;
}

}  // namespace flac_host
