// afec_amd/csrc/flac/afx_flac_index.cpp -- the host's half of FLAC input: STREAMINFO and the frame index.
// Host code only, no device, no CRC-16, no residual: a search for 0xFF and a few header bytes per frame.  The header
// parse is the one the device's walk uses (afx_flac_decode.h).  Third-party callers of the C-ABI and afec_amd/host share it.

#include <cstring>

#include "afx.h"
#include "afx_flac_decode.h"

namespace {

using afx::flac::FrameHeader;

inline uint32_t be24(const uint8_t* p) { return (uint32_t)p[0] << 16 | (uint32_t)p[1] << 8 | p[2]; }

// the last metadata block's end, STREAMINFO read on the way
int probe(const uint8_t* p, int64_t n, afx_flac_info* info) {
  std::memset(info, 0, sizeof(*info));
  int64_t at = 0;
  // a leading ID3v2 tag, stepped over as libFLAC does (stream_decoder.c, find_metadata_): 10 bytes + a 28-bit size
  if (n >= 10 && p[0] == 'I' && p[1] == 'D' && p[2] == '3') {
    const int64_t size = (int64_t)(p[6] & 0x7F) << 21 | (int64_t)(p[7] & 0x7F) << 14 | (int64_t)(p[8] & 0x7F) << 7 | (int64_t)(p[9] & 0x7F);
    at = 10 + size;
  }
  if (at > n - 4) return AFX_ERR_BAD_BUFFER;
  if (std::memcmp(p + at, "OggS", 4) == 0) return AFX_ERR_UNSUPPORTED;
  if (std::memcmp(p + at, "fLaC", 4) != 0) return AFX_ERR_BAD_BUFFER;
  at += 4;
  bool last = false, first = true;
  while (!last) {
    if (at > n - 4) return AFX_ERR_BAD_BUFFER;
    last = (p[at] & 0x80) != 0;
    const int type = p[at] & 0x7F;
    const int64_t size = be24(p + at + 1);
    at += 4;
    if (size > n - at) return AFX_ERR_BAD_BUFFER;
    if (first) {
      if (type != 0 || size < 34) return AFX_ERR_BAD_BUFFER;   // STREAMINFO comes first
      const uint8_t* s = p + at;
      info->min_blocksize = s[0] << 8 | s[1];
      info->max_blocksize = s[2] << 8 | s[3];
      info->sample_rate = (int32_t)(be24(s + 10) >> 4);
      info->channels = ((s[12] >> 1) & 7) + 1;
      info->bits_per_sample = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
      info->total_samples = (int64_t)(s[13] & 15) << 32 | (int64_t)s[14] << 24 | (int64_t)s[15] << 16 | (int64_t)s[16] << 8 | s[17];
      first = false;
    }
    at += size;
  }
  info->first_frame_off = at;
  if (info->bits_per_sample != 8 && info->bits_per_sample != 16 && info->bits_per_sample != 24) return AFX_ERR_UNSUPPORTED;
  if (info->sample_rate <= 0 || info->max_blocksize < 1 || at >= n) return AFX_ERR_BAD_BUFFER;
  return AFX_OK;
}

}  // namespace

extern "C" {

int afx_flac_probe(const void* image, int64_t bytes, afx_flac_info* info) {
  if (!image || !info || bytes < 0) return AFX_ERR_INVALID_ARG;
  return probe((const uint8_t*)image, bytes, info);
}

int afx_flac_build_index(const void* image, int64_t bytes, afx_flac_frame* index, int32_t capacity, int32_t* n_index,
                         int64_t* total_samples) {
  if (!image || !n_index || !total_samples || bytes < 0 || capacity < 0 || (capacity > 0 && !index)) return AFX_ERR_INVALID_ARG;
  *n_index = 0;
  *total_samples = 0;
  afx_flac_info info;
  const int st = probe((const uint8_t*)image, bytes, &info);
  if (st != AFX_OK) return st;
  const uint8_t* p = (const uint8_t*)image + info.first_frame_off;
  int64_t n = bytes - info.first_frame_off;
  // an ID3v1 tag behind the last frame (128 bytes, "TAG") is no part of it
  if (n > 128 + 7 && std::memcmp(p + n - 128, "TAG", 3) == 0) n -= 128;

  int64_t frames = 0, samples = 0, at = 0;
  int variable = 0;
  bool short_seen = false;   // a fixed-blocksize stream's frame of another blocksize than STREAMINFO's: its last
  while (at < n && frames < 0x7FFFFFF0) {
    // the next 0xFF from `at` on whose header passes every check
    FrameHeader h;
    int head = 0;
    int64_t c = at;
    for (; c < n; ++c) {
      const uint8_t* hit = (const uint8_t*)std::memchr(p + c, 0xFF, (size_t)(n - c));
      if (!hit) { c = n; break; }
      c = hit - p;
      head = afx::flac::parse_frame_header(p + c, n - c, &h);
      if (head == 0) continue;
      if (frames == 0) variable = h.variable;
      const int64_t expect = variable ? samples : frames;
      const bool good = h.variable == variable && afx::flac::crc8(p + c, head - 1) == p[c + head - 1] &&
                        (h.rate == 0 || h.rate == info.sample_rate) && (h.bits == 0 || h.bits == info.bits_per_sample) &&
                        h.channels == info.channels && h.number == expect && h.blocksize <= info.max_blocksize &&
                        c + head + 2 <= n;
      if (good) break;
      head = 0;
      if (frames == 0) break;   // the first frame stands right behind the metadata or the file is refused
    }
    if (head == 0) {
      if (frames == 0) return AFX_ERR_BAD_BUFFER;
      break;   // no further frame: what is left belongs to the last one (the device's CRC-16 and end check judge it)
    }
    if (frames == 0 && c != 0) return AFX_ERR_BAD_BUFFER;
    // a fixed-blocksize stream states STREAMINFO's blocksize in every frame but the last: a frame behind a short one
    // refuses the file (without this a STREAMINFO whose total is 0 would take the shortened sum for the total)
    if (short_seen) return AFX_ERR_BAD_BUFFER;
    if (!variable && h.blocksize != info.max_blocksize) short_seen = true;
    if (frames < capacity) index[frames] = afx_flac_frame{c, samples};
    ++frames;
    samples += h.blocksize;
    at = c + head + 2;   // no frame is shorter than its header and its CRC-16
  }
  *n_index = (int32_t)frames;
  // The sum of the blocksizes is STREAMINFO's total, or becomes it where that is 0 (FlacFile.cpp:270-335 finds it "the
  // hard way", by decoding); a gap in the numbers ends the walk early and shows here.
  if (info.total_samples != 0 && samples != info.total_samples) return AFX_ERR_BAD_BUFFER;
  *total_samples = samples;
  if (frames + 1 > capacity) return AFX_ERR_OUT_OF_MEMORY;
  index[frames] = afx_flac_frame{n, samples};
  return AFX_OK;
}

}  // extern "C"
