// afec_amd/csrc/flac/afx_flac_decode.h -- the FLAC decoder proper: one frame's bit walk, one subframe's restore, one
// sample frame's output.  Plain functions over a byte pointer and a length, compiled twice: by hipcc as the
// bodies of the three kernels of afx_flac.hip, and by g++ for tests/host/flac_decode_main.cpp and the sanitizer program
// (tests/sanitize/flac_decode_main.cpp) -- the CPU tests run the very code the GPU executes.
//
// What every function here keeps, for ANY bytes: no read outside [p, p + len), no write outside the frame's own part of
// the work area and its own records, every loop bounded by len or by the blocksize, arithmetic that wraps (unsigned)
// where a malformed stream could overflow.  For a valid stream the integers are libFLAC's (lpc.c, fixed.c).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AFX_FLAC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define AFX_FLAC_HD inline
#endif

namespace afx {
namespace flac {

enum : int32_t {   // what a frame's walk answers
  kFrameOk = 0,
  kFrameHeader = 1,      // sync, reserved bits or codes; blocksize, channels or depth other than the index / STREAMINFO say
  kFrameSubframe = 2,    // reserved subframe type, wasted bits >= depth, order > blocksize, bad precision / shift / method
  kFrameOverrun = 3,     // the bits ran out inside the frame
  kFrameEnd = 4,         // the walk did not end at the frame's CRC-16
  kFrameCrc16 = 5
};

enum : int32_t { kSubConstant = 0, kSubVerbatim = 1, kSubFixed = 2, kSubLpc = 3, kSubSkip = 4 /* frame failed: restore nothing */ };

constexpr int kMaxLpcOrder = 32;
constexpr int kMaxBlocksize = 65535;
constexpr int kMaxFrameBytes = 1 << 24;   // 65 535 samples x 8 channels x 4 bytes is 2 MiB; the index is held to this bound

// One subframe as the bit walk leaves it for the restore: the work area holds warm-ups followed by residuals (or the
// verbatim samples, or the constant in element 0)
struct Subframe {
  int32_t kind;       // kSub*
  int32_t order;      // FIXED 0..4, LPC 1..32
  int32_t shift;      // LPC: 0..15
  int32_t wasted;     // left shift after the restore
  int32_t coef[kMaxLpcOrder];
};
static_assert(sizeof(Subframe) == 144, "record layout");

// What the kernels take on trust, checked on the host before an index goes to the device: {0, 0} first, offsets and
// samples strictly rising, no frame above kMaxFrameBytes or kMaxBlocksize, the sentinel equal to the stream's bytes and
// samples.  `Frame` is afx_flac_frame (afx.h); every address the three stages form follows from such an index.
template <class Frame>
inline bool index_ok(const Frame* index, int32_t n_index, int64_t frames_bytes, int64_t n_samples) {
  if (!index || n_index < 1 || frames_bytes < 1 || n_samples < 1) return false;
  if (index[0].byte_off != 0 || index[0].first_sample != 0) return false;
  for (int32_t k = 0; k < n_index; ++k) {
    // every entry inside the stream before any two are subtracted: the values are the caller's, and a difference of
    // two arbitrary int64 may overflow
    const Frame& here = index[k];
    const Frame& next = index[k + 1];
    if (here.byte_off < 0 || here.byte_off > frames_bytes || here.first_sample < 0 || here.first_sample > n_samples) return false;
    if (next.byte_off < 0 || next.byte_off > frames_bytes || next.first_sample < 0 || next.first_sample > n_samples) return false;
    const int64_t bytes = next.byte_off - here.byte_off, samples = next.first_sample - here.first_sample;
    if (bytes < 1 || bytes > kMaxFrameBytes || samples < 1 || samples > kMaxBlocksize) return false;
  }
  return index[n_index].byte_off == frames_bytes && index[n_index].first_sample == n_samples;
}

AFX_FLAC_HD uint32_t load_be32(const uint8_t* p) {
  uint32_t w;
  __builtin_memcpy(&w, p, 4);
  return __builtin_bswap32(w);
}

// CRC-16 of FLAC (x^16 + x^15 + x^2 + 1, MSB first, initial value 0) without a table: for a byte x the table entry is
// (parity(x) ? 0x8003 : 0) ^ (x << 2) ^ (x << 1)
AFX_FLAC_HD uint32_t crc16_byte(uint32_t crc, uint32_t byte) {
  const uint32_t x = ((crc >> 8) ^ byte) & 0xFFu;
  const uint32_t par = (uint32_t)__builtin_popcount(x) & 1u;
  return ((crc << 8) & 0xFFFFu) ^ (par ? 0x8003u : 0u) ^ (x << 2) ^ (x << 1);
}
AFX_FLAC_HD uint32_t crc16(const uint8_t* p, int64_t len) {
  uint32_t crc = 0;
  int64_t i = 0;
  for (; i + 4 <= len; i += 4) {
    const uint32_t w = load_be32(p + i);
    crc = crc16_byte(crc, w >> 24);
    crc = crc16_byte(crc, (w >> 16) & 0xFFu);
    crc = crc16_byte(crc, (w >> 8) & 0xFFu);
    crc = crc16_byte(crc, w & 0xFFu);
  }
  for (; i < len; ++i) crc = crc16_byte(crc, p[i]);
  return crc;
}
// CRC-8 of a frame header (x^8 + x^2 + x + 1, initial value 0); a header has at most 16 bytes
AFX_FLAC_HD uint32_t crc8(const uint8_t* p, int len) {
  uint32_t crc = 0;
  for (int i = 0; i < len; ++i) {
    crc ^= p[i];
    for (int b = 0; b < 8; ++b) crc = ((crc << 1) ^ ((crc & 0x80u) ? 0x07u : 0u)) & 0xFFu;
  }
  return crc;
}

// The fixed part of a frame header, shared by the host's indexer and the device's walk.  Returns the header's length
// with its CRC-8 byte (5..16), or 0 when the bytes are no frame header: sync code, reserved bits or a reserved code.
struct FrameHeader {
  int32_t variable;      // blocking strategy bit
  int32_t blocksize;
  int32_t rate;          // 0 = STREAMINFO's
  int32_t channels;
  int32_t assignment;    // 0 independent, 1 left/side, 2 side/right, 3 mid/side
  int32_t bits;          // 0 = STREAMINFO's
  int64_t number;        // frame number (fixed blocksize) or first sample (variable)
};
AFX_FLAC_HD int parse_frame_header(const uint8_t* p, int64_t len, FrameHeader* h) {
  if (len < 5 || p[0] != 0xFFu || (p[1] & 0xFEu) != 0xF8u) return 0;   // 14-bit sync, the reserved bit behind it
  h->variable = p[1] & 1;
  const int bs_code = p[2] >> 4, rate_code = p[2] & 15, ch_code = p[3] >> 4, size_code = (p[3] >> 1) & 7;
  if (bs_code == 0 || rate_code == 15 || ch_code > 10 || size_code == 3 || size_code == 7 || (p[3] & 1)) return 0;
  // the coded number: 1..7 bytes in the manner of UTF-8
  int at = 4;
  const uint32_t lead = p[at++];
  int more = 0;
  uint64_t number = lead;
  if (lead & 0x80u) {
    if ((lead & 0xE0u) == 0xC0u) more = 1, number = lead & 0x1Fu;
    else if ((lead & 0xF0u) == 0xE0u) more = 2, number = lead & 0x0Fu;
    else if ((lead & 0xF8u) == 0xF0u) more = 3, number = lead & 0x07u;
    else if ((lead & 0xFCu) == 0xF8u) more = 4, number = lead & 0x03u;
    else if ((lead & 0xFEu) == 0xFCu) more = 5, number = lead & 0x01u;
    else if (lead == 0xFEu) more = 6, number = 0;
    else return 0;
    if (more == 6 && !h->variable) return 0;   // a frame number has 31 bits
  }
  const int tail = (bs_code == 6 ? 1 : bs_code == 7 ? 2 : 0) + (rate_code == 12 ? 1 : rate_code >= 13 ? 2 : 0);
  if (len < at + more + tail + 1) return 0;
  for (int i = 0; i < more; ++i) {
    const uint32_t c = p[at++];
    if ((c & 0xC0u) != 0x80u) return 0;
    number = (number << 6) | (c & 0x3Fu);
  }
  h->number = (int64_t)number;
  int blocksize;
  if (bs_code == 1) blocksize = 192;
  else if (bs_code <= 5) blocksize = 576 << (bs_code - 2);
  else if (bs_code == 6) blocksize = (int)p[at++] + 1;
  else if (bs_code == 7) { blocksize = ((int)p[at] << 8 | (int)p[at + 1]) + 1; at += 2; }
  else blocksize = 256 << (bs_code - 8);
  h->blocksize = blocksize;
  int rate = 0;
  switch (rate_code) {
    case 0: rate = 0; break;
    case 1: rate = 88200; break;
    case 2: rate = 176400; break;
    case 3: rate = 192000; break;
    case 4: rate = 8000; break;
    case 5: rate = 16000; break;
    case 6: rate = 22050; break;
    case 7: rate = 24000; break;
    case 8: rate = 32000; break;
    case 9: rate = 44100; break;
    case 10: rate = 48000; break;
    case 11: rate = 96000; break;
    case 12: rate = (int)p[at++] * 1000; break;
    case 13: rate = (int)p[at] << 8 | (int)p[at + 1]; at += 2; break;
    default: rate = ((int)p[at] << 8 | (int)p[at + 1]) * 10; at += 2; break;
  }
  h->rate = rate;
  h->channels = ch_code < 8 ? ch_code + 1 : 2;
  h->assignment = ch_code < 8 ? 0 : ch_code - 7;
  h->bits = size_code == 0 ? 0 : size_code == 1 ? 8 : size_code == 2 ? 12 : size_code == 4 ? 16 : size_code == 5 ? 20 : 24;
  return at + 1;   // the CRC-8 byte is p[at]
}

// Big-endian bit reader over [p, p + len): a 64-bit window, its valid bits at the top and zeros below them.  A read
// past the end sets `over` and gives zeros; nothing is ever loaded from outside the range.
struct BitReader {
  const uint8_t* p;
  int64_t len, pos;     // pos: the next byte to load
  uint64_t acc;
  int32_t bits;         // valid bits in acc
  int32_t over;
};
AFX_FLAC_HD void br_open(BitReader& r, const uint8_t* p, int64_t len, int64_t at) {
  r.p = p; r.len = len; r.pos = at; r.acc = 0; r.bits = 0; r.over = 0;
}
AFX_FLAC_HD void br_refill(BitReader& r) {
  // One unaligned dword while four bytes are left (the window then holds 32 bits or more, which is the most a read asks
  // for); single bytes only for the frame's last three.  On the device a refill is a load the whole wave waits for, its
  // lanes being at different places of different frames: one load per refill, not a dword and a chain of bytes behind it.
  if (r.pos + 4 <= r.len) {
    if (r.bits <= 32) {
      r.acc |= (uint64_t)load_be32(r.p + r.pos) << (32 - r.bits);
      r.bits += 32; r.pos += 4;
    }
    return;
  }
  while (r.bits <= 56 && r.pos < r.len) {
    r.acc |= (uint64_t)r.p[r.pos++] << (56 - r.bits);
    r.bits += 8;
  }
}
AFX_FLAC_HD uint32_t br_read(BitReader& r, int n) {   // 0 <= n <= 32
  if (n == 0) return 0;
  if (r.bits < n) {
    br_refill(r);
    if (r.bits < n) { r.over = 1; r.acc = 0; r.bits = 0; return 0; }
  }
  const uint32_t v = (uint32_t)(r.acc >> (64 - n));
  r.acc <<= n;
  r.bits -= n;
  return v;
}
AFX_FLAC_HD int32_t br_read_signed(BitReader& r, int n) {   // 0 <= n <= 32
  if (n == 0) return 0;
  const uint32_t v = br_read(r, n);
  const uint32_t sign = 1u << (n - 1);
  return (int32_t)((v ^ sign) - sign);
}
AFX_FLAC_HD uint32_t br_unary(BitReader& r) {   // zeros in front of the next one; the run may cross any number of refills
  uint32_t q = 0;
  for (;;) {
    if (r.acc == 0) {
      q += (uint32_t)r.bits;
      r.bits = 0;
      br_refill(r);
      if (r.bits == 0) { r.over = 1; return 0; }   // the bytes are used up: the loop ends with the frame at the latest
      continue;
    }
    const int z = __builtin_clzll(r.acc);   // < bits: what lies below the valid bits is zero
    q += (uint32_t)z;
    r.acc <<= z;
    r.acc <<= 1;
    r.bits -= z + 1;
    return q;
  }
}
AFX_FLAC_HD int64_t br_bytes_used(const BitReader& r) { return r.pos - (r.bits >> 3); }   // after br_align

// Stage 1, the bit walk of ONE frame.  p[0 .. len) is the frame from its sync code to the end of its CRC-16, as the
// index delimits it.  work[0 .. stream_channels x blocksize) receives, per subframe, warm-ups and residuals; sub[0 ..
// stream_channels) the records; *assignment the channel assignment.  The blocksize is the index's: a header that states
// another fails the frame, so no count read from the stream ever sizes a loop or an address.
AFX_FLAC_HD int32_t walk_frame(const uint8_t* p, int64_t len, int32_t blocksize, int32_t stream_channels, int32_t stream_bits,
                               int32_t* work, Subframe* sub, int32_t* assignment) {
  *assignment = 0;
  FrameHeader h;
  const int head = parse_frame_header(p, len, &h);
  if (head == 0 || len < head + 2 || len > kMaxFrameBytes) return kFrameHeader;
  if (h.blocksize != blocksize || h.channels != stream_channels || (h.bits != 0 && h.bits != stream_bits)) return kFrameHeader;
  *assignment = h.assignment;
  const int64_t body_end = len - 2;
  if (crc16(p, body_end) != ((uint32_t)p[body_end] << 8 | (uint32_t)p[body_end + 1])) return kFrameCrc16;
  BitReader r;
  br_open(r, p, body_end, head);
  for (int c = 0; c < stream_channels; ++c) {
    Subframe& s = sub[c];
    int32_t* out = work + (int64_t)c * blocksize;
    const uint32_t lead = br_read(r, 8);   // zero bit, six bits of type, the wasted-bits flag
    if (lead & 0x80u) return kFrameSubframe;
    const uint32_t type = (lead >> 1) & 0x3Fu;
    uint32_t wasted = 0;
    if (lead & 1u) wasted = br_unary(r) + 1;
    const bool side = (h.assignment == 1 && c == 1) || (h.assignment == 2 && c == 0) || (h.assignment == 3 && c == 1);
    const int32_t depth = stream_bits + (side ? 1 : 0);
    if (r.over) return kFrameOverrun;
    if (wasted >= (uint32_t)depth) return kFrameSubframe;
    const int bps = depth - (int)wasted;   // 1..25
    s.wasted = (int32_t)wasted; s.order = 0; s.shift = 0;
    int order = 0;
    if (type == 0) {
      s.kind = kSubConstant;
      out[0] = br_read_signed(r, bps);
      continue;
    } else if (type == 1) {
      s.kind = kSubVerbatim;
      for (int i = 0; i < blocksize && !r.over; ++i) out[i] = br_read_signed(r, bps);
      continue;
    } else if (type >= 8 && type <= 12) {
      s.kind = kSubFixed;
      order = (int)type - 8;
    } else if (type >= 32) {
      s.kind = kSubLpc;
      order = (int)type - 31;
    } else {
      return kFrameSubframe;
    }
    if (order > blocksize) return kFrameSubframe;
    s.order = order;
    for (int i = 0; i < order; ++i) out[i] = br_read_signed(r, bps);
    if (s.kind == kSubLpc) {
      const int precision = (int)br_read(r, 4) + 1;
      const int32_t shift = br_read_signed(r, 5);
      if (precision == 16 || shift < 0) return r.over ? kFrameOverrun : kFrameSubframe;
      s.shift = shift;
      for (int i = 0; i < order; ++i) s.coef[i] = br_read_signed(r, precision);
    }
    // the residual: method, partition order, then 2^order partitions of Rice-coded or raw values
    const uint32_t method = br_read(r, 2);
    const int po = (int)br_read(r, 4);
    if (r.over) return kFrameOverrun;
    if (method > 1) return kFrameSubframe;
    const int param_bits = method == 0 ? 4 : 5;
    const uint32_t escape = method == 0 ? 15u : 31u;
    const int per_part = blocksize >> po;
    if ((po > 0 && ((per_part << po) != blocksize || per_part < order))) return kFrameSubframe;
    int at = order;
    for (int part = 0; part < (1 << po) && !r.over; ++part) {
      const int n = (part == 0) ? per_part - order : per_part;   // >= 0: order <= blocksize, and <= per_part when po > 0
      const uint32_t k = br_read(r, param_bits);
      if (k == escape) {
        const int raw = (int)br_read(r, 5);
        for (int i = 0; i < n && !r.over; ++i) out[at + i] = br_read_signed(r, raw);
      } else {
        for (int i = 0; i < n && !r.over; ++i) {
          const uint32_t q = br_unary(r);
          const uint32_t u = (q << k) | br_read(r, (int)k);
          out[at + i] = (int32_t)((u >> 1) ^ (0u - (u & 1u)));
        }
      }
      at += n;
    }
  }
  if (r.over) return kFrameOverrun;
  // zero padding up to the byte boundary, then the CRC-16: the walk has to stand exactly in front of it
  r.acc <<= (r.bits & 7);
  r.bits &= ~7;
  return br_bytes_used(r) == body_end ? kFrameOk : kFrameEnd;
}

// Stage 2, the restore of ONE subframe in place: data[0 .. blocksize) holds what the walk wrote and then the samples.
// 64-bit accumulation throughout (lpc.c's wide path; its 32-bit path gives the same integers wherever it is allowed).
AFX_FLAC_HD void restore_subframe(const Subframe& s, int32_t* data, int32_t blocksize) {
  const int order = s.order;
  if (s.kind == kSubSkip || order < 0 || order > kMaxLpcOrder || order > blocksize) return;
  if (s.kind == kSubConstant) {
    const int32_t v = data[0];
    for (int i = 1; i < blocksize; ++i) data[i] = v;
  } else if (s.kind == kSubFixed) {
    // fixed.c: the predictors 0, a, 2a - b, 3a - 3b + c, 4a - 6b + 4c - d on the last four samples
    uint32_t a = 0, b = 0, c = 0, d = 0;
    if (order > 0) a = (uint32_t)data[order - 1];
    if (order > 1) b = (uint32_t)data[order - 2];
    if (order > 2) c = (uint32_t)data[order - 3];
    if (order > 3) d = (uint32_t)data[order - 4];
    for (int i = order; i < blocksize; ++i) {
      uint32_t pred = 0;
      if (order == 1) pred = a;
      else if (order == 2) pred = 2u * a - b;
      else if (order == 3) pred = 3u * a - 3u * b + c;
      else if (order == 4) pred = 4u * a - 6u * b + 4u * c - d;
      const uint32_t v = (uint32_t)data[i] + pred;
      data[i] = (int32_t)v;
      d = c; c = b; b = a; a = v;
    }
  } else if (s.kind == kSubLpc) {
    const int shift = s.shift & 31;
    for (int i = order; i < blocksize; ++i) {
      uint64_t sum = 0;
      for (int j = 0; j < order; ++j) sum += (uint64_t)((int64_t)s.coef[j] * (int64_t)data[i - j - 1]);
      data[i] = (int32_t)((uint32_t)data[i] + (uint32_t)((int64_t)sum >> shift));
    }
  }
  if (s.wasted > 0) {
    const int w = s.wasted & 31;
    for (int i = 0; i < blocksize; ++i) data[i] = (int32_t)((uint32_t)data[i] << w);
  }
}

// Stage 3, ONE sample frame: the first two channels out of the frame's restored subframes, the stereo decorrelation
// undone.  ch0 / ch1: sample i of subframes 0 and 1 (ch1 unused for a mono stream).
AFX_FLAC_HD void undo_assignment(int32_t assignment, int32_t ch0, int32_t ch1, int32_t* left, int32_t* right) {
  const uint32_t a = (uint32_t)ch0, b = (uint32_t)ch1;
  if (assignment == 1) { *left = ch0; *right = (int32_t)(a - b); }          // left, side = left - right
  else if (assignment == 2) { *left = (int32_t)(a + b); *right = ch1; }     // side, right
  else if (assignment == 3) {                                               // mid = (l + r) >> 1 lost its low bit: it is side's
    const uint32_t mid = (a << 1) | (b & 1u);
    *left = (int32_t)(mid + b) >> 1;
    *right = (int32_t)(mid - b) >> 1;
  } else { *left = ch0; *right = ch1; }
}
// the native sample at dst: 16-bit -> int16, 8-bit -> int16 `v << 8` (AifFile.h: S8BitSignedTo16BitFloat), 24-bit -> packed
AFX_FLAC_HD void store_native(uint8_t* dst, int32_t v, int32_t stream_bits) {
  uint32_t u = (uint32_t)v;
  if (stream_bits == 8) u <<= 8;
  dst[0] = (uint8_t)u;
  dst[1] = (uint8_t)(u >> 8);
  if (stream_bits == 24) dst[2] = (uint8_t)(u >> 16);
}

}  // namespace flac
}  // namespace afx
