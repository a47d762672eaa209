// afec_amd/csrc/afx_raw_plan.h -- everything afx_batch_create_from_raw decides before it enqueues anything: which buffers
// are refused and why, the tables the kernels read, every offset in the raw arena, what goes up from where, and the layout
// of the page-locked block.  Header-only and pure: no HIP call, no workspace; afx_batch_create.cpp enqueues
// from the record, tests/host/raw_plan_main.cpp checks it on the CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/afx.h"
#include "afx_internal.h"
#include "flac/afx_flac.h"
#include "rawpcm/afx_rawpcm.h"

namespace afx {
namespace host {

// The raw arena, in this order; every slot starts on a 16-byte boundary and is padded to one:
//   [0, conv_off)                     decoded PCM, one slot per accepted buffer in the caller's order (a FLAC's slot holds
//                                     the PCM of its first two channels once it is decoded)
//   [conv_off, flac_off)              per converted file its mono mix with kResampleMargin zeros either side, then its
//                                     converted samples
//   [flac_off, flac_work_off)         per FLAC file its frames as they lie in the file and behind them its index (the order
//                                     a staging buffer holds them in, so one transfer can move both)
//   [flac_work_off, flac_table_off)   per FLAC file, written on the device only: int32 work area, subframe records, the
//                                     frames' channel assignments
//   [flac_table_off, flac_status_off) the decoder's table;  [flac_status_off, ..) one status word per FLAC file
// The page-locked block: the file table, (64-byte aligned) the byte-order kernel's table -- both go up in one copy of
// tables_bytes --, the scan results and the FLAC status words on their way down.
struct RawPlan {
  struct Piece { const char* src; int64_t dst, bytes; int32_t buf; };   // host memory -> byte offset in the arena
  struct Pin { size_t be_off, tables_bytes, scan_off, scan_bytes, flac_status_off, flac_status_bytes, bytes; };
  int32_t n_bufs = 0;
  std::vector<int32_t> status;          // [n_bufs]
  std::vector<LoadFile> files;          // [n_bufs]: what the scan kernels read; a converted file is {out_off, n_out, 1, kRawMonoFloat}
  std::vector<int32_t> file_rate;       // [n_bufs]: 0 = the plan's
  std::vector<ResampleFile> conv;       // files at another rate than the plan's: converted on the GPU first
  std::vector<RawNativeFile> be;        // big-endian files: made native in place before anything reads them
  std::vector<FlacFile> flac;           // AFX_RAW_FLAC files: decoded first of all
  std::vector<int32_t> conv_buf, flac_buf;   // the buffer index of each entry
  int64_t group_slots = 0, conv_blocks = 0, conv_max_in = 0;
  int64_t be_tiles = 0;                 // -1: beyond the kernel's 32-bit prefix, the batch is refused
  int64_t flac_frames = 0, flac_tiles = 0;
  int64_t conv_off = 0, flac_off = 0, flac_work_off = 0, flac_table_off = 0, flac_status_off = 0, arena_bytes = 0;
  std::vector<Piece> pieces;            // the caller's bytes of the accepted buffers, in buffer order
  Pin pin{};
};

inline int64_t pad16(int64_t bytes) { return (bytes + 15) & ~(int64_t)15; }
inline size_t pad64(size_t bytes) { return (bytes + 63) & ~(size_t)63; }

// bytes per sample of the decoded PCM formats (0: unknown format)
inline int raw_bytes_per_sample(int format) {
  switch (format) {
    case AFX_RAW_I16: case AFX_RAW_I16_BE: return 2;
    case AFX_RAW_I24: case AFX_RAW_I24_BE: return 3;
    case AFX_RAW_F32: case AFX_RAW_I32: case AFX_RAW_F32_BE: case AFX_RAW_I32_BE: return 4;
    case AFX_RAW_F64: case AFX_RAW_F64_BE: return 8;
    default: return 0;
  }
}

// of afx_raw::format, the caller's, and of nothing else: the native format of the same width and meaning
// (raw_native_kernel turns the bytes round); -1 for a native format
inline int native_twin(int format) {
  switch (format) {
    case AFX_RAW_I16_BE: return AFX_RAW_I16;
    case AFX_RAW_I24_BE: return AFX_RAW_I24;
    case AFX_RAW_F32_BE: return AFX_RAW_F32;
    case AFX_RAW_I32_BE: return AFX_RAW_I32;
    case AFX_RAW_F64_BE: return AFX_RAW_F64;
    default: return -1;
  }
}

// A FLAC buffer as the caller describes it: the native format its samples are decoded to (-1: a depth that is not
// decoded), and whether the descriptor and its index can be handed to the kernels as they are.  The kernels form every
// address from the index, so it is held to: {0, 0} first, offsets and samples strictly rising, no frame above
// kMaxFrameBytes or kMaxBlocksize, the sentinel equal to the stream's bytes and the buffer's sample count.
inline int flac_native_format(const afx_flac_stream& s) {
  return s.bits_per_sample == 16 || s.bits_per_sample == 8 ? AFX_RAW_I16 : s.bits_per_sample == 24 ? AFX_RAW_I24 : -1;
}
inline bool flac_descriptor_ok(const afx_raw& f, const afx_flac_stream& s) {
  if (!s.frames || !s.index || s.n_index < 1 || s.frames_bytes < 1 || s.frames_bytes >= ((int64_t)1 << 40)) return false;
  if (s.stream_channels < 1 || s.stream_channels > 8 || f.channels != std::min(s.stream_channels, 2)) return false;
  return flac::index_ok(s.index, s.n_index, s.frames_bytes, f.n_frames);
}

// AFX_OK and the native format of the buffer's PCM slot, or why the buffer is refused (SampleAnalyser.cpp:472-482: 1..8
// channels, non-empty).  `frames` and `tiles` are the FLAC files accepted in front of it.
inline int32_t check_raw(const afx_raw& f, bool have_raw_native, bool have_flac_decode, int64_t frames, int64_t tiles, int* native) {
  const bool shaped = f.data && f.n_frames > 0 && f.n_frames < 0x7FFFFFFF && f.sample_rate >= 0;
  if (f.format != AFX_RAW_FLAC) {
    if (!shaped || !raw_bytes_per_sample(f.format) || f.channels < 1 || f.channels > 8) return AFX_ERR_BAD_BUFFER;
    // a build without the byte-order kernel (the mock device) refuses a big-endian file like any other it cannot take
    if (native_twin(f.format) >= 0 && !have_raw_native) return AFX_ERR_UNSUPPORTED;
    *native = native_twin(f.format) >= 0 ? native_twin(f.format) : f.format;
    return AFX_OK;
  }
  if (!shaped) return AFX_ERR_BAD_BUFFER;
  // a build without the decoder (the mock device) refuses the file like any other it cannot take, its descriptor unread
  if (!have_flac_decode) return AFX_ERR_UNSUPPORTED;
  const afx_flac_stream& s = *(const afx_flac_stream*)f.data;
  if ((*native = flac_native_format(s)) < 0) return AFX_ERR_UNSUPPORTED;
  if (!flac_descriptor_ok(f, s)) return AFX_ERR_BAD_BUFFER;
  // the kernels' prefixes over frames and output tiles are 32-bit: the file that would take a batch beyond them is
  // refused, for itself alone (as a conversion beyond the resampler's block count is)
  return frames > 0x3FFFFFFF - s.n_index || tiles > 0x7FFFFFFF - flac_output_tiles(f.n_frames) ? AFX_ERR_UNSUPPORTED : AFX_OK;
}

inline RawPlan plan_raw_arena(const afx_raw* raws, int32_t n_bufs, int32_t plan_rate, bool have_raw_native, bool have_flac_decode) {
  RawPlan p;
  p.n_bufs = n_bufs;
  p.status.assign((size_t)n_bufs, AFX_OK);
  p.files.assign((size_t)n_bufs, LoadFile{0, 0, 0, 0});
  p.file_rate.assign((size_t)n_bufs, 0);
  // the PCM slots, back to back: a buffer refused here takes no space, one refused below keeps its slot
  std::vector<int64_t> slot((size_t)n_bufs, 0);
  for (int64_t i = 0, frames = 0, tiles = 0; i < n_bufs; ++i) {
    const afx_raw& f = raws[i];
    int native = -1;
    if ((p.status[(size_t)i] = check_raw(f, have_raw_native, have_flac_decode, frames, tiles, &native)) != AFX_OK) continue;
    if (f.format == AFX_RAW_FLAC) frames += ((const afx_flac_stream*)f.data)->n_index, tiles += flac_output_tiles(f.n_frames);
    p.files[(size_t)i] = LoadFile{slot[(size_t)i] = p.conv_off, f.n_frames, f.channels, native};
    p.conv_off += pad16(f.n_frames * f.channels * raw_bytes_per_sample(native));
  }
  // Sample-rate conversion (SampleAnalyser.cpp:563-607): Speed = file rate / analyser rate in double, the converter runs
  // at factor 1 / Speed and fills NewSizeInSamples = max(1, d2iRound(n / Speed)) samples; the LoadSample kernels then read
  // the converted samples as a mono file of "16-bit floats".
  // What is refused, for that buffer only (AFX_ERR_UNSUPPORTED -> a "Sample failed to load" row; the reference would
  // convert these too): a file above 16 x the analyser's rate (705.6 kHz: outside what the kernels' zero margins cover),
  // and a file whose conversion yields 2^30 samples or more (6.8 hours at 44.1 kHz, 4 GiB of floats; the kernels index a
  // file's samples with 32 bits) -- a header that claims 1 Hz makes a 96 KB file 2^31 samples.  Until round 5 the bounds
  // were a rate below the analyser's / 64 and 2^28 samples: a two-hour 48 kHz recording became a failed row.  The
  // crawler cuts batches by the converted size (TCrawlOptions::mDeviceBytesPerBatch), so a long file travels alone.
  constexpr double kMaxConvertedSamples = 1073741824.0;
  p.flac_off = p.conv_off;
  for (int i = 0; i < n_bufs; ++i) {
    const afx_raw& f = raws[i];
    if (p.status[(size_t)i] != AFX_OK || f.sample_rate == 0 || f.sample_rate == plan_rate) continue;
    p.file_rate[(size_t)i] = f.sample_rate;
    const double speed = (double)f.sample_rate / (double)plan_rate;
    if (speed == 1.0) continue;
    const double factor = 1.0 / speed, scaled = (double)(int)f.n_frames / speed;
    const double n_out_d = std::floor(scaled + 0.5);               // TMath::d2iRound of a positive value (InlineMath.inl:823-826)
    if (n_out_d >= kMaxConvertedSamples || factor < 1.0 / 16.0 || p.conv_blocks > 0x7FFFFFF0) {
      p.status[(size_t)i] = AFX_ERR_UNSUPPORTED;
      p.files[(size_t)i] = LoadFile{0, 0, 0, 0};
      continue;
    }
    ResampleFile c{};
    c.raw_off = slot[(size_t)i]; c.n_in = f.n_frames; c.channels = f.channels; c.format = p.files[(size_t)i].format; c.factor = factor;
    c.n_out = std::max<int64_t>(1, (int64_t)n_out_d);
    c.mono_off = p.flac_off;
    c.out_off = c.mono_off + pad16((c.n_in + 2 * kResampleMargin) * 4);
    p.flac_off = c.out_off + pad16(c.n_out * 4);
    c.group_off = p.group_slots;                      // one record per 16 output samples
    p.group_slots += (c.n_out + 15) / 16;
    c.block_off = p.conv_blocks;
    p.conv_blocks += resample_blocks(c.n_out);
    p.conv_max_in = std::max(p.conv_max_in, c.n_in);
    p.conv.push_back(c);
    p.conv_buf.push_back(i);
    p.files[(size_t)i] = LoadFile{c.out_off, c.n_out, 1, kRawMonoFloat};
  }
  // what goes up of the buffers that are still good, and the tables of the steps that make it native PCM
  p.flac_work_off = p.flac_off;
  for (int i = 0; i < n_bufs; ++i) {
    const afx_raw& f = raws[i];
    if (p.status[(size_t)i] != AFX_OK) continue;
    if (f.format == AFX_RAW_FLAC) {
      const afx_flac_stream& s = *(const afx_flac_stream*)f.data;
      const int64_t index_bytes = ((int64_t)s.n_index + 1) * (int64_t)sizeof(afx_flac_frame);
      FlacFile d{};
      d.out_off = slot[(size_t)i];
      d.n_samples = f.n_frames; d.n_index = s.n_index; d.bits = s.bits_per_sample; d.stream_channels = s.stream_channels;
      d.bytes_off = p.flac_work_off;
      d.index_off = d.bytes_off + pad16(s.frames_bytes);
      p.flac_work_off = d.index_off + index_bytes;
      d.frame_first = (int32_t)p.flac_frames;
      d.tile_first = (int32_t)p.flac_tiles;
      p.flac_frames += s.n_index;
      p.flac_tiles += flac_output_tiles(d.n_samples);
      p.flac.push_back(d);
      p.flac_buf.push_back(i);
      p.pieces.push_back(RawPlan::Piece{(const char*)s.frames, d.bytes_off, s.frames_bytes, i});
      p.pieces.push_back(RawPlan::Piece{(const char*)s.index, d.index_off, index_bytes, i});
      continue;
    }
    const int bps = raw_bytes_per_sample(f.format);
    const int64_t bytes = f.n_frames * f.channels * bps;
    p.pieces.push_back(RawPlan::Piece{(const char*)f.data, slot[(size_t)i], bytes, i});
    if (native_twin(f.format) < 0 || p.be_tiles < 0) continue;
    if (p.be_tiles > 0x7FFFFFFF - raw_native_tiles(bytes)) { p.be_tiles = -1; continue; }
    p.be.push_back(RawNativeFile{slot[(size_t)i], bytes, bps, (int32_t)p.be_tiles});
    p.be_tiles += raw_native_tiles(bytes);
  }
  p.flac_table_off = p.flac_work_off;
  for (FlacFile& d : p.flac) {
    d.work_off = p.flac_table_off;
    d.sub_off = d.work_off + pad16(d.n_samples * d.stream_channels * 4);
    d.assign_off = d.sub_off + (int64_t)d.n_index * d.stream_channels * (int64_t)sizeof(flac::Subframe);
    p.flac_table_off = d.assign_off + pad16((int64_t)d.n_index * 4);
  }
  RawPlan::Pin& pin = p.pin;
  pin.flac_status_bytes = p.flac.size() * sizeof(int32_t);
  p.flac_status_off = p.flac_table_off + pad16((int64_t)(p.flac.size() * sizeof(FlacFile)));
  p.arena_bytes = p.flac_status_off + pad16((int64_t)pin.flac_status_bytes) + 16;
  const size_t files_bytes = p.files.size() * sizeof(LoadFile), be_bytes = p.be.size() * sizeof(RawNativeFile);
  pin.be_off = pad64(files_bytes);
  pin.tables_bytes = be_bytes ? pin.be_off + be_bytes : files_bytes;
  pin.scan_off = pad64(pin.tables_bytes);
  pin.scan_bytes = (size_t)n_bufs * sizeof(LoadScan);
  pin.flac_status_off = pad64(pin.scan_off + pin.scan_bytes);
  pin.bytes = pin.flac_status_off + pin.flac_status_bytes;
  return p;
}

}  // namespace host
}  // namespace afx
