// afec_amd/csrc/devio/afx_devio_raw_plan.h -- everything LoadSample on device-resident audio decides before it enqueues
// anything: the caller's afx_raw_device buffers as check_raw / plan_raw_arena (afx_raw_plan.h) are to see
// them, the gather's table and tile prefix from RawPlan::pieces, and the sample export's extent and refusals.
// Header-only and pure, as afx_devio_plan.h is: what the runtime says of a pointer comes in as a DevioAlloc;
// afx_device_io.cpp asks the runtime and enqueues from the record, tests/host/devio_raw_plan_main.cpp checks it on the CPU.
#pragma once

#include <cstdint>
#include <vector>

#include "../../../include/afx.h"
#include "../afx_raw_plan.h"
#include "afx_devio_plan.h"
#include "afx_devio_raw.h"

namespace afx {
namespace host {

// ---- input ----

// the buffers check_raw would go on to accept as PCM: only these have a range to check (a FLAC stream never: its index
// would have to be read on the host)
inline bool devio_raw_is_read(const afx_raw_device& d) {
  return d.format != AFX_RAW_FLAC && d.data && d.n_frames > 0 && d.n_frames < 0x7FFFFFFF && d.sample_rate >= 0 &&
         raw_bytes_per_sample(d.format) != 0 && d.channels >= 1 && d.channels <= 8;
}

// The bytes from `data` that the gather may read of a buffer of devio_raw_is_read: n_frames x channels x bps interleaved,
// ((channels - 1) x channel_stride + n_frames) x bps planar.  false: a layout that is neither of the two, a planar
// channel_stride below n_frames, or an extent that overflows.
inline bool devio_raw_extent(const afx_raw_device& d, uint64_t* bytes) {
  const int64_t bps = raw_bytes_per_sample(d.format);
  int64_t samples = 0;
  if (d.layout == AFX_RAW_INTERLEAVED) {
    samples = d.n_frames * d.channels;   // below 2^34
  } else if (d.layout == AFX_RAW_PLANAR) {
    if (d.channel_stride < d.n_frames || !devio_mul_add(d.channels - 1, d.channel_stride, d.n_frames, &samples)) return false;
  } else {
    return false;
  }
  if (samples > INT64_MAX / 8) return false;
  *bytes = (uint64_t)samples * (uint64_t)bps;
  return true;
}

// The caller's buffers as check_raw is to see them: a buffer whose layout, stride or extent is refused, or whose range is
// not inside one allocation of the device, has a null `data` from here on, which check_raw refuses with
// AFX_ERR_BAD_BUFFER.  Everything else goes through unchanged and gets check_raw's own status; a FLAC stream keeps its
// format and is refused by a plan made without the decoder (AFX_ERR_UNSUPPORTED), its descriptor unread.
// allocs[i] is read for the buffers of devio_raw_is_read only.
inline std::vector<afx_raw> devio_raw_checked(const afx_raw_device* raws, const DevioAlloc* allocs, int32_t n_bufs, int32_t device) {
  std::vector<afx_raw> out((size_t)(n_bufs > 0 ? n_bufs : 0));
  for (int32_t i = 0; i < n_bufs; ++i) {
    const afx_raw_device& d = raws[i];
    out[(size_t)i] = afx_raw{d.data, d.format, d.channels, d.sample_rate, 0, d.n_frames};
    if (!devio_raw_is_read(d)) continue;
    uint64_t bytes = 0;
    if (!devio_raw_extent(d, &bytes) || !devio_range_ok(allocs[i], device, d.data, bytes)) out[(size_t)i].data = nullptr;
  }
  return out;
}

// The gather's table: one entry per piece of the plan (one per accepted buffer, in the caller's order: a plan made
// without the FLAC decoder has no other pieces), the planar ones carrying channels, sample size and plane stride, with the
// prefix of their tiles.  ok = false: beyond the kernel's 32-bit tile prefix, the batch is refused.
struct RawGatherPlan {
  std::vector<DevioRawBuf> table;
  int64_t tiles = 0;
  bool ok = true;
};
inline RawGatherPlan plan_raw_gather(const RawPlan& plan, const afx_raw_device* raws) {
  RawGatherPlan g;
  for (const RawPlan::Piece& p : plan.pieces) {
    const afx_raw_device& d = raws[p.buf];
    const int64_t t = devio_raw_tiles(d.n_frames);
    if (g.tiles > 0x7FFFFFFF - t) { g.ok = false; g.table.clear(); g.tiles = 0; return g; }
    const bool planar = d.layout == AFX_RAW_PLANAR;
    g.table.push_back(DevioRawBuf{p.src, p.dst, d.n_frames, planar ? d.channel_stride : 0, (int32_t)g.tiles, d.channels,
                                  raw_bytes_per_sample(d.format), planar ? 1 : 0});
    g.tiles += t;
  }
  return g;
}

// ---- output ----

struct SamplesExportPlan {
  int status = AFX_OK;        // AFX_OK or AFX_ERR_INVALID_ARG
  const char* why = "";
  uint64_t extent_bytes = 0;  // what the launch may write counts from dst (0: nothing)
  int32_t tiles_per_row = 0;
  int32_t f32 = 0;
};
// used: [n_bufs], the analysed prefixes' lengths
inline SamplesExportPlan plan_export_samples(const int64_t* used, int32_t n_bufs, const void* dst, int32_t dtype, int64_t buf_stride) {
  SamplesExportPlan p;
  auto refused = [&](const char* why) { p = SamplesExportPlan{}; p.status = AFX_ERR_INVALID_ARG; p.why = why; return p; };
  if (!dst) return refused("null destination");
  if (dtype != AFX_PCM_F32 && dtype != AFX_PCM_F64) return refused("bad destination dtype");
  int64_t longest = 0;
  for (int32_t i = 0; i < n_bufs; ++i) longest = used[i] > longest ? used[i] : longest;
  if (buf_stride < longest) return refused("buf_stride below the longest file's samples");
  p.f32 = dtype == AFX_PCM_F32 ? 1 : 0;
  if (n_bufs <= 0 || buf_stride == 0) return p;
  // (n_bufs - 1) x buf_stride + buf_stride elements
  int64_t elements = 0;
  if (!devio_mul_add(n_bufs - 1, buf_stride, buf_stride, &elements) || elements > INT64_MAX / 8) return refused("destination extent overflows");
  const int64_t tiles = (buf_stride - 1) / kDevioSampleTile + 1;
  if (tiles > 0x7FFFFFFF / n_bufs) return refused("more tiles than one launch covers");
  p.tiles_per_row = (int32_t)tiles;
  p.extent_bytes = (uint64_t)elements * (p.f32 ? 4 : 8);
  return p;
}

}  // namespace host
}  // namespace afx
