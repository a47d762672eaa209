// afec_amd/csrc/devio/afx_devio_plan.h -- everything the device-resident input and output decide before they enqueue
// anything: which source buffers are refused, the gather's per-buffer table and tile prefix, the export's
// per-series table, the extent of every destination, and every refusal.  Header-only and pure, in the manner of
// afx_raw_plan.h: no HIP call -- what the runtime says of a pointer comes in as a DevioAlloc; afx_device_io.cpp asks the
// runtime and enqueues from the record, tests/host/devio_plan_main.cpp checks it on the CPU.
#pragma once

#include <cstdint>
#include <vector>

#include "../../../include/afx.h"
#include "afx_devio.h"

namespace afx {
namespace host {

// What the runtime says of a pointer: whether it is device memory, on which device, and the allocation around it.
struct DevioAlloc {
  bool device = false;
  int32_t ordinal = -1;
  uint64_t base = 0, size = 0;
};

// [p, p + bytes) lies inside the allocation, and that on `device`
inline bool devio_range_ok(const DevioAlloc& a, int32_t device, const void* p, uint64_t bytes) {
  const uint64_t at = (uint64_t)(uintptr_t)p;
  return a.device && a.ordinal == device && at >= a.base && bytes <= a.size && at - a.base <= a.size - bytes;
}

// ---- input ----

// the buffers afx_batch_create's rule would go on to read: only these have a range to check
inline bool devio_buffer_is_read(const afx_buf& s) {
  return s.n_samples > 0 && s.pcm && (s.dtype == AFX_PCM_F32 || s.dtype == AFX_PCM_F64);
}

// The caller's buffers as afx_batch_create's rule is to see them: a buffer whose range is not inside one allocation of
// the device carries a negative length from here on, which that rule refuses with AFX_ERR_BAD_BUFFER (and which keeps
// the buffer from deciding the batch's dtype).  allocs[i] is read for the buffers of devio_buffer_is_read only.
inline std::vector<afx_buf> devio_checked_buffers(const afx_buf* bufs, const DevioAlloc* allocs, int32_t n_bufs, int32_t device) {
  std::vector<afx_buf> out(bufs, bufs + (n_bufs > 0 ? n_bufs : 0));
  for (int32_t i = 0; i < n_bufs; ++i) {
    if (!devio_buffer_is_read(bufs[i])) continue;
    const uint64_t esz = bufs[i].dtype == AFX_PCM_F64 ? 8 : 4;
    const bool fits = (uint64_t)bufs[i].n_samples <= (uint64_t)INT64_MAX / 8;
    if (!fits || !devio_range_ok(allocs[i], device, bufs[i].pcm, (uint64_t)bufs[i].n_samples * esz)) out[(size_t)i].n_samples = -1;
  }
  return out;
}

// The gather's table: one entry per buffer that keeps samples in the arena (used[i] > 0), in the caller's order, with the
// prefix of their tiles.  ok = false: beyond the kernel's 32-bit tile prefix, the batch is refused.
struct GatherPlan {
  std::vector<DevioBuf> table;
  int64_t tiles = 0;
  bool ok = true;
};
inline GatherPlan plan_gather(const afx_buf* bufs, const int64_t* used, const int64_t* arena_off, int32_t n_bufs) {
  GatherPlan p;
  for (int32_t i = 0; i < n_bufs; ++i) {
    if (used[i] <= 0) continue;
    const int64_t t = devio_tiles(used[i]);
    if (p.tiles > 0x7FFFFFFF - t) { p.ok = false; p.table.clear(); p.tiles = 0; return p; }
    p.table.push_back(DevioBuf{bufs[i].pcm, arena_off[i], used[i], (int32_t)p.tiles, 0});
    p.tiles += t;
  }
  return p;
}

// ---- output ----

// what an export needs to know of the batch
struct ExportShape {
  bool ran = false;
  int32_t n_bufs = 0;
  const int64_t* frame_offset = nullptr;   // [n_bufs + 1], host
  int32_t stride = 0;                      // of a record row
  const int32_t* offsets = nullptr;        // [AFX_NUM_SERIES]: first column, -1 = not in the mask
  const int32_t* widths = nullptr;         // [AFX_NUM_SERIES]
  bool has_magnitude = false;              // AFX_D_MAGNITUDE in the mask
  bool has_statistics = false;             // AFX_D_STATISTICS in the mask
};

struct ExportPlan {
  int status = AFX_OK;        // AFX_OK or AFX_ERR_INVALID_ARG
  const char* why = "";
  DevioExportArgs args{};     // rec, mag and frame_offset are the enqueuing side's to set
  std::vector<uint64_t> extent_bytes;   // [n_outs]: what the launch may write counts from dst (0: nothing)
  bool needs_frame_offsets = false;     // the kernel reads the device copy of frame_offset
};

inline ExportPlan export_refused(const char* why) {
  ExportPlan p;
  p.status = AFX_ERR_INVALID_ARG;
  p.why = why;
  return p;
}

// a * b + c in int64, false on overflow (all three are >= 0 here)
inline bool devio_mul_add(int64_t a, int64_t b, int64_t c, int64_t* out) {
  int64_t m = 0;
  return !__builtin_mul_overflow(a, b, &m) && !__builtin_add_overflow(m, c, out);
}

// series number -> first column and width; false: not a series of this batch
inline bool devio_series(const ExportShape& s, int32_t series, bool statistics, int32_t* col, int32_t* width, int32_t* from_mag) {
  if (series == AFX_SERIES_MAGNITUDE) {
    if (statistics || !s.has_magnitude) return false;
    *col = 0; *width = 1024; *from_mag = 1;
    return true;
  }
  if (series < 0 || series >= AFX_NUM_SERIES || s.offsets[series] < 0) return false;
  *col = s.offsets[series]; *width = s.widths[series]; *from_mag = 0;
  return true;
}

inline ExportPlan plan_export(const ExportShape& s, const afx_device_out* outs, int32_t n_outs, int32_t layout, int64_t max_frames,
                              double pad_value) {
  if (!s.ran) return export_refused("export before afx_batch_run");
  if (n_outs < 0 || n_outs > kDevioMaxOuts || (n_outs > 0 && !outs)) return export_refused("bad number of destinations");
  if (layout != AFX_EXPORT_PACKED && layout != AFX_EXPORT_PADDED) return export_refused("bad layout");
  if (s.stride > kDevioMaxStride) return export_refused("record wider than the export kernel's tile");
  const bool padded = layout == AFX_EXPORT_PADDED;
  const int64_t frames = s.n_bufs > 0 ? s.frame_offset[s.n_bufs] : 0;
  int64_t longest = 0;
  for (int32_t i = 0; i < s.n_bufs; ++i) longest = s.frame_offset[i + 1] - s.frame_offset[i] > longest ? s.frame_offset[i + 1] - s.frame_offset[i] : longest;
  ExportPlan p;
  DevioExportArgs& a = p.args;
  a.frames = frames;
  a.stride = s.stride; a.n_bufs = s.n_bufs; a.n_outs = n_outs; a.padded = padded ? 1 : 0;
  a.pad_value = pad_value;
  a.data_tiles = (uint32_t)((frames + kDevioRows - 1) / kDevioRows);   // frames < 2^31 (build_batch)
  if (padded) {
    if (max_frames < longest) return export_refused("max_frames below the longest file");
    int64_t slots = 0;
    if (!devio_mul_add(s.n_bufs, max_frames, 0, &slots)) return export_refused("n_bufs x max_frames overflows");
    a.max_frames = max_frames;
    a.pad_rows = slots - frames;
    if ((a.pad_rows + kDevioRows - 1) / kDevioRows + a.data_tiles > 0x7FFFFFFF) return export_refused("more padding rows than one launch covers");
    p.needs_frame_offsets = s.n_bufs > 0;
  }
  p.extent_bytes.assign((size_t)n_outs, 0);
  for (int32_t k = 0; k < n_outs; ++k) {
    const afx_device_out& o = outs[k];
    DevioSeries& d = a.outs[k];
    if (!o.dst) return export_refused("null destination");
    if (o.dtype != AFX_PCM_F32 && o.dtype != AFX_PCM_F64) return export_refused("bad destination dtype");
    if (!devio_series(s, o.series, false, &d.col, &d.width, &d.from_mag)) return export_refused("series not in the batch mask");
    if (o.row_stride < d.width) return export_refused("row_stride below the series' width");
    d.dst = o.dst; d.row_stride = o.row_stride; d.f32 = o.dtype == AFX_PCM_F32 ? 1 : 0;
    int64_t elements = 0;
    if (padded) {
      int64_t slot = 0;
      if (!devio_mul_add(max_frames, o.row_stride, 0, &slot)) return export_refused("max_frames x row_stride overflows");
      if (o.buf_stride < slot) return export_refused("buf_stride below max_frames x row_stride");
      d.buf_stride = o.buf_stride;
      if (s.n_bufs > 0 && max_frames > 0) {
        int64_t last_row = 0;
        if (!devio_mul_add(s.n_bufs - 1, o.buf_stride, 0, &elements) || !devio_mul_add(max_frames - 1, o.row_stride, d.width, &last_row) ||
            __builtin_add_overflow(elements, last_row, &elements))
          return export_refused("destination extent overflows");
      }
    } else if (frames > 0 && !devio_mul_add(frames - 1, o.row_stride, d.width, &elements)) {
      return export_refused("destination extent overflows");
    }
    if (elements > INT64_MAX / 8) return export_refused("destination extent overflows");
    p.extent_bytes[(size_t)k] = (uint64_t)elements * (d.f32 ? 4 : 8);
  }
  return p;
}

struct StatsExportPlan {
  int status = AFX_OK;
  const char* why = "";
  DevioStatsArgs args{};      // stats is the enqueuing side's to set
  std::vector<uint64_t> extent_bytes;
};
inline StatsExportPlan plan_export_statistics(const ExportShape& s, const afx_device_out* outs, int32_t n_outs) {
  StatsExportPlan p;
  auto refused = [&](const char* why) { p.status = AFX_ERR_INVALID_ARG; p.why = why; p.extent_bytes.clear(); return p; };
  if (!s.ran) return refused("export before afx_batch_run");
  if (!s.has_statistics) return refused("AFX_D_STATISTICS was not in the batch mask");
  if (n_outs < 0 || n_outs > kDevioMaxOuts || (n_outs > 0 && !outs)) return refused("bad number of destinations");
  p.args.stride = s.stride; p.args.n_bufs = s.n_bufs; p.args.n_outs = n_outs;
  p.extent_bytes.assign((size_t)n_outs, 0);
  for (int32_t k = 0; k < n_outs; ++k) {
    const afx_device_out& o = outs[k];
    DevioSeries& d = p.args.outs[k];
    if (!o.dst) return refused("null destination");
    if (o.dtype != AFX_PCM_F32 && o.dtype != AFX_PCM_F64) return refused("bad destination dtype");
    if (!devio_series(s, o.series, true, &d.col, &d.width, &d.from_mag)) return refused("series not in the batch mask");
    d.dst = o.dst; d.f32 = o.dtype == AFX_PCM_F32 ? 1 : 0;
    p.extent_bytes[(size_t)k] = (uint64_t)s.n_bufs * (uint64_t)d.width * AFX_NUM_STATISTICS * (d.f32 ? 4 : 8);
  }
  return p;
}

// every destination's extent inside one allocation of the device (allocs[k] is read where the extent is not empty)
inline bool devio_extents_ok(const afx_device_out* outs, const std::vector<uint64_t>& extent_bytes, const DevioAlloc* allocs, int32_t device) {
  for (size_t k = 0; k < extent_bytes.size(); ++k)
    if (extent_bytes[k] > 0 && !devio_range_ok(allocs[k], device, outs[k].dst, extent_bytes[k])) return false;
  return true;
}

}  // namespace host
}  // namespace afx
