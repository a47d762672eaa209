// tests/host/devio_plan_main.cpp -- afec_amd/csrc/devio/afx_devio_plan.h on the CPU: what the device-resident input and
// output decide before anything is enqueued.  Literal tile prefixes of a ragged batch, the extents of packed and padded
// destinations, every refusal of include/afx.h, and the overflows.  Driven by tests/test_devio_plan_cpu.py, plain and
// under AddressSanitizer + UBSan.  Prints "ok <checks>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "devio/afx_devio_plan.h"

using namespace afx::host;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) { ++g_failed; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } \
  } while (0)

static const void* at(uint64_t a) { return (const void*)(uintptr_t)a; }
static afx_buf buf(uint64_t p, int dtype, int64_t n) { return afx_buf{at(p), dtype, 0, n}; }
static DevioAlloc dev(uint64_t base, uint64_t size, int ordinal = 0) { DevioAlloc a; a.device = true; a.ordinal = ordinal; a.base = base; a.size = size; return a; }

static void ranges() {
  const DevioAlloc a = dev(0x1000, 0x100);
  CHECK(devio_range_ok(a, 0, at(0x1000), 0x100));
  CHECK(devio_range_ok(a, 0, at(0x10FC), 4));
  CHECK(!devio_range_ok(a, 0, at(0x10FC), 5));          // leaves the allocation by one byte
  CHECK(!devio_range_ok(a, 0, at(0x0FFF), 4));          // starts in front of it
  CHECK(!devio_range_ok(a, 1, at(0x1000), 4));          // another device's
  CHECK(!devio_range_ok(DevioAlloc{}, 0, at(0x1000), 4));   // host memory
  CHECK(!devio_range_ok(a, 0, at(0x1000), ~(uint64_t)0));   // no wrap-around
  CHECK(!devio_range_ok(dev(~(uint64_t)0 - 15, 16), 0, at(~(uint64_t)0 - 7), 16));
}

static void sources() {
  // valid f32, host pointer, valid f32 slice one element in, range that leaves, another device, null with samples, negative
  // length, second dtype, unknown dtype, empty, a length whose bytes overflow
  const afx_buf bufs[] = {buf(0x1000, AFX_PCM_F32, 64), buf(0x9000, AFX_PCM_F32, 8), buf(0x1004, AFX_PCM_F32, 63), buf(0x1004, AFX_PCM_F32, 64),
                          buf(0x2000, AFX_PCM_F32, 4), buf(0, AFX_PCM_F32, 5), buf(0x1000, AFX_PCM_F32, -3), buf(0x3000, AFX_PCM_F64, 8),
                          buf(0x1000, 7, 8), buf(0x1000, AFX_PCM_F32, 0), buf(0x1000, AFX_PCM_F64, INT64_MAX / 4)};
  const int n = (int)(sizeof(bufs) / sizeof(bufs[0]));
  std::vector<DevioAlloc> allocs((size_t)n, dev(0x1000, 256));
  allocs[1] = DevioAlloc{};
  allocs[4] = dev(0x2000, 256, 3);
  allocs[7] = dev(0x3000, 64);
  const std::vector<afx_buf> c = devio_checked_buffers(bufs, allocs.data(), n, 0);
  const int64_t want[] = {64, -1, 63, -1, -1, 5, -3, 8, 8, 0, -1};
  for (int i = 0; i < n; ++i) {
    CHECK(c[(size_t)i].n_samples == want[i]);
    CHECK(c[(size_t)i].pcm == bufs[i].pcm && c[(size_t)i].dtype == bufs[i].dtype);
  }
  CHECK(devio_checked_buffers(nullptr, nullptr, 0, 0).empty());
}

static void gather() {
  const int64_t T = afx::kDevioTileSamples;
  const int64_t used[] = {0, 1, T - 1, T, T + 1, 0, 3 * T + 1};
  const int64_t off[] = {0, 0, 4, T + 4, 2 * T + 4, 0, 4 * T + 8};
  afx_buf bufs[7];
  for (int i = 0; i < 7; ++i) bufs[i] = buf(0x10000 + 0x100000 * (uint64_t)i, AFX_PCM_F32, used[i]);
  const GatherPlan p = plan_gather(bufs, used, off, 7);
  CHECK(p.ok && p.tiles == 9 && p.table.size() == 5);
  const int32_t first[] = {0, 1, 2, 3, 5};
  const int which[] = {1, 2, 3, 4, 6};
  for (size_t k = 0; k < p.table.size(); ++k) {
    CHECK(p.table[k].tile_first == first[k]);
    CHECK(p.table[k].src == bufs[which[k]].pcm && p.table[k].n == used[which[k]] && p.table[k].dst_off == off[which[k]]);
    if (k) CHECK(p.table[k].tile_first > p.table[k - 1].tile_first);
  }
  CHECK(afx::devio_tiles(0) == 0 && afx::devio_tiles(1) == 1 && afx::devio_tiles(T) == 1 && afx::devio_tiles(T + 1) == 2);
  const GatherPlan none = plan_gather(bufs, used, off, 0);
  CHECK(none.ok && none.tiles == 0 && none.table.empty());
  // beyond the 32-bit tile prefix: refused as a whole
  const int64_t huge[] = {T * 0x40000000LL, T * 0x40000000LL};
  const GatherPlan over = plan_gather(bufs, huge, off, 2);
  CHECK(!over.ok && over.table.empty());
  const int64_t fits[] = {T * 0x40000000LL, T * 0x3FFFFFFFLL};
  CHECK(plan_gather(bufs, fits, off, 2).ok);
}

struct Shape : ExportShape {
  int32_t off[AFX_NUM_SERIES], wid[AFX_NUM_SERIES];
  std::vector<int64_t> fo;
  Shape(std::vector<int64_t> first_frames, bool mag, bool stats) : fo(std::move(first_frames)) {
    // series 0 (14 wide) at column 0, series 1 at 14, series 9 (28 wide) at 15; the others are not in the mask
    for (int i = 0; i < AFX_NUM_SERIES; ++i) off[i] = -1, wid[i] = 1;
    wid[0] = 14; wid[9] = 28;
    off[0] = 0; off[1] = 14; off[9] = 15;
    ran = true; n_bufs = (int32_t)fo.size() - 1; frame_offset = fo.data(); stride = 43; offsets = off; widths = wid;
    has_magnitude = mag; has_statistics = stats;
  }
};

static afx_device_out out(uint64_t dst, int series, int dtype, int64_t row_stride, int64_t buf_stride) {
  afx_device_out o;
  o.dst = (void*)(uintptr_t)dst; o.series = series; o.dtype = dtype; o.row_stride = row_stride; o.buf_stride = buf_stride;
  return o;
}

static bool refused(const ExportPlan& p) { return p.status == AFX_ERR_INVALID_ARG && p.why[0] != 0; }

static void exports() {
  // files of 3, 0, 5 and 2 frames (the last but one refused or empty files own zero rows)
  Shape s({0, 3, 3, 8, 10}, true, true);
  {
    const afx_device_out o[] = {out(0x1000, 0, AFX_PCM_F64, 20, 0), out(0x2000, 1, AFX_PCM_F32, 1, 0), out(0x3000, AFX_SERIES_MAGNITUDE, AFX_PCM_F32, 1024, 0)};
    const ExportPlan p = plan_export(s, o, 3, AFX_EXPORT_PACKED, 0, 0.0);
    CHECK(p.status == AFX_OK && !p.needs_frame_offsets);
    CHECK(p.extent_bytes[0] == (9 * 20 + 14) * 8 && p.extent_bytes[1] == 10 * 4 && p.extent_bytes[2] == 10 * 1024 * 4);
    CHECK(p.args.frames == 10 && p.args.data_tiles == 1 && p.args.pad_rows == 0 && p.args.padded == 0 && p.args.n_outs == 3 && p.args.stride == 43);
    CHECK(p.args.outs[0].col == 0 && p.args.outs[0].width == 14 && !p.args.outs[0].f32 && !p.args.outs[0].from_mag && p.args.outs[0].buf_stride == 0);
    CHECK(p.args.outs[1].col == 14 && p.args.outs[1].width == 1 && p.args.outs[1].f32);
    CHECK(p.args.outs[2].from_mag && p.args.outs[2].width == 1024 && p.args.outs[2].row_stride == 1024);
  }
  {
    const afx_device_out o[] = {out(0x1000, 9, AFX_PCM_F32, 43, 7 * 43 + 2), out(0x2000, 0, AFX_PCM_F64, 14, 7 * 14)};
    const ExportPlan p = plan_export(s, o, 2, AFX_EXPORT_PADDED, 7, -0.0);
    CHECK(p.status == AFX_OK && p.needs_frame_offsets);
    CHECK(p.extent_bytes[0] == (uint64_t)(3 * (7 * 43 + 2) + 6 * 43 + 28) * 4 && p.extent_bytes[1] == (uint64_t)(3 * 98 + 6 * 14 + 14) * 8);
    CHECK(p.args.max_frames == 7 && p.args.pad_rows == 4 * 7 - 10 && p.args.padded == 1 && p.args.n_bufs == 4);
    CHECK(std::signbit(p.args.pad_value) && p.args.pad_value == 0.0);
    CHECK(p.args.outs[0].col == 15 && p.args.outs[0].buf_stride == 7 * 43 + 2);
  }
  {
    // max_frames exactly the longest file; no frames at all; no files at all
    const afx_device_out o[] = {out(0x1000, 0, AFX_PCM_F64, 14, 5 * 14)};
    const ExportPlan p = plan_export(s, o, 1, AFX_EXPORT_PADDED, 5, 0.0);
    CHECK(p.status == AFX_OK && p.args.pad_rows == 10 && p.extent_bytes[0] == (uint64_t)(3 * 70 + 4 * 14 + 14) * 8);
    Shape empty({0, 0, 0}, true, true);
    const ExportPlan q = plan_export(empty, o, 1, AFX_EXPORT_PADDED, 0, 0.0);
    CHECK(q.status == AFX_OK && q.extent_bytes[0] == 0 && q.args.pad_rows == 0 && q.args.data_tiles == 0);
    const ExportPlan q2 = plan_export(empty, o, 1, AFX_EXPORT_PACKED, 0, 0.0);
    CHECK(q2.status == AFX_OK && q2.extent_bytes[0] == 0);
    const ExportPlan q3 = plan_export(empty, o, 1, AFX_EXPORT_PADDED, 5, 0.0);
    CHECK(q3.status == AFX_OK && q3.args.pad_rows == 10 && q3.extent_bytes[0] == (uint64_t)(70 + 4 * 14 + 14) * 8);
    Shape nothing({0}, true, true);
    const ExportPlan q4 = plan_export(nothing, o, 1, AFX_EXPORT_PADDED, 5, 0.0);
    CHECK(q4.status == AFX_OK && q4.extent_bytes[0] == 0 && !q4.needs_frame_offsets);
    CHECK(plan_export(s, nullptr, 0, AFX_EXPORT_PACKED, 0, 0.0).status == AFX_OK);
  }
  // every refusal
  const afx_device_out good = out(0x1000, 0, AFX_PCM_F64, 14, 5 * 14);
  auto one = [&](afx_device_out o, int layout, int64_t max_frames) { return plan_export(s, &o, 1, layout, max_frames, 0.0); };
  CHECK(one(good, AFX_EXPORT_PADDED, 5).status == AFX_OK);
  {
    Shape fresh({0, 3, 3, 8, 10}, true, true);
    fresh.ran = false;
    CHECK(refused(plan_export(fresh, &good, 1, AFX_EXPORT_PADDED, 5, 0.0)));                 // before the first run
    CHECK(plan_export_statistics(fresh, &good, 1).status == AFX_ERR_INVALID_ARG);
  }
  { afx_device_out o = good; o.series = 2; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }    // not in the mask
  { afx_device_out o = good; o.series = -1; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }
  { afx_device_out o = good; o.series = AFX_NUM_SERIES + 1; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }
  { afx_device_out o = good; o.series = AFX_SERIES_MAGNITUDE; o.row_stride = 1024;
    Shape nomag({0, 3, 3, 8, 10}, false, true);
    CHECK(refused(plan_export(nomag, &o, 1, AFX_EXPORT_PACKED, 0, 0.0)));
    CHECK(one(o, AFX_EXPORT_PACKED, 0).status == AFX_OK);
    o.row_stride = 1023; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }
  { afx_device_out o = good; o.row_stride = 13; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }  // below the width
  CHECK(refused(one(good, AFX_EXPORT_PADDED, 4)));                                               // below the longest file
  { afx_device_out o = good; o.buf_stride = 5 * 14 - 1; CHECK(refused(one(o, AFX_EXPORT_PADDED, 5))); }
  { afx_device_out o = good; o.dtype = 2; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }
  { afx_device_out o = good; o.dtype = -1; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }
  CHECK(refused(one(good, 2, 5)) && refused(one(good, -1, 5)));                                  // layout
  { afx_device_out o = good; o.dst = nullptr; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }
  CHECK(refused(plan_export(s, &good, -1, AFX_EXPORT_PACKED, 0, 0.0)));
  CHECK(refused(plan_export(s, nullptr, 1, AFX_EXPORT_PACKED, 0, 0.0)));
  { std::vector<afx_device_out> many(afx::kDevioMaxOuts + 1, good);
    CHECK(refused(plan_export(s, many.data(), (int32_t)many.size(), AFX_EXPORT_PACKED, 0, 0.0)));
    CHECK(plan_export(s, many.data(), afx::kDevioMaxOuts, AFX_EXPORT_PACKED, 0, 0.0).status == AFX_OK); }
  // overflows: buf_stride x n_bufs, max_frames x row_stride, n_bufs x max_frames, frames x row_stride, bytes
  { afx_device_out o = good; o.buf_stride = INT64_MAX / 2; CHECK(refused(one(o, AFX_EXPORT_PADDED, 5))); }
  { afx_device_out o = good; o.buf_stride = INT64_MAX / 3; CHECK(refused(one(o, AFX_EXPORT_PADDED, 5))); }   // the sum, and the bytes
  { afx_device_out o = good; o.buf_stride = INT64_MAX / 20; CHECK(refused(one(o, AFX_EXPORT_PADDED, 5))); }  // the bytes alone: 3/20 of 2^63 elements of 8
  { afx_device_out o = good; o.buf_stride = INT64_MAX / 40; CHECK(one(o, AFX_EXPORT_PADDED, 5).status == AFX_OK); }
  { afx_device_out o = good; o.row_stride = INT64_MAX / 2; o.buf_stride = INT64_MAX; CHECK(refused(one(o, AFX_EXPORT_PADDED, 5))); }
  { afx_device_out o = good; o.buf_stride = INT64_MAX; CHECK(refused(one(o, AFX_EXPORT_PADDED, INT64_MAX / 2))); }
  { afx_device_out o = good; o.row_stride = INT64_MAX / 4; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }
  { afx_device_out o = good; o.buf_stride = INT64_MAX / 64; o.row_stride = 14;                                // more padding rows than a launch covers
    CHECK(refused(one(o, AFX_EXPORT_PADDED, (int64_t)1 << 40))); }
}

static void statistics() {
  Shape s({0, 3, 3, 8, 10}, true, true);
  const afx_device_out o[] = {out(0x1000, 9, AFX_PCM_F64, 0, 0), out(0x2000, 1, AFX_PCM_F32, 0, 0)};
  const StatsExportPlan p = plan_export_statistics(s, o, 2);
  CHECK(p.status == AFX_OK && p.extent_bytes[0] == 4 * 28 * 13 * 8 && p.extent_bytes[1] == 4 * 13 * 4);
  CHECK(p.args.outs[0].col == 15 && p.args.outs[0].width == 28 && p.args.outs[1].f32 && p.args.n_bufs == 4 && p.args.stride == 43);
  Shape nostats({0, 3, 3, 8, 10}, true, false);
  CHECK(plan_export_statistics(nostats, o, 2).status == AFX_ERR_INVALID_ARG);
  afx_device_out bad = o[0];
  bad.series = AFX_SERIES_MAGNITUDE; CHECK(plan_export_statistics(s, &bad, 1).status == AFX_ERR_INVALID_ARG);
  bad.series = 3; CHECK(plan_export_statistics(s, &bad, 1).status == AFX_ERR_INVALID_ARG);
  bad = o[0]; bad.dst = nullptr; CHECK(plan_export_statistics(s, &bad, 1).status == AFX_ERR_INVALID_ARG);
  bad = o[0]; bad.dtype = 5; CHECK(plan_export_statistics(s, &bad, 1).status == AFX_ERR_INVALID_ARG);
  CHECK(plan_export_statistics(s, o, afx::kDevioMaxOuts + 1).status == AFX_ERR_INVALID_ARG);
}

static void extents() {
  const afx_device_out o[] = {out(0x1000, 0, AFX_PCM_F64, 14, 0), out(0x5000, 1, AFX_PCM_F64, 1, 0), out(1, 1, AFX_PCM_F64, 1, 0)};
  const DevioAlloc allocs[] = {dev(0x1000, 0x200), dev(0x4000, 0x2000), DevioAlloc{}};
  CHECK(devio_extents_ok(o, {0x200, 0x1000, 0}, allocs, 0));      // an empty extent is not looked up
  CHECK(!devio_extents_ok(o, {0x201, 0x1000, 0}, allocs, 0));     // one byte beyond its allocation
  CHECK(!devio_extents_ok(o, {0x200, 0x1001, 0}, allocs, 0));
  CHECK(!devio_extents_ok(o, {0x200, 0x1000, 8}, allocs, 0));     // host memory
  CHECK(!devio_extents_ok(o, {0x200, 0x1000, 0}, allocs, 1));     // another device
}

int main() {
  ranges();
  sources();
  gather();
  exports();
  statistics();
  extents();
  if (g_failed) {
    std::printf("%d of %d checks failed\n", g_failed, g_checks);
    return 1;
  }
  std::printf("ok %d\n", g_checks);
  return 0;
}
