// tests/host/devio_raw_plan_main.cpp -- afec_amd/csrc/devio/afx_devio_raw_plan.h on the CPU: what LoadSample on
// device-resident audio decides before anything is enqueued.  Every refusal of include/afx.h with its status, check_raw's
// own statuses untouched, plane extents at and one past the allocation's last byte, the overflows, the gather's table and
// its tile prefix at the 32-bit bound, the sample export's extent and refusals.  Driven by tests/test_devio_raw_plan_cpu.py,
// plain and under AddressSanitizer + UBSan.  Prints "ok <checks>".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "devio/afx_devio_raw_plan.h"

namespace afx {
int64_t resample_blocks(int64_t n_out) { return (n_out + 4096 - 1) / 4096; }   // afx_resample.hip's (kRsBlockOut), as the mock restates it
}

using namespace afx::host;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) { ++g_failed; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } \
  } while (0)

static const void* at(uint64_t a) { return (const void*)(uintptr_t)a; }
static DevioAlloc dev(uint64_t base, uint64_t size, int ordinal = 0) { DevioAlloc a; a.device = true; a.ordinal = ordinal; a.base = base; a.size = size; return a; }
static afx_raw_device raw(uint64_t p, int format, int channels, int64_t n_frames, int layout = AFX_RAW_INTERLEAVED, int64_t stride = 0, int rate = 0) {
  afx_raw_device d;
  d.data = at(p); d.format = format; d.channels = channels; d.sample_rate = rate; d.layout = layout; d.n_frames = n_frames; d.channel_stride = stride;
  return d;
}

// the statuses of the device path: the checked buffers through afx_batch_create_from_raw's plan, made without the decoder
static RawPlan planned(const std::vector<afx_raw_device>& raws, const std::vector<DevioAlloc>& allocs, std::vector<afx_raw>* seen = nullptr) {
  const std::vector<afx_raw> checked = devio_raw_checked(raws.data(), allocs.data(), (int32_t)raws.size(), 0);
  if (seen) *seen = checked;
  return plan_raw_arena(checked.data(), (int32_t)raws.size(), 44100, true, false);
}
static int32_t status_of(const afx_raw_device& d, const DevioAlloc& a) { return planned({d}, {a}).status[0]; }

static void extents() {
  uint64_t b = 0;
  CHECK(devio_raw_extent(raw(0x1000, AFX_RAW_I16, 2, 100), &b) && b == 400);
  CHECK(devio_raw_extent(raw(0x1000, AFX_RAW_I24_BE, 3, 7), &b) && b == 63);
  CHECK(devio_raw_extent(raw(0x1000, AFX_RAW_F64, 8, 0x7FFFFFFE), &b) && b == (uint64_t)0x7FFFFFFE * 64);
  CHECK(devio_raw_extent(raw(0x1000, AFX_RAW_I24, 3, 7, AFX_RAW_PLANAR, 7), &b) && b == 63);
  CHECK(devio_raw_extent(raw(0x1000, AFX_RAW_I24, 3, 7, AFX_RAW_PLANAR, 10), &b) && b == 81);       // (2 x 10 + 7) x 3
  CHECK(devio_raw_extent(raw(0x1000, AFX_RAW_F32, 1, 7, AFX_RAW_PLANAR, 7), &b) && b == 28);
  CHECK(devio_raw_extent(raw(0x1000, AFX_RAW_F32, 1, 7, AFX_RAW_PLANAR, 1000), &b) && b == 28);     // one plane: the stride reaches nothing
  CHECK(!devio_raw_extent(raw(0x1000, AFX_RAW_F32, 2, 7, AFX_RAW_PLANAR, 6), &b));                  // planes overlap
  CHECK(!devio_raw_extent(raw(0x1000, AFX_RAW_F32, 1, 7, AFX_RAW_PLANAR, 6), &b));
  CHECK(!devio_raw_extent(raw(0x1000, AFX_RAW_F32, 2, 7, AFX_RAW_PLANAR, -1), &b));
  CHECK(!devio_raw_extent(raw(0x1000, AFX_RAW_F32, 2, 7, 2, 7), &b) && !devio_raw_extent(raw(0x1000, AFX_RAW_F32, 2, 7, -1, 7), &b));
  // channel_stride x (channels - 1): the product, the sum, and the bytes alone
  CHECK(!devio_raw_extent(raw(0x1000, AFX_RAW_I16, 8, 7, AFX_RAW_PLANAR, INT64_MAX / 7 + 1), &b));
  CHECK(!devio_raw_extent(raw(0x1000, AFX_RAW_I16, 2, 7, AFX_RAW_PLANAR, INT64_MAX - 3), &b));
  CHECK(!devio_raw_extent(raw(0x1000, AFX_RAW_I16, 2, 7, AFX_RAW_PLANAR, INT64_MAX / 8), &b));
  CHECK(devio_raw_extent(raw(0x1000, AFX_RAW_F64, 2, 7, AFX_RAW_PLANAR, INT64_MAX / 8 - 7), &b) && b == (uint64_t)(INT64_MAX / 8) * 8);
}

static void refusals() {
  const DevioAlloc a = dev(0x1000, 4096);
  // accepted: the whole allocation, a slice at an odd byte (packed int24), the last byte
  CHECK(status_of(raw(0x1000, AFX_RAW_I16, 2, 1024), a) == AFX_OK);
  CHECK(status_of(raw(0x1001, AFX_RAW_I24, 1, 1365), a) == AFX_OK);                                 // 0x1001 + 4095 = the end
  CHECK(status_of(raw(0x1001, AFX_RAW_I24, 1, 1366), a) == AFX_ERR_BAD_BUFFER);
  CHECK(status_of(raw(0x1002, AFX_RAW_I16, 1, 2047), a) == AFX_OK);
  CHECK(status_of(raw(0x1002, AFX_RAW_I16, 1, 2048), a) == AFX_ERR_BAD_BUFFER);                     // one sample too long
  CHECK(status_of(raw(0x0FFE, AFX_RAW_I16, 1, 8), a) == AFX_ERR_BAD_BUFFER);                        // starts in front
  CHECK(status_of(raw(0x1000, AFX_RAW_I16, 1, 8), DevioAlloc{}) == AFX_ERR_BAD_BUFFER);             // host memory
  CHECK(status_of(raw(0x1000, AFX_RAW_I16, 1, 8), dev(0x1000, 4096, 1)) == AFX_ERR_BAD_BUFFER);     // another device's
  // planar: the extent at the allocation's last byte and one past it
  CHECK(status_of(raw(0x1000, AFX_RAW_F32, 2, 24, AFX_RAW_PLANAR, 1000), a) == AFX_OK);             // (1000 + 24) x 4 = 4096
  CHECK(status_of(raw(0x1000, AFX_RAW_F32, 2, 25, AFX_RAW_PLANAR, 1000), a) == AFX_ERR_BAD_BUFFER);
  CHECK(status_of(raw(0x1000, AFX_RAW_F32, 2, 24, AFX_RAW_PLANAR, 1001), a) == AFX_ERR_BAD_BUFFER);
  CHECK(status_of(raw(0x1001, AFX_RAW_I24_BE, 3, 5, AFX_RAW_PLANAR, 680), a) == AFX_OK);            // 1 + (1360 + 5) x 3 = 4096
  CHECK(status_of(raw(0x1002, AFX_RAW_I24_BE, 3, 5, AFX_RAW_PLANAR, 680), a) == AFX_ERR_BAD_BUFFER);
  CHECK(status_of(raw(0x1000, AFX_RAW_F32, 2, 24, AFX_RAW_PLANAR, 23), a) == AFX_ERR_BAD_BUFFER);   // short channel_stride
  CHECK(status_of(raw(0x1000, AFX_RAW_F32, 2, 24, 2, 24), a) == AFX_ERR_BAD_BUFFER);                // a layout that is neither
  CHECK(status_of(raw(0x1000, AFX_RAW_F32, 2, 24, -1, 24), a) == AFX_ERR_BAD_BUFFER);
  CHECK(status_of(raw(0x1000, AFX_RAW_I16, 8, 7, AFX_RAW_PLANAR, INT64_MAX / 7 + 1), a) == AFX_ERR_BAD_BUFFER);   // overflows
  CHECK(status_of(raw(0x1000, AFX_RAW_I16, 2, 7, AFX_RAW_PLANAR, INT64_MAX - 3), a) == AFX_ERR_BAD_BUFFER);
  // FLAC: refused for what it is, whatever its pointer (nothing is read through it)
  CHECK(status_of(raw(0x1000, AFX_RAW_FLAC, 2, 1024), a) == AFX_ERR_UNSUPPORTED);
  CHECK(status_of(raw(0x9000, AFX_RAW_FLAC, 1, 1024), DevioAlloc{}) == AFX_ERR_UNSUPPORTED);
  CHECK(!devio_raw_is_read(raw(0x1000, AFX_RAW_FLAC, 2, 1024)));
}

// what check_raw itself refuses, and the conversions' bounds: the statuses of the same buffers given as afx_raw
static void untouched_statuses() {
  const std::vector<afx_raw_device> raws = {
      raw(0x1000, AFX_RAW_I16, 1, 64),                       // accepted
      raw(0x1000, AFX_RAW_I16, 0, 64),                       // 0 channels
      raw(0x1000, AFX_RAW_I16, 9, 64),                       // 9 channels
      raw(0x1000, AFX_RAW_I16, 1, 0),                        // no frames
      raw(0x1000, AFX_RAW_I16, 1, -4),
      raw(0, AFX_RAW_I16, 1, 64),                            // null
      raw(0x1000, 11, 1, 64),                                // unknown format
      raw(0x1000, -1, 1, 64),
      raw(0x1000, AFX_RAW_I16, 1, 64, AFX_RAW_INTERLEAVED, 0, -5),          // negative rate
      raw(0x1000, AFX_RAW_I16, 1, 0x7FFFFFFF),               // too many frames
      raw(0x1000, AFX_RAW_I16, 1, 64, AFX_RAW_INTERLEAVED, 0, 44100 * 16 + 1),   // above 16 x the plan's rate
      raw(0x1000, AFX_RAW_I16, 1, 64, AFX_RAW_INTERLEAVED, 0, 44100 * 16),       // at the bound
      raw(0x1000, AFX_RAW_I16, 2, 64, AFX_RAW_PLANAR, 64, 48000),           // a conversion of a planar file
      raw(0x1000, AFX_RAW_I16_BE, 2, 64),                    // big-endian
      raw(0x1000, AFX_RAW_F64_BE, 8, 64, AFX_RAW_PLANAR, 64),
      raw(0x1000, AFX_RAW_I16, 1, 64, AFX_RAW_INTERLEAVED, 0, 1),           // 1 Hz: 2^30 converted samples or more?  64 x 44100 is far below
      raw(0x1000, AFX_RAW_I16, 1, 30000, AFX_RAW_INTERLEAVED, 0, 1),        // 30000 x 44100 = 1.3e9 >= 2^30
  };
  const std::vector<DevioAlloc> allocs(raws.size(), dev(0x1000, 1 << 20));
  std::vector<afx_raw> as_raw;
  for (const afx_raw_device& d : raws) as_raw.push_back(afx_raw{d.data, d.format, d.channels, d.sample_rate, 0, d.n_frames});
  const RawPlan host = plan_raw_arena(as_raw.data(), (int32_t)as_raw.size(), 44100, true, false);
  std::vector<afx_raw> seen;
  const RawPlan device = planned(raws, allocs, &seen);
  const int32_t want[] = {AFX_OK, AFX_ERR_BAD_BUFFER, AFX_ERR_BAD_BUFFER, AFX_ERR_BAD_BUFFER, AFX_ERR_BAD_BUFFER, AFX_ERR_BAD_BUFFER,
                          AFX_ERR_BAD_BUFFER, AFX_ERR_BAD_BUFFER, AFX_ERR_BAD_BUFFER, AFX_ERR_BAD_BUFFER, AFX_ERR_UNSUPPORTED, AFX_OK,
                          AFX_OK, AFX_OK, AFX_OK, AFX_OK, AFX_ERR_UNSUPPORTED};
  for (size_t i = 0; i < raws.size(); ++i) {
    CHECK(device.status[i] == host.status[i]);
    CHECK(device.status[i] == want[i]);
    // a buffer that is not refused for its memory goes through unchanged
    CHECK(seen[i].data == raws[i].data && seen[i].format == raws[i].format && seen[i].channels == raws[i].channels &&
          seen[i].sample_rate == raws[i].sample_rate && seen[i].n_frames == raws[i].n_frames && seen[i].reserved == 0);
  }
  // the same arena, tables and pieces either way
  CHECK(device.arena_bytes == host.arena_bytes && device.conv.size() == host.conv.size() && device.be.size() == host.be.size());
  CHECK(device.pieces.size() == host.pieces.size() && device.conv.size() == 3 && device.be.size() == 2);
  for (size_t k = 0; k < device.pieces.size(); ++k)
    CHECK(device.pieces[k].src == host.pieces[k].src && device.pieces[k].dst == host.pieces[k].dst && device.pieces[k].bytes == host.pieces[k].bytes &&
          device.pieces[k].buf == host.pieces[k].buf);
  CHECK(devio_raw_checked(nullptr, nullptr, 0, 0).empty());
}

static void gather() {
  const int64_t T = afx::kDevioRawTileFrames;
  CHECK(afx::devio_raw_tiles(0) == 0 && afx::devio_raw_tiles(1) == 1 && afx::devio_raw_tiles(T) == 1 && afx::devio_raw_tiles(T + 1) == 2);
  // a ragged batch with refused buffers between the accepted: host memory, FLAC, 9 channels, a file above 16 x the rate
  const std::vector<afx_raw_device> raws = {
      raw(0x10000, AFX_RAW_I16, 2, 1), raw(0x9000, AFX_RAW_I16, 1, 8), raw(0x10101, AFX_RAW_I24, 3, T - 1),
      raw(0x20000, AFX_RAW_FLAC, 2, 100), raw(0x20000, AFX_RAW_F32, 2, T, AFX_RAW_PLANAR, T + 7), raw(0x20000, AFX_RAW_F32, 9, T),
      raw(0x40002, AFX_RAW_I16_BE, 1, T + 1), raw(0x40000, AFX_RAW_I16, 1, 64, AFX_RAW_INTERLEAVED, 0, 44100 * 17),
      raw(0x50000, AFX_RAW_F64_BE, 8, 2 * T + 5, AFX_RAW_PLANAR, 2 * T + 5, 48000)};
  std::vector<DevioAlloc> allocs(raws.size(), dev(0x10000, 0x1000000));
  allocs[1] = DevioAlloc{};
  const RawPlan p = planned(raws, allocs);
  const RawGatherPlan g = plan_raw_gather(p, raws.data());
  CHECK(g.ok && g.tiles == 1 + 1 + 1 + 2 + 3 && g.table.size() == 5 && p.pieces.size() == 5);
  const int which[] = {0, 2, 4, 6, 8};
  const int32_t first[] = {0, 1, 2, 3, 5};
  const int32_t bps[] = {2, 3, 4, 2, 8};
  for (size_t k = 0; k < g.table.size(); ++k) {
    const afx::DevioRawBuf& e = g.table[k];
    const afx_raw_device& d = raws[(size_t)which[k]];
    CHECK(e.src == d.data && e.n_frames == d.n_frames && e.channels == d.channels && e.bps == bps[k] && e.tile_first == first[k]);
    CHECK(e.planar == (d.layout == AFX_RAW_PLANAR) && e.plane_stride == (e.planar ? d.channel_stride : 0));
    CHECK(e.dst_off == p.pieces[k].dst && e.dst_off % 16 == 0 && p.pieces[k].bytes == e.n_frames * e.channels * e.bps);
    CHECK(e.dst_off == p.files[(size_t)which[k]].raw_off || p.file_rate[(size_t)which[k]] != 0);   // the slot the scan (or the converter) reads
    // every tile's arena side on a 16-byte boundary
    CHECK((T * e.channels * e.bps) % 16 == 0);
    if (k) CHECK(e.dst_off >= g.table[k - 1].dst_off + p.pieces[k - 1].bytes);
  }
  const RawPlan none = planned({}, {});
  CHECK(plan_raw_gather(none, nullptr).ok && plan_raw_gather(none, nullptr).table.empty());
  // the tile prefix at its 32-bit bound: files of 2^20 tiles each
  const int64_t longest = 0x7FFFFFFE;
  CHECK(afx::devio_raw_tiles(longest) == (1 << 20));
  std::vector<afx_raw_device> many(2048, raw(0x1000, AFX_RAW_I16, 1, longest));
  const std::vector<DevioAlloc> huge(many.size(), dev(0x1000, (uint64_t)1 << 40));
  CHECK(!plan_raw_gather(planned(many, huge), many.data()).ok);                   // 2^31 tiles
  CHECK(plan_raw_gather(planned(many, huge), many.data()).table.empty());
  many.back().n_frames = longest - T;                                            // one tile fewer: 2^31 - 1
  const RawGatherPlan fits = plan_raw_gather(planned(many, huge), many.data());
  CHECK(fits.ok && fits.tiles == 0x7FFFFFFF && fits.table.back().tile_first == 0x7FFFFFFF - ((1 << 20) - 1));
}

static bool refused(const SamplesExportPlan& p) { return p.status == AFX_ERR_INVALID_ARG && p.why[0] != 0 && p.extent_bytes == 0 && p.tiles_per_row == 0; }

static void samples_export() {
  const int64_t S = afx::kDevioSampleTile;
  const int64_t used[] = {3072, 0, S + 1, 100};
  const void* dst = at(0x1000);
  {
    const SamplesExportPlan p = plan_export_samples(used, 4, dst, AFX_PCM_F32, S + 1);
    CHECK(p.status == AFX_OK && p.f32 == 1 && p.tiles_per_row == 2 && p.extent_bytes == (uint64_t)4 * (S + 1) * 4);
    const SamplesExportPlan q = plan_export_samples(used, 4, dst, AFX_PCM_F64, 3 * S);
    CHECK(q.status == AFX_OK && q.f32 == 0 && q.tiles_per_row == 3 && q.extent_bytes == (uint64_t)4 * 3 * S * 8);
    // the extent at the allocation's end and one byte past it
    const DevioAlloc a = dev(0x1000, p.extent_bytes);
    CHECK(devio_range_ok(a, 0, dst, p.extent_bytes));
    CHECK(!devio_range_ok(dev(0x1000, p.extent_bytes - 1), 0, dst, p.extent_bytes));
    CHECK(!devio_range_ok(a, 0, at(0x1001), p.extent_bytes));
    CHECK(!devio_range_ok(DevioAlloc{}, 0, dst, p.extent_bytes) && !devio_range_ok(a, 1, dst, p.extent_bytes));
  }
  CHECK(refused(plan_export_samples(used, 4, dst, AFX_PCM_F32, S)));              // below the longest
  CHECK(refused(plan_export_samples(used, 4, dst, AFX_PCM_F32, -1)));
  CHECK(refused(plan_export_samples(used, 4, dst, 2, S + 1)) && refused(plan_export_samples(used, 4, dst, -1, S + 1)));
  CHECK(refused(plan_export_samples(used, 4, nullptr, AFX_PCM_F32, S + 1)));
  CHECK(refused(plan_export_samples(used, 4, dst, AFX_PCM_F64, INT64_MAX / 2)));   // n_bufs x buf_stride overflows
  CHECK(refused(plan_export_samples(used, 4, dst, AFX_PCM_F64, INT64_MAX / 16)));  // the bytes alone
  CHECK(refused(plan_export_samples(used, 4, dst, AFX_PCM_F32, INT64_MAX / 64)));  // more tiles than a launch covers
  CHECK(plan_export_samples(used, 4, dst, AFX_PCM_F32, S * (0x7FFFFFFF / 4)).status == AFX_OK);
  CHECK(refused(plan_export_samples(used, 4, dst, AFX_PCM_F32, S * (0x7FFFFFFF / 4) + 1)));
  // nothing to write: no file, or rows of no element
  const int64_t silent[] = {0, 0};
  const SamplesExportPlan e = plan_export_samples(silent, 2, dst, AFX_PCM_F32, 0);
  CHECK(e.status == AFX_OK && e.extent_bytes == 0 && e.tiles_per_row == 0);
  const SamplesExportPlan n = plan_export_samples(nullptr, 0, dst, AFX_PCM_F64, 10);
  CHECK(n.status == AFX_OK && n.extent_bytes == 0 && n.tiles_per_row == 0);
  CHECK(refused(plan_export_samples(nullptr, 0, nullptr, AFX_PCM_F64, 10)));
}

int main() {
  extents();
  refusals();
  untouched_statuses();
  gather();
  samples_export();
  if (g_failed) {
    std::printf("%d of %d checks failed\n", g_failed, g_checks);
    return 1;
  }
  std::printf("ok %d\n", g_checks);
  return 0;
}
