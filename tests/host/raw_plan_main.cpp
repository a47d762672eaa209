// tests/host/raw_plan_main.cpp -- the plan of the raw arena (afec_amd/csrc/afx_raw_plan.h) on the CPU, no device and no mock:
// tests/test_raw_plan_cpu.py compiles it with g++, plain and with -fsanitize=address,undefined, and runs it.
//
//   raw_plan_main [random batches] [seed]   -> "ok plans <n> checks <n>" and exit status 0, or the first broken check and 1
//
// Hand-made batches whose offsets are written out as numbers (worked out from the layout rules of DESIGN 4.6 by hand), then
// seeded random batches -- every AFX_RAW_* format, malformed buffers, rates from 0 to beyond 16 x the plan's, FLAC
// descriptors with synthesised indices, good and bad -- each planned for all four combinations of the two optional
// launchers and held to the invariants below.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <string>
#include <vector>

#include "afx_raw_plan.h"

namespace afx {
int64_t resample_blocks(int64_t n_out) { return (n_out + 4096 - 1) / 4096; }   // afx_resample.hip's (kRsBlockOut), as the mock restates it
}

using namespace afx;
using namespace afx::host;

namespace {

long g_checks = 0, g_plans = 0;
std::string g_case;
#define CHECK(cond)                                                                          \
  do {                                                                                       \
    ++g_checks;                                                                              \
    if (!(cond)) {                                                                           \
      std::printf("%s: line %d: %s\n", g_case.c_str(), __LINE__, #cond);                     \
      std::exit(1);                                                                          \
    }                                                                                        \
  } while (0)

constexpr int kPlanRate = 44100;
char g_pcm[5000 * 8 * 8];   // what the PCM buffers point at: the plan never reads it

struct Flac {   // a descriptor with a synthesised index; never decoded
  afx_flac_stream stream{};
  std::vector<afx_flac_frame> index;
};
std::deque<Flac> g_flacs;

// `blocks` frames' sample counts; frame k takes bytes[k % n] bytes
Flac& make_flac(const std::vector<int>& blocks, const std::vector<int>& bytes, int bits, int channels) {
  g_flacs.emplace_back();
  Flac& f = g_flacs.back();
  int64_t off = 0, sample = 0;
  for (size_t k = 0; k < blocks.size(); ++k) {
    f.index.push_back(afx_flac_frame{off, sample});
    off += bytes[k % bytes.size()];
    sample += blocks[k];
  }
  f.index.push_back(afx_flac_frame{off, sample});
  f.stream = afx_flac_stream{g_pcm, off, f.index.data(), (int32_t)blocks.size(), bits, channels, 0};
  return f;
}

bool same(const LoadFile& a, const LoadFile& b) {
  return a.raw_off == b.raw_off && a.n_frames == b.n_frames && a.channels == b.channels && a.format == b.format;
}
bool is_be(int format) { return format >= AFX_RAW_I16_BE && format <= AFX_RAW_F64_BE; }
int width(int format) {   // bytes per sample, restated
  const int w[10] = {2, 3, 4, 4, 8, 2, 3, 4, 4, 8};
  return w[format];
}

struct Slot { int64_t off, bytes; const char* what; };

// the invariants every plan keeps, whatever the batch
void check_plan(const std::vector<afx_raw>& raws, const RawPlan& p, bool have_native, bool have_flac) {
  const int n = (int)raws.size();
  CHECK(p.n_bufs == n && (int)p.status.size() == n && (int)p.files.size() == n && (int)p.file_rate.size() == n);
  CHECK(p.conv.size() == p.conv_buf.size() && p.flac.size() == p.flac_buf.size());
  if (!have_native) CHECK(p.be.empty());
  if (!have_flac) CHECK(p.flac.empty());
  std::vector<int> conv_of((size_t)n, -1), flac_of((size_t)n, -1);
  for (size_t k = 0; k < p.conv.size(); ++k) {
    CHECK(p.conv_buf[k] >= 0 && p.conv_buf[k] < n && (k == 0 || p.conv_buf[k] > p.conv_buf[k - 1]));
    conv_of[(size_t)p.conv_buf[k]] = (int)k;
  }
  for (size_t k = 0; k < p.flac.size(); ++k) {
    CHECK(p.flac_buf[k] >= 0 && p.flac_buf[k] < n && (k == 0 || p.flac_buf[k] > p.flac_buf[k - 1]));
    flac_of[(size_t)p.flac_buf[k]] = (int)k;
  }
  // 1: every slot on a 16-byte boundary, inside the arena, inside its section, and apart from every other slot
  std::vector<Slot> slots;
  size_t next_be = 0, next_piece = 0;
  int64_t be_tiles = 0, frames = 0, tiles = 0, groups = 0, blocks = 0, max_in = 0;
  for (int i = 0; i < n; ++i) {
    const afx_raw& f = raws[(size_t)i];
    const LoadFile& lf = p.files[(size_t)i];
    if (p.status[(size_t)i] != AFX_OK) {   // 4: a refused buffer is in no table and in no piece
      CHECK(p.status[(size_t)i] == AFX_ERR_BAD_BUFFER || p.status[(size_t)i] == AFX_ERR_UNSUPPORTED);
      CHECK(same(lf, LoadFile{0, 0, 0, 0}) && conv_of[(size_t)i] < 0 && flac_of[(size_t)i] < 0);
      for (const RawPlan::Piece& piece : p.pieces) CHECK(piece.buf != i);
      continue;
    }
    const bool flac = f.format == AFX_RAW_FLAC;
    CHECK(flac == (flac_of[(size_t)i] >= 0));
    const int c = conv_of[(size_t)i];
    CHECK((c >= 0) == (f.sample_rate != 0 && f.sample_rate != kPlanRate));
    CHECK(p.file_rate[(size_t)i] == (c >= 0 ? f.sample_rate : 0));
    const int native = c >= 0 ? p.conv[(size_t)c].format : lf.format;
    CHECK(native >= AFX_RAW_I16 && native <= AFX_RAW_F64);   // 5: no *_BE, no AFX_RAW_FLAC in a device table
    const int64_t slot = c >= 0 ? p.conv[(size_t)c].raw_off : lf.raw_off;
    const int64_t payload = f.n_frames * f.channels * width(native);
    slots.push_back(Slot{slot, payload, "pcm"});
    CHECK(slot + payload <= p.conv_off);
    if (c >= 0) {   // 5, 6: the converted file's entry, the resampler's prefixes
      const ResampleFile& r = p.conv[(size_t)c];
      CHECK(same(lf, LoadFile{r.out_off, r.n_out, 1, kRawMonoFloat}));
      CHECK(r.n_in == f.n_frames && r.channels == f.channels && r.factor == 1.0 / ((double)f.sample_rate / kPlanRate));
      const double exact = (double)f.n_frames * kPlanRate / f.sample_rate;
      CHECK(r.n_out >= 1 && r.n_out >= exact - 1 && r.n_out <= exact + 1);
      CHECK(r.group_off == groups && r.block_off == blocks);
      groups += (r.n_out + 15) / 16, blocks += resample_blocks(r.n_out), max_in = std::max(max_in, r.n_in);
      slots.push_back(Slot{r.mono_off, (r.n_in + 2 * kResampleMargin) * 4, "mono mix"});
      slots.push_back(Slot{r.out_off, r.n_out * 4, "converted"});
      CHECK(r.mono_off >= p.conv_off && r.out_off + r.n_out * 4 <= p.flac_off);
    } else {
      CHECK(lf.n_frames == f.n_frames && lf.channels == f.channels);
    }
    // 2: the pieces of this buffer, in buffer order: its bytes, all of them, once, to its own slots
    if (flac) {
      const afx_flac_stream& s = *(const afx_flac_stream*)f.data;
      const FlacFile& d = p.flac[(size_t)flac_of[(size_t)i]];
      CHECK(native == (s.bits_per_sample == 24 ? AFX_RAW_I24 : AFX_RAW_I16) && f.channels == std::min(s.stream_channels, 2));
      CHECK(d.out_off == slot && d.n_samples == f.n_frames && d.n_index == s.n_index && d.bits == s.bits_per_sample && d.stream_channels == s.stream_channels);
      CHECK(d.frame_first == frames && d.tile_first == tiles);   // 6
      frames += s.n_index, tiles += (f.n_frames + 255) / 256;
      const int64_t index_bytes = ((int64_t)s.n_index + 1) * 16;
      slots.push_back(Slot{d.bytes_off, s.frames_bytes, "flac frames"});
      slots.push_back(Slot{d.index_off, index_bytes, "flac index"});
      slots.push_back(Slot{d.work_off, d.n_samples * d.stream_channels * 4, "flac work"});
      slots.push_back(Slot{d.sub_off, (int64_t)d.n_index * d.stream_channels * 144, "flac subframes"});
      slots.push_back(Slot{d.assign_off, (int64_t)d.n_index * 4, "flac assignments"});
      CHECK(d.bytes_off >= p.flac_off && d.index_off + index_bytes <= p.flac_work_off);
      CHECK(d.work_off >= p.flac_work_off && d.assign_off + d.n_index * 4 <= p.flac_table_off);
      CHECK(next_piece + 2 <= p.pieces.size());
      const RawPlan::Piece &a = p.pieces[next_piece], &b = p.pieces[next_piece + 1];
      CHECK(a.buf == i && a.src == (const char*)s.frames && a.dst == d.bytes_off && a.bytes == s.frames_bytes);
      CHECK(b.buf == i && b.src == (const char*)s.index && b.dst == d.index_off && b.bytes == index_bytes);
      next_piece += 2;
    } else {
      CHECK(next_piece < p.pieces.size());
      const RawPlan::Piece& a = p.pieces[next_piece++];
      CHECK(a.buf == i && a.src == (const char*)f.data && a.dst == slot && a.bytes == f.n_frames * f.channels * width(f.format));
      if (!is_be(f.format)) {
        CHECK(native == f.format);
      } else {   // 6: the byte-order kernel's table, in buffer order
        const int twin[5] = {AFX_RAW_I16, AFX_RAW_I24, AFX_RAW_F32, AFX_RAW_I32, AFX_RAW_F64};
        CHECK(native == twin[f.format - AFX_RAW_I16_BE] && next_be < p.be.size());
        const RawNativeFile& b = p.be[next_be++];
        CHECK(b.raw_off == slot && b.bytes == a.bytes && b.kind == width(f.format) && b.tile_first == be_tiles);
        be_tiles += (((a.bytes + 15) & ~(int64_t)15) + 12287) / 12288;
      }
    }
  }
  CHECK(next_piece == p.pieces.size() && next_be == p.be.size());
  CHECK(be_tiles == p.be_tiles && frames == p.flac_frames && tiles == p.flac_tiles);
  CHECK(groups == p.group_slots && blocks == p.conv_blocks && max_in == p.conv_max_in);
  slots.push_back(Slot{p.flac_table_off, (int64_t)p.flac.size() * 80, "flac table"});
  slots.push_back(Slot{p.flac_status_off, (int64_t)p.flac.size() * 4, "flac status"});
  CHECK(0 <= p.conv_off && p.conv_off <= p.flac_off && p.flac_off <= p.flac_work_off && p.flac_work_off <= p.flac_table_off);
  CHECK(p.flac_table_off <= p.flac_status_off && p.flac_status_off <= p.arena_bytes);
  for (size_t a = 0; a < slots.size(); ++a) {
    const int64_t end = (slots[a].off + slots[a].bytes + 15) & ~(int64_t)15;
    CHECK(slots[a].off >= 0 && slots[a].off % 16 == 0 && slots[a].bytes >= 0 && end <= p.arena_bytes);
    for (size_t b = 0; b < a; ++b) {
      const int64_t other_end = (slots[b].off + slots[b].bytes + 15) & ~(int64_t)15;
      CHECK(end <= slots[b].off || other_end <= slots[a].off);
    }
  }
  // 3: the page-locked block: file table, byte-order table, scan results, FLAC status words, one behind the other
  const RawPlan::Pin& pin = p.pin;
  const size_t files_bytes = (size_t)n * sizeof(LoadFile), be_bytes = p.be.size() * sizeof(RawNativeFile);
  CHECK(pin.tables_bytes >= files_bytes && pin.scan_bytes == (size_t)n * sizeof(LoadScan) && pin.flac_status_bytes == p.flac.size() * 4);
  if (be_bytes) CHECK(pin.be_off >= files_bytes && pin.be_off % 8 == 0 && pin.be_off + be_bytes <= pin.tables_bytes);
  CHECK(pin.scan_off >= pin.tables_bytes && pin.scan_off % 8 == 0);
  CHECK(pin.flac_status_off >= pin.scan_off + pin.scan_bytes && pin.flac_status_off % 4 == 0);
  CHECK(pin.flac_status_off + pin.flac_status_bytes <= pin.bytes);
}

// 4, second half: a buffer refused before layout takes no arena space; one refused by the conversion keeps its slot.  The
// same batch with every rate 0 has no conversion: there the slots are the running sum over the accepted buffers, and with
// the rates back every buffer that is still accepted lies where it lay.
void check_slots_against_rate_zero(std::vector<afx_raw> raws, const RawPlan& p, bool have_native, bool have_flac) {
  for (afx_raw& f : raws) f.sample_rate = f.sample_rate < 0 ? f.sample_rate : 0;
  const RawPlan z = plan_raw_arena(raws.data(), (int32_t)raws.size(), kPlanRate, have_native, have_flac);
  CHECK(z.conv.empty() && z.conv_off == z.flac_off);
  int64_t at = 0;
  for (size_t i = 0; i < raws.size(); ++i) {
    if (z.status[i] != AFX_OK) { CHECK(p.status[i] == z.status[i]); continue; }
    const int64_t here = at;
    CHECK(z.files[i].raw_off == here);
    at += (raws[i].n_frames * raws[i].channels * width(z.files[i].format) + 15) & ~(int64_t)15;
    if (p.status[i] != AFX_OK) { CHECK(p.status[i] == AFX_ERR_UNSUPPORTED); continue; }
    int64_t slot = p.files[i].raw_off;
    for (size_t k = 0; k < p.conv.size(); ++k)
      if (p.conv_buf[k] == (int32_t)i) slot = p.conv[k].raw_off;
    CHECK(slot == here);
  }
  CHECK(z.conv_off == at && p.conv_off == at);
}

RawPlan plan_and_check(const std::vector<afx_raw>& raws, bool have_native, bool have_flac) {
  const RawPlan p = plan_raw_arena(raws.data(), (int32_t)raws.size(), kPlanRate, have_native, have_flac);
  ++g_plans;
  check_plan(raws, p, have_native, have_flac);
  check_slots_against_rate_zero(raws, p, have_native, have_flac);
  return p;
}

// 7: offsets as numbers.  native stereo I16 (1001 frames, 4004 bytes), I24_BE mono (3003 bytes), I16 mono at 48 kHz (4800
// frames -> 4410), a 16-bit stereo FLAC of three frames (4096 + 4096 + 1000 samples in 2000 + 2000 + 1000 bytes)
void hand_made() {
  g_case = "hand-made";
  const afx_flac_stream* fl = &make_flac({4096, 4096, 1000}, {2000, 2000, 1000}, 16, 2).stream;
  const std::vector<afx_raw> raws = {{g_pcm, AFX_RAW_I16, 2, 0, 0, 1001},
                                     {g_pcm + 4096, AFX_RAW_I24_BE, 1, kPlanRate, 0, 1001},
                                     {g_pcm + 8192, AFX_RAW_I16, 1, 48000, 0, 4800},
                                     {fl, AFX_RAW_FLAC, 2, 0, 0, 9192}};
  const RawPlan p = plan_and_check(raws, true, true);
  for (int32_t s : p.status) CHECK(s == AFX_OK);
  CHECK(same(p.files[0], LoadFile{0, 1001, 2, AFX_RAW_I16}));
  CHECK(same(p.files[1], LoadFile{4016, 1001, 1, AFX_RAW_I24}));
  CHECK(same(p.files[2], LoadFile{75152, 4410, 1, kRawMonoFloat}));
  CHECK(same(p.files[3], LoadFile{16624, 9192, 2, AFX_RAW_I16}));
  CHECK(p.conv_off == 53392 && p.flac_off == 92800 && p.flac_work_off == 97872 && p.flac_table_off == 172288);
  CHECK(p.flac_status_off == 172368 && p.arena_bytes == 172400);
  CHECK(p.conv.size() == 1 && p.conv_buf[0] == 2 && p.file_rate[2] == 48000 && p.file_rate[1] == 0);
  const ResampleFile& c = p.conv[0];
  CHECK(c.raw_off == 7024 && c.mono_off == 53392 && c.out_off == 75152 && c.n_in == 4800 && c.n_out == 4410);
  CHECK(c.group_off == 0 && c.block_off == 0 && c.channels == 1 && c.format == AFX_RAW_I16);
  CHECK(p.group_slots == 276 && p.conv_blocks == 2 && p.conv_max_in == 4800);
  CHECK(p.be.size() == 1 && p.be[0].raw_off == 4016 && p.be[0].bytes == 3003 && p.be[0].kind == 3 && p.be[0].tile_first == 0 && p.be_tiles == 1);
  CHECK(p.flac.size() == 1 && p.flac_buf[0] == 3 && p.flac_frames == 3 && p.flac_tiles == 36);
  const FlacFile& d = p.flac[0];
  CHECK(d.out_off == 16624 && d.bytes_off == 92800 && d.index_off == 97808 && d.work_off == 97872 && d.sub_off == 171408 && d.assign_off == 172272);
  CHECK(d.n_samples == 9192 && d.n_index == 3 && d.bits == 16 && d.stream_channels == 2 && d.frame_first == 0 && d.tile_first == 0);
  const int64_t dst[5] = {0, 4016, 7024, 92800, 97808}, bytes[5] = {4004, 3003, 9600, 5000, 64};
  CHECK(p.pieces.size() == 5);
  for (int k = 0; k < 5; ++k) CHECK(p.pieces[(size_t)k].dst == dst[k] && p.pieces[(size_t)k].bytes == bytes[k]);
  CHECK(p.pin.be_off == 128 && p.pin.tables_bytes == 152 && p.pin.scan_off == 192 && p.pin.scan_bytes == 128);
  CHECK(p.pin.flac_status_off == 320 && p.pin.flac_status_bytes == 4 && p.pin.bytes == 324);

  // a build without either launcher: both are refused as unsupported and take no space; the file table goes up alone
  const RawPlan q = plan_and_check(raws, false, false);
  CHECK(q.status[0] == AFX_OK && q.status[1] == AFX_ERR_UNSUPPORTED && q.status[2] == AFX_OK && q.status[3] == AFX_ERR_UNSUPPORTED);
  CHECK(q.conv_off == 4016 + 9600 && q.conv[0].raw_off == 4016 && q.conv[0].mono_off == 13616 && q.conv[0].out_off == 35376);
  CHECK(q.flac_table_off == 53024 && q.arena_bytes == 53040 && q.pin.tables_bytes == 96 && q.pin.scan_off == 128 && q.pin.bytes == 256);

  // a file at 17 x the plan's rate is refused by the conversion and keeps its slot: its neighbour lies behind it, and
  // nothing of it goes up
  g_case = "hand-made, refused by the conversion";
  const std::vector<afx_raw> two = {{g_pcm, AFX_RAW_I16, 1, 17 * kPlanRate, 0, 100}, {g_pcm + 4096, AFX_RAW_I16, 1, 0, 0, 10}};
  const RawPlan r = plan_and_check(two, true, true);
  CHECK(r.status[0] == AFX_ERR_UNSUPPORTED && r.status[1] == AFX_OK && same(r.files[1], LoadFile{208, 10, 1, AFX_RAW_I16}));
  CHECK(r.pieces.size() == 1 && r.pieces[0].dst == 208 && r.pieces[0].bytes == 20 && r.arena_bytes == 256);
  // 16 x is the last rate taken
  const std::vector<afx_raw> sixteen = {{g_pcm, AFX_RAW_F32, 2, 16 * kPlanRate, 0, 1600}};
  CHECK(plan_and_check(sixteen, true, true).conv[0].n_out == 100);
}

// a descriptor whose launcher is absent is refused unread: this one points nowhere
void unread_descriptor() {
  g_case = "descriptor unread";
  const std::vector<afx_raw> raws = {{(const void*)16, AFX_RAW_FLAC, 2, 0, 0, 1000}, {g_pcm, AFX_RAW_F64, 1, 0, 0, 7}};
  const RawPlan p = plan_and_check(raws, true, false);
  CHECK(p.status[0] == AFX_ERR_UNSUPPORTED && p.status[1] == AFX_OK && p.files[1].raw_off == 0);
}

struct Made { afx_raw raw; int32_t with_all; bool be, flac; };   // with_all: the status in a build with both launchers

Made random_buffer(std::mt19937& rng) {
  auto pick = [&rng](int lo, int hi) { return (int)(rng() % (unsigned)(hi - lo + 1)) + lo; };
  const int rates[9] = {0, kPlanRate, 8000, 11025, 22050, 48000, 96000, 192000, 17 * kPlanRate};
  Made m{};
  afx_raw& f = m.raw;
  f.sample_rate = rates[pick(0, 8)];
  f.n_frames = pick(0, 3) ? pick(1, 5000) : pick(1, 40);
  f.channels = pick(1, 8);
  f.format = pick(AFX_RAW_I16, AFX_RAW_FLAC);
  f.data = g_pcm + 16 * pick(0, 64);
  m.be = is_be(f.format);
  m.flac = f.format == AFX_RAW_FLAC;
  m.with_all = f.sample_rate > 16 * kPlanRate ? AFX_ERR_UNSUPPORTED : AFX_OK;
  int32_t descriptor = AFX_OK;
  if (m.flac) {
    std::vector<int> blocks, bytes = {pick(14, 3000), pick(14, 3000), pick(14, 3000)};
    for (int64_t left = f.n_frames; left > 0;) {
      const int b = (int)std::min<int64_t>(left, pick(1, 1500));
      blocks.push_back(b);
      left -= b;
    }
    const int bits[3] = {8, 16, 24};
    const int stream_channels = pick(1, 8);
    f.channels = std::min(stream_channels, 2);
    Flac& made = make_flac(blocks, bytes, bits[pick(0, 2)], stream_channels);
    f.data = &made.stream;
    switch (pick(0, 11)) {   // a bad descriptor in a third of them
      case 0: made.stream.bits_per_sample = 20; descriptor = AFX_ERR_UNSUPPORTED; break;
      case 1: made.index.back().first_sample += 1; descriptor = AFX_ERR_BAD_BUFFER; break;
      case 2: made.index[blocks.size() / 2].byte_off = made.stream.frames_bytes + 7; descriptor = AFX_ERR_BAD_BUFFER; break;
      case 3: made.stream.stream_channels = 9; descriptor = AFX_ERR_BAD_BUFFER; break;
      default: break;
    }
  }
  switch (pick(0, 19)) {   // a malformed buffer in a quarter of them: refused before anything else is looked at
    case 0: f.data = nullptr; m.with_all = AFX_ERR_BAD_BUFFER; break;
    case 1: f.n_frames = pick(-3, 0); m.with_all = AFX_ERR_BAD_BUFFER; break;
    case 2: f.sample_rate = -pick(1, 48000); m.with_all = AFX_ERR_BAD_BUFFER; break;
    case 3: if (!m.flac) { f.channels = pick(0, 1) ? 0 : 9; m.with_all = AFX_ERR_BAD_BUFFER; } break;
    case 4: if (!m.flac) { f.format = pick(0, 1) ? 11 : -1; m.be = false; m.with_all = AFX_ERR_BAD_BUFFER; } break;
    default: break;
  }
  if (m.with_all != AFX_ERR_BAD_BUFFER && descriptor != AFX_OK) m.with_all = descriptor;
  return m;
}

void random_batches(int count, unsigned seed) {
  std::mt19937 rng(seed);
  for (int b = 0; b < count; ++b) {
    g_flacs.clear();
    std::vector<Made> made((size_t)(rng() % 9));
    std::vector<afx_raw> raws;
    for (Made& m : made) raws.push_back((m = random_buffer(rng)).raw);
    for (int have = 0; have < 4; ++have) {
      const bool have_native = have & 1, have_flac = have & 2;
      g_case = "random batch " + std::to_string(b) + " of seed " + std::to_string(seed) + ", launchers " + std::to_string(have);
      const RawPlan p = plan_and_check(raws, have_native, have_flac);
      for (size_t i = 0; i < made.size(); ++i) {
        // the launcher's absence comes behind the shape and in front of the descriptor and the rate
        const bool shaped = made[i].with_all != AFX_ERR_BAD_BUFFER || (made[i].flac && raws[i].data && raws[i].n_frames > 0 && raws[i].sample_rate >= 0);
        const bool absent = (made[i].be && !have_native) || (made[i].flac && !have_flac);
        CHECK(p.status[i] == (shaped && absent ? AFX_ERR_UNSUPPORTED : made[i].with_all));
      }
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  const int count = argc > 1 ? std::atoi(argv[1]) : 300;
  const unsigned seed = argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u;
  hand_made();
  unread_descriptor();
  random_batches(count, seed);
  std::printf("ok plans %ld checks %ld\n", g_plans, g_checks);
  return 0;
}
