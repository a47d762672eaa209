// tests/sanitize/fuzz_host_abi.cpp -- TEST INFRASTRUCTURE ONLY.  The C-ABI's host code (afec_amd/csrc/afx_plan.cpp,
// afx_workspace.cpp, afx_batch_plan.cpp, afx_batch_create.cpp, afx_batch_run.cpp, afx_batch_fetch.cpp, afx_high_level.cpp,
// afx_classification.cpp, afx_class_decision.cpp, afx_model.cpp) compiled by g++ under AddressSanitizer + UndefinedBehaviorSanitizer (or ThreadSanitizer) on the
// mock device of tests/sanitize/hipstub + mock_kernels.cpp, driven through include/afx.h with fuzzed ragged batches:
//
//   * afx_batch_create: 0 .. 1 100 buffers of 0 .. 300 000 samples (0-frame buffers, exactly one frame, a buffer that
//     claims 2^30 + samples behind the 20 s cap), bad buffers, float / double, every kind of descriptor mask; run, fetch
//     into exactly-sized arrays, statistics, repeated runs (the work-queue counters), destroy;
//   * afx_batch_create_from_raw: every sample type, 1 .. 8 channels, silence at either end, all-silent files, files at other
//     rates (converted; refused: above 16 x the rate, >= 2^30 converted samples), contiguous staging and scattered
//     buffers, >= 768 files (whole-file whitening chunks), the rhythm tracker's long-file path, afx_batch_set_file_info;
//     afx_batch_store_records of random bytes over the run's records, statistics and rhythm scalars, fetched back and
//     compared byte for byte, with its refusals (before the run, a part the mask lacks, a null batch);
//   * the fetches above a run (afx_block.h lays out their blocks): batches of 0, 1, 2, 3 and 5 buffers -- none, one, three
//     and 65 frames, a refused one -- through afx_batch_fetch_high_level, _classification_features, _class_signature and
//     _class_decision in random order on the one reused result block, with and without levels, with a class model, a
//     category model of 2, 7 or 64 classes or both, every optional output NULL in turn, exactly-sized arrays, every value
//     checked against the mock kernels' closed forms; afx_model_evaluate_features and afx_decide on arrays of the driver's
//     own; a mask that lacks an input, a fetch before the run; an allocation failure inside a fetch, then the same fetch again;
//   * device out of memory at the n-th allocation, and a memory limit that only the pool trim gets under;
//   * several threads on one plan.
// The mock kernels assert the chunk-table / queue / placement invariants (mock_kernels.cpp) and write values that depend
// on a frame's own samples only: the driver checks them row by row, so a fetch that unpacks the wrong column or a chunk
// table that sends a frame to the wrong row fails here, without a GPU.
//
// usage: fuzz_host_abi [rounds per thread = 300] [seed = 1] [threads = 1]
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/afx.h"

namespace {

std::atomic<long> g_batches{0}, g_frames{0}, g_refused{0}, g_oom{0}, g_fetch_batches{0}, g_fetches{0}, g_fetch_oom{0}, g_stores{0};

[[noreturn]] void die(const char* what, long long a = 0, long long b = 0) {
  std::fprintf(stderr, "fuzz_host_abi: FAILED: %s (%lld, %lld); last error: %s\n", what, a, b, afx_last_error());
  std::abort();
}
#define REQUIRE(cond, ...) do { if (!(cond)) die(#cond, ##__VA_ARGS__); } while (0)

struct Rng {
  std::mt19937_64 g;
  explicit Rng(uint64_t seed) : g(seed) {}
  int64_t range(int64_t lo, int64_t hi) { return lo + (int64_t)(g() % (uint64_t)(hi - lo + 1)); }
  bool chance(int percent) { return (int)(g() % 100) < percent; }
  template <typename T> T pick(std::initializer_list<T> l) { return *(l.begin() + (size_t)(g() % l.size())); }
};

// the mock frame kernel's value of a frame (mock_kernels.cpp: frame_key)
template <typename T>
double key_of(const T* x, int64_t off) { return (double)x[off] + 0.5 * (double)x[off + 511] + 0.25 * (double)x[off + 1024] + 0.125 * (double)x[off + 2047]; }

int64_t frames_of(int64_t n, int64_t cap) {
  const int64_t len = cap > 0 ? std::min(n, cap) : n;
  return len >= 2048 ? (len - 2048) / 1024 + 1 : 0;
}

uint32_t random_mask(Rng& r, bool allow_whole_buffer) {
  uint32_t m = r.pick<uint32_t>({AFX_D_C2, AFX_D_MFCC | AFX_D_SPECTRAL_RMS | AFX_D_SPECTRAL_CENTROID | AFX_D_SPECTRAL_ROLLOFF, 0xFFu, AFX_D_ALL_LOW_LEVEL,
                                 AFX_D_ALL_PER_FRAME, AFX_D_NEIGHBOURS, AFX_D_MFCC | AFX_D_MAGNITUDE, AFX_D_SPECTRAL_FLUX, AFX_D_BAND_FEATURES | AFX_D_MFCC,
                                 AFX_D_AUTO_CORRELATION | AFX_D_MFCC, AFX_D_F0, AFX_D_SPECTRAL_COMPLEXITY | AFX_D_MFCC, AFX_D_AMPLITUDE_PEAK | AFX_D_AMPLITUDE_RMS,
                                 0u});
  if (m == 0u) m = (uint32_t)r.range(1, 0x3FFFFF) & (AFX_D_ALL_PER_FRAME | AFX_D_MAGNITUDE);
  if (m == 0u) m = AFX_D_MFCC;
  if (r.chance(50)) m |= AFX_D_STATISTICS;
  if (allow_whole_buffer && r.chance(25)) m |= AFX_D_EFFECTIVE_LENGTH;
  if (allow_whole_buffer && r.chance(25)) m |= AFX_D_RHYTHM;
  return m;
}

// the device runs out of memory while a batch is being created: at the n-th allocation from now, or because it is full
// up to (nearly) what is in use -- the idle pooled workspaces included, which ws_reserve gives back before it gives up
void inject_fault(Rng& r) {
  if (r.chance(50)) hipstub::fail_allocation_after(r.range(0, 3));
  else hipstub::set_memory_limit(hipstub::device_bytes_in_use() + (size_t)r.range(0, 1 << 20));
}
void clear_fault() {
  hipstub::fail_allocation_after(-1);
  hipstub::set_memory_limit(0);
}

// ---- afx_batch_create on the caller's buffers ----
void round_create(afx_plan* plan, int64_t cap_samples, Rng& r, bool inject) {
  const bool f64 = r.chance(30);
  const int n_bufs = (int)r.pick<int64_t>({0, 1, 1, 2, 3, 5, 17, 64, 300, 800, 1100});
  const bool giant = cap_samples > 0 && n_bufs > 0 && n_bufs < 20 && r.chance(15);
  const uint32_t mask = random_mask(r, !giant);
  std::vector<std::unique_ptr<float[]>> f32s;
  std::vector<std::unique_ptr<double[]>> f64s;
  std::vector<afx_buf> bufs((size_t)n_bufs);
  std::vector<int64_t> claimed((size_t)n_bufs), frames((size_t)n_bufs);
  std::vector<char> good((size_t)n_bufs, 1);
  const int64_t longest = n_bufs > 300 ? 6000 : (n_bufs > 20 ? 40000 : 300000);
  for (int i = 0; i < n_bufs; ++i) {
    int64_t n = r.pick<int64_t>({0, r.range(1, 2047), 2048, r.range(2049, 4096), r.range(2048, longest), r.range(2048, longest), 3072, 2048 + 1024 * r.range(0, 40)});
    int64_t backed = n;
    if (giant && i == 0) { n = ((int64_t)1 << 30) + r.range(0, 100000); backed = cap_samples + 2048; }   // only the analysed prefix (+ 64) is read
    claimed[(size_t)i] = n;
    void* p = nullptr;
    if (f64) { f64s.emplace_back(new double[(size_t)std::max<int64_t>(backed, 1)]); p = f64s.back().get(); for (int64_t k = 0; k < backed; ++k) f64s.back()[(size_t)k] = (double)(int64_t)(r.g() % 2001) / 1000.0 - 1.0; f32s.emplace_back(nullptr); }
    else { f32s.emplace_back(new float[(size_t)std::max<int64_t>(backed, 1)]); p = f32s.back().get(); for (int64_t k = 0; k < backed; ++k) f32s.back()[(size_t)k] = (float)(int64_t)(r.g() % 2001) / 1000.0f - 1.0f; f64s.emplace_back(nullptr); }
    bufs[(size_t)i] = afx_buf{p, f64 ? AFX_PCM_F64 : AFX_PCM_F32, 0, n};
    if (r.chance(4)) { bufs[(size_t)i].pcm = nullptr; good[(size_t)i] = n == 0; }
    else if (r.chance(3)) { bufs[(size_t)i].n_samples = -5; good[(size_t)i] = 0; }
    else if (r.chance(3)) { bufs[(size_t)i].dtype = 7; good[(size_t)i] = 0; }
    else if (i > 0 && r.chance(3)) { bufs[(size_t)i].dtype = f64 ? AFX_PCM_F32 : AFX_PCM_F64; good[(size_t)i] = 0; bufs[(size_t)i].n_samples = std::min<int64_t>(n, 100); }
    frames[(size_t)i] = good[(size_t)i] ? frames_of(bufs[(size_t)i].n_samples, cap_samples) : 0;
  }
  // (the first VALID buffer decides the batch's PCM type: when buffer 0 is bad and a later one has the other type, that one wins)
  int batch_dtype = -1;
  for (int i = 0; i < n_bufs && batch_dtype < 0; ++i)
    if (bufs[(size_t)i].n_samples >= 0 && (bufs[(size_t)i].n_samples == 0 || bufs[(size_t)i].pcm) && (bufs[(size_t)i].dtype == AFX_PCM_F32 || bufs[(size_t)i].dtype == AFX_PCM_F64)) batch_dtype = bufs[(size_t)i].dtype;
  for (int i = 0; i < n_bufs; ++i) {
    const afx_buf& s = bufs[(size_t)i];
    const bool valid = s.n_samples >= 0 && (s.n_samples == 0 || s.pcm) && (s.dtype == AFX_PCM_F32 || s.dtype == AFX_PCM_F64) && s.dtype == batch_dtype;
    good[(size_t)i] = valid;
    frames[(size_t)i] = valid ? frames_of(s.n_samples, cap_samples) : 0;
  }
  if (inject) inject_fault(r);
  afx_batch* b = nullptr;
  int st = afx_batch_create(plan, n_bufs ? bufs.data() : nullptr, n_bufs, mask, &b);
  clear_fault();
  if (st != AFX_OK) {
    REQUIRE(inject && (st == AFX_ERR_OUT_OF_MEMORY || st == AFX_ERR_HIP), st);
    REQUIRE(b == nullptr);
    ++g_oom;
    return;
  }
  int64_t total = 0;
  for (int64_t f : frames) total += f;
  REQUIRE(afx_batch_total_frames(b) == total, afx_batch_total_frames(b), total);
  afx_batch_info info{};
  REQUIRE(afx_batch_get_info(b, &info) == AFX_OK);
  REQUIRE(total == 0 || (info.chunk_frames >= 1 && info.chunk_frames <= 32 && info.n_chunks >= 1), info.chunk_frames, info.n_chunks);
  if (mask & AFX_D_RHYTHM) {
    std::vector<afx_file_info> fi((size_t)n_bufs);
    for (int i = 0; i < n_bufs; ++i) fi[(size_t)i] = afx_file_info{(int32_t)r.pick<int64_t>({0, 44100, 48000}), (int32_t)r.range(-500, 500), r.range(1, 1 << 20)};
    if (n_bufs > 0 && r.chance(50)) REQUIRE(afx_batch_set_file_info(b, fi.data()) == AFX_OK);
  }
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 0) { REQUIRE(afx_batch_run(b) == AFX_OK); REQUIRE(afx_batch_sync(b) == AFX_OK); }
    else { float ms = 0; REQUIRE(afx_batch_run_timed(b, (int32_t)r.range(1, 3), &ms) == AFX_OK); }
    // fetch into exactly-sized arrays
    afx_out out{};
    std::vector<double> mfcc, srms, bands, subc, mag, f0, eff;
    std::vector<int64_t> off((size_t)n_bufs + 1, -1);
    std::vector<int32_t> status((size_t)n_bufs, 99);
    if (mask & AFX_D_MFCC) { mfcc.assign((size_t)total * 14, -7.0); out.mfcc = mfcc.data(); }
    if (mask & AFX_D_SPECTRAL_RMS) { srms.assign((size_t)total, -7.0); out.spectral_rms = srms.data(); }
    if (mask & AFX_D_SPECTRUM_BANDS) { bands.assign((size_t)total * 28, -7.0); out.spectrum_bands = bands.data(); }
    if (mask & AFX_D_BAND_FEATURES) { subc.assign((size_t)total * 14, -7.0); out.sub_contrast = subc.data(); }
    if ((mask & AFX_D_MAGNITUDE) && total < 20000) { mag.assign((size_t)total * 1024, -7.0); out.magnitude = mag.data(); }
    if (mask & AFX_D_F0) { f0.assign((size_t)total, -7.0); out.failsafe_f0 = f0.data(); }
    if (mask & AFX_D_EFFECTIVE_LENGTH) { eff.assign((size_t)n_bufs * 3, -7.0); out.effective_length = eff.data(); }
    out.frame_offset = off.data();
    out.buf_status = status.data();
    REQUIRE(afx_batch_fetch(b, &out) == AFX_OK);
    int64_t row = 0;
    for (int i = 0; i < n_bufs; ++i) {
      REQUIRE(off[(size_t)i] == row, i, off[(size_t)i]);
      REQUIRE((status[(size_t)i] == AFX_OK) == (bool)good[(size_t)i], i, status[(size_t)i]);
      for (int64_t f = 0; f < frames[(size_t)i]; ++f, ++row) {
        const double key = f64 ? key_of(f64s[(size_t)i].get(), f * 1024) : key_of(f32s[(size_t)i].get(), f * 1024);
        if (out.mfcc) REQUIRE(mfcc[(size_t)row * 14] == key && mfcc[(size_t)row * 14 + 13] == key + 1e-3 * 13, i, f);
        if (out.spectral_rms && !(mask & (AFX_D_BAND_FEATURES | AFX_D_SPECTRAL_FLUX | AFX_D_SPECTRUM_BANDS))) REQUIRE(srms[(size_t)row] == key + 1, i, f);
        if (out.magnitude) REQUIRE(mag[(size_t)row * 1024 + 1023] == std::fabs(key) + 1023, i, f);
        if (out.sub_contrast) REQUIRE(subc[(size_t)row * 14] != -7.0, i, f);
        if (out.failsafe_f0) REQUIRE(f0[(size_t)row] != -7.0, i, f);
      }
    }
    REQUIRE(off[(size_t)n_bufs] == total);
    if (mask & AFX_D_STATISTICS) {
      afx_stats_out so{};
      std::vector<double> smfcc;
      std::vector<int32_t> sst((size_t)n_bufs, 99);
      if (mask & AFX_D_MFCC) { smfcc.assign((size_t)n_bufs * 14 * 13, -7.0); so.mfcc = smfcc.data(); }
      so.stats_status = sst.data();
      REQUIRE(afx_batch_fetch_statistics(b, &so) == AFX_OK);
    }
    if (mask & AFX_D_RHYTHM) {
      std::vector<int64_t> roff((size_t)n_bufs + 1);
      const int64_t rows = afx_batch_rhythm_frames(b, roff.data());
      std::vector<double> onsets((size_t)rows * 2), scalars((size_t)n_bufs * 14), ostats((size_t)n_bufs * 26);
      REQUIRE(afx_batch_fetch_rhythm(b, onsets.data(), scalars.data(), (mask & AFX_D_STATISTICS) ? ostats.data() : nullptr) == AFX_OK);
      std::vector<float> odf((size_t)rows * 2 + 1);
      REQUIRE(afx_batch_fetch_onset_functions(b, odf.data()) == AFX_OK);
    }
  }
  {
    // afx_batch_store_records refuses by the mask, whatever the batch holds (an empty one included); what it accepts on a
    // batch without buffers or frames moves nothing
    const double one = 0.0;
    if (!(mask & AFX_D_STATISTICS)) REQUIRE(afx_batch_store_records(b, nullptr, &one, nullptr) == AFX_ERR_INVALID_ARG && std::strcmp(afx_last_error(), "AFX_D_STATISTICS was not in the batch mask") == 0);
    if (!(mask & AFX_D_RHYTHM)) REQUIRE(afx_batch_store_records(b, nullptr, nullptr, &one) == AFX_ERR_INVALID_ARG && std::strcmp(afx_last_error(), "AFX_D_RHYTHM was not in the batch mask") == 0);
    if (total == 0) REQUIRE(afx_batch_store_records(b, &one, (mask & AFX_D_STATISTICS) ? &one : nullptr, (mask & AFX_D_RHYTHM) ? &one : nullptr) == AFX_OK);
  }
  g_frames += total;
  ++g_batches;
  afx_batch_destroy(b);
}

// ---- afx_batch_create_from_raw: decoded files through the LoadSample front end ----
void round_raw(afx_plan* plan, Rng& r, bool inject) {
  const int n = (int)r.pick<int64_t>({1, 2, 7, 64, 200, 513, 900});
  const bool contiguous = r.chance(50);
  const int64_t longest = n > 300 ? 3000 : (n > 20 ? 30000 : 150000);
  struct File { int format, channels, rate; int64_t frames; size_t bytes; bool ok; };
  std::vector<File> files((size_t)n);
  size_t arena_bytes = 0;
  for (File& f : files) {
    f.format = (int)r.pick<int64_t>({AFX_RAW_I16, AFX_RAW_I16, AFX_RAW_I16, AFX_RAW_I24, AFX_RAW_F32, AFX_RAW_I32, AFX_RAW_F64});
    f.channels = (int)r.pick<int64_t>({1, 1, 2, 2, 3, 8});
    f.rate = (int)r.pick<int64_t>({0, 44100, 44100, 44100, 48000, 22050, 96000, 11025, 8000});
    f.frames = r.pick<int64_t>({1, r.range(2, 500), r.range(500, longest), r.range(500, longest), 44100, 2048});
    f.ok = true;
    const int bps = f.format == AFX_RAW_I16 ? 2 : f.format == AFX_RAW_I24 ? 3 : f.format == AFX_RAW_F64 ? 8 : 4;
    f.bytes = (size_t)f.frames * f.channels * bps;
    arena_bytes += (f.bytes + 15) & ~(size_t)15;
  }
  // headers that lie: a rate above 16 x the analyser's, and one that makes the conversion 2^30 samples or more
  if (r.chance(30)) { files[0].rate = 800000; files[0].ok = false; }
  if (n > 1 && r.chance(30)) { files[1].rate = 1; files[1].frames = std::max<int64_t>(files[1].frames, 30000); files[1].ok = false;
    const int bps = files[1].format == AFX_RAW_I16 ? 2 : files[1].format == AFX_RAW_I24 ? 3 : files[1].format == AFX_RAW_F64 ? 8 : 4;
    arena_bytes -= (files[1].bytes + 15) & ~(size_t)15; files[1].bytes = (size_t)files[1].frames * files[1].channels * bps; arena_bytes += (files[1].bytes + 15) & ~(size_t)15; }
  std::unique_ptr<unsigned char[]> arena(new unsigned char[arena_bytes + 16]);
  std::vector<std::unique_ptr<unsigned char[]>> scattered;
  std::vector<afx_raw> raws((size_t)n);
  unsigned char* base = arena.get() + ((16 - ((uintptr_t)arena.get() & 15)) & 15);
  size_t at = 0;
  for (int i = 0; i < n; ++i) {
    File& f = files[(size_t)i];
    unsigned char* p;
    if (contiguous) { p = base + at; at += (f.bytes + 15) & ~(size_t)15; }
    else { scattered.emplace_back(new unsigned char[f.bytes ? f.bytes : 1]); p = scattered.back().get(); }
    const int bps = (int)(f.bytes / (size_t)(f.frames * f.channels));
    const int64_t lead = r.chance(40) ? r.range(0, f.frames) : 0, trail = r.chance(40) ? r.range(0, f.frames - lead) : 0;
    for (int64_t k = 0; k < f.frames; ++k)
      for (int c = 0; c < f.channels; ++c) {
        unsigned char* q = p + ((size_t)k * f.channels + c) * bps;
        const bool silent = k < lead || k >= f.frames - trail;
        const double v = silent ? 0.0 : (double)(int64_t)(r.g() % 20001) / 10000.0 - 1.0;
        switch (f.format) {
          case AFX_RAW_I16: { const int16_t s = (int16_t)(v * 32767.0); std::memcpy(q, &s, 2); break; }
          case AFX_RAW_I24: { const int32_t s = (int32_t)(v * 8388607.0); q[0] = (unsigned char)s; q[1] = (unsigned char)(s >> 8); q[2] = (unsigned char)(s >> 16); break; }
          case AFX_RAW_I32: { const int32_t s = (int32_t)(v * 2147483000.0); std::memcpy(q, &s, 4); break; }
          case AFX_RAW_F64: std::memcpy(q, &v, 8); break;
          default: { const float s = (float)v; std::memcpy(q, &s, 4); }
        }
      }
    raws[(size_t)i] = afx_raw{p, f.format, f.channels, f.rate, 0, f.frames};
    if (r.chance(2)) { raws[(size_t)i].channels = 9; f.ok = false; }
    else if (r.chance(2)) { raws[(size_t)i].format = 11; f.ok = false; }
  }
  if (!contiguous || true) {
    // (a bad file in a contiguous staging buffer takes no place in the device arena: the library then uploads file by file)
  }
  const uint32_t mask = random_mask(r, true);
  std::vector<afx_load_info> info((size_t)n);
  if (inject) inject_fault(r);
  afx_batch* b = nullptr;
  const int st = afx_batch_create_from_raw(plan, raws.data(), n, mask, &b, r.chance(80) ? info.data() : nullptr);
  clear_fault();
  if (st != AFX_OK) {
    REQUIRE(inject && (st == AFX_ERR_OUT_OF_MEMORY || st == AFX_ERR_HIP), st);
    ++g_oom;
    return;
  }
  {
    // afx_batch_store_records has nothing to overwrite before the first run, and no batch to do it in without one
    const double one = 0.0;
    REQUIRE(afx_batch_store_records(b, &one, nullptr, nullptr) == AFX_ERR_INVALID_ARG);
    REQUIRE(std::strstr(afx_last_error(), "afx_batch_store_records before afx_batch_run") == afx_last_error());
    REQUIRE(afx_batch_store_records(nullptr, &one, nullptr, nullptr) == AFX_ERR_INVALID_ARG && std::strcmp(afx_last_error(), "null batch") == 0);
  }
  REQUIRE(afx_batch_run(b) == AFX_OK);
  int32_t stride = 0, offsets[AFX_NUM_SERIES], widths[AFX_NUM_SERIES];
  REQUIRE(afx_batch_record_layout(b, &stride, offsets, widths) == AFX_OK);
  const int64_t total = afx_batch_total_frames(b);
  std::vector<double> rec((size_t)total * stride), stats((mask & AFX_D_STATISTICS) ? (size_t)n * stride * 13 : 0), eff((mask & AFX_D_EFFECTIVE_LENGTH) ? (size_t)n * 3 : 0);
  std::vector<int64_t> off((size_t)n + 1);
  std::vector<int32_t> status((size_t)n);
  REQUIRE(afx_batch_fetch_records(b, rec.data(), stats.empty() ? nullptr : stats.data(), off.data(), status.data(), eff.empty() ? nullptr : eff.data()) == AFX_OK);
  for (int i = 0; i < n; ++i) {
    const File& f = files[(size_t)i];
    if (!f.ok) { REQUIRE(status[(size_t)i] != AFX_OK, i); REQUIRE(off[(size_t)i + 1] == off[(size_t)i], i); ++g_refused; continue; }
    REQUIRE(status[(size_t)i] == AFX_OK, i, status[(size_t)i]);
    REQUIRE(off[(size_t)i + 1] - off[(size_t)i] >= 1, i);         // LoadSample pads every file to at least one frame
  }
  if (mask & AFX_D_RHYTHM) {
    std::vector<int64_t> roff((size_t)n + 1);
    const int64_t rows = afx_batch_rhythm_frames(b, roff.data());
    std::vector<double> onsets((size_t)rows * 2), scalars((size_t)n * 14), ostats((size_t)n * 26);
    REQUIRE(afx_batch_fetch_rhythm(b, onsets.data(), scalars.data(), (mask & AFX_D_STATISTICS) ? ostats.data() : nullptr) == AFX_OK);
  }
  {
    // afx_batch_store_records: what is stored comes back byte for byte (NaNs with a payload among it), a NULL part stays
    // as it was, the parts the mask lacks are refused, and offsets and status are the batch's own
    const bool with_stats = (mask & AFX_D_STATISTICS) != 0, with_rhythm = (mask & AFX_D_RHYTHM) != 0;
    auto scribble = [&r](std::vector<double>& v) {
      for (double& x : v) {
        const uint64_t bits = r.chance(10) ? 0x7FF8000000000000ull | (r.g() & 0xFFFFFull) : r.g();
        std::memcpy(&x, &bits, 8);
      }
    };
    std::vector<double> rec2(rec.size()), stats2(stats.size()), rhythm2(with_rhythm ? (size_t)n * AFX_NUM_RHYTHM_SCALARS : 0);
    scribble(rec2); scribble(stats2); scribble(rhythm2);
    const double one = 0.0;
    if (!with_stats) {
      REQUIRE(afx_batch_store_records(b, nullptr, &one, nullptr) == AFX_ERR_INVALID_ARG && std::strcmp(afx_last_error(), "AFX_D_STATISTICS was not in the batch mask") == 0);
    }
    if (!with_rhythm) {
      REQUIRE(afx_batch_store_records(b, nullptr, nullptr, &one) == AFX_ERR_INVALID_ARG && std::strcmp(afx_last_error(), "AFX_D_RHYTHM was not in the batch mask") == 0);
    }
    REQUIRE(afx_batch_store_records(b, nullptr, nullptr, nullptr) == AFX_OK);
    const bool skip_records = r.chance(20);
    REQUIRE(afx_batch_store_records(b, skip_records || rec2.empty() ? nullptr : rec2.data(), with_stats ? stats2.data() : nullptr,
                                    with_rhythm ? rhythm2.data() : nullptr) == AFX_OK);
    std::vector<double> rec3(rec.size()), stats3(stats.size()), rhythm3(rhythm2.size());
    std::vector<int64_t> off3((size_t)n + 1);
    std::vector<int32_t> status3((size_t)n);
    REQUIRE(afx_batch_fetch_records(b, rec3.empty() ? nullptr : rec3.data(), stats3.empty() ? nullptr : stats3.data(), off3.data(), status3.data(), nullptr) == AFX_OK);
    const std::vector<double>& rec_want = skip_records ? rec : rec2;
    REQUIRE(rec3.empty() || std::memcmp(rec3.data(), rec_want.data(), rec3.size() * sizeof(double)) == 0);
    // (a batch without frames moves nothing: its statistics stay the run's)
    const std::vector<double>& stats_want = total > 0 ? stats2 : stats;
    REQUIRE(stats3.empty() || std::memcmp(stats3.data(), stats_want.data(), stats3.size() * sizeof(double)) == 0);
    REQUIRE(off3 == off && status3 == status);
    if (with_rhythm && total > 0) {
      REQUIRE(afx_batch_fetch_rhythm(b, nullptr, rhythm3.data(), nullptr) == AFX_OK);
      REQUIRE(std::memcmp(rhythm3.data(), rhythm2.data(), rhythm3.size() * sizeof(double)) == 0);
    }
    ++g_stores;
  }
  {
    const int pick = (int)r.range(0, n - 1);
    std::vector<double> samples(4096);
    REQUIRE(afx_batch_fetch_samples(b, pick, samples.data(), 4096) == AFX_OK);
  }
  REQUIRE(afx_batch_run(b) == AFX_OK);       // once more: queue counters, pooled buffers
  REQUIRE(afx_batch_sync(b) == AFX_OK);
  g_frames += total;
  ++g_batches;
  afx_batch_destroy(b);
}


// ---- the fetches above a run: high-level, classification features, class signature, class decision ----

// an array of exactly n elements on the heap (n == 0: a pointer that may not be read or written at all)
template <typename T>
struct Exact {
  std::unique_ptr<T[]> p;
  size_t n;
  Exact(size_t count, T fill) : p(new T[count]), n(count) { for (size_t i = 0; i < n; ++i) p[i] = fill; }
  T* data() { return p.get(); }
  T& operator[](size_t i) { return p[i]; }
};

// a LightGBM v3 text of `iterations` x `classes` trees: stumps of two leaves and single leaves
std::string stump_model(int classes, int iterations, bool ova) {
  std::string t = "tree\nversion=v3\nnum_class=" + std::to_string(classes) + "\nnum_tree_per_iteration=" + std::to_string(classes) +
                  "\nlabel_index=0\nmax_feature_idx=1679\nobjective=" + (ova ? "multiclassova num_class:" : "multiclass num_class:") + std::to_string(classes) +
                  (ova ? " sigmoid:1" : "") + "\nfeature_names=a b\n\n";
  for (int i = 0; i < classes * iterations; ++i) {
    t += "Tree=" + std::to_string(i);
    if (i % 3 == 0) t += "\nnum_leaves=2\nnum_cat=0\nsplit_feature=" + std::to_string((i * 37) % 1680) +
                         "\nsplit_gain=1\nthreshold=0.5\ndecision_type=2\nleft_child=-1\nright_child=-2\nleaf_value=0.125 -0.25";
    else t += "\nnum_leaves=1\nnum_cat=0\nleaf_value=0.5";
    t += "\nis_linear=0\nshrinkage=1\n\n\n";
  }
  return t + "end of trees\n";
}

afx_model* make_model(afx_plan* plan, int classes, int n_models) {
  std::vector<std::string> texts;
  for (int i = 0; i < n_models; ++i) texts.push_back(stump_model(classes, 1 + i, i % 2 == 1));
  std::vector<const char*> ptrs;
  std::vector<size_t> lens;
  for (const std::string& t : texts) { ptrs.push_back(t.data()); lens.push_back(t.size()); }
  const std::vector<double> scale(AFX_NUM_CLASSIFICATION_FEATURES, 1.0), offset(AFX_NUM_CLASSIFICATION_FEATURES, 0.0), limits(AFX_NUM_CLASSIFICATION_FEATURES, 3.0);
  afx_model* m = nullptr;
  REQUIRE(afx_model_create_from_lightgbm(plan, ptrs.data(), lens.data(), n_models, scale.data(), offset.data(), limits.data(), 10, 10.0, &m) == AFX_OK);
  int32_t c = 0, k = 0;
  REQUIRE(afx_model_get_info(m, &c, &k, nullptr) == AFX_OK && c == classes && k == n_models, c, k);
  return m;
}

// the mock kernels' closed forms (mock_kernels.cpp)
double mock_feature(int file, int j) { return 5e3 * file + j + 0.375; }
float mock_signature(const double* features, int c) { return (float)(features[AFX_NUM_CLASSIFICATION_FEATURES - 1 - c] + 0.5 * (c + 1)); }
float mock_batch_signature(int file, int c) { return (float)(mock_feature(file, AFX_NUM_CLASSIFICATION_FEATURES - 1 - c) + 0.5 * (c + 1)); }
template <typename T>
bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// one batch as the fetches see it, with what the driver needs to predict their answers
struct FetchBatch {
  afx_batch* b = nullptr;
  int n = 0;
  int64_t total = 0;
  std::vector<int64_t> frames, row0;
  std::vector<char> good;
  std::vector<double> scalar_sum, peak_sum;   // per file: what the decision mock makes of its scalars and its peaks
  bool live(int i) const { return good[(size_t)i] && frames[(size_t)i] > 0; }
};

// An allocation failure inside `fetch` (when `fault`): the status says so or the fetch needed no memory; nothing is left
// behind that keeps the same fetch from succeeding afterwards.  Returns after a fetch that succeeded.
template <typename F>
void fetch_with_fault(Rng& r, bool fault, F fetch) {
  if (fault) {
    inject_fault(r);
    const int st = fetch();
    clear_fault();
    REQUIRE(st == AFX_OK || st == AFX_ERR_OUT_OF_MEMORY || st == AFX_ERR_HIP, st);
    if (st != AFX_OK) ++g_fetch_oom;
  }
  REQUIRE(fetch() == AFX_OK);
  ++g_fetches;
}

void fetch_high_level(FetchBatch& fb, Rng& r, bool fault) {
  const size_t n = (size_t)fb.n, F = (size_t)fb.total;
  const bool with_levels = r.chance(60);
  std::vector<afx_load_info> levels(n);
  for (size_t i = 0; i < n; ++i) { levels[i] = afx_load_info{}; levels[i].peak_value = 0.5f + (float)i; levels[i].rms_value = 0.25f + (float)i; }
  Exact<double> scalars(n * AFX_NUM_HL_SCALARS, -7.0), signature(n * 64 * 14, -7.0), pitch(F, -7.0), peak(F, -7.0);
  Exact<int32_t> status(n, 99);
  const int drop = (int)r.range(0, 7);   // 0..4: that output is NULL (a partial fetch)
  afx_high_out out{drop == 0 ? nullptr : scalars.data(), drop == 1 ? nullptr : signature.data(), drop == 2 ? nullptr : pitch.data(),
                   drop == 3 ? nullptr : peak.data(), drop == 4 ? nullptr : status.data()};
  fetch_with_fault(r, fault, [&] { return afx_batch_fetch_high_level(fb.b, with_levels ? levels.data() : nullptr, &out); });
  for (int i = 0; i < fb.n; ++i) {
    const bool live = fb.frames[(size_t)i] > 0;
    for (int s = 0; s < AFX_NUM_HL_SCALARS && out.scalars; ++s) {
      const double got = scalars[(size_t)i * AFX_NUM_HL_SCALARS + s];
      if (!live) REQUIRE(got == 0.0, i, s);
      else if (s < 2 && !with_levels) REQUIRE(std::isnan(got), i, s);
      else REQUIRE(got == (s == 0 ? 0.5 + i : s == 1 ? 0.25 + i : 1e3 * i + s + 0.25), i, s);
    }
    for (int j = 0; j < 64 * 14 && out.signature; ++j) REQUIRE(signature[(size_t)i * 896 + j] == (live ? 2e3 * i + j + 0.5 : 0.0), i, j);
    for (int64_t p = 0; p < fb.frames[(size_t)i]; ++p) {
      if (out.pitch) REQUIRE(pitch[(size_t)(fb.row0[(size_t)i] + p)] == 3e3 * i + (double)p + 0.125, i, p);
      if (out.peak) REQUIRE(peak[(size_t)(fb.row0[(size_t)i] + p)] == 4e3 * i + (double)p + 0.0625, i, p);
    }
    if (out.status) REQUIRE((status[(size_t)i] == AFX_OK) == (bool)fb.good[(size_t)i], i, status[(size_t)i]);
  }
}

void fetch_features(FetchBatch& fb, Rng& r, bool fault) {
  const size_t n = (size_t)fb.n;
  Exact<double> features(n * AFX_NUM_CLASSIFICATION_FEATURES, -7.0);
  Exact<int32_t> bad(n, 99), status(n, 99);
  const int drop = (int)r.range(0, 3);
  int32_t* const p_bad = drop == 0 ? nullptr : bad.data();
  int32_t* const p_status = drop == 1 ? nullptr : status.data();
  fetch_with_fault(r, fault, [&] { return afx_batch_fetch_classification_features(fb.b, features.data(), p_bad, p_status); });
  for (int i = 0; i < fb.n; ++i) {
    for (int j = 0; j < AFX_NUM_CLASSIFICATION_FEATURES; ++j)
      REQUIRE(features[(size_t)i * AFX_NUM_CLASSIFICATION_FEATURES + j] == (fb.live(i) ? mock_feature(i, j) : 0.0), i, j);
    if (p_bad) REQUIRE(bad[(size_t)i] == (fb.live(i) ? 7 * i + 1 : 0), i, bad[(size_t)i]);
    if (p_status) REQUIRE((status[(size_t)i] == AFX_OK) == (bool)fb.good[(size_t)i], i, status[(size_t)i]);
  }
}

void fetch_signature(FetchBatch& fb, Rng& r, bool fault, const afx_model* model, int classes, int n_models) {
  const size_t n = (size_t)fb.n;
  Exact<float> signature(n * (size_t)classes, -7.0f);
  Exact<int32_t> used(n * (size_t)n_models, 99), bad(n, 99);
  const int drop = (int)r.range(0, 3);
  int32_t* const p_used = drop == 0 ? nullptr : used.data();
  int32_t* const p_bad = drop == 1 ? nullptr : bad.data();
  fetch_with_fault(r, fault, [&] { return afx_batch_fetch_class_signature(fb.b, model, signature.data(), p_used, p_bad); });
  for (int i = 0; i < fb.n; ++i) {
    for (int c = 0; c < classes; ++c) REQUIRE(same_bits(signature[(size_t)i * classes + c], fb.live(i) ? mock_batch_signature(i, c) : 0.0f), i, c);
    for (int m = 0; m < n_models && p_used; ++m) REQUIRE(used[(size_t)i * n_models + m] == (fb.live(i) ? 100 * i + m + 1 : 0), i, m);
    if (p_bad) REQUIRE(bad[(size_t)i] == 0, i, bad[(size_t)i]);
  }
}

// the outputs of a decision, each exactly sized, and what the decision mock writes into them
struct DecisionArrays {
  size_t n, k;
  Exact<float> class_signature, category_signature;
  Exact<double> class_strengths, category_strengths, confidences;
  Exact<int32_t> classes, categories, flags, bad;
  afx_decision_out out;
  DecisionArrays(size_t n_files, size_t n_categories, int drop)
      : n(n_files), k(n_categories), class_signature(n * 2, -7.0f), category_signature(n * k, -7.0f), class_strengths(n * 2, -7.0), category_strengths(n * k, -7.0),
        confidences(n * 2, -7.0), classes(n * 2, 99), categories(n * k, 99), flags(n, 99), bad(n, 99) {
    out = afx_decision_out{class_signature.data(), class_strengths.data(), classes.data(), category_signature.data(), category_strengths.data(),
                           categories.data(), confidences.data(), flags.data(), bad.data()};
    void** const slots[9] = {(void**)&out.class_signature, (void**)&out.class_strengths, (void**)&out.classes, (void**)&out.category_signature,
                             (void**)&out.category_strengths, (void**)&out.categories, (void**)&out.confidences, (void**)&out.flags, (void**)&out.non_finite};
    if (drop >= 0 && drop < 9) *slots[drop] = nullptr;
  }
  // file i: `zeros` as the kernel answers for a buffer it does not decide; csig / gsig: the signatures it read (NULL: no such model)
  void check(int i, bool zeros, const float* csig, const float* gsig, double scalar_sum, double peak_sum, int bad_in, int flag_bits) {
    const size_t f = (size_t)i;
    for (size_t c = 0; c < 2; ++c) {
      if (out.class_signature) REQUIRE(same_bits(class_signature[f * 2 + c], csig ? csig[c] : -7.0f), i, (long long)c);
      // without a class model nothing is written for the classes
      if (out.class_strengths) REQUIRE(class_strengths[f * 2 + c] == (!csig ? -7.0 : zeros ? 0.0 : (double)csig[c] + 0.25), i, (long long)c);
      if (out.classes) REQUIRE(classes[f * 2 + c] == (!csig ? 99 : zeros ? -1 : 10 * i + (int)c), i, (long long)c);
    }
    for (size_t j = 0; j < k; ++j) {
      if (out.category_signature) REQUIRE(same_bits(category_signature[f * k + j], gsig[j]), i, (long long)j);
      if (out.category_strengths) REQUIRE(category_strengths[f * k + j] == (zeros ? 0.0 : (double)gsig[j] + 0.75), i, (long long)j);
      if (out.categories) REQUIRE(categories[f * k + j] == (zeros ? -1 : 1000 + 100 * i + (int)j), i, (long long)j);
    }
    if (out.confidences) REQUIRE(same_bits(confidences[f * 2], zeros ? -1.0 : scalar_sum) && same_bits(confidences[f * 2 + 1], zeros ? -1.0 : peak_sum), i);
    if (out.flags) REQUIRE(flags[f] == (zeros ? 0 : 64 * i + 32 + flag_bits), i, flags[f]);
    if (out.non_finite) REQUIRE(bad[f] == bad_in, i, bad[f]);
  }
};

void fetch_decision(FetchBatch& fb, Rng& r, bool fault, const afx_model* class_model, const afx_model* category_model, int k) {
  const int which = (int)r.range(0, 2);   // both models, the class model alone, the category model alone
  afx_decision_desc desc{};
  desc.class_model = which == 2 ? nullptr : class_model;
  desc.category_model = which == 1 ? nullptr : category_model;
  desc.loop_class = (int32_t)r.range(0, 1);
  desc.oneshot_class = 1 - desc.loop_class;
  desc.use_heuristics = (int32_t)r.pick<int64_t>({0, 1, 5});
  const int cats = desc.category_model ? k : 0;
  desc.category_none_class = (int32_t)r.range(-1, cats - 1);
  DecisionArrays d((size_t)fb.n, (size_t)cats, (int)r.range(0, 12));
  fetch_with_fault(r, fault, [&] { return afx_batch_fetch_class_decision(fb.b, &desc, &d.out); });
  const int flag_bits = 16 * (desc.category_none_class >= 0 ? 1 : 0) + 2 * (desc.use_heuristics != 0) + desc.loop_class;
  for (int i = 0; i < fb.n; ++i) {
    float csig[2], gsig[64];
    for (int c = 0; c < 2; ++c) csig[c] = fb.live(i) ? mock_batch_signature(i, c) : 0.0f;
    for (int j = 0; j < cats; ++j) gsig[j] = fb.live(i) ? mock_batch_signature(i, j) : 0.0f;
    d.check(i, !fb.live(i), desc.class_model ? csig : nullptr, gsig, fb.scalar_sum[(size_t)i], fb.peak_sum[(size_t)i], 0, flag_bits);
  }
}

// afx_model_evaluate_features: vectors of the driver's own, some with values that are not finite
void evaluate_features(Rng& r, bool fault, const afx_model* model, int classes, int n_models) {
  const size_t n = (size_t)r.pick<int64_t>({0, 1, 2, 3, 5});
  Exact<double> features(n * AFX_NUM_CLASSIFICATION_FEATURES, 0.0);
  std::vector<int> bad_in(n, 0);
  for (size_t i = 0; i < features.n; ++i) features[i] = (double)r.range(-8000, 8000) * 0.125;
  for (size_t v = 0; v < n; ++v)
    if (r.chance(30)) {
      bad_in[v] = (int)r.range(1, 3);
      for (int q = 0; q < bad_in[v]; ++q) features[v * AFX_NUM_CLASSIFICATION_FEATURES + (size_t)(q * 800 + 3)] = q ? INFINITY : NAN;
    }
  Exact<float> signature(n * (size_t)classes, -7.0f);
  Exact<int32_t> used(n * (size_t)n_models, 99), bad(n, 99);
  const int drop = (int)r.range(0, 3);
  int32_t* const p_used = drop == 0 ? nullptr : used.data();
  int32_t* const p_bad = drop == 1 ? nullptr : bad.data();
  if (fault && n > 0) {
    hipstub::fail_allocation_after(0);
    REQUIRE(afx_model_evaluate_features(model, features.data(), (int32_t)n, signature.data(), p_used, p_bad) == AFX_ERR_OUT_OF_MEMORY);
    REQUIRE(std::strcmp(afx_last_error(), "device memory for the feature vectors") == 0);
    clear_fault();
    ++g_fetch_oom;
  }
  REQUIRE(afx_model_evaluate_features(model, features.data(), (int32_t)n, signature.data(), p_used, p_bad) == AFX_OK);
  ++g_fetches;
  for (size_t v = 0; v < n; ++v) {
    const double* f = features.data() + v * AFX_NUM_CLASSIFICATION_FEATURES;
    for (int c = 0; c < classes; ++c) REQUIRE(same_bits(signature[v * classes + c], bad_in[v] ? 0.0f : mock_signature(f, c)), (long long)v, c);
    for (int m = 0; m < n_models && p_used; ++m) REQUIRE(used[v * n_models + m] == (bad_in[v] ? 0 : 100 * (int)v + m + 1), (long long)v, m);
    if (p_bad) REQUIRE(bad[v] == bad_in[v], (long long)v, bad[v]);
  }
}

// afx_decide: signatures, peaks and scalars of the driver's own
void decide(afx_plan* plan, Rng& r, bool fault) {
  const size_t n = (size_t)r.pick<int64_t>({0, 1, 2, 3, 5});
  const int which = (int)r.range(0, 2);
  const size_t k = which == 1 ? 0 : (size_t)r.pick<int64_t>({2, 7, 64});
  std::vector<int64_t> offset(n + 1, 0);
  for (size_t i = 0; i < n; ++i) offset[i + 1] = offset[i] + r.pick<int64_t>({0, 1, 3, 65});
  Exact<double> peaks((size_t)offset[n], 0.0), scalars(n * AFX_NUM_DECISION_SCALARS, 0.0);
  Exact<float> csig(n * 2, 0.0f), gsig(n * k, 0.0f);
  Exact<int32_t> bad_in(n, 0);
  for (size_t i = 0; i < peaks.n; ++i) peaks[i] = (double)r.range(0, 1000) / 1000.0;
  for (size_t i = 0; i < scalars.n; ++i) scalars[i] = (double)r.range(0, 4000) / 500.0;
  for (size_t i = 0; i < csig.n; ++i) csig[i] = (float)r.range(0, 1000) / 1000.0f;
  for (size_t i = 0; i < gsig.n; ++i) gsig[i] = (float)r.range(0, 1000) / 1000.0f;
  const bool with_bad = r.chance(50);
  for (size_t i = 0; i < n && with_bad; ++i) bad_in[i] = r.chance(30) ? (int32_t)r.range(1, 9) : 0;
  afx_decision_in in{};
  in.n_files = (int32_t)n;
  in.n_categories = (int32_t)k;
  in.class_signature = which == 2 ? nullptr : csig.data();
  in.category_signature = k ? gsig.data() : nullptr;
  in.peaks = peaks.data();
  in.frame_offset = offset.data();
  in.scalars = scalars.data();
  in.non_finite = with_bad ? bad_in.data() : nullptr;
  in.loop_class = (int32_t)r.range(0, 1);
  in.oneshot_class = 1 - in.loop_class;
  in.use_heuristics = (int32_t)r.range(0, 1);
  in.category_none_class = (int32_t)r.range(-1, (int64_t)k - 1);
  DecisionArrays d(n, k, (int)r.range(0, 12));
  if (fault && n > 0) {
    hipstub::fail_allocation_after(0);
    REQUIRE(afx_decide(plan, &in, &d.out) == AFX_ERR_OUT_OF_MEMORY);
    REQUIRE(std::strcmp(afx_last_error(), "device memory for the decision's inputs") == 0);
    clear_fault();
    ++g_fetch_oom;
  }
  REQUIRE(afx_decide(plan, &in, &d.out) == AFX_OK);
  ++g_fetches;
  const int flag_bits = 16 * (in.category_none_class >= 0 ? 1 : 0) + 2 * in.use_heuristics + in.loop_class;
  for (size_t i = 0; i < n; ++i) {
    double scalar_sum = 0.0, peak_sum = 0.0;
    for (int q = 0; q < AFX_NUM_DECISION_SCALARS; ++q) scalar_sum += scalars[i * AFX_NUM_DECISION_SCALARS + (size_t)q];
    for (int64_t f = offset[i]; f < offset[i + 1]; ++f) peak_sum += peaks[(size_t)f];
    const int bad = with_bad ? bad_in[i] : 0;
    d.check((int)i, offset[i + 1] == offset[i] || bad != 0, in.class_signature ? csig.data() + i * 2 : nullptr, gsig.data() + i * k, scalar_sum, peak_sum, bad, flag_bits);
  }
}

void round_fetches(afx_plan* plan, Rng& r, bool inject) {
  const uint32_t mask = AFX_D_HIGH_LEVEL_INPUTS | AFX_D_CLASS_DECISION_INPUTS;
  FetchBatch fb;
  fb.n = (int)r.pick<int64_t>({0, 1, 2, 3, 5});
  // no samples, one frame, three frames, 65 frames (past time position 44), a refused buffer: all five in a batch of five
  std::vector<int> kinds = {0, 1, 2, 3, 4};
  for (size_t i = kinds.size(); i > 1; --i) std::swap(kinds[i - 1], kinds[(size_t)r.range(0, (int64_t)i - 1)]);
  std::vector<std::vector<float>> pcm((size_t)fb.n);
  std::vector<afx_buf> bufs((size_t)fb.n);
  for (int i = 0; i < fb.n; ++i) {
    const int kind = kinds[(size_t)i];
    const int64_t samples = kind == 0 ? 0 : kind == 1 ? 2048 : kind == 2 ? 2048 + 2 * 1024 : kind == 3 ? 2048 + 64 * 1024 : 4096;
    pcm[(size_t)i].resize((size_t)samples);
    for (float& v : pcm[(size_t)i]) v = (float)(int64_t)(r.g() % 2001) / 1000.0f - 1.0f;
    bufs[(size_t)i] = afx_buf{pcm[(size_t)i].data(), AFX_PCM_F32, 0, samples};
    if (kind == 4) bufs[(size_t)i].n_samples = -5;
    fb.good.push_back(kind != 4);
    fb.frames.push_back(kind == 4 ? 0 : frames_of(samples, 0));
    fb.row0.push_back(fb.total);
    fb.total += fb.frames.back();
  }
  const int k = (int)r.pick<int64_t>({2, 7, 64});
  const int class_models = (int)r.range(1, 3), category_models = (int)r.range(1, 2);
  afx_model* const class_model = make_model(plan, 2, class_models);
  afx_model* const category_model = make_model(plan, k, category_models);
  float one_signature[64];
  DecisionArrays none(0, 0, -1);
  const afx_decision_desc desc{class_model, 0, 1, 1, category_model, -1};

  // a batch whose mask lacks an input: every fetch says which, and says it again
  {
    afx_batch* lacking = nullptr;
    REQUIRE(afx_batch_create(plan, fb.n ? bufs.data() : nullptr, fb.n, AFX_D_MFCC | AFX_D_AMPLITUDE_PEAK | (r.chance(50) ? (uint32_t)AFX_D_STATISTICS : 0u), &lacking) == AFX_OK);
    REQUIRE(afx_batch_run(lacking) == AFX_OK);
    afx_high_out ho{};
    double feature;
    REQUIRE(afx_batch_fetch_high_level(lacking, nullptr, &ho) == AFX_ERR_INVALID_ARG);
    REQUIRE(std::strcmp(afx_last_error(), "the batch mask lacks a series the high-level descriptors read (AFX_D_HIGH_LEVEL_INPUTS)") == 0);
    const char* const lacks = "the batch mask lacks an input of the classification features (AFX_D_CLASSIFICATION_INPUTS)";
    REQUIRE(afx_batch_fetch_classification_features(lacking, &feature, nullptr, nullptr) == AFX_ERR_INVALID_ARG && std::strcmp(afx_last_error(), lacks) == 0);
    REQUIRE(afx_batch_fetch_class_signature(lacking, class_model, one_signature, nullptr, nullptr) == AFX_ERR_INVALID_ARG && std::strcmp(afx_last_error(), lacks) == 0);
    REQUIRE(afx_batch_fetch_class_decision(lacking, &desc, &none.out) == AFX_ERR_INVALID_ARG && std::strcmp(afx_last_error(), lacks) == 0);
    afx_batch_destroy(lacking);
    REQUIRE(afx_batch_create(plan, fb.n ? bufs.data() : nullptr, fb.n, mask & ~(uint32_t)AFX_D_AMPLITUDE_PEAK, &lacking) == AFX_OK);
    REQUIRE(afx_batch_run(lacking) == AFX_OK);
    REQUIRE(afx_batch_fetch_class_decision(lacking, &desc, &none.out) == AFX_ERR_INVALID_ARG);
    REQUIRE(std::strcmp(afx_last_error(), "the batch mask lacks AFX_D_AMPLITUDE_PEAK (AFX_D_CLASS_DECISION_INPUTS)") == 0);
    afx_batch_destroy(lacking);
  }

  REQUIRE(afx_batch_create(plan, fb.n ? bufs.data() : nullptr, fb.n, mask, &fb.b) == AFX_OK);
  // before the run
  {
    afx_high_out ho{};
    double feature;
    REQUIRE(afx_batch_fetch_high_level(fb.b, nullptr, &ho) == AFX_ERR_INVALID_ARG && std::strcmp(afx_last_error(), "afx_batch_fetch_high_level before afx_batch_run") == 0);
    REQUIRE(afx_batch_fetch_classification_features(fb.b, &feature, nullptr, nullptr) == AFX_ERR_INVALID_ARG);
    REQUIRE(std::strcmp(afx_last_error(), "afx_batch_fetch_classification_features before afx_batch_run") == 0);
    REQUIRE(afx_batch_fetch_class_signature(fb.b, class_model, one_signature, nullptr, nullptr) == AFX_ERR_INVALID_ARG);
    REQUIRE(std::strcmp(afx_last_error(), "afx_batch_fetch_class_signature before afx_batch_run") == 0);
    REQUIRE(afx_batch_fetch_class_decision(fb.b, &desc, &none.out) == AFX_ERR_INVALID_ARG);
    REQUIRE(std::strcmp(afx_last_error(), "afx_batch_fetch_class_decision before afx_batch_run") == 0);
  }
  REQUIRE(afx_batch_total_frames(fb.b) == fb.total, afx_batch_total_frames(fb.b), fb.total);
  REQUIRE(afx_batch_run(fb.b) == AFX_OK);

  // what the decision mock reads where the run left it: effectve_length_24dB, three rhythm scalars, the mean of
  // spectral_flux, and the amplitude_peak column
  {
    const size_t n = (size_t)fb.n;
    std::vector<double> eff(n * 3), peak((size_t)fb.total), flux(n * AFX_NUM_STATISTICS), rhythm(n * AFX_NUM_RHYTHM_SCALARS);
    afx_out out{};
    out.effective_length = eff.data();
    out.amplitude_peak = peak.data();
    REQUIRE(afx_batch_fetch(fb.b, &out) == AFX_OK);
    afx_stats_out so{};
    so.spectral_flux = flux.data();
    REQUIRE(afx_batch_fetch_statistics(fb.b, &so) == AFX_OK);
    REQUIRE(afx_batch_fetch_rhythm(fb.b, nullptr, rhythm.data(), nullptr) == AFX_OK);
    for (size_t i = 0; i < n; ++i) {
      double sum = 0.0, peaks = 0.0;
      sum += eff[i * 3 + 1];
      sum += rhythm[i * AFX_NUM_RHYTHM_SCALARS + AFX_R_PERCUSSIVE_ONSET_COUNT];
      sum += rhythm[i * AFX_NUM_RHYTHM_SCALARS + AFX_R_PERCUSSIVE_TEMPO_CONFIDENCE];
      sum += rhythm[i * AFX_NUM_RHYTHM_SCALARS + AFX_R_COMPLEX_TEMPO_CONFIDENCE];
      sum += flux[i * AFX_NUM_STATISTICS + AFX_S_MEAN];
      for (int64_t p = 0; p < fb.frames[i]; ++p) peaks += peak[(size_t)(fb.row0[i] + p)];
      fb.scalar_sum.push_back(sum);
      fb.peak_sum.push_back(peaks);
    }
  }

  // the four fetches in random order on the one reused block: a later, smaller layout must not read an earlier one's leftovers
  const int calls = (int)r.range(6, 10);
  for (int c = 0; c < calls; ++c) {
    const bool fault = inject && r.chance(25);
    switch ((c < 4 ? (c + (int)fb.total) : (int)r.range(0, 3)) % 4) {
      case 0: fetch_high_level(fb, r, fault); break;
      case 1: fetch_features(fb, r, fault); break;
      case 2: if (r.chance(50)) fetch_signature(fb, r, fault, class_model, 2, class_models); else fetch_signature(fb, r, fault, category_model, k, category_models); break;
      default: fetch_decision(fb, r, fault, class_model, category_model, k);
    }
  }
  if (r.chance(50)) evaluate_features(r, inject && r.chance(25), class_model, 2, class_models);
  else evaluate_features(r, inject && r.chance(25), category_model, k, category_models);
  decide(plan, r, inject && r.chance(25));
  ++g_fetch_batches;
  afx_batch_destroy(fb.b);
  afx_model_destroy(class_model);
  afx_model_destroy(category_model);
}

void worker(afx_plan* capped, afx_plan* uncapped, int rounds, uint64_t seed, bool inject) {
  Rng r(seed);
  for (int k = 0; k < rounds; ++k) {
    const bool oom = inject && r.chance(20);
    switch (k % 3) {
      case 0: round_create(capped, 882000, r, oom); break;
      case 1: round_raw(capped, r, oom); break;
      default: round_create(uncapped, 0, r, oom);
    }
    round_fetches((k & 1) ? capped : uncapped, r, inject);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 300;
  const uint64_t seed = argc > 2 ? (uint64_t)std::atoll(argv[2]) : 1;
  const int threads = argc > 3 ? std::atoi(argv[3]) : 1;
  afx_plan_desc desc = {44100, 2048, 1024, 0, AFX_PRECISION_F64, 20000, AFX_FRAME_KERNEL_AUTO, 0};
  afx_plan *capped = nullptr, *uncapped = nullptr, *pinned = nullptr;
  REQUIRE(afx_plan_create(&desc, &capped) == AFX_OK);
  desc.max_analysis_ms = 0;
  desc.frame_kernel = AFX_FRAME_KERNEL_HALFWAVE;      // every batch the half-wave layout serves takes it: its chunk pairs and queue
  REQUIRE(afx_plan_create(&desc, &uncapped) == AFX_OK);
  desc.device = 3;
  REQUIRE(afx_plan_create(&desc, &pinned) == AFX_ERR_NO_DEVICE && pinned == nullptr);   // one mock device: ordinal 3 does not exist
  REQUIRE(afx_device_count() == 1);
  REQUIRE(afx_plan_probe_device(capped) == AFX_OK);
  afx_plan_set_blocking_wait(capped, 1);             // the sleeping waits' path (polls an event)

  if (threads <= 1) worker(capped, uncapped, rounds, seed, true);
  else {
    // several threads on the two plans (allocation faults are process-wide in the stub: off here)
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) pool.emplace_back(worker, capped, uncapped, rounds, seed * 1000 + (uint64_t)t, false);
    for (std::thread& t : pool) t.join();
  }

  // a device that is full until the idle pool gives its memory back: two idle workspaces, a large one and a small one (the
  // next batch is handed the small one, must grow it, finds the device full, ws_reserve trims the pool -- the large one
  // goes -- and the second attempt succeeds)
  {
    std::vector<float> x(2048 + 1024 * 4000, 0.25f);
    afx_buf big{x.data(), AFX_PCM_F32, 0, (int64_t)x.size()}, tiny{x.data(), AFX_PCM_F32, 0, 4096}, mid{x.data(), AFX_PCM_F32, 0, 2048 + 1024 * 3000};
    afx_batch *a = nullptr, *t = nullptr, *b = nullptr;
    REQUIRE(afx_batch_create(uncapped, &big, 1, AFX_D_ALL_LOW_LEVEL, &a) == AFX_OK);
    REQUIRE(afx_batch_create(uncapped, &tiny, 1, AFX_D_ALL_LOW_LEVEL, &t) == AFX_OK);
    afx_batch_destroy(a);
    afx_batch_destroy(t);        // the pool hands out the workspace released last: the tiny one
    hipstub::set_memory_limit(hipstub::device_bytes_in_use() + 4096);
    REQUIRE(afx_batch_create(uncapped, &mid, 1, AFX_D_ALL_LOW_LEVEL, &b) == AFX_OK);
    REQUIRE(afx_batch_run(b) == AFX_OK);
    afx_batch_destroy(b);
    hipstub::set_memory_limit(0);
  }
  // a lost device: every call fails with AFX_ERR_HIP, the probe says so, nothing crashes; afterwards it is back
  {
    hipstub::lose_device(0, true);
    REQUIRE(afx_plan_probe_device(capped) == AFX_ERR_HIP);
    std::vector<float> x(4096, 0.5f);
    afx_buf one{x.data(), AFX_PCM_F32, 0, 4096};
    afx_batch* b = nullptr;
    REQUIRE(afx_batch_create(capped, &one, 1, AFX_D_C2, &b) != AFX_OK && b == nullptr);
    hipstub::lose_device(0, false);
    REQUIRE(afx_plan_probe_device(capped) == AFX_OK);
    REQUIRE(afx_batch_create(capped, &one, 1, AFX_D_C2, &b) == AFX_OK);
    afx_batch_destroy(b);
  }
  afx_plan_destroy(capped);
  afx_plan_destroy(uncapped);
  REQUIRE(hipstub::device_bytes_in_use() == 0, (long long)hipstub::device_bytes_in_use());
  REQUIRE(hipstub::live_streams() == 0 && hipstub::live_events() == 0, hipstub::live_streams(), hipstub::live_events());
  std::printf("fuzz_host_abi: %ld batches, %ld frames, %ld refused files, %ld injected allocation failures survived; %ld batches through %ld fetches above a run, "
              "%ld allocation failures inside a fetch survived; %ld stored records read back; %d thread(s), seed %llu: clean\n",
              g_batches.load(), g_frames.load(), g_refused.load(), g_oom.load(), g_fetch_batches.load(), g_fetches.load(), g_fetch_oom.load(), g_stores.load(), threads,
              (unsigned long long)seed);
  return 0;
}
