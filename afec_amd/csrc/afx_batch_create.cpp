// afec_amd/csrc/afx_batch_create.cpp -- the ways a batch comes to be: the caller's normalised buffers
// (afx_batch_create), decoded files through the LoadSample front end on the GPU (afx_batch_create_from_raw,
// SampleAnalyser.cpp:484-718), and the one-call form (afx_extract_batch).  See afx_host.h for the map of the host side.

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "afx_host.h"
#include "afx_raw_plan.h"

namespace afx {
// A weak reference: the library defines the launcher (rawpcm/afx_rawpcm.hip); the mock builds of tests/sanitize link this
// file from a fixed list without it, find it null and refuse big-endian buffers
extern hipError_t launch_raw_native(unsigned char* raw, const RawNativeFile* files, int n_files, int64_t n_tiles, hipStream_t stream)
    __attribute__((weak));
// likewise the FLAC decoder (flac/afx_flac.hip): absent from the mock builds, which refuse an AFX_RAW_FLAC buffer
extern hipError_t launch_flac_decode(unsigned char* raw, const FlacFile* files, int n_files, int64_t n_frames, int64_t n_tiles,
                                     int32_t* status, hipStream_t stream) __attribute__((weak));

namespace host {

namespace {

// AFX_TIMING=1 in the environment: wall time of the phases of afx_batch_create_from_raw, summed over calls and printed
// when the process ends (diagnostic for pipelines; three clock reads per call otherwise)
struct CreateTiming {
  std::atomic<long long> ns[4]{};   // upload + scan + wait, host placement, build + LoadSample write + wait, calls
  bool on = std::getenv("AFX_TIMING") != nullptr;
  ~CreateTiming() {
    if (on && ns[3].load())
      std::fprintf(stderr, "[afx timing] create_from_raw x%lld: upload + scan + wait %.1f ms, placement %.1f ms, build + write + wait %.1f ms\n",
                   ns[3].load(), ns[0].load() * 1e-6, ns[1].load() * 1e-6, ns[2].load() * 1e-6);
  }
};
CreateTiming g_create_timing;

inline long long now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct CallerBuffers {   // fill() of afx_batch_create: the caller's PCM, one transfer per buffer
  const afx_buf* bufs;
  int32_t n_bufs;
  size_t esz;
};
int fill_from_caller(afx_batch* b, void* ctx) {
  const CallerBuffers& c = *(const CallerBuffers*)ctx;
  for (int i = 0; i < c.n_bufs; ++i)
    if (b->used[i] > 0) {
      hipError_t e = hipMemcpyAsync((char*)b->d_pcm + (size_t)b->arena_off[i] * c.esz, c.bufs[i].pcm,
                                    (size_t)b->used[i] * c.esz, hipMemcpyHostToDevice, b->stream);
      if (e != hipSuccess) return hip_fail(e, "hipMemcpy(pcm)");
    }
  return AFX_OK;
}

}  // namespace

// first valid buffer's PCM type (the arena of a call is homogeneous); -1 when there is none
int first_valid_dtype(const afx_buf* bufs, int32_t n_bufs) {
  for (int i = 0; i < n_bufs; ++i) {
    const afx_buf& s = bufs[i];
    if (s.n_samples >= 0 && (s.n_samples == 0 || s.pcm) && (s.dtype == AFX_PCM_F32 || s.dtype == AFX_PCM_F64)) return s.dtype;
  }
  return -1;
}

// afx_batch_create with the PCM type of the whole call given (afx_extract_batch cuts large calls into groups: the
// type is decided once, over all buffers, not per group)
int batch_create_typed(afx_plan* plan, const afx_buf* bufs, int32_t n_bufs, uint32_t mask, int dtype, afx_batch** out_batch) {
  return batch_create_filled(plan, bufs, n_bufs, mask, dtype, nullptr, nullptr, out_batch);
}

// ... and with the way the accepted buffers reach the arena given: fill == nullptr is the caller's host memory, one
// transfer per buffer; afx_device_io.cpp brings a gather launch for device memory.  Which buffers are accepted, their
// statuses and the dtype rule are decided here, once, for both.
int batch_create_filled(afx_plan* plan, const afx_buf* bufs, int32_t n_bufs, uint32_t mask, int dtype,
                        int (*fill)(afx_batch* b, void* ctx), void* fill_ctx, afx_batch** out_batch) {
  if (!plan || !out_batch || n_bufs < 0 || (n_bufs > 0 && !bufs))
    return fail(AFX_ERR_INVALID_ARG, "null argument");
  *out_batch = nullptr;
  if (!mask_ok(mask)) return fail(AFX_ERR_INVALID_ARG, "bad descriptor mask");
  HIP_TRY(hipSetDevice(plan->desc.device));

  // one PCM dtype per batch (the arena is homogeneous); first valid buffer of the call decides
  std::vector<int32_t> status((size_t)n_bufs, AFX_OK);
  std::vector<int64_t> lengths((size_t)n_bufs, 0);
  for (int i = 0; i < n_bufs; ++i) {
    const afx_buf& s = bufs[i];
    const bool good = s.n_samples >= 0 && (s.n_samples == 0 || s.pcm) &&
                      (s.dtype == AFX_PCM_F32 || s.dtype == AFX_PCM_F64);
    if (!good) { status[i] = AFX_ERR_BAD_BUFFER; continue; }
    if (dtype < 0) dtype = s.dtype;
    if (s.dtype != dtype) { status[i] = AFX_ERR_BAD_BUFFER; continue; }
    lengths[i] = s.n_samples;
  }
  if (dtype < 0) dtype = AFX_PCM_F32;
  CallerBuffers caller{bufs, n_bufs, (dtype == AFX_PCM_F64) ? (size_t)8 : (size_t)4};
  BatchSource src;
  src.n_bufs = n_bufs; src.mask = mask; src.dtype = dtype; src.lengths = &lengths; src.status = &status;
  src.fill = fill ? fill : fill_from_caller; src.fill_ctx = fill ? fill_ctx : &caller;
  return build_batch(plan, src, out_batch);
}

namespace {

// The steps of afx_batch_create_from_raw share this: the plan of the raw arena (afx_raw_plan.h: what is refused, every
// table, every offset, decided before anything is enqueued) and what the steps add to it.
struct RawBatch : RawPlan {
  afx_plan* plan;
  std::vector<LoadScan> scan;           // [n_bufs]: the scan kernels' results
  std::vector<LoadPlace> place;         // [n_bufs]
  std::vector<int64_t> lengths;         // [n_bufs]: samples of the normalised, trimmed, padded buffer
  Workspace* ws = nullptr;
  unsigned char* d_raw = nullptr;
  LoadFile* d_files = nullptr;
};

hipError_t reserve_buffers(RawBatch& r) {
  Workspace* ws = r.ws;
  hipError_t e;
  if (r.be_tiles < 0) return hipErrorInvalidValue;   // beyond the byte-order kernel's 32-bit tile prefix
  if ((e = ws_reserve(r.plan, ws->raw, (size_t)r.arena_bytes)) != hipSuccess) return e;
  if ((e = ws_reserve(r.plan, ws->files, r.pin.tables_bytes)) != hipSuccess) return e;
  if ((e = ws_reserve(r.plan, ws->scan, r.pin.scan_bytes)) != hipSuccess) return e;
  if ((e = ws_reserve(r.plan, ws->partial, (size_t)r.n_bufs * load_scan_blocks_per_file(r.n_bufs) * 16)) != hipSuccess) return e;
  r.d_raw = (unsigned char*)ws->raw.p;
  r.d_files = (LoadFile*)ws->files.p;
  return ws_pin_reserve(ws, r.pin.bytes);
}

// The decoder's table, and its status words cleared, in front of the upload (pageable source: the copy has left `flac`
// when the scan has been waited for, as the conversions' table has)
hipError_t send_flac_table(RawBatch& r) {
  if (r.flac.empty()) return hipSuccess;
  const hipError_t e = hipMemcpyAsync(r.d_raw + r.flac_table_off, r.flac.data(), r.flac.size() * sizeof(FlacFile), hipMemcpyHostToDevice, r.ws->stream);
  if (e != hipSuccess) return e;
  return hipMemsetAsync(r.d_raw + r.flac_status_off, 0, r.pin.flac_status_bytes, r.ws->stream);
}

// The file table and behind it the byte-order kernel's, in ONE copy out of the page-locked block (pageable copies are
// staged by the runtime on this thread and complete through its event thread: host CPU a crawl's workers do not have to
// spend).  Behind the upload for every batch: a copy on the batch's stream in front of it, beside the plan's upload
// stream, cost the WAV crawl a tenth of its rate (HISTORY 23).
hipError_t send_file_tables(RawBatch& r) {
  unsigned char* pin = (unsigned char*)r.ws->h_pin;
  std::memcpy(pin, r.files.data(), r.files.size() * sizeof(LoadFile));
  if (!r.be.empty()) std::memcpy(pin + r.pin.be_off, r.be.data(), r.be.size() * sizeof(RawNativeFile));
  return hipMemcpyAsync(r.d_files, pin, r.pin.tables_bytes, hipMemcpyHostToDevice, r.ws->stream);
}

// The caller's bytes into the raw arena.  Pieces that follow each other in host memory as they do in the arena, with less
// than 16 bytes of padding between them, travel as one run: a pipeline's staging buffer, laid out like the arena, is one
// run and goes through the plan's upload stream; otherwise one transfer per run (each costs ~10 us of runtime overhead,
// which dominates for thousands of short files).  Only bytes of accepted buffers are read: what lies behind a buffer, or
// in a refused one, is not the library's to read (a buffer may end at the end of a mapping).
hipError_t upload_pieces(RawBatch& r, void*) {
  std::vector<RawPlan::Piece> runs;
  for (const RawPlan::Piece& p : r.pieces) {
    if (!runs.empty()) {
      RawPlan::Piece& last = runs.back();
      const int64_t gap = p.dst - (last.dst + last.bytes);
      if (gap >= 0 && gap < 16 && p.src - last.src == p.dst - last.dst) { last.bytes = p.dst + p.bytes - last.dst; continue; }
    }
    runs.push_back(p);
  }
  if (runs.size() == 1) return upload_through_plan(r.plan, r.ws, r.d_raw + runs[0].dst, runs[0].src, (size_t)runs[0].bytes);
  for (const RawPlan::Piece& p : runs) {
    const hipError_t e = hipMemcpyAsync(r.d_raw + p.dst, p.src, (size_t)p.bytes, hipMemcpyHostToDevice, r.ws->stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// FLAC frames become native PCM at their files' slots, ahead of everything that reads PCM (flac/afx_flac.hip); the status
// words come down into the page-locked block.  Behind the upload as every step below is: upload_through_plan returns when
// its transfer has landed (the host waits, afx_workspace.cpp), the per-run copies are on the stream themselves.
hipError_t decode_flac(RawBatch& r) {
  if (r.flac.empty()) return hipSuccess;
  hipStream_t s = r.ws->stream;
  int32_t* d_status = (int32_t*)(r.d_raw + r.flac_status_off);
  const hipError_t e = launch_flac_decode(r.d_raw, (const FlacFile*)(r.d_raw + r.flac_table_off), (int)r.flac.size(), r.flac_frames,
                                          r.flac_tiles, d_status, s);
  if (e != hipSuccess) return e;
  return hipMemcpyAsync((unsigned char*)r.ws->h_pin + r.pin.flac_status_off, d_status, r.pin.flac_status_bytes, hipMemcpyDeviceToHost, s);
}

// big-endian files become native in place, one launch for the batch (rawpcm/afx_rawpcm.hip)
hipError_t make_native(RawBatch& r) {
  if (r.be.empty()) return hipSuccess;
  const RawNativeFile* d_be = (const RawNativeFile*)((const unsigned char*)r.d_files + r.pin.be_off);
  return launch_raw_native(r.d_raw, d_be, (int)r.be.size(), r.be_tiles, r.ws->stream);
}

// files at another rate than the plan's: mono mix and converted samples behind the batch's PCM (afx_resample.hip)
hipError_t resample(RawBatch& r) {
  if (r.conv.empty()) return hipSuccess;
  Workspace* ws = r.ws;
  hipError_t e;
  if ((e = resample_filter_table(r.plan)) != hipSuccess) return e;
  if ((e = ws_reserve(r.plan, ws->rs_files, r.conv.size() * sizeof(ResampleFile))) != hipSuccess) return e;
  if ((e = ws_reserve(r.plan, ws->rs_groups, (size_t)r.group_slots * sizeof(ResampleGroup))) != hipSuccess) return e;
  // (pageable source: the copy has left `conv` when the scan has been waited for)
  if ((e = hipMemcpyAsync(ws->rs_files.p, r.conv.data(), r.conv.size() * sizeof(ResampleFile), hipMemcpyHostToDevice, ws->stream)) != hipSuccess) return e;
  return launch_resample(r.d_raw, (const ResampleFile*)ws->rs_files.p, (int)r.conv.size(), r.conv_blocks, r.conv_max_in,
                         (ResampleGroup*)ws->rs_groups.p, r.plan->dev.rs_filter, ws->stream);
}

// the scan kernels (peak, rms, first / last sample above the floor); their results come down into the page-locked block
hipError_t scan_files(RawBatch& r) {
  // -48 dB of full scale (MSilenceThresholdDb, SampleAnalyser.cpp:51, 648-649)
  const double silence_floor = 32768.0 * std::exp(-48.0 * (std::log(10.0) / 20.0));
  LoadScan* d_scan = (LoadScan*)r.ws->scan.p;
  const hipError_t e = launch_load_scan(r.d_raw, r.d_files, r.n_bufs, silence_floor, r.ws->partial.p, d_scan, r.ws->stream);
  if (e != hipSuccess) return e;
  return hipMemcpyAsync((unsigned char*)r.ws->h_pin + r.pin.scan_off, d_scan, r.pin.scan_bytes, hipMemcpyDeviceToHost, r.ws->stream);
}

// what a caller brings in upload_pieces' place (afx_host.h: RawMove)
hipError_t move_by_caller(RawBatch& r, void* ctx) {
  const RawMoveStep& step = *(const RawMoveStep*)ctx;
  return step.move(r, r.plan, r.ws, r.d_raw, step.ctx);
}

// upload and tables -> (FLAC decode) -> (byte order) -> (conversion) -> scan -> results on the host, with one wait.
// move_pieces is the one step that touches the caller's memory: upload_pieces, or the caller's own
hipError_t stage_and_scan(RawBatch& r, const char** what, hipError_t (*move_pieces)(RawBatch&, void*), void* move_ctx) {
  hipError_t e;
  *what = "hipMalloc(raw staging)";
  if ((e = reserve_buffers(r)) != hipSuccess) return e;
  *what = "flac_decode";
  if ((e = send_flac_table(r)) != hipSuccess) return e;
  *what = "hipMemcpy(raw)";
  if ((e = move_pieces(r, move_ctx)) != hipSuccess) return e;
  *what = "hipMemcpy(tables)";
  if ((e = send_file_tables(r)) != hipSuccess) return e;
  *what = "flac_decode";
  if ((e = decode_flac(r)) != hipSuccess) return e;
  *what = "raw_native";
  if ((e = make_native(r)) != hipSuccess) return e;
  *what = "resample";
  if ((e = resample(r)) != hipSuccess) return e;
  *what = "load_scan";
  if ((e = scan_files(r)) != hipSuccess) return e;
  *what = "hipStreamSynchronize";
  if ((e = wait_for_stream(r.ws, r.ws->stream)) != hipSuccess) return e;
  const unsigned char* pin = (const unsigned char*)r.ws->h_pin;
  std::memcpy(r.scan.data(), pin + r.pin.scan_off, r.pin.scan_bytes);
  // a frame whose CRC-16 or structure did not hold fails its file; what the scan read of it is dropped with it
  for (size_t k = 0; k < r.flac.size(); ++k)
    if (((const int32_t*)(pin + r.pin.flac_status_off))[k] != 0) {
      r.status[(size_t)r.flac_buf[k]] = AFX_ERR_BAD_BUFFER;
      r.files[(size_t)r.flac_buf[k]] = LoadFile{0, 0, 0, 0};
    }
  return hipSuccess;
}

// padding rules of SampleAnalyser.cpp:681-701: where the audible part of every file goes and how long its buffer is
void place_files(RawBatch& r, afx_load_info* info) {
  const int fft = r.plan->desc.fft_size;
  for (int i = 0; i < r.n_bufs; ++i) {
    r.place[(size_t)i] = LoadPlace{};
    if (r.status[(size_t)i] != AFX_OK) { if (info) info[i] = afx_load_info{}; continue; }
    // silent leading samples = index of the first sample above the floor (all of them when there is none); the
    // trailing scan stops above that sample (SampleAnalyser.cpp:651-669)
    const LoadScan& sc = r.scan[(size_t)i];
    const int64_t n = r.files[(size_t)i].n_frames;
    const int64_t lead = (sc.trail < 0) ? n : sc.lead, trail = (sc.trail < 0) ? 0 : n - 1 - sc.trail;
    const int64_t audible = n - lead - trail;
    const int64_t end_pad = ((audible % fft) < fft / 2) ? fft / 2 : 0;
    const int64_t start_pad = (audible + end_pad < fft) ? fft - audible - end_pad : 0;
    r.lengths[(size_t)i] = audible + start_pad + end_pad;
    LoadPlace& pl = r.place[(size_t)i];
    pl.lead = lead; pl.audible = audible; pl.start_pad = start_pad;
    pl.scaling = sc.amplification / 32768.0;      // FinalScaling, SampleAnalyser.cpp:712
    if (info) {
      info[i].peak_value = (float)std::min(1.0, (double)sc.max_amp / 32768.0);
      info[i].rms_value = (float)std::min(1.0, std::sqrt(sc.sum_sq / (double)n));
      info[i].data_offset = (int32_t)(-lead + start_pad);
      info[i].silent_leading = (int32_t)lead;
      info[i].silent_trailing = (int32_t)trail;
      info[i].reserved = 0;
      info[i].n_samples = r.lengths[(size_t)i];
    }
  }
}

// fill() of the LoadSample batches: the write kernel stores the float mono signal behind the start pad
int fill_from_staging(afx_batch* b, void* ctx) {
  RawBatch& r = *(RawBatch*)ctx;
  for (int i = 0; i < r.n_bufs; ++i) r.place[(size_t)i].out_off = b->arena_off[i], r.place[(size_t)i].out_n = b->used[i];
  hipError_t e = ws_reserve(r.plan, r.ws->place, r.place.size() * sizeof(LoadPlace));
  if (e != hipSuccess) return hip_fail(e, "hipMalloc(place)");
  LoadPlace* d_place = (LoadPlace*)r.ws->place.p;
  b->h_place = r.place;   // the batch's own copy: the upload and the write kernel need not be waited for here
  e = hipMemcpyAsync(d_place, b->h_place.data(), b->h_place.size() * sizeof(LoadPlace), hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) e = launch_load_write(r.d_raw, r.d_files, d_place, r.n_bufs, (float*)b->d_pcm, b->stream);
  return e == hipSuccess ? AFX_OK : hip_fail(e, "load_write");
}

}  // namespace

// afx_batch_create_from_raw behind its plan: `planned` is plan_raw_arena's record of `raws`; move == nullptr is the
// caller's host memory (upload_pieces); afx_device_io.cpp brings a gather launch for device memory.
int batch_create_from_raw_plan(afx_plan* plan, RawPlan&& planned, const afx_raw* raws, uint32_t mask, RawMove move, void* move_ctx,
                               afx_batch** out_batch, afx_load_info* info) {
  const int32_t n_bufs = planned.n_bufs;
  RawBatch r{std::move(planned), plan};
  r.scan.resize((size_t)n_bufs);
  r.place.resize((size_t)n_bufs);
  r.lengths.assign((size_t)n_bufs, 0);

  const long long t_begin = now_ns();
  // device staging of the decoded PCM and the scan results lives in the batch's pooled workspace
  hipError_t e = hipSuccess;
  r.ws = ws_acquire(plan, &e);
  if (!r.ws) return hip_fail(e, "workspace");
  if (n_bufs > 0) {
    const char* what = "";
    RawMoveStep step{move, move_ctx};
    if ((e = move ? stage_and_scan(r, &what, move_by_caller, &step) : stage_and_scan(r, &what, upload_pieces, nullptr)) != hipSuccess) {
      ws_release(plan, r.ws);
      return hip_fail(e, what);
    }
  }
  const long long t_scanned = now_ns();
  place_files(r, info);
  // the workspace (with the staged PCM in it) moves into the batch; build_batch releases it on failure.
  // The arena keeps LoadSample's float signal; a sample of TSampleData::mData is (double)float * FinalScaling
  // (SampleAnalyser.cpp:710-718), formed by the kernels as they load it
  std::vector<int64_t> file_samples((size_t)n_bufs, 0);
  std::vector<int32_t> file_offset((size_t)n_bufs, 0);
  std::vector<double> scales((size_t)n_bufs, 1.0);
  for (int i = 0; i < n_bufs; ++i)
    if (r.status[(size_t)i] == AFX_OK) {
      const afx::LoadPlace& pl = r.place[(size_t)i];
      scales[(size_t)i] = pl.scaling;
      file_samples[(size_t)i] = raws[i].n_frames;                      // mOriginalNumberOfSamples, SampleAnalyser.cpp:464 (before the conversion)
      file_offset[(size_t)i] = (int32_t)(-pl.lead + pl.start_pad);     // mDataOffset, SampleAnalyser.cpp:701
    }
  const long long t_placed = now_ns();
  // the decoded PCM has arrived (the scan was waited for): nothing of the caller's is read after this point
  BatchSource src;
  src.n_bufs = n_bufs; src.mask = mask; src.dtype = afx::kPcmScaledF32; src.lengths = &r.lengths; src.status = &r.status;
  src.fill = fill_from_staging; src.fill_ctx = &r; src.acquired = r.ws;
  src.file_samples = &file_samples; src.file_offset = &file_offset; src.file_rate = &r.file_rate; src.scales = &scales;
  src.wait_for_uploads = false;
  const int st = build_batch(plan, src, out_batch);
  if (g_create_timing.on) {
    const long long t_end = now_ns();
    g_create_timing.ns[0] += t_scanned - t_begin; g_create_timing.ns[1] += t_placed - t_scanned;
    g_create_timing.ns[2] += t_end - t_placed; g_create_timing.ns[3] += 1;
  }
  return st;
}

}  // namespace host
}  // namespace afx

using namespace afx::host;

extern "C" {

int afx_batch_create(afx_plan* plan, const afx_buf* bufs, int32_t n_bufs, uint32_t mask,
                     afx_batch** out_batch) {
  if (!plan || !out_batch || n_bufs < 0 || (n_bufs > 0 && !bufs))
    return fail(AFX_ERR_INVALID_ARG, "null argument");
  return batch_create_typed(plan, bufs, n_bufs, mask, first_valid_dtype(bufs, n_bufs), out_batch);
}

// LoadSample front end (SampleAnalyser.cpp:484-718) on the GPU: decoded interleaved PCM in,
// peak-normalised, silence-trimmed, padded mono signal in the analysis arena out.
int afx_batch_create_from_raw(afx_plan* plan, const afx_raw* raws, int32_t n_bufs, uint32_t mask,
                              afx_batch** out_batch, afx_load_info* info) {
  if (!plan || !out_batch || n_bufs < 0 || (n_bufs > 0 && !raws))
    return fail(AFX_ERR_INVALID_ARG, "null argument");
  *out_batch = nullptr;
  if (!mask_ok(mask)) return fail(AFX_ERR_INVALID_ARG, "bad descriptor mask");
  HIP_TRY(hipSetDevice(plan->desc.device));

  // the launchers a build lacks (weak references, above) decide what the plan refuses
  return batch_create_from_raw_plan(plan, plan_raw_arena(raws, n_bufs, plan->desc.sample_rate, afx::launch_raw_native != nullptr,
                                                         afx::launch_flac_decode != nullptr),
                                    raws, mask, nullptr, nullptr, out_batch, info);
}

int afx_extract_batch(afx_plan* plan, const afx_buf* bufs, int32_t n_bufs, uint32_t mask, afx_out* out) {
  if (!out) return fail(AFX_ERR_INVALID_ARG, "null output");
  if (!plan || n_bufs < 0 || (n_bufs > 0 && !bufs)) return fail(AFX_ERR_INVALID_ARG, "null argument");
  // Large calls (a crawler handing over 10^5 files) are cut into groups of buffers of at most
  // kSplitFrames frames so that the device workspace (8 KiB of magnitudes per frame when the band
  // descriptors are on) stays bounded; results land at the right rows of the caller's arrays.
  constexpr int64_t kSplitFrames = 1 << 19;
  int64_t total = 0;
  for (int i = 0; i < n_bufs; ++i) total += (bufs[i].n_samples > 0) ? num_frames(plan, bufs[i].n_samples) : 0;
  if (total <= kSplitFrames || n_bufs <= 1) {
    afx_batch* b = nullptr;
    int st = afx_batch_create(plan, bufs, n_bufs, mask, &b);
    if (st != AFX_OK) return st;
    st = afx_batch_run(b);
    if (st == AFX_OK) st = afx_batch_fetch(b, out);
    afx_batch_destroy(b);
    return st;
  }
  const int call_dtype = first_valid_dtype(bufs, n_bufs);
  struct Col { double* afx_out::*field; int width; };
  std::vector<Col> cols;
  for (const FieldDesc& d : kFields) cols.push_back(Col{d.out, d.width});
  cols.push_back(Col{&afx_out::magnitude, 1024});
  int64_t row0 = 0;
  int32_t first = 0;
  if (out->frame_offset) out->frame_offset[0] = 0;
  while (first < n_bufs) {
    int32_t last = first;
    int64_t group = 0;
    while (last < n_bufs) {
      const int64_t f = (bufs[last].n_samples > 0) ? num_frames(plan, bufs[last].n_samples) : 0;
      if (last > first && group + f > kSplitFrames) break;
      group += f;
      ++last;
    }
    afx_out part = *out;
    for (const Col& c : cols)
      if (out->*(c.field)) part.*(c.field) = out->*(c.field) + row0 * c.width;
    std::vector<int64_t> off((size_t)(last - first) + 1);
    part.frame_offset = off.data();
    part.buf_status = out->buf_status ? out->buf_status + first : nullptr;
    part.effective_length = out->effective_length ? out->effective_length + (size_t)first * 3 : nullptr;
    afx_batch* b = nullptr;
    int st = batch_create_typed(plan, bufs + first, last - first, mask, call_dtype, &b);
    if (st != AFX_OK) return st;
    st = afx_batch_run(b);
    if (st == AFX_OK) st = afx_batch_fetch(b, &part);
    afx_batch_destroy(b);
    if (st != AFX_OK) return st;
    if (out->frame_offset)
      for (int32_t i = first; i < last; ++i) out->frame_offset[i + 1] = row0 + off[(size_t)(i - first) + 1];
    row0 += off.back();
    first = last;
  }
  return AFX_OK;
}

}  // extern "C"
