// afec_amd/csrc/afx_device_io.cpp -- device-resident input and output: a batch from device pointers
// (afx_batch_create_from_device: afx_batch_create's rules, one gather launch in place of its transfers) and chosen series
// of a batch's records into device memory of the caller's (afx_batch_export_device and its two companions); and (DESIGN
// 4.21) LoadSample on raw PCM in device memory (afx_batch_create_from_raw_device: afx_batch_create_from_raw's plan and
// steps, one gather launch in place of its transfers) and the analysed samples into device memory
// (afx_batch_export_samples_device, afx_batch_export_sample_counts_device).  Everything is decided by
// devio/afx_devio_plan.h and devio/afx_devio_raw_plan.h before anything is enqueued; here the runtime is asked what the
// caller's pointers are, and the record is enqueued.  See afx_host.h for the map of the host side.

#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "afx_host.h"
#include "devio/afx_devio.h"
#include "devio/afx_devio_plan.h"
#include "devio/afx_devio_raw.h"
#include "devio/afx_devio_raw_plan.h"

using namespace afx::host;

namespace {

hipError_t devio_event(Workspace* ws) {
  return ws->ev_devio ? hipSuccess : hipEventCreateWithFlags(&ws->ev_devio, hipEventDisableTiming);
}

struct DeviceBuffers {   // fill() of afx_batch_create_from_device: the caller's device memory, one gather launch
  const afx_buf* bufs;   // as devio_checked_buffers left them
  int32_t n_bufs;
  hipStream_t producer;
  GatherPlan gather;     // lives until the create has waited for its upload
};
int fill_from_device(afx_batch* b, void* ctx) {
  DeviceBuffers& c = *(DeviceBuffers*)ctx;
  c.gather = plan_gather(c.bufs, b->used.data(), b->arena_off.data(), c.n_bufs);
  if (!c.gather.ok) return fail(AFX_ERR_INVALID_ARG, "more samples than one gather launch covers");
  if (c.gather.table.empty()) return AFX_OK;
  Workspace* ws = b->ws;
  const size_t bytes = c.gather.table.size() * sizeof(afx::DevioBuf);
  hipError_t e = ws_reserve(b->plan, ws->devio_in, bytes);
  if (e != hipSuccess) return hip_fail(e, "hipMalloc(gather table)");
  // what the producer has enqueued so far is in front of the gather
  if ((e = devio_event(ws)) != hipSuccess) return hip_fail(e, "hipEventCreate");
  if ((e = hipEventRecord(ws->ev_devio, c.producer)) != hipSuccess) return hip_fail(e, "hipEventRecord(producer)");
  if ((e = hipStreamWaitEvent(b->stream, ws->ev_devio, 0)) != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
  if ((e = hipMemcpyAsync(ws->devio_in.p, c.gather.table.data(), bytes, hipMemcpyHostToDevice, b->stream)) != hipSuccess)
    return hip_fail(e, "hipMemcpy(gather table)");
  e = afx::launch_devio_gather(b->d_pcm, (const afx::DevioBuf*)ws->devio_in.p, (int)c.gather.table.size(), c.gather.tiles,
                               b->pcm_dtype == afx::kPcmF64 ? 8 : 4, b->stream);
  return e == hipSuccess ? AFX_OK : hip_fail(e, "devio_gather");
}

struct BatchShape : ExportShape {
  int32_t off[AFX_NUM_SERIES], wid[AFX_NUM_SERIES];
  explicit BatchShape(const afx_batch* b) {
    int i = 0;
    for (const FieldDesc& d : kFields) { off[i] = b->lay.*(d.off); wid[i] = d.width; ++i; }
    ran = b->ran;
    n_bufs = b->n_bufs;
    frame_offset = b->frame_offset.data();
    stride = b->lay.stride;
    offsets = off; widths = wid;
    has_magnitude = (b->mask & AFX_D_MAGNITUDE) != 0 && (b->d_mag || b->total_frames == 0);
    has_statistics = b->d_stats != nullptr || b->n_bufs == 0;
  }
  BatchShape(const BatchShape&) = delete;
};

// every destination's extent inside one allocation of the plan's device
bool destinations_ok(const afx_batch* b, const afx_device_out* outs, const std::vector<uint64_t>& extent_bytes) {
  std::vector<DevioAlloc> allocs(extent_bytes.size());
  for (size_t k = 0; k < extent_bytes.size(); ++k)
    if (extent_bytes[k] > 0) allocs[k] = devio_ask_runtime(outs[k].dst);
  return devio_extents_ok(outs, extent_bytes, allocs.data(), b->plan->desc.device);
}

// frame_offset on the device, uploaded once per batch behind whatever its stream holds (the host copy is the batch's own)
int device_frame_offsets(afx_batch* b) {
  if (b->d_devio_foff) return AFX_OK;
  const size_t bytes = b->frame_offset.size() * sizeof(int64_t);
  HIP_TRY(ws_reserve(b->plan, b->ws->devio_out, bytes));
  HIP_TRY(hipMemcpyAsync(b->ws->devio_out.p, b->frame_offset.data(), bytes, hipMemcpyHostToDevice, b->stream));
  b->d_devio_foff = (int64_t*)b->ws->devio_out.p;
  return AFX_OK;
}

struct RawDeviceBuffers {   // RawMove of afx_batch_create_from_raw_device: one gather launch in place of the transfers
  hipStream_t producer;
  const RawGatherPlan* gather;   // lives until the create has waited for its scan
  int elementwise;
};
hipError_t gather_raw(const RawPlan&, afx_plan* plan, Workspace* ws, unsigned char* d_raw, void* ctx) {
  const RawDeviceBuffers& c = *(const RawDeviceBuffers*)ctx;
  if (c.gather->table.empty()) return hipSuccess;
  const size_t bytes = c.gather->table.size() * sizeof(afx::DevioRawBuf);
  hipError_t e;
  if ((e = ws_reserve(plan, ws->devio_in, bytes)) != hipSuccess) return e;
  // what the producer has enqueued so far is in front of the gather
  if ((e = devio_event(ws)) != hipSuccess) return e;
  if ((e = hipEventRecord(ws->ev_devio, c.producer)) != hipSuccess) return e;
  if ((e = hipStreamWaitEvent(ws->stream, ws->ev_devio, 0)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(ws->devio_in.p, c.gather->table.data(), bytes, hipMemcpyHostToDevice, ws->stream)) != hipSuccess) return e;
  return afx::launch_devio_raw_gather(d_raw, (const afx::DevioRawBuf*)ws->devio_in.p, (int)c.gather->table.size(), c.gather->tiles,
                                      c.elementwise, ws->stream);
}

// arena_off, used and the scalings on the device, uploaded once per batch behind whatever its stream holds
int device_sample_rows(afx_batch* b) {
  if (b->d_devio_rows || b->n_bufs == 0) return AFX_OK;
  const size_t n = (size_t)b->n_bufs;
  b->h_devio_rows.assign(3 * n, 0);
  for (size_t i = 0; i < n; ++i) {
    const double scale = b->pcm_dtype == afx::kPcmScaledF32 ? b->buf_scale[i] : 1.0;
    b->h_devio_rows[i] = b->arena_off[i];
    b->h_devio_rows[n + i] = b->used[i];
    std::memcpy(&b->h_devio_rows[2 * n + i], &scale, sizeof(double));
  }
  const size_t bytes = 3 * n * sizeof(int64_t);
  HIP_TRY(ws_reserve(b->plan, b->ws->devio_rows, bytes));
  HIP_TRY(hipMemcpyAsync(b->ws->devio_rows.p, b->h_devio_rows.data(), bytes, hipMemcpyHostToDevice, b->stream));
  b->d_devio_rows = (int64_t*)b->ws->devio_rows.p;
  return AFX_OK;
}

}  // namespace

namespace afx {
namespace host {

// what the runtime says of a pointer (nothing is enqueued, nothing is read through it)
DevioAlloc devio_ask_runtime(const void* p) {
  DevioAlloc a;
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();   // a pointer the runtime does not know is an answer, not a failure of the call
    return a;
  }
  if (attr.type != hipMemoryTypeDevice) return a;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
    (void)hipGetLastError();
    return a;
  }
  a.device = true;
  a.ordinal = attr.device;
  a.base = (uint64_t)(uintptr_t)base;
  a.size = (uint64_t)size;
  return a;
}

// the consumer's stream behind the launch, or the host
int devio_hand_over(afx_batch* b, void* consumer_stream) {
  if (!consumer_stream) {
    HIP_TRY(wait_for_stream(b->ws, b->stream));
    return AFX_OK;
  }
  HIP_TRY(devio_event(b->ws));
  HIP_TRY(hipEventRecord(b->ws->ev_devio, b->stream));
  HIP_TRY(hipStreamWaitEvent((hipStream_t)consumer_stream, b->ws->ev_devio, 0));
  return AFX_OK;
}

}  // namespace host
}  // namespace afx

extern "C" {

int afx_batch_create_from_device(afx_plan* plan, const afx_buf* bufs, int32_t n_bufs, uint32_t mask, void* producer_stream,
                                 afx_batch** out_batch) {
  if (!plan || !out_batch || n_bufs < 0 || (n_bufs > 0 && !bufs))
    return fail(AFX_ERR_INVALID_ARG, "null argument");
  *out_batch = nullptr;
  HIP_TRY(hipSetDevice(plan->desc.device));
  std::vector<DevioAlloc> allocs((size_t)n_bufs);
  for (int32_t i = 0; i < n_bufs; ++i)
    if (devio_buffer_is_read(bufs[i])) allocs[(size_t)i] = devio_ask_runtime(bufs[i].pcm);
  const std::vector<afx_buf> checked = devio_checked_buffers(bufs, allocs.data(), n_bufs, plan->desc.device);
  DeviceBuffers ctx{checked.data(), n_bufs, (hipStream_t)producer_stream, {}};
  return batch_create_filled(plan, checked.data(), n_bufs, mask, first_valid_dtype(checked.data(), n_bufs), fill_from_device, &ctx,
                             out_batch);
}

int afx_batch_export_device(afx_batch* b, const afx_device_out* outs, int32_t n_outs, int32_t layout, int64_t max_frames,
                            double pad_value, void* consumer_stream) {
  if (!b) return fail(AFX_ERR_INVALID_ARG, "null batch");
  const BatchShape shape(b);
  ExportPlan p = plan_export(shape, outs, n_outs, layout, max_frames, pad_value);
  if (p.status != AFX_OK) return fail(p.status, p.why);
  HIP_TRY(hipSetDevice(b->plan->desc.device));
  if (!destinations_ok(b, outs, p.extent_bytes))
    return fail(AFX_ERR_INVALID_ARG, "a destination's extent does not lie inside one device allocation on the plan's device");
  if (p.needs_frame_offsets) {
    const int st = device_frame_offsets(b);
    if (st != AFX_OK) return st;
  }
  p.args.rec = b->d_rec;
  p.args.mag = b->d_mag;
  p.args.frame_offset = b->d_devio_foff;
  HIP_TRY(afx::launch_devio_export(p.args, b->stream));
  return devio_hand_over(b, consumer_stream);
}

int afx_batch_export_statistics_device(afx_batch* b, const afx_device_out* outs, int32_t n_outs, void* consumer_stream) {
  if (!b) return fail(AFX_ERR_INVALID_ARG, "null batch");
  const BatchShape shape(b);
  StatsExportPlan p = plan_export_statistics(shape, outs, n_outs);
  if (p.status != AFX_OK) return fail(p.status, p.why);
  HIP_TRY(hipSetDevice(b->plan->desc.device));
  if (!destinations_ok(b, outs, p.extent_bytes))
    return fail(AFX_ERR_INVALID_ARG, "a destination's extent does not lie inside one device allocation on the plan's device");
  p.args.stats = b->d_stats;
  HIP_TRY(afx::launch_devio_export_stats(p.args, b->stream));
  return devio_hand_over(b, consumer_stream);
}

int afx_batch_export_frame_counts_device(afx_batch* b, int64_t* d_counts, void* consumer_stream) {
  if (!b) return fail(AFX_ERR_INVALID_ARG, "null batch");
  if (!b->ran) return fail(AFX_ERR_INVALID_ARG, "export before afx_batch_run");
  if (b->n_bufs > 0 && !d_counts) return fail(AFX_ERR_INVALID_ARG, "null destination");
  HIP_TRY(hipSetDevice(b->plan->desc.device));
  if (b->n_bufs > 0) {
    afx_device_out out{};
    out.dst = d_counts;
    if (!destinations_ok(b, &out, std::vector<uint64_t>{(uint64_t)b->n_bufs * sizeof(int64_t)}))
      return fail(AFX_ERR_INVALID_ARG, "the destination does not lie inside one device allocation on the plan's device");
    const int st = device_frame_offsets(b);
    if (st != AFX_OK) return st;
    HIP_TRY(afx::launch_devio_frame_counts(b->d_devio_foff, b->n_bufs, d_counts, b->stream));
  }
  return devio_hand_over(b, consumer_stream);
}

int afx_batch_create_from_raw_device(afx_plan* plan, const afx_raw_device* raws, int32_t n_bufs, uint32_t mask, void* producer_stream,
                                     afx_batch** out_batch, afx_load_info* info) {
  if (!plan || !out_batch || n_bufs < 0 || (n_bufs > 0 && !raws))
    return fail(AFX_ERR_INVALID_ARG, "null argument");
  *out_batch = nullptr;
  if (!mask_ok(mask)) return fail(AFX_ERR_INVALID_ARG, "bad descriptor mask");
  HIP_TRY(hipSetDevice(plan->desc.device));
  std::vector<DevioAlloc> allocs((size_t)n_bufs);
  for (int32_t i = 0; i < n_bufs; ++i)
    if (devio_raw_is_read(raws[i])) allocs[(size_t)i] = devio_ask_runtime(raws[i].data);
  const std::vector<afx_raw> checked = devio_raw_checked(raws, allocs.data(), n_bufs, plan->desc.device);
  // afx_batch_create_from_raw's plan of the same buffers, made without the FLAC decoder: a stream's descriptor would be
  // read on the host
  RawPlan planned = plan_raw_arena(checked.data(), n_bufs, plan->desc.sample_rate, true, false);
  const RawGatherPlan gather = plan_raw_gather(planned, raws);
  if (!gather.ok) return fail(AFX_ERR_INVALID_ARG, "more sample frames than one gather launch covers");
  // AFX_DEVIO_RAW_ELEMENTWISE in the environment: misaligned interleaved buffers element by element (diagnostic, for
  // tools/devio_raw_cost.py's comparison of the two forms)
  static const int elementwise = std::getenv("AFX_DEVIO_RAW_ELEMENTWISE") != nullptr;
  RawDeviceBuffers ctx{(hipStream_t)producer_stream, &gather, elementwise};
  return batch_create_from_raw_plan(plan, std::move(planned), checked.data(), mask, gather_raw, &ctx, out_batch, info);
}

int afx_batch_export_samples_device(afx_batch* b, void* dst, int32_t dtype, int64_t buf_stride, double pad_value, void* consumer_stream) {
  if (!b) return fail(AFX_ERR_INVALID_ARG, "null batch");
  const SamplesExportPlan p = plan_export_samples(b->used.data(), b->n_bufs, dst, dtype, buf_stride);
  if (p.status != AFX_OK) return fail(p.status, p.why);
  HIP_TRY(hipSetDevice(b->plan->desc.device));
  if (p.extent_bytes > 0) {
    if (!devio_range_ok(devio_ask_runtime(dst), b->plan->desc.device, dst, p.extent_bytes))
      return fail(AFX_ERR_INVALID_ARG, "the destination's extent does not lie inside one device allocation on the plan's device");
    const int st = device_sample_rows(b);
    if (st != AFX_OK) return st;
    afx::DevioSamplesArgs a{};
    a.pcm = b->d_pcm; a.rows = b->d_devio_rows; a.dst = dst; a.buf_stride = buf_stride; a.pad_value = pad_value;
    a.n_bufs = b->n_bufs; a.pcm_kind = b->pcm_dtype; a.f32 = p.f32; a.tiles_per_row = p.tiles_per_row;
    HIP_TRY(afx::launch_devio_samples(a, b->stream));
  }
  return devio_hand_over(b, consumer_stream);
}

int afx_batch_export_sample_counts_device(afx_batch* b, int64_t* d_counts, void* consumer_stream) {
  if (!b) return fail(AFX_ERR_INVALID_ARG, "null batch");
  if (b->n_bufs > 0 && !d_counts) return fail(AFX_ERR_INVALID_ARG, "null destination");
  HIP_TRY(hipSetDevice(b->plan->desc.device));
  if (b->n_bufs > 0) {
    if (!devio_range_ok(devio_ask_runtime(d_counts), b->plan->desc.device, d_counts, (uint64_t)b->n_bufs * sizeof(int64_t)))
      return fail(AFX_ERR_INVALID_ARG, "the destination does not lie inside one device allocation on the plan's device");
    const int st = device_sample_rows(b);
    if (st != AFX_OK) return st;
    HIP_TRY(afx::launch_devio_sample_counts(b->d_devio_rows, b->n_bufs, d_counts, b->stream));
  }
  return devio_hand_over(b, consumer_stream);
}

}  // extern "C"
