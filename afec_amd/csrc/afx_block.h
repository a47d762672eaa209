// afec_amd/csrc/afx_block.h -- how the fetches above a run (afx_high_level.cpp, afx_high_level_text.cpp,
// afx_classification.cpp, afx_class_decision.cpp, afx_high_level_row.cpp) lay out memory, host only.  A block holds typed arrays behind one
// another, the same way on the
// device and on the host, so that one transfer moves a run of them.  Layout hands out the offsets and is the only place a
// byte offset is formed; each fetch names its block once as a struct of offsets with point() (the kernel's arguments into a
// block at `base`) and hand_out() (the host copy into the caller's arrays).  ResultBlock is the batch's reused block behind
// the checks every such fetch starts with, DeviceBlock the memory of an entry point that has no batch.
#pragma once

#include <cstring>

#include "afx_host.h"
#include "classify/afx_classify.h"
#include "highlevel/afx_highlevel.h"

namespace afx {
namespace host {

// Every array starts at a multiple of 8 bytes, the alignment of the widest type a block holds: an odd number of int32 or
// float in front of doubles costs four bytes, and any array's offset is a place where a transfer may start or end.
class Layout {
 public:
  template <typename T>
  size_t take(size_t count) {
    static_assert(alignof(T) <= 8, "a block is aligned for doubles");
    const size_t at = bytes_;
    bytes_ = (at + count * sizeof(T) + 7) & ~(size_t)7;
    return at;
  }
  size_t bytes() const { return bytes_; }   // so far: where the next array will start

 private:
  size_t bytes_ = 0;
};

template <typename T>
T* at(char* base, size_t offset) { return reinterpret_cast<T*>(base + offset); }
template <typename T>
const T* at(const char* base, size_t offset) { return reinterpret_cast<const T*>(base + offset); }

// The workspace's result buffer on the device and the page-locked one it lands in, reserved for one fetch's layout (the
// fetches are synchronous: one at a time uses them).  n: the batch's buffers; 0: nothing reserved, nothing to launch.
// `uploaded`: an event the enqueue halves below record on the batch's stream directly behind each copy out of `host`, for a
// caller that returns without waiting for the stream (afx_device_file_io.cpp) and so has to know when `host` may be written
// again; nullptr (every synchronous fetch): nothing is recorded.
struct ResultBlock {
  size_t n = 0;
  char *dev = nullptr, *host = nullptr;
  hipEvent_t uploaded = nullptr;
};

#define AFX_TRY(expr)                   \
  do {                                  \
    const int st_ = (expr);             \
    if (st_ != AFX_OK) return st_;      \
  } while (0)

// What every fetch above a run starts with.  `has_inputs`: the batch's mask holds what the fetch reads (`lacks` is the
// text when not); `who` names the entry point for "... before afx_batch_run".  AFX_OK with rb->n == 0: an empty batch.
inline int reserve_result_block(afx_batch* b, bool has_inputs, const char* lacks, const char* who, const Layout& layout, ResultBlock* rb) {
  if (!has_inputs) return fail(AFX_ERR_INVALID_ARG, lacks);
  if (!b->ran) return fail(AFX_ERR_INVALID_ARG, std::string(who) + " before afx_batch_run");
  if (b->n_bufs == 0) return AFX_OK;
  HIP_TRY(hipSetDevice(b->plan->desc.device));
  HIP_TRY(ws_reserve(b->plan, b->ws->high, layout.bytes()));
  HIP_TRY(ws_result_pin_reserve(b->ws, layout.bytes()));
  rb->n = (size_t)b->n_bufs;
  rb->dev = (char*)b->ws->high.p;
  rb->host = (char*)b->ws->h_high;
  return AFX_OK;
}

// [from, to) of the block from the device to the host: waits for the batch's stream first, then for the transfer
inline hipError_t download_result(afx_batch* b, const ResultBlock& rb, size_t from, size_t to) {
  const Download item{rb.host + from, rb.dev + from, to - from};
  return download_through_plan(b, &item, 1);
}

// Device memory of a call's own, freed when it leaves scope.
class DeviceBlock {
 public:
  DeviceBlock() = default;
  DeviceBlock(const DeviceBlock&) = delete;
  DeviceBlock& operator=(const DeviceBlock&) = delete;
  ~DeviceBlock() {
    if (p_) (void)hipFree(p_);
  }
  int allocate(size_t bytes, const char* what) {   // `what`: the text of AFX_ERR_OUT_OF_MEMORY
    const hipError_t e = hipMalloc(&p_, bytes);
    if (e == hipSuccess) return AFX_OK;
    p_ = nullptr;
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      return fail(AFX_ERR_OUT_OF_MEMORY, what);
    }
    return hip_fail(e, "hipMalloc");
  }
  char* get() const { return (char*)p_; }

 private:
  void* p_ = nullptr;
};

// The high-level block: what high_level_kernel writes and the fetch brings back (scalars, signature, pitch, peak), behind
// it the caller's peak / rms pairs on their way up.
struct HighBlock {
  size_t n, frames, scalars, signature, pitch, peak, levels;
  HighBlock(Layout& l, size_t n_bufs, size_t total_frames) : n(n_bufs), frames(total_frames) {
    scalars = l.take<double>(n * kHighScalars);
    signature = l.take<double>(n * kHighSignatureFrames * kHighSignatureBands);
    pitch = l.take<double>(frames);
    peak = l.take<double>(frames);
    levels = l.take<float>(n * 2);
  }
  void point(HighArgs* a, char* base, bool with_levels) const {
    a->scalars = at<double>(base, scalars);
    a->signature = at<double>(base, signature);
    a->pitch = at<double>(base, pitch);
    a->peak = at<double>(base, peak);
    a->levels = with_levels ? at<float>(base, levels) : nullptr;
  }
  void hand_out(const char* host, afx_high_out* out) const {
    if (out->scalars) std::memcpy(out->scalars, host + scalars, n * kHighScalars * sizeof(double));
    if (out->signature) std::memcpy(out->signature, host + signature, n * kHighSignatureFrames * kHighSignatureBands * sizeof(double));
    if (out->pitch && frames) std::memcpy(out->pitch, host + pitch, frames * sizeof(double));
    if (out->peak && frames) std::memcpy(out->peak, host + peak, frames * sizeof(double));
  }
};

// afx_high_level.cpp: the launch the two high-level fetches share.  Reserves the batch's result block for `layout` (which
// starts with `hb`) behind the checks of afx_batch_fetch_high_level, uploads the levels where there are any and launches
// high_level_kernel, all on the batch's stream; nothing is downloaded.  rb->n == 0: an empty batch, nothing launched.
int launch_high_level_block(afx_batch* b, const char* who, const afx_load_info* levels, const Layout& layout, const HighBlock& hb, ResultBlock* rb);
// Its two halves, for a fetch whose one layout holds the blocks of several fetches (afx_high_level_row.cpp): what it asks of
// the batch's mask, and the upload and launch into `hb` wherever that lies in a block already reserved.
bool has_high_level_inputs(const afx_batch* b);
extern const char* const kLacksHighLevelInputs;
int enqueue_high_level(afx_batch* b, const afx_load_info* levels, const HighBlock& hb, const ResultBlock& rb);

// What classification_features_kernel writes and the feature fetch brings back (features, counts), then what goes up for it
// in one transfer: effectve_length_12dB for the features, effectve_length_24dB for the class decision's heuristics, the
// buffers' status.  A fetch that runs kernels of its own on the features takes its arrays from the same Layout behind it.
struct FeatureBlock {
  size_t n, features, non_finite, efflen12, efflen24, status, end;
  FeatureBlock(Layout& l, size_t n_bufs) : n(n_bufs) {
    features = l.take<double>(n * kClassifyFeatures);
    non_finite = l.take<int32_t>(n);
    efflen12 = l.take<double>(n);
    efflen24 = l.take<double>(n);
    status = l.take<int32_t>(n);
    end = l.bytes();
  }
  void point(ClassifyArgs* a, char* base) const {
    a->features = at<double>(base, features);
    a->non_finite = at<int32_t>(base, non_finite);
    a->efflen12 = at<double>(base, efflen12);
    a->status = at<int32_t>(base, status);
  }
  void hand_out(const char* host, double* out_features, int32_t* out_non_finite) const {
    std::memcpy(out_features, host + features, n * kClassifyFeatures * sizeof(double));
    if (out_non_finite) std::memcpy(out_non_finite, host + non_finite, n * sizeof(int32_t));
  }
};

// afx_classification.cpp: the launch the three batch fetches of the features share.  Reserves the batch's result block for
// `layout` (which starts with `fb`), uploads the kernel's small inputs and launches it, all on the batch's stream; nothing
// is downloaded and nothing waited for behind the launch.  rb->n == 0: an empty batch, nothing launched.
int launch_features(afx_batch* b, const char* who, const Layout& layout, const FeatureBlock& fb, ResultBlock* rb);
// Its two halves, as above: the mask's check, and the upload and launch into `fb` anywhere in a reserved block.
bool has_feature_inputs(const afx_batch* b);
extern const char* const kLacksFeatureInputs;
int enqueue_features(afx_batch* b, const FeatureBlock& fb, const ResultBlock& rb);

}  // namespace host
}  // namespace afx
