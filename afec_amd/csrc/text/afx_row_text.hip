// afec_amd/csrc/text/afx_row_text.hip -- the class decision's arrays in device memory as the six text columns the reference's
// high-level database stores for them (SToJSON, SqliteSampleDescriptorPool.cpp:316-358, 884-904):
//   class_signature_VR, class_strengths_VR, category_signature_VR, category_strengths_VR   "[a,b]", every number as
//       ToString(double, "%.9g") writes it (text/afx_g9.h); the signatures are floats, widened as SampleAnalyser.cpp:1097
//       and 1190 widen them
//   classes_VS, categories_VS   ["Name","Other"]: the names of the picked indices in pick order, copied verbatim (the
//       reference neither escapes nor quotes inside), "[]" when nothing was picked
// A host thread would otherwise run "%.9g" on 4 + 2 K numbers per file and build two string lists.
//
// One wave per file, four files per workgroup as json_g9_kernel has four columns.  A model has at most 64 classes, so every
// column is one stride of the wave:
//   numbers   a lane makes its value's digits and length, an inclusive scan (DPP, afx_device.h) places them, the lanes
//             write into an LDS stage that starts at the slot's offset in its 4-byte word, the wave copies whole words out
//   names     lane j holds pick j; the list is the picks in front of the first index that names no class; a scan of
//             len + 3 places them; the wave then copies name after name, lanes over the bytes
// The slots are the host's (afx_row_text.h): no cursor is shared between waves, nothing behind `length` is written.

#include <hip/hip_runtime.h>

#include "afx_row_text.h"
#include "afx_g9.h"
#include "../afx_device.h"

namespace afx {
namespace {

constexpr int kWaves = 4;                                   // files per workgroup (the waves share nothing but the launch)
constexpr int kMaxPerValue = 1 + kG9MaxChars + 1;           // "[" or ",", the number, the column's "]"
constexpr int kStageWords = (3 + 64 * kMaxPerValue + 3) / 4;

// "[a,b,...]" of lane j's `v`, j < n <= 64, at `out`; returns its length
__device__ __forceinline__ int write_numbers(double v, int n, int lane, char* out, const G9Limbs& limbs, uint32_t* stage_words) {
  if (n <= 0) {   // SToJSON of an empty list
    if (lane < 2) out[lane] = lane ? ']' : '[';
    return 2;
  }
  char* stage = reinterpret_cast<char*>(stage_words);
  const bool inside = lane < n;
  G9 g{};
  int len = 0;
  if (inside) {
    g = g9_digits(v, limbs);
    len = 1 + g9_length(g) + (lane == n - 1 ? 1 : 0);
  }
  const int incl = wave_scan_incl(len);
  const int total = __builtin_amdgcn_readlane(incl, 63);
  // the stage's byte 0 is the first byte of the aligned word that holds the column's first character
  const int skew = (int)((uintptr_t)out & 3u);
  if (inside) {
    char* s = stage + skew + (incl - len);
    *s++ = lane == 0 ? '[' : ',';
    s += g9_write(g, s);
    if (lane == n - 1) *s++ = ']';
  }
  wave_lds_fence();
  char* dst = out - skew;   // aligned
  const int end = skew + total;
  for (int w = lane; 4 * w < end; w += 64) {
    const int b0 = 4 * w;
    if (b0 >= skew && b0 + 4 <= end) {
      *reinterpret_cast<uint32_t*>(dst + b0) = stage_words[w];
    } else {
      for (int k = 0; k < 4; ++k)
        if (b0 + k >= skew && b0 + k < end) dst[b0 + k] = stage[b0 + k];
    }
  }
  wave_lds_fence();   // the next column writes the stage again
  return total;
}

// ["Name","Other"] of the picks in front of the first one that names no class, at `out`; returns its length
__device__ __forceinline__ int write_names(const RowTextArgs& a, const RowTextModel& m, int64_t file, int lane, char* out) {
  int pick = -1;
  if (lane < m.count) pick = m.picks[file * m.count + lane];
  const bool named = pick >= 0 && pick < m.count;
  const uint64_t ends = ~__ballot(named);                     // lanes from m.count on are set: the list ends there at the latest
  int picked = __builtin_amdgcn_readfirstlane(ends ? __builtin_ctzll(ends) : 64);
  int offset = 0, bytes = 0;
  if (lane < picked) {
    offset = a.name_offset[m.first_name + pick];
    bytes = a.name_length[m.first_name + pick];
  }
  const int len = lane < picked ? bytes + 3 : 0;              // "[" or ",", two quotes
  const int incl = wave_scan_incl(len);
  int total = __builtin_amdgcn_readlane(incl, 63) + 1;       // "]"
  if (picked == 0 || total > m.names_slot) {                  // (an index picked twice could outgrow the slot: no such list)
    if (lane < 2) out[lane] = lane ? ']' : '[';
    return 2;
  }
  if (lane < picked) {
    char* s = out + (incl - len);
    s[0] = lane == 0 ? '[' : ',';
    s[1] = '"';
    s[2 + bytes] = '"';
  }
  if (lane == 0) out[total - 1] = ']';
  for (int e = 0; e < picked; ++e) {
    const int at = __shfl(incl - len, e) + 2, n = __shfl(bytes, e), from = __shfl(offset, e);
    for (int t = lane; t < n; t += 64) out[at + t] = a.name_bytes[from + t];
  }
  return total;
}

__global__ __launch_bounds__(64 * kWaves) void class_text_kernel(RowTextArgs a) {
  __shared__ uint32_t limbs_all[kWaves * kG9Limbs * 64];
  __shared__ uint32_t stage_all[kWaves * kStageWords];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int file = (int)blockIdx.x * kWaves + wave;
  if (file >= a.n_files) return;
  const G9Limbs limbs{limbs_all + wave * (kG9Limbs * 64) + lane, 64};
  uint32_t* stage_words = stage_all + wave * kStageWords;
  int64_t slot = a.file_slot[file];

  for (int column = 0; column < kRowTextColumns; ++column) {
    const bool second = column >= 3;
    const RowTextModel& m = second ? a.categories : a.classes;
    const int count = __builtin_amdgcn_readfirstlane(m.count), kind = column - (second ? 3 : 0);
    char* out = a.text + slot;
    int length;
    if (kind == 1) {
      length = write_names(a, m, file, lane, out);
      slot += m.names_slot;
    } else {
      double v = 0.0;
      if (lane < count) v = kind == 0 ? (double)m.signature[(int64_t)file * count + lane] : m.strengths[(int64_t)file * count + lane];
      length = write_numbers(v, count, lane, out, limbs, stage_words);
      slot += text_slot_bytes(count, 0);
    }
    if (lane == 0) {
      a.begin[(int64_t)file * kRowTextColumns + column] = out - a.text;
      a.length[(int64_t)file * kRowTextColumns + column] = length;
    }
  }
}

}  // namespace

hipError_t launch_row_text(const RowTextArgs& a, const TextArgs* vectors, hipStream_t stream) {
  if (a.n_files > 0) {
    const int blocks = (a.n_files + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(class_text_kernel, dim3(blocks), dim3(64 * kWaves), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return vectors ? launch_json_g9(*vectors, stream) : hipSuccess;
}

}  // namespace afx
