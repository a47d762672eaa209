// afec_amd/csrc/text/afx_text.hip -- columns of doubles in device memory as the JSON text the reference's high-level database
// stores (SToJSON, SqliteSampleDescriptorPool.cpp:316-419: "[a,b]" or "[[a,b],[c,d]]", "," alone between the numbers, every
// number as ToString(double, "%.9g") writes it -- text/afx_g9.h).  The host would spend 0.1 - 0.3 us per number on this;
// a file has 1 000 to 2 600 of them.
//
// One wave per column, lanes over its values in strides of 64:
//   1. a lane makes its value's nine digits and exponent (g9_digits; integer arithmetic, the limbs of the rare values
//      outside 1e-18 .. 1e26 in LDS, a column of 34 per lane) and the length of its characters with the brackets and the
//      comma that go in front of and behind it
//   2. an inclusive scan of the lengths (DPP, afx_device.h) places the lanes' characters in the stride, a carried position
//      places the stride in the column's slot
//   3. the lanes write their characters into an LDS stage that starts at the slot position's offset in its 4-byte word, so
//      the wave then copies the stage out in whole aligned words (bytes only at the two ends)
// The slot is the host's (text_slot_bytes): no cursor is shared between waves, and the text of a column is the same bytes
// at the same place on every run.  Nothing here is bound by arithmetic: the stores are.

#include <hip/hip_runtime.h>

#include "afx_text.h"
#include "afx_g9.h"
#include "../afx_device.h"

namespace afx {
namespace {

constexpr int kWaves = 4;                                   // columns per workgroup (the waves share nothing but the launch)
constexpr int kMaxPerValue = 2 + kG9MaxChars + 2;           // ",[" or "[[", the number, "]" and the column's "]"
constexpr int kStageWords = (3 + 64 * kMaxPerValue + 3) / 4;

__global__ __launch_bounds__(64 * kWaves) void json_g9_kernel(TextArgs a) {
  __shared__ uint32_t limbs_all[kWaves * kG9Limbs * 64];
  __shared__ uint32_t stage_all[kWaves * kStageWords];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int column = (int)blockIdx.x * kWaves + wave;
  if (column >= a.n_columns) return;
  const G9Limbs limbs{limbs_all + wave * (kG9Limbs * 64) + lane, 64};
  uint32_t* stage_words = stage_all + wave * kStageWords;
  char* stage = reinterpret_cast<char*>(stage_words);
  const TextColumn c = a.columns[column];
  const int n = __builtin_amdgcn_readfirstlane(c.count), inner = __builtin_amdgcn_readfirstlane(c.inner);
  const double* values = a.values + c.first;
  char* out = a.text + c.slot;
  int pos = 0;   // characters of the column written so far

  for (int base = 0; base < n; base += 64) {
    const int j = base + lane;
    const bool inside = j < n;
    G9 g{};
    int before = 0, behind = 0, len = 0;
    bool opens_column = false, opens_row = false;
    if (inside) {
      g = g9_digits(values[j], limbs);
      const int at = inner > 0 ? j % inner : -1;
      opens_column = j == 0;
      opens_row = at == 0;
      before = opens_row ? 2 : 1;                                // "[[" or ",[" in front of a row, else "[" or ","
      behind = (inner > 0 && at == inner - 1 ? 1 : 0) + (j == n - 1 ? 1 : 0);
      len = before + g9_length(g) + behind;
    }
    const int incl = wave_scan_incl(len);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    // the stage's byte 0 is the first byte of the aligned word that holds the stride's first character
    const int skew = (int)((uintptr_t)(out + pos) & 3u);
    if (inside) {
      char* s = stage + skew + (incl - len);
      *s++ = opens_column ? '[' : ',';
      if (opens_row) *s++ = '[';
      s += g9_write(g, s);
      for (int k = 0; k < 2; ++k)
        if (k < behind) *s++ = ']';
    }
    wave_lds_fence();
    char* dst = out + pos - skew;   // aligned
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
    wave_lds_fence();   // the next stride writes the stage again
    pos += total;
  }
  if (lane == 0) {
    if (n <= 0) {   // SToJSON of an empty list
      out[0] = '[';
      out[1] = ']';
      pos = 2;
    }
    a.begin[column] = c.slot;
    a.length[column] = pos;
  }
}

}  // namespace

hipError_t launch_json_g9(const TextArgs& a, hipStream_t stream) {
  if (a.n_columns <= 0) return hipSuccess;
  const int blocks = (a.n_columns + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(json_g9_kernel, dim3(blocks), dim3(64 * kWaves), 0, stream, a);
  return hipGetLastError();
}

}  // namespace afx
