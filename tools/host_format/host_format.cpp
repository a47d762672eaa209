// tools/host_format/host_format.cpp -- what a host thread pays for the text of the high-level vector columns when the
// doubles come down instead (tools/high_level_text_cost.py): SToJSON's layout around snprintf("%.9g"), the
// reference's own call, or around std::to_chars(general, 9), the fastest standard one.  A measurement aid, not the product.
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace {

template <bool kToChars>
char* number(char* p, double v) {
  if (std::isnan(v)) return (char*)std::memcpy(p, "NaN", 3) + 3;
  if (std::isinf(v)) {
    const int n = v < 0 ? 4 : 3;
    return (char*)std::memcpy(p, v < 0 ? "-INF" : "INF", (size_t)n) + n;
  }
  if (kToChars) return std::to_chars(p, p + 32, v, std::chars_format::general, 9).ptr;
  return p + std::snprintf(p, 32, "%.9g", v);
}

template <bool kToChars>
char* column(char* p, const double* v, int64_t count, int inner) {
  *p++ = '[';
  for (int64_t j = 0; j < count; ++j) {
    if (j > 0) *p++ = ',';
    if (inner > 0 && j % inner == 0) *p++ = '[';
    p = number<kToChars>(p, v[j]);
    if (inner > 0 && j % inner == inner - 1) *p++ = ']';
  }
  *p++ = ']';
  return p;
}

template <bool kToChars>
int64_t all(const double* signature, const double* pitch, const double* peak, const int64_t* frame_offset, int32_t n, char* out) {
  char* p = out;
  for (int32_t i = 0; i < n; ++i) {
    const int64_t row0 = frame_offset[i], frames = frame_offset[i + 1] - row0;
    p = column<kToChars>(p, signature + (int64_t)i * 896, 896, 14);
    p = column<kToChars>(p, pitch + row0, frames, 0);
    p = column<kToChars>(p, peak + row0, frames, 0);
  }
  return p - out;
}

}  // namespace

// the three columns of n files behind one another at `out` (room for 33 bytes a value); returns the bytes of text
extern "C" int64_t host_format_columns(const double* signature, const double* pitch, const double* peak, const int64_t* frame_offset, int32_t n,
                                       int32_t to_chars, char* out) {
  return to_chars ? all<true>(signature, pitch, peak, frame_offset, n, out) : all<false>(signature, pitch, peak, frame_offset, n, out);
}
