// tools/host_format/host_format.cpp -- what a host thread pays for the text of the high-level vector columns when the
// doubles come down instead (tools/high_level_text_cost.py), and for the six class columns when the class
// decision's arrays come down (tools/high_level_row_cost.py): SToJSON's layout around snprintf("%.9g"), the
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

// SToJSON of the names of the picked indices, up to the first -1
char* names(char* p, const int32_t* picks, int32_t count, const char* bytes, const int32_t* offset, const int32_t* length) {
  *p++ = '[';
  for (int32_t j = 0; j < count && picks[j] >= 0; ++j) {
    if (j > 0) *p++ = ',';
    *p++ = '"';
    std::memcpy(p, bytes + offset[picks[j]], (size_t)length[picks[j]]);
    p += length[picks[j]];
    *p++ = '"';
  }
  *p++ = ']';
  return p;
}

template <bool kToChars>
char* model(char* p, const float* signature, const double* strengths, const int32_t* picks, int32_t count, const char* bytes,
            const int32_t* offset, const int32_t* length) {
  double wide[64];
  for (int32_t j = 0; j < count; ++j) wide[j] = (double)signature[j];
  p = column<kToChars>(p, wide, count, 0);
  p = names(p, picks, count, bytes, offset, length);
  return column<kToChars>(p, strengths, count, 0);
}

}  // namespace

// the six class columns of n files behind one another at `out`: the class model's three (2 classes) and the category
// model's three (k <= 64 classes) from the arrays of a class decision; the names' bytes with an offset and a length per index,
// the two class names first.  Returns the bytes of text.
extern "C" int64_t host_format_class_columns(const float* class_signature, const double* class_strengths, const int32_t* classes,
                                             const float* category_signature, const double* category_strengths, const int32_t* categories,
                                             int32_t k, const char* name_bytes, const int32_t* name_offset, const int32_t* name_length, int32_t n,
                                             int32_t to_chars, char* out) {
  char* p = out;
  for (int64_t i = 0; i < n; ++i) {
    if (to_chars) {
      p = model<true>(p, class_signature + i * 2, class_strengths + i * 2, classes + i * 2, 2, name_bytes, name_offset, name_length);
      p = model<true>(p, category_signature + i * k, category_strengths + i * k, categories + i * k, k, name_bytes, name_offset + 2, name_length + 2);
    } else {
      p = model<false>(p, class_signature + i * 2, class_strengths + i * 2, classes + i * 2, 2, name_bytes, name_offset, name_length);
      p = model<false>(p, category_signature + i * k, category_strengths + i * k, categories + i * k, k, name_bytes, name_offset + 2, name_length + 2);
    }
  }
  return p - out;
}

// the three columns of n files behind one another at `out` (room for 33 bytes a value); returns the bytes of text
extern "C" int64_t host_format_columns(const double* signature, const double* pitch, const double* peak, const int64_t* frame_offset, int32_t n,
                                       int32_t to_chars, char* out) {
  return to_chars ? all<true>(signature, pitch, peak, frame_offset, n, out) : all<false>(signature, pitch, peak, frame_offset, n, out);
}
