// tests/sanitize/text_main.cpp -- afec_amd/csrc/afx_high_level_text.cpp (afx_batch_fetch_high_level_text,
// afx_batch_high_level_text_capacity, afx_format_json_g9) as a stand-alone program on the mock device of
// tests/sanitize/hipstub, for -fsanitize=address,undefined (tools/sanitize_text.sh builds and runs it;
// tests/test_text_format_cpu.py runs it without a sanitizer).  The kernels are tests/sanitize/mock_kernels.cpp and, for the
// text, the mock launch_json_g9 below: it checks what the entry points hand the kernel -- every column inside the values,
// every slot inside the text and apart from the others, aligned arrays -- and formats for real, a column after the other,
// with the device's own header text/afx_g9.h.  The driver holds every result against its own serial formatting:
//   * batches of 0 to 5 buffers (none, one, three and 65 frames, a refused one) through both high-level fetches on the one
//     reused result block, with and without levels, optional outputs NULL, exactly-sized arrays
//   * afx_format_json_g9 on columns of 0 .. 130 values, flat and in rows, and every argument it refuses
//   * a capacity one byte short (nothing written), an allocation failure.   TEST INFRASTRUCTURE.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../afec_amd/csrc/text/afx_g9.h"
#include "../../afec_amd/csrc/text/afx_text.h"
#include "../../include/afx.h"

#define REQUIRE(cond)                                                          \
  do {                                                                         \
    if (!(cond)) {                                                             \
      std::fprintf(stderr, "%s:%d: REQUIRE(%s)\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                            \
    }                                                                          \
  } while (0)

namespace {

// SToJSON (SqliteSampleDescriptorPool.cpp:316-419) with text/afx_g9.h for the numbers, one value after the other
std::string serial_json(const double* v, int64_t count, int32_t inner) {
  std::string s = "[";
  char number[afx::kG9MaxChars];
  for (int64_t j = 0; j < count; ++j) {
    if (j > 0) s += ',';
    if (inner > 0 && j % inner == 0) s += '[';
    s.append(number, (size_t)afx::g9_format(v[j], number));
    if (inner > 0 && j % inner == inner - 1) s += ']';
  }
  return s + "]";
}

long long g_columns = 0, g_bytes = 0;

}  // namespace

namespace afx {

hipError_t launch_json_g9(const TextArgs& a, hipStream_t) {
  if (a.n_columns <= 0) return hipSuccess;
  REQUIRE(a.columns && a.text && a.begin && a.length);
  REQUIRE((uintptr_t)a.columns % alignof(TextColumn) == 0 && (uintptr_t)a.begin % 8 == 0 && (uintptr_t)a.length % 4 == 0 && (uintptr_t)a.text % 4 == 0);
  REQUIRE((uintptr_t)a.values % 8 == 0);
  int64_t slots_end = 0;
  for (int32_t c = 0; c < a.n_columns; ++c) {
    const TextColumn& col = a.columns[c];
    REQUIRE(col.count >= 0 && col.inner >= 0 && col.first >= 0 && (col.inner == 0 || col.count % col.inner == 0));
    REQUIRE(col.count == 0 || a.values != nullptr);
    REQUIRE(col.slot == slots_end);   // the entry points place slot behind slot
    slots_end += text_slot_bytes(col.count, col.inner);
    const std::string s = serial_json(a.values + col.first, col.count, col.inner);   // reads every value: the sanitizer's bound check
    REQUIRE((int64_t)s.size() <= text_slot_bytes(col.count, col.inner));
    std::memcpy(a.text + col.slot, s.data(), s.size());
    a.begin[c] = col.slot;
    a.length[c] = (int32_t)s.size();
  }
  // the arrays the kernel writes lie apart from what it reads
  const char* const written[3][2] = {{(const char*)a.begin, (const char*)(a.begin + a.n_columns)},
                                     {(const char*)a.length, (const char*)(a.length + a.n_columns)},
                                     {a.text, a.text + slots_end}};
  const char* const table[2] = {(const char*)a.columns, (const char*)(a.columns + a.n_columns)};
  for (int i = 0; i < 3; ++i) {
    REQUIRE(written[i][1] <= table[0] || table[1] <= written[i][0]);
    for (int j = i + 1; j < 3; ++j) REQUIRE(written[i][1] <= written[j][0] || written[j][1] <= written[i][0]);
  }
  return hipSuccess;
}

}  // namespace afx

namespace {

void known_answers() {
  const struct { double v; const char* text; } known[] = {
      {100000000.5, "100000000"}, {100000001.5, "100000002"}, {12345678.25, "12345678.2"}, {12345678.75, "12345678.8"},
      {1000000005.0, "1e+09"}, {1000000015.0, "1.00000002e+09"}, {999999999.5, "1e+09"}, {99999999.95, "100000000"},
      {9.9999999995e-05, "0.0001"}, {1e-05, "1e-05"}, {123456789.0, "123456789"}, {1234567890.0, "1.23456789e+09"},
      {4.9406564584124654e-324, "4.94065646e-324"}, {1.7976931348623157e308, "1.79769313e+308"}, {-0.0, "-0"}, {0.1, "0.1"},
      {std::nan(""), "NaN"}, {INFINITY, "INF"}, {-INFINITY, "-INF"}};
  for (const auto& k : known) {
    char number[afx::kG9MaxChars];
    const int n = afx::g9_format(k.v, number);
    REQUIRE(std::string(number, (size_t)n) == k.text);
  }
}

// adversarial and plain values, the same on every run
std::vector<double> some_values(size_t n, unsigned seed) {
  const double special[] = {0.0, -0.0, 1.0, 0.1, 100000000.5, 999999999.5, 1e-5, 9.9999999995e-05, 1e22, 1e-300, 1.7976931348623157e308,
                            4.9406564584124654e-324, std::nan(""), INFINITY, -INFINITY, 1e-18, 1e27, 123456789.0, -1234567890.0};
  std::vector<double> v(n);
  unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
  for (size_t i = 0; i < n; ++i) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    if (i % 3 == 0) v[i] = special[(i / 3 + seed) % (sizeof special / sizeof special[0])];
    else if (i % 3 == 1) v[i] = (double)(long long)(s % 2000001) / 1000.0 - 1000.0;
    else std::memcpy(&v[i], &s, 8);   // any bit pattern
  }
  return v;
}

void format_entry(afx_plan* plan) {
  const int32_t counts[] = {0, 1, 63, 64, 65, 129, 0, 28, 130};
  const int32_t inners[] = {0, 0, 0, 1, 0, 0, 14, 14, 13};
  const int32_t n_columns = (int32_t)(sizeof counts / sizeof counts[0]);
  std::vector<int64_t> offset(1, 0);
  int64_t capacity = 0;
  for (int32_t c = 0; c < n_columns; ++c) {
    offset.push_back(offset.back() + counts[c]);
    capacity += afx::text_slot_bytes(counts[c], inners[c]);
  }
  const std::vector<double> values = some_values((size_t)offset.back(), 7);
  // exactly sized heap arrays: a write past the end is the sanitizer's
  std::vector<char> text((size_t)capacity);
  std::vector<int64_t> begin((size_t)n_columns);
  std::vector<int32_t> length((size_t)n_columns);
  REQUIRE(afx_format_json_g9(plan, values.data(), (int64_t)values.size(), offset.data(), inners, n_columns, text.data(), capacity, begin.data(),
                             length.data()) == AFX_OK);
  int64_t last_end = 0;
  for (int32_t c = 0; c < n_columns; ++c) {
    const std::string want = serial_json(values.data() + offset[(size_t)c], counts[c], inners[c]);
    REQUIRE(begin[(size_t)c] >= last_end && begin[(size_t)c] + length[(size_t)c] <= capacity);
    REQUIRE(std::string(text.data() + begin[(size_t)c], (size_t)length[(size_t)c]) == want);
    last_end = begin[(size_t)c] + length[(size_t)c];
    ++g_columns;
    g_bytes += length[(size_t)c];
  }
  REQUIRE(std::string(text.data() + begin[0], (size_t)length[0]) == "[]" && std::string(text.data() + begin[6], (size_t)length[6]) == "[]");

  // what it refuses, before anything follows the offsets; nothing is written
  std::vector<char> untouched((size_t)capacity, '#');
  auto refused = [&](const int64_t* off, const int32_t* in, int64_t n_values, int64_t cap, const char* why) {
    REQUIRE(afx_format_json_g9(plan, values.data(), n_values, off, in, n_columns, untouched.data(), cap, begin.data(), length.data()) == AFX_ERR_INVALID_ARG);
    REQUIRE(std::strcmp(afx_last_error(), why) == 0);
    for (char ch : untouched) REQUIRE(ch == '#');
  };
  const int64_t n_values = (int64_t)values.size();
  refused(offset.data(), inners, n_values, capacity - 1, "text_capacity is below the sum of 2 + 17 values + 2 rows over the columns");
  std::vector<int64_t> bad = offset;
  bad[0] = 1;
  refused(bad.data(), inners, n_values, capacity, "column_offset[0] is not 0");
  bad = offset;
  bad[3] = bad[2] - 1;
  refused(bad.data(), inners, n_values, capacity, "column_offset steps back");
  bad = offset;
  bad.back() += 1;
  refused(bad.data(), inners, n_values, capacity + 17, "column_offset leaves the values");
  refused(offset.data(), inners, n_values + 1, capacity, "column_offset does not end at n_values");
  std::vector<int32_t> bad_inner(inners, inners + n_columns);
  bad_inner[8] = 14;   // 130 values in rows of 14
  refused(offset.data(), bad_inner.data(), n_values, capacity + 64, "inner does not divide its column");
  bad_inner[8] = -1;
  refused(offset.data(), bad_inner.data(), n_values, capacity + 64, "inner does not divide its column");
  REQUIRE(afx_format_json_g9(nullptr, values.data(), n_values, offset.data(), inners, n_columns, text.data(), capacity, begin.data(), length.data()) == AFX_ERR_INVALID_ARG);
  REQUIRE(afx_format_json_g9(plan, values.data(), n_values, offset.data(), inners, n_columns, nullptr, capacity, begin.data(), length.data()) == AFX_ERR_INVALID_ARG);
  REQUIRE(afx_format_json_g9(plan, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr) == AFX_OK);   // no column: nothing to do

  // the device has no memory left for the call's block
  hipstub::fail_allocation_after(0);
  REQUIRE(afx_format_json_g9(plan, values.data(), n_values, offset.data(), inners, n_columns, untouched.data(), capacity, begin.data(), length.data()) ==
          AFX_ERR_OUT_OF_MEMORY);
  REQUIRE(std::strcmp(afx_last_error(), "device memory for the values and their text") == 0);
  hipstub::fail_allocation_after(-1);
  for (char ch : untouched) REQUIRE(ch == '#');
  REQUIRE(afx_format_json_g9(plan, values.data(), n_values, offset.data(), inners, n_columns, text.data(), capacity, begin.data(), length.data()) == AFX_OK);
}

void batch_entry(afx_plan* plan, int n_bufs, unsigned seed) {
  // no samples, one frame, three frames, 65 frames, a refused buffer; rotated by the seed
  const int64_t samples_of[5] = {0, 2048, 2048 + 2 * 1024, 2048 + 64 * 1024, 4096}, frames_of[5] = {0, 1, 3, 65, 0};
  std::vector<std::vector<float>> pcm((size_t)n_bufs);
  std::vector<afx_buf> bufs((size_t)n_bufs);
  for (int i = 0; i < n_bufs; ++i) {
    const int kind = (i + (int)seed) % 5;
    pcm[(size_t)i].assign((size_t)samples_of[kind], 0.25f);
    bufs[(size_t)i] = afx_buf{pcm[(size_t)i].data(), AFX_PCM_F32, 0, kind == 4 ? -5 : samples_of[kind]};
  }
  const uint32_t mask = AFX_D_HIGH_LEVEL_INPUTS;
  afx_batch* b = nullptr;
  REQUIRE(afx_batch_create(plan, n_bufs ? bufs.data() : nullptr, n_bufs, mask, &b) == AFX_OK);
  const size_t n = (size_t)n_bufs, F = (size_t)afx_batch_total_frames(b);
  const int64_t capacity = afx_batch_high_level_text_capacity(b);
  REQUIRE(capacity == (int64_t)n * (2 + 17 * 896 + 2 * 64) + 2 * (2 * (int64_t)n + 17 * (int64_t)F));
  std::vector<char> text((size_t)capacity);
  std::vector<int64_t> begin(n * AFX_NUM_HLT_COLUMNS);
  std::vector<int32_t> length(n * AFX_NUM_HLT_COLUMNS), status(n);
  std::vector<double> scalars(n * AFX_NUM_HL_SCALARS);
  afx_high_text_out out{scalars.data(), text.data(), capacity, begin.data(), length.data(), status.data()};
  REQUIRE(afx_batch_fetch_high_level_text(b, nullptr, &out) == AFX_ERR_INVALID_ARG);
  REQUIRE(std::strcmp(afx_last_error(), "afx_batch_fetch_high_level_text before afx_batch_run") == 0);
  REQUIRE(afx_batch_run(b) == AFX_OK);

  std::vector<afx_load_info> levels(n);
  for (size_t i = 0; i < n; ++i) {
    levels[i] = afx_load_info{};
    levels[i].peak_value = 0.5f + (float)i;
    levels[i].rms_value = 0.25f + (float)i;
  }
  // the arrays the text is, by definition, the text of
  std::vector<double> want_scalars(n * AFX_NUM_HL_SCALARS), signature(n * 896), pitch(F), peak(F);
  std::vector<int32_t> want_status(n);
  afx_high_out high{want_scalars.data(), signature.data(), pitch.data(), peak.data(), want_status.data()};

  for (int round = 0; round < 4; ++round) {
    const bool with_levels = round % 2 == 1;
    REQUIRE(afx_batch_fetch_high_level(b, with_levels ? levels.data() : nullptr, &high) == AFX_OK);
    std::fill(text.begin(), text.end(), '#');
    out.scalars = round == 2 ? nullptr : scalars.data();
    out.status = round == 3 ? nullptr : status.data();
    REQUIRE(afx_batch_fetch_high_level_text(b, with_levels ? levels.data() : nullptr, &out) == AFX_OK);
    if (out.scalars) REQUIRE(n == 0 || std::memcmp(scalars.data(), want_scalars.data(), scalars.size() * sizeof(double)) == 0);
    if (out.status) REQUIRE(status == want_status);
    int64_t last_end = 0, row0 = 0;
    std::vector<char> is_text((size_t)capacity, 0);
    for (size_t i = 0; i < n; ++i) {
      const int64_t frames = frames_of[(i + seed) % 5];
      const std::string want[AFX_NUM_HLT_COLUMNS] = {serial_json(signature.data() + i * 896, 896, 14), serial_json(pitch.data() + row0, frames, 0),
                                                     serial_json(peak.data() + row0, frames, 0)};
      for (int c = 0; c < AFX_NUM_HLT_COLUMNS; ++c) {
        const int64_t at = begin[i * AFX_NUM_HLT_COLUMNS + (size_t)c];
        const int32_t len = length[i * AFX_NUM_HLT_COLUMNS + (size_t)c];
        REQUIRE(at >= last_end && at + len <= capacity);
        REQUIRE(std::string(text.data() + at, (size_t)len) == want[c]);
        std::fill(is_text.begin() + at, is_text.begin() + at + len, 1);
        last_end = at + len;
        ++g_columns;
        g_bytes += len;
      }
      if (frames == 0) REQUIRE(want[1] == "[]" && want[2] == "[]");
      row0 += frames;
    }
    REQUIRE(row0 == (int64_t)F);
    for (size_t k = 0; k < text.size(); ++k) REQUIRE(is_text[k] || text[k] == '#');   // only text is handed out
  }

  // a capacity one byte short: refused, nothing written; an allocation failure cannot happen here once the block is reserved
  if (capacity > 0) {
    std::fill(text.begin(), text.end(), '#');
    std::vector<int64_t> begin_before = begin;
    out.scalars = scalars.data();
    out.status = status.data();
    out.text_capacity = capacity - 1;
    REQUIRE(afx_batch_fetch_high_level_text(b, nullptr, &out) == AFX_ERR_INVALID_ARG);
    REQUIRE(std::strcmp(afx_last_error(), "text_capacity is below afx_batch_high_level_text_capacity") == 0);
    for (char ch : text) REQUIRE(ch == '#');
    REQUIRE(begin == begin_before);
    out.text_capacity = capacity;
  }
  afx_batch_destroy(b);

  // a fresh batch, whose workspace may have to grow for the text: the device refuses the memory, then gives it
  REQUIRE(afx_batch_create(plan, n_bufs ? bufs.data() : nullptr, n_bufs, mask, &b) == AFX_OK);
  REQUIRE(afx_batch_run(b) == AFX_OK);
  hipstub::fail_allocation_after(0);
  const int st = afx_batch_fetch_high_level_text(b, nullptr, &out);
  hipstub::fail_allocation_after(-1);
  REQUIRE(st == AFX_OK || st == AFX_ERR_OUT_OF_MEMORY || st == AFX_ERR_HIP);
  REQUIRE(afx_batch_fetch_high_level_text(b, nullptr, &out) == AFX_OK);
  afx_batch_destroy(b);

  // a batch whose mask lacks an input
  REQUIRE(afx_batch_create(plan, n_bufs ? bufs.data() : nullptr, n_bufs, AFX_D_MFCC, &b) == AFX_OK);
  REQUIRE(afx_batch_run(b) == AFX_OK);
  REQUIRE(afx_batch_fetch_high_level_text(b, nullptr, &out) == AFX_ERR_INVALID_ARG);
  REQUIRE(std::strcmp(afx_last_error(), "the batch mask lacks a series the high-level descriptors read (AFX_D_HIGH_LEVEL_INPUTS)") == 0);
  afx_batch_destroy(b);
}

}  // namespace

int main() {
  known_answers();
  afx_plan_desc desc = {44100, 2048, 1024, 0, AFX_PRECISION_F64, 20000, AFX_FRAME_KERNEL_AUTO, 0};
  afx_plan* plan = nullptr;
  REQUIRE(afx_plan_create(&desc, &plan) == AFX_OK);
  REQUIRE(afx_batch_high_level_text_capacity(nullptr) == -1);
  afx_high_text_out none{};
  REQUIRE(afx_batch_fetch_high_level_text(nullptr, nullptr, &none) == AFX_ERR_INVALID_ARG);
  format_entry(plan);
  unsigned seed = 0;
  for (int n_bufs : {0, 1, 2, 3, 4, 5, 5, 5})
    batch_entry(plan, n_bufs, seed++);
  afx_plan_destroy(plan);
  std::printf("text_main: %lld columns, %lld bytes of text, all equal to the serial formatting\n", g_columns, g_bytes);
  return 0;
}
