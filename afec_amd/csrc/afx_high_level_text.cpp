// afec_amd/csrc/afx_high_level_text.cpp -- the high-level vector columns as the text the reference's database stores (SToJSON,
// SqliteSampleDescriptorPool.cpp:316-419; every number as ToString(double, "%.9g"), Str.cpp:4027-4070).
// afx_batch_fetch_high_level_text shares the high-level fetch's launch (launch_high_level_block, afx_high_level.cpp): the same
// kernel into the same block, the text kernel (text/afx_text.hip) behind it on the same stream over that block's signature,
// pitch and peak, which stay on the device; the scalars, the text and its index come back.  afx_format_json_g9 runs the text
// kernel on doubles the caller holds, in a device block of its own.  The host decides only where a column's text may lie:
// a slot per column, sized for the longest text its values can have, so that no wave waits for another one's length.
// This is the only translation unit that names launch_json_g9: the mock builds that list their host files by name
// (tests/sanitize/build.sh) link without it.

#include <cstring>
#include <vector>

#include "afx_text_columns.h"

using namespace afx::host;

namespace {

constexpr int64_t kMaxColumnValues = 100000000;   // a column's text length is an int32: 17 bytes a value and 2 a row have to fit

// What json_g9_kernel reads besides the values and what it writes: the columns' table on its way up, then the index and the
// text, which come back in one piece.
struct TextBlock {
  size_t n_columns, columns, begin, length, text, end;
  TextBlock(Layout& l, size_t columns_, size_t capacity) : n_columns(columns_) {
    static_assert(sizeof(afx::TextColumn) == 24 && alignof(afx::TextColumn) == 8, "the table is an array in a block");
    columns = l.take<afx::TextColumn>(n_columns);
    begin = l.take<int64_t>(n_columns);
    length = l.take<int32_t>(n_columns);
    text = l.take<char>(capacity);
    end = l.bytes();
  }
  void point(afx::TextArgs* a, char* base, const double* values) const {
    a->values = values;
    a->columns = at<afx::TextColumn>(base, columns);
    a->n_columns = (int32_t)n_columns;
    a->text = base + text;
    a->begin = at<int64_t>(base, begin);
    a->length = at<int32_t>(base, length);
  }
  // the index, and of every slot the part that is text
  void hand_out(const char* host, char* out_text, int64_t* out_begin, int32_t* out_length) const {
    const int64_t* const b = at<int64_t>(host, begin);
    const int32_t* const n = at<int32_t>(host, length);
    std::memcpy(out_begin, b, n_columns * sizeof(int64_t));
    std::memcpy(out_length, n, n_columns * sizeof(int32_t));
    for (size_t c = 0; c < n_columns; ++c) std::memcpy(out_text + b[c], host + text + b[c], (size_t)n[c]);
  }
};

}  // namespace

extern "C" {

int64_t afx_batch_high_level_text_capacity(const afx_batch* b) {
  if (!b) return -1;
  return high_level_columns(b, nullptr);
}

int afx_batch_fetch_high_level_text(afx_batch* b, const afx_load_info* levels, afx_high_text_out* out) {
  if (!b || !out) return fail(AFX_ERR_INVALID_ARG, "null argument");
  const int64_t capacity = high_level_columns(b, nullptr);
  if (out->text_capacity < capacity) return fail(AFX_ERR_INVALID_ARG, "text_capacity is below afx_batch_high_level_text_capacity");
  if (b->n_bufs > 0 && (!out->text || !out->begin || !out->length)) return fail(AFX_ERR_INVALID_ARG, "null argument");
  Layout layout;
  const HighBlock hb(layout, (size_t)b->n_bufs, (size_t)b->total_frames);
  const TextBlock tb(layout, (size_t)b->n_bufs * AFX_NUM_HLT_COLUMNS, (size_t)capacity);
  ResultBlock rb;
  const int st = launch_high_level_block(b, "afx_batch_fetch_high_level_text", levels, layout, hb, &rb);
  if (st != AFX_OK || rb.n == 0) return st;

  // the columns' values are the block's own arrays
  afx::TextColumn* const table = at<afx::TextColumn>(rb.host, tb.columns);
  high_level_columns(b, table);
  count_from_signature(table, rb.n, hb);
  HIP_TRY(hipMemcpyAsync(rb.dev + tb.columns, table, tb.begin - tb.columns, hipMemcpyHostToDevice, b->stream));
  afx::TextArgs t{};
  tb.point(&t, rb.dev, at<double>(rb.dev, hb.signature));
  HIP_TRY(afx::launch_json_g9(t, b->stream));
  const Download items[2] = {{rb.host + hb.scalars, rb.dev + hb.scalars, hb.signature - hb.scalars},
                             {rb.host + tb.begin, rb.dev + tb.begin, tb.end - tb.begin}};
  HIP_TRY(download_through_plan(b, items, 2));
  if (out->scalars) std::memcpy(out->scalars, rb.host + hb.scalars, rb.n * afx::kHighScalars * sizeof(double));
  tb.hand_out(rb.host, out->text, out->begin, out->length);
  if (out->status) std::memcpy(out->status, b->buf_status.data(), rb.n * sizeof(int32_t));
  return AFX_OK;
}

int afx_format_json_g9(const afx_plan* plan, const double* values, int64_t n_values, const int64_t* column_offset, const int32_t* inner,
                       int32_t n_columns, char* text, int64_t text_capacity, int64_t* begin, int32_t* length) {
  if (!plan || n_values < 0 || n_columns < 0 || text_capacity < 0) return fail(AFX_ERR_INVALID_ARG, "bad argument");
  if (n_columns == 0) return n_values == 0 ? AFX_OK : fail(AFX_ERR_INVALID_ARG, "values without a column");
  if (!column_offset || !inner || !text || !begin || !length || (n_values > 0 && !values)) return fail(AFX_ERR_INVALID_ARG, "null argument");
  // the kernel follows the table into the values and the text: every column inside the values, every slot inside the text
  if (column_offset[0] != 0) return fail(AFX_ERR_INVALID_ARG, "column_offset[0] is not 0");
  const size_t n = (size_t)n_columns;
  std::vector<afx::TextColumn> table(n);
  int64_t capacity = 0;
  for (size_t c = 0; c < n; ++c) {
    const int64_t count = column_offset[c + 1] - column_offset[c];
    if (count < 0) return fail(AFX_ERR_INVALID_ARG, "column_offset steps back");
    if (column_offset[c + 1] > n_values) return fail(AFX_ERR_INVALID_ARG, "column_offset leaves the values");
    if (count > kMaxColumnValues) return fail(AFX_ERR_INVALID_ARG, "a column of more than 100 000 000 values");
    if (inner[c] < 0 || (inner[c] > 0 && count % inner[c] != 0)) return fail(AFX_ERR_INVALID_ARG, "inner does not divide its column");
    table[c] = afx::TextColumn{column_offset[c], capacity, (int32_t)count, inner[c]};
    capacity += afx::text_slot_bytes(count, inner[c]);
  }
  if (column_offset[n] != n_values) return fail(AFX_ERR_INVALID_ARG, "column_offset does not end at n_values");
  if (text_capacity < capacity) return fail(AFX_ERR_INVALID_ARG, "text_capacity is below the sum of 2 + 17 values + 2 rows over the columns");
  HIP_TRY(hipSetDevice(plan->desc.device));
  // one block of its own (this is not the crawl's path: no batch, no workspace): the values, which go up from the caller's
  // own array, then the text block
  Layout layout;
  const size_t doubles = layout.take<double>((size_t)n_values);
  const TextBlock tb(layout, n, (size_t)capacity);
  DeviceBlock dev;
  AFX_TRY(dev.allocate(layout.bytes(), "device memory for the values and their text"));
  if (n_values > 0) HIP_TRY(hipMemcpy(dev.get() + doubles, values, (size_t)n_values * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dev.get() + tb.columns, table.data(), n * sizeof(afx::TextColumn), hipMemcpyHostToDevice));
  afx::TextArgs t{};
  tb.point(&t, dev.get(), at<double>(dev.get(), doubles));
  HIP_TRY(afx::launch_json_g9(t, nullptr));
  std::vector<char> host(tb.end);
  HIP_TRY(hipMemcpy(host.data() + tb.begin, dev.get() + tb.begin, tb.end - tb.begin, hipMemcpyDeviceToHost));   // waits for the kernel
  tb.hand_out(host.data(), text, begin, length);
  return AFX_OK;
}

}  // extern "C"
