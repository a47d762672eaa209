// afec_amd/csrc/afx_high_level_row.cpp -- the whole row of the reference's high-level database out of one fetch, in the
// form sqlite binds.  afx_batch_fetch_high_level_row is the high-level text fetch (afx_high_level_text.cpp) and the class
// decision fetch (afx_class_decision.cpp) in one: the checks of both, ONE reservation of the batch's result block for one
// layout that holds the blocks of both, their kernels on the batch's stream, the class columns' text kernel
// (text/afx_row_text.hip) and the vector columns' kernel behind them, one download of the scalars, the decision's small
// outputs and the text with its index.  The doubles, the features and the signatures stay on the device.
// afx_format_class_json runs the class columns' kernel on arrays the caller holds, in a device block of its own.
// The host decides only where a column's text may lie (text/afx_row_text.h) and refuses names the reference would turn
// into text no JSON reader accepts.  This is the only translation unit that names launch_row_text: the mock builds that
// list their host files by name (tests/sanitize/build.sh) link without it.

#include <cstring>
#include <vector>

#include "afx_decision_block.h"
#include "afx_text_columns.h"
#include "text/afx_row_text.h"

using namespace afx::host;

namespace {

// The names of both models as the kernel reads them: the bytes behind one another, an offset and a length per index, the
// class model's names first.
struct Names {
  std::vector<char> bytes;
  std::vector<int32_t> offset, length;
  int32_t count[2] = {0, 0}, slot[2] = {2, 2};   // per model: its names, names_slot_bytes of them

  // AFX_OK or why the fetch refuses them
  int read(int m, const afx_name* names, int32_t n) {
    if (n < 0 || n > afx::kRowTextMaxNames) return fail(AFX_ERR_INVALID_ARG, "more than 64 names for a model");
    if (n > 0 && !names) return fail(AFX_ERR_INVALID_ARG, "null argument");
    int64_t sum = 0;
    for (int32_t i = 0; i < n; ++i) {
      if (names[i].length < 0 || names[i].length > afx::kRowTextMaxNameBytes) return fail(AFX_ERR_INVALID_ARG, "a name longer than 255 bytes");
      if (names[i].length > 0 && !names[i].text) return fail(AFX_ERR_INVALID_ARG, "null argument");
      for (int32_t j = 0; j < names[i].length; ++j) {
        const unsigned char c = (unsigned char)names[i].text[j];
        if (c == '"' || c == '\\' || c < 0x20)
          return fail(AFX_ERR_INVALID_ARG, "a name holds '\"', '\\' or a control character: its list would be no JSON");
      }
      offset.push_back((int32_t)bytes.size());
      length.push_back(names[i].length);
      bytes.insert(bytes.end(), names[i].text, names[i].text + names[i].length);
      sum += names[i].length;
    }
    count[m] = n;
    slot[m] = (int32_t)afx::names_slot_bytes(sum, n);
    return AFX_OK;
  }
  int64_t file_bytes() const { return afx::row_text_file_bytes(count[0], slot[0], count[1], slot[1]); }
};

// What class_text_kernel reads besides the decision block, on its way up in one piece with the vector columns' table, then
// what the two text kernels write, which comes back in one piece.
struct RowTextBlock {
  size_t n, n_names, name_bytes, name_offset, name_length, file_slot, columns, up_end, class_begin, class_length, vector_begin,
      vector_length, text, end;
  RowTextBlock(Layout& l, size_t n_files, const Names& names, size_t n_vector_columns, size_t capacity) : n(n_files), n_names(names.offset.size()) {
    static_assert(sizeof(afx::TextColumn) == 24 && alignof(afx::TextColumn) == 8, "the table is an array in a block");
    name_bytes = l.take<char>(names.bytes.size());
    name_offset = l.take<int32_t>(n_names);
    name_length = l.take<int32_t>(n_names);
    file_slot = l.take<int64_t>(n);
    columns = l.take<afx::TextColumn>(n_vector_columns);
    up_end = l.bytes();
    class_begin = l.take<int64_t>(n * afx::kRowTextColumns);
    class_length = l.take<int32_t>(n * afx::kRowTextColumns);
    vector_begin = l.take<int64_t>(n_vector_columns);
    vector_length = l.take<int32_t>(n_vector_columns);
    text = l.take<char>(capacity);
    end = l.bytes();
  }
  // the names and every file's first slot, `stride` bytes apart
  void fill(char* host, const Names& names, int64_t stride) const {
    if (!names.bytes.empty()) std::memcpy(host + name_bytes, names.bytes.data(), names.bytes.size());
    if (n_names) {
      std::memcpy(host + name_offset, names.offset.data(), n_names * sizeof(int32_t));
      std::memcpy(host + name_length, names.length.data(), n_names * sizeof(int32_t));
    }
    for (size_t i = 0; i < n; ++i) at<int64_t>(host, file_slot)[i] = (int64_t)i * stride;
  }
  void point(afx::RowTextArgs* a, char* base, const Names& names) const {
    a->classes.count = names.count[0];
    a->classes.first_name = 0;
    a->classes.names_slot = names.slot[0];
    a->categories.count = names.count[1];
    a->categories.first_name = names.count[0];
    a->categories.names_slot = names.slot[1];
    a->n_files = (int32_t)n;
    a->name_bytes = base + name_bytes;
    a->name_offset = at<int32_t>(base, name_offset);
    a->name_length = at<int32_t>(base, name_length);
    a->file_slot = at<int64_t>(base, file_slot);
    a->text = base + text;
    a->begin = at<int64_t>(base, class_begin);
    a->length = at<int32_t>(base, class_length);
  }
  // the class columns' index, and of every slot the part that is text; `stride`: the columns of a file in the caller's index
  void hand_out_classes(const char* host, char* out_text, int64_t* out_begin, int32_t* out_length, size_t stride) const {
    const int64_t* const b = at<int64_t>(host, class_begin);
    const int32_t* const len = at<int32_t>(host, class_length);
    for (size_t i = 0; i < n; ++i)
      for (size_t c = 0; c < (size_t)afx::kRowTextColumns; ++c) {
        const size_t from = i * afx::kRowTextColumns + c, to = i * stride + c;
        out_begin[to] = b[from];
        out_length[to] = len[from];
        std::memcpy(out_text + b[from], host + text + b[from], (size_t)len[from]);
      }
  }
};

}  // namespace

extern "C" {

int64_t afx_batch_high_level_row_capacity(const afx_batch* b, const afx_row_desc* desc) {
  if (!b || !desc) return -1;
  Names names;
  if (names.read(0, desc->class_names, desc->n_class_names) != AFX_OK || names.read(1, desc->category_names, desc->n_category_names) != AFX_OK)
    return -1;
  return high_level_columns(b, nullptr, names.file_bytes());
}

int afx_batch_fetch_high_level_row(afx_batch* b, const afx_load_info* levels, const afx_row_desc* desc, afx_row_out* out) {
  if (!b || !desc || !out) return fail(AFX_ERR_INVALID_ARG, "null argument");
  const afx_model* const models[2] = {desc->decision.class_model, desc->decision.category_model};
  const bool decides = models[0] || models[1];
  size_t k = 0;
  if (decides) AFX_TRY(check_decision_desc(b, &desc->decision, &k));
  Names names;
  AFX_TRY(names.read(0, desc->class_names, desc->n_class_names));
  AFX_TRY(names.read(1, desc->category_names, desc->n_category_names));
  if (names.count[0] != (models[0] ? afx::kDecideClasses : 0) || names.count[1] != (int32_t)k)
    return fail(AFX_ERR_INVALID_ARG, "a name count is not its model's class count (0 without the model)");
  const int64_t capacity = high_level_columns(b, nullptr, names.file_bytes());
  if (out->text_capacity < capacity) return fail(AFX_ERR_INVALID_ARG, "text_capacity is below afx_batch_high_level_row_capacity");
  if (b->n_bufs > 0 && (!out->text || !out->begin || !out->length)) return fail(AFX_ERR_INVALID_ARG, "null argument");

  const size_t n = (size_t)b->n_bufs;
  Layout layout;
  const HighBlock hb(layout, n, (size_t)b->total_frames);
  const FeatureBlock fb(layout, decides ? n : 0);
  const DecisionScratch scratch(layout, decides ? n : 0, models);
  const DecisionBlock db(layout, decides ? n : 0, models[0] != nullptr, k);
  const RowTextBlock tb(layout, n, names, n * AFX_NUM_HLT_COLUMNS, (size_t)capacity);
  ResultBlock rb;
  if (decides && !has_feature_inputs(b)) return fail(AFX_ERR_INVALID_ARG, kLacksFeatureInputs);
  const int st = reserve_result_block(b, has_high_level_inputs(b), kLacksHighLevelInputs, "afx_batch_fetch_high_level_row", layout, &rb);
  if (st != AFX_OK || rb.n == 0) return st;

  // the features' launch waits for the batch's stream and reads the effective lengths on the host: first, while nothing
  // of this fetch is on the stream; from then on the host only enqueues
  if (decides) {
    AFX_TRY(enqueue_features(b, fb, rb));
    AFX_TRY(enqueue_class_decision(b, &desc->decision, fb, scratch, db, rb));
  }
  AFX_TRY(enqueue_high_level(b, levels, hb, rb));
  // the text: every file's six class slots, then its three vector slots, whose values are the high-level block's own arrays
  tb.fill(rb.host, names, 0);
  afx::TextColumn* const table = at<afx::TextColumn>(rb.host, tb.columns);
  high_level_columns(b, table, names.file_bytes());
  count_from_signature(table, n, hb);
  int64_t* const file_slot = at<int64_t>(rb.host, tb.file_slot);
  for (size_t i = 0; i < n; ++i) file_slot[i] = table[i * AFX_NUM_HLT_COLUMNS].slot - names.file_bytes();
  HIP_TRY(hipMemcpyAsync(rb.dev + tb.name_bytes, rb.host + tb.name_bytes, tb.up_end - tb.name_bytes, hipMemcpyHostToDevice, b->stream));
  afx::RowTextArgs a{};
  tb.point(&a, rb.dev, names);
  if (models[0]) a.classes = {at<float>(rb.dev, db.signature[0]), at<double>(rb.dev, db.class_strengths), at<int32_t>(rb.dev, db.classes),
                              a.classes.count, a.classes.first_name, a.classes.names_slot};
  if (models[1]) a.categories = {at<float>(rb.dev, db.signature[1]), at<double>(rb.dev, db.category_strengths), at<int32_t>(rb.dev, db.categories),
                                 a.categories.count, a.categories.first_name, a.categories.names_slot};
  afx::TextArgs t{};
  t.values = at<double>(rb.dev, hb.signature);
  t.columns = at<afx::TextColumn>(rb.dev, tb.columns);
  t.n_columns = (int32_t)(n * AFX_NUM_HLT_COLUMNS);
  t.text = rb.dev + tb.text;
  t.begin = at<int64_t>(rb.dev, tb.vector_begin);
  t.length = at<int32_t>(rb.dev, tb.vector_length);
  HIP_TRY(afx::launch_row_text(a, &t, b->stream));

  const Download items[4] = {{rb.host + hb.scalars, rb.dev + hb.scalars, hb.signature - hb.scalars},
                             {rb.host + db.confidences, rb.dev + db.confidences, decides ? db.category_strengths - db.confidences : 0},
                             {rb.host + db.flags, rb.dev + db.flags, decides ? db.end - db.flags : 0},
                             {rb.host + tb.class_begin, rb.dev + tb.class_begin, tb.end - tb.class_begin}};
  HIP_TRY(download_through_plan(b, items, 4));

  if (out->scalars) std::memcpy(out->scalars, rb.host + hb.scalars, n * afx::kHighScalars * sizeof(double));
  tb.hand_out_classes(rb.host, out->text, out->begin, out->length, AFX_NUM_HLR_COLUMNS);
  const int64_t* const vb = at<int64_t>(rb.host, tb.vector_begin);
  const int32_t* const vl = at<int32_t>(rb.host, tb.vector_length);
  for (size_t i = 0; i < n; ++i)
    for (size_t c = 0; c < AFX_NUM_HLT_COLUMNS; ++c) {
      const size_t from = i * AFX_NUM_HLT_COLUMNS + c, to = i * AFX_NUM_HLR_COLUMNS + AFX_HLR_SPECTRUM_SIGNATURE + c;
      out->begin[to] = vb[from];
      out->length[to] = vl[from];
      std::memcpy(out->text + vb[from], rb.host + tb.text + vb[from], (size_t)vl[from]);
    }
  if (decides) {
    if (out->confidences) std::memcpy(out->confidences, rb.host + db.confidences, n * 2 * sizeof(double));
    if (out->flags) std::memcpy(out->flags, rb.host + db.flags, n * sizeof(int32_t));
    if (out->non_finite) std::memcpy(out->non_finite, rb.host + db.non_finite, n * sizeof(int32_t));
  } else {   // the reference's two `none`s: nothing was evaluated
    for (size_t i = 0; i < n; ++i) {
      if (out->confidences) out->confidences[2 * i] = out->confidences[2 * i + 1] = -1.0;
      if (out->flags) out->flags[i] = 0;
      if (out->non_finite) out->non_finite[i] = 0;
    }
  }
  if (out->status) std::memcpy(out->status, b->buf_status.data(), n * sizeof(int32_t));
  return AFX_OK;
}

int afx_format_class_json(const afx_plan* plan, const afx_class_json_in* in, char* text, int64_t capacity, int64_t* begin, int32_t* length) {
  if (!plan || !in || in->n_files < 0 || capacity < 0) return fail(AFX_ERR_INVALID_ARG, "bad argument");
  const bool with_classes = in->class_signature || in->class_strengths || in->classes;
  const bool with_categories = in->category_signature || in->category_strengths || in->categories;
  if (with_classes && !(in->class_signature && in->class_strengths && in->classes))
    return fail(AFX_ERR_INVALID_ARG, "the three class arrays are all given or all NULL");
  if (with_categories && !(in->category_signature && in->category_strengths && in->categories))
    return fail(AFX_ERR_INVALID_ARG, "the three category arrays are all given or all NULL");
  if (with_categories && (in->n_categories < 2 || in->n_categories > afx::kDecideMaxCategories))
    return fail(AFX_ERR_INVALID_ARG, "n_categories outside 2..64");
  const size_t n = (size_t)in->n_files, k = with_categories ? (size_t)in->n_categories : 0, counts[2] = {with_classes ? (size_t)2 : 0, k};
  Names names;
  AFX_TRY(names.read(0, in->class_names, (int32_t)counts[0]));
  AFX_TRY(names.read(1, in->category_names, (int32_t)k));
  // the kernel follows a pick into the names, and a slot holds every name once
  const int32_t* const picks[2] = {in->classes, in->categories};
  for (int m = 0; m < 2; ++m)
    for (size_t i = 0; i < n && counts[m]; ++i) {
      uint64_t seen = 0;
      bool ended = false;
      for (size_t j = 0; j < counts[m]; ++j) {
        const int32_t p = picks[m][i * counts[m] + j];
        if (p < -1 || p >= (int32_t)counts[m]) return fail(AFX_ERR_INVALID_ARG, "a pick names no class of its model");
        if (p < 0) ended = true;
        if (p < 0 || ended) continue;
        if (seen >> p & 1) return fail(AFX_ERR_INVALID_ARG, "a class picked twice in one list");
        seen |= (uint64_t)1 << p;
      }
    }
  const int64_t stride = names.file_bytes();
  if (capacity < (int64_t)n * stride) return fail(AFX_ERR_INVALID_ARG, "capacity is below n_files x the bytes of one file's six slots");
  if (n == 0) return AFX_OK;
  if (!text || !begin || !length) return fail(AFX_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(plan->desc.device));
  // one block of its own (this is not the crawl's path: no batch, no workspace): what goes up -- the six arrays, the names
  // and the slots -- then what the kernel writes
  Layout layout;
  const size_t signature[2] = {layout.take<float>(n * counts[0]), layout.take<float>(n * k)};
  const size_t strengths[2] = {layout.take<double>(n * counts[0]), layout.take<double>(n * k)};
  const size_t picked[2] = {layout.take<int32_t>(n * counts[0]), layout.take<int32_t>(n * k)};
  const RowTextBlock tb(layout, n, names, 0, (size_t)((int64_t)n * stride));
  std::vector<char> host(tb.end, 0);
  if (with_classes) {
    std::memcpy(host.data() + signature[0], in->class_signature, n * 2 * sizeof(float));
    std::memcpy(host.data() + strengths[0], in->class_strengths, n * 2 * sizeof(double));
    std::memcpy(host.data() + picked[0], in->classes, n * 2 * sizeof(int32_t));
  }
  if (with_categories) {
    std::memcpy(host.data() + signature[1], in->category_signature, n * k * sizeof(float));
    std::memcpy(host.data() + strengths[1], in->category_strengths, n * k * sizeof(double));
    std::memcpy(host.data() + picked[1], in->categories, n * k * sizeof(int32_t));
  }
  tb.fill(host.data(), names, stride);
  DeviceBlock dev;
  AFX_TRY(dev.allocate(layout.bytes(), "device memory for the class columns and their text"));
  afx::RowTextArgs a{};
  tb.point(&a, dev.get(), names);
  a.classes.signature = at<float>(dev.get(), signature[0]);
  a.classes.strengths = at<double>(dev.get(), strengths[0]);
  a.classes.picks = at<int32_t>(dev.get(), picked[0]);
  a.categories.signature = at<float>(dev.get(), signature[1]);
  a.categories.strengths = at<double>(dev.get(), strengths[1]);
  a.categories.picks = at<int32_t>(dev.get(), picked[1]);
  HIP_TRY(hipMemcpy(dev.get(), host.data(), tb.up_end, hipMemcpyHostToDevice));
  HIP_TRY(afx::launch_row_text(a, nullptr, nullptr));
  HIP_TRY(hipMemcpy(host.data() + tb.class_begin, dev.get() + tb.class_begin, tb.end - tb.class_begin, hipMemcpyDeviceToHost));   // waits for the kernel
  tb.hand_out_classes(host.data(), text, begin, length, afx::kRowTextColumns);
  return AFX_OK;
}

}  // extern "C"
