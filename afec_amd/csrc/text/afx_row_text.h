// afec_amd/csrc/text/afx_row_text.h -- the kernel that writes the class decision's arrays as the six text columns of the
// reference's high-level database (afx_row_text.hip: class_signature_VR, classes_VS, class_strengths_VR and the three
// category columns; SToJSON, SqliteSampleDescriptorPool.cpp:316-358, 884-904) and the launcher that puts it in front of the
// vector columns' kernel (afx_text.h), shared with the entry points afx_batch_fetch_high_level_row and afx_format_class_json
// (afx_high_level_row.cpp).  The slot arithmetic is host code and plain C++: tests/sanitize/row_main.cpp includes this
// header without a device.
#pragma once

#include <stdint.h>

#include "afx_text.h"

namespace afx {

constexpr int kRowTextColumns = 6;      // per file: signature, names, strengths of the class model, then of the category model
constexpr int kRowTextMaxNames = 64;    // kDecideMaxCategories
constexpr int kRowTextMaxNameBytes = 255;

// the longest text of a column of names: "[" "]", per name two quotes and a comma (the first has none) -- every name picked
// once, which is the most a pick can hold
constexpr int64_t names_slot_bytes(int64_t sum_of_lengths, int64_t count) { return 2 + sum_of_lengths + 3 * count; }

// What one model's three columns read.  count = 0: the model is not there, the three columns are "[]" and nothing is read.
struct RowTextModel {
  const float* signature;     // [n_files][count]: written widened to double (SampleAnalyser.cpp:1097, 1190)
  const double* strengths;    // [n_files][count]
  const int32_t* picks;       // [n_files][count]: indices in pick order, the list ends at the first one outside 0 .. count-1
  int32_t count;              // 0, or 2 .. kRowTextMaxNames
  int32_t first_name;         // the model's names are name_offset / name_length [first_name .. first_name + count)
  int32_t names_slot;         // names_slot_bytes of all its names: a list that would not fit is written as "[]"
};

struct RowTextArgs {
  RowTextModel classes, categories;
  int32_t n_files;
  const char* name_bytes;       // the bytes of all names, copied verbatim
  const int32_t* name_offset;   // [classes.count + categories.count] into name_bytes
  const int32_t* name_length;
  const int64_t* file_slot;     // [n_files]: where the file's six slots start in `text`, one behind the other in column order
  char* text;                   // 4-byte aligned
  int64_t* begin;               // [n_files][kRowTextColumns]
  int32_t* length;              // [n_files][kRowTextColumns]
};

// the bytes of one file's six slots: they depend on the models' sizes and the names' lengths alone
constexpr int64_t row_text_file_bytes(int32_t n_classes, int32_t class_names_slot, int32_t n_categories, int32_t category_names_slot) {
  return 2 * text_slot_bytes(n_classes, 0) + class_names_slot + 2 * text_slot_bytes(n_categories, 0) + category_names_slot;
}

// one wave per file, on `stream`; then, where `vectors` holds columns, the vector columns' kernel behind it
hipError_t launch_row_text(const RowTextArgs& a, const TextArgs* vectors, hipStream_t stream);

}  // namespace afx
