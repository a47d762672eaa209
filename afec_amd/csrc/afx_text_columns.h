// afec_amd/csrc/afx_text_columns.h -- where the three vector columns of a batch's buffers (AFX_HLT_*) lie, host only: shared
// by the fetch that brings them back alone (afx_high_level_text.cpp) and the one that brings the whole high-level row
// (afx_high_level_row.cpp), whose files have the class columns' slots in front of them.
#pragma once

#include "afx_block.h"
#include "text/afx_text.h"

namespace afx {
namespace host {

// the three columns of every buffer, slot behind slot in the order of AFX_HLT_*, `lead` bytes of another kernel's slots in
// front of every buffer's; returns the bytes of all slots.  `first` counts the doubles of each column's own array.
inline int64_t high_level_columns(const afx_batch* b, afx::TextColumn* table, int64_t lead = 0) {
  constexpr int64_t kSignature = afx::kHighSignatureFrames * afx::kHighSignatureBands;
  int64_t slot = 0;
  for (int32_t i = 0; i < b->n_bufs; ++i) {
    const int64_t row0 = b->frame_offset[(size_t)i], frames = b->frame_offset[(size_t)i + 1] - row0;
    const afx::TextColumn columns[AFX_NUM_HLT_COLUMNS] = {
        {(int64_t)i * kSignature, 0, (int32_t)kSignature, afx::kHighSignatureBands}, {row0, 0, (int32_t)frames, 0}, {row0, 0, (int32_t)frames, 0}};
    slot += lead;
    for (int c = 0; c < AFX_NUM_HLT_COLUMNS; ++c) {
      if (table) {
        table[(size_t)i * AFX_NUM_HLT_COLUMNS + c] = columns[c];
        table[(size_t)i * AFX_NUM_HLT_COLUMNS + c].slot = slot;
      }
      slot += afx::text_slot_bytes(columns[c].count, columns[c].inner);
    }
  }
  return slot;
}

// the table's `first` of pitch and peak counted from the signature on, which the text kernel takes as its values: the three
// arrays lie in one block (every array of a block starts at a multiple of 8 bytes)
inline void count_from_signature(afx::TextColumn* table, size_t n, const HighBlock& hb) {
  for (size_t i = 0; i < n; ++i) {
    table[i * AFX_NUM_HLT_COLUMNS + AFX_HLT_PITCH].first += (int64_t)((hb.pitch - hb.signature) / sizeof(double));
    table[i * AFX_NUM_HLT_COLUMNS + AFX_HLT_PEAK].first += (int64_t)((hb.peak - hb.signature) / sizeof(double));
  }
}

}  // namespace host
}  // namespace afx
