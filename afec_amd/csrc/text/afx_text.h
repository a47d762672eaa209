// afec_amd/csrc/text/afx_text.h -- the kernel that writes columns of doubles as the JSON text of the reference's high-level
// database (afx_text.hip: SToJSON, SqliteSampleDescriptorPool.cpp:316-419, every number by text/afx_g9.h) and its launcher,
// shared with the entry points afx_batch_fetch_high_level_text and afx_format_json_g9 (afx_high_level_text.cpp).  Kept apart
// from afx_internal.h like the launchers of the other fetches above a run; a device mock implements launch_json_g9 with the
// same header on the host (tests/sanitize/text_main.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../afx_internal.h"

namespace afx {

// One column: `count` doubles from values[first] on.  inner = 0: a flat list [a,b,c] (VR); inner = W > 0, W divides count:
// rows of W, [[..],[..]] (VVR).  Its text goes to text[slot ..], a slot of text_slot_bytes(count, inner) of the host's
// choosing: placement does not depend on the order the waves run in, so a repeated fetch is bit-equal.
struct TextColumn {
  int64_t first;
  int64_t slot;
  int32_t count;
  int32_t inner;
};

// the longest text of a column: "[" "]", per number 16 characters and a comma (the first has none), per row "[" "],"
constexpr int64_t text_slot_bytes(int64_t count, int64_t inner) { return 2 + 17 * count + (inner > 0 ? 2 * (count / inner) : 0); }

struct TextArgs {
  const double* values;
  const TextColumn* columns;   // [n_columns], device
  int32_t n_columns;
  char* text;                  // 4-byte aligned
  int64_t* begin;              // [n_columns]: where a column's text starts in `text` (its slot)
  int32_t* length;             // [n_columns]: how long it is
};
// one wave per column, on `stream`
hipError_t launch_json_g9(const TextArgs& a, hipStream_t stream);

}  // namespace afx
