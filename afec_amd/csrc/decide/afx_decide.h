// afec_amd/csrc/decide/afx_decide.h -- the class decision's kernel (afx_decide.hip) and its launcher, shared with the entry
// points of afx_class_decision.cpp.  Kept apart from afx_internal.h for the reason highlevel/afx_highlevel.h gives; a device
// mock implements this launcher too.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../afx_internal.h"

namespace afx {

constexpr int kDecideClasses = 2;          // "Loop" and "OneShot": the only class model the reference accepts (SA:1109)
constexpr int kDecideMaxCategories = 64;   // kGbdtMaxClasses: a category is a lane where the results are stored

// one double per file, `stride` doubles apart: the batch reads its scalars where the run's kernels left them (the rhythm
// tracker's 14 per file, the 13 statistics of every record column), the record-free entry from the caller's five per file
struct DecideScalar {
  const double* p;
  int64_t stride;
  __host__ __device__ double at(int file) const { return p[(int64_t)file * stride]; }
};

struct DecideArgs {
  const float* class_signature;      // [n_files][2] as class_signature_kernel wrote it, or NULL: no class model
  const float* category_signature;   // [n_files][n_categories], or NULL: no category model
  int32_t n_categories;              // 2..kDecideMaxCategories (0 without a category model)
  int32_t loop_class, oneshot_class; // {0, 1} in either order
  int32_t use_heuristics;
  int32_t none_category;             // the index of the "None" category, or -1
  const double* peak;                // amplitude_peak of frame f of a file: peak[(frame_offset[file] + f) * peak_stride]
  int64_t peak_stride;
  const int64_t* frame_offset;       // [n_files + 1], device
  DecideScalar efflen24;             // effectve_length_24dB, seconds
  DecideScalar onset_count;          // rhythm_percussive_onset_count
  DecideScalar percussive_confidence, complex_confidence;   // rhythm_*_tempo_confidence
  DecideScalar flux_mean;            // the mean of spectral_flux
  const int32_t* status;             // [n_files]: buf_status, or NULL: all 0
  const int32_t* non_finite_in;      // [n_files]: the signature kernel's count, or NULL: all 0
  double silence_floor;              // DbToLin(-24)
  int32_t n_files;
  double* class_strengths;           // [n_files][2]
  int32_t* classes;                  // [n_files][2]
  double* category_strengths;        // [n_files][n_categories]
  int32_t* categories;               // [n_files][n_categories]
  double* confidences;               // [n_files][2]: IsOneShot, IsLoop
  int32_t* flags;                    // [n_files]
  int32_t* non_finite;               // [n_files]
};
// one wave per file, on `stream`
hipError_t launch_class_decision(const DecideArgs& a, hipStream_t stream);

}  // namespace afx
