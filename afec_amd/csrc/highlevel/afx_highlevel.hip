// afec_amd/csrc/highlevel/afx_highlevel.hip -- the model-free high-level descriptors of a file,
// TSampleAnalyser::AnalyzeHighLevelDescriptors (SampleAnalyser.cpp:1234-1606), from what a batch holds in device memory
// after afx_batch_run: its per-frame records and the rhythm tracker's scalars.  Nothing here touches audio samples.
//
// One wave per file, lanes over frames (frame p = lane + 64 k; the record stride lies between the lanes, so every column
// read costs a cache line per frame -- each column is read once, in the first pass):
//   1. one pass over the records: the audible-frame sums, minimum and maxima of the nine series the scalars need, and the
//      copy of amplitude_peak (mHighLevelPeak); cross-lane by DPP (afx_device.h), no LDS
//   2. the confidence class from the audible mean of f0_confidence, then a pass over f0 / f0_confidence / silence (one
//      cache line of the record) that counts the confident pitches, finds the first audible one and leaves their
//      order-preserving keys in LDS (series of up to kLdsKeys frames; longer ones are read again from the records)
//   3. the exact lower median (TStatistics::Median, Statistics.cpp:316-413: the element of rank (n-1)/2) by a
//      most-significant-digit radix select over the keys, eight passes of eight bits (the method of afx_stats.hip's
//      long series), and the two passes of the base note's standard-deviation penalty
//   4. the pitch track: "last confident audible frame at or before p" is an inclusive maximum scan of the frame indices
//      (DPP inside 64 frames, one carried value between the tiles)
//   5. the spectrum signature: lane i is output position i of the 64; it merges and compresses the bands of the four
//      frames its cubic needs (4 x 14 pow per lane instead of 14 per frame)
// Sums are formed in another order than the reference's serial TStatistics::Sum; everything that decides something
// (the thresholds on f0 and its confidence, the rank of the median, the truncation of the resampling position) reads the
// same bits as the reference would.

#include <hip/hip_runtime.h>

#include <limits.h>

#include "afx_highlevel.h"
#include "../afx_device.h"

namespace afx {
namespace {

using u64 = unsigned long long;

constexpr int kWaves = 4;        // files per workgroup (the waves share nothing but the launch)
constexpr int kLdsKeys = 1024;   // keys of a series of up to this many frames stay in LDS (8 KiB a wave; 20 s = 860 frames)

// positive doubles order as their bit patterns; 0 marks a frame without a confident pitch (no f0 > 20 Hz has that key)
__device__ __forceinline__ u64 pitch_key(double f0) { return (u64)__double_as_longlong(f0) | 0x8000000000000000ull; }
__device__ __forceinline__ double key_pitch(u64 k) { return __longlong_as_double((long long)(k & 0x7FFFFFFFFFFFFFFFull)); }

// aubio_freqtomidi (aubio mathutils.c:535-546, smpl_t = double), the literal for log 2 included
__device__ __forceinline__ double freq_to_midi(double freq) {
  if (freq < 2.0 || freq > 100000.0) return 0.0;
  double midi = freq / 6.875;
  midi = log(midi) / 0.69314718055995;
  midi *= 12.0;
  midi -= 3.0;
  return midi;
}

// TAudioMath::LinToDb, the float overload (AudioMath.inl:38-53: mPeakValue and mRmsValue are floats): the logarithm in
// double, the result rounded to float; MEpsilon = 1e-12f, MMinusInfInDb = -200
__device__ __forceinline__ double lin_to_db(float v) {
  if (v == 1.0f) return 0.0;
  if (v > 1e-12f) return (double)(float)(log((double)v) * (20.0 / 2.30258509299404568402));
  return -200.0;
}

// TMath::Quantize(Value, Step, kRoundToNearest) (InlineMath.inl:625-636): half a step away from zero, then d2i truncates
__device__ __forceinline__ double quantize_nearest(double v, double step) {
  v = (v > 0.0) ? v + step / 2.0 : v - step / 2.0;
  return (double)(int)(v / step) * step;
}

// SInterpolateCubic (SampleAnalyser.cpp:139-156); x = Pos - floor(Pos)
__device__ __forceinline__ double interpolate_cubic(double ym1, double y0, double y1, double y2, double x) {
  const double xx = x * x;
  const double xxx = xx * x;
  const double a = -0.5 * xxx + xx - 0.5 * x;
  const double b = 1.5 * xxx - 2.5 * xx + 1.0;
  const double c = -1.5 * xxx + 2.0 * xx + 0.5 * x;
  const double d = 0.5 * xxx - 0.5 * xx;
  return a * ym1 + b * y0 + c * y1 + d * y2;
}

// the pitch test of SampleAnalyser.cpp:1236-1253 for the chosen class
__device__ __forceinline__ bool confident(double f0, double conf, double threshold, double quarter_rate) {
  return conf > threshold && f0 > 20.0 && f0 < quarter_rate;
}

// What the passes over the confident pitches read: the keys in LDS, or (series of more than kLdsKeys frames) the records.
struct PitchSource {
  const u64* keys;      // nullptr: from the records
  const double* rec;    // the file's first record
  int64_t stride;
  int32_t f0, f0_conf;
  double threshold, quarter_rate;
  __device__ __forceinline__ u64 key(int p) const {
    if (keys) return keys[p];
    const double* r = rec + (int64_t)p * stride;
    const double f = r[f0];
    return confident(f, r[f0_conf], threshold, quarter_rate) ? pitch_key(f) : 0ull;
  }
};

// the key of rank `rank` (0-based, ascending) among the non-zero keys of frames 0..n-1
__device__ u64 select_key(const PitchSource& src, int n, int rank, int lane, unsigned* hist) {
  u64 prefix = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    wave_lds_fence();
#pragma unroll
    for (int i = 0; i < 4; ++i) hist[4 * lane + i] = 0;
    wave_lds_fence();
    for (int p = lane; p < n; p += 64) {
      const u64 k = src.key(p);
      const bool match = k != 0 && ((shift == 56) || ((k >> (shift + 8)) == (prefix >> (shift + 8))));
      if (match) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
    }
    wave_lds_fence();
    unsigned c[4], local = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      c[i] = hist[4 * lane + i];
      local += c[i];
    }
    const unsigned incl = (unsigned)wave_scan_incl((int)local);
    const unsigned base = incl - local;
    const bool mine = (unsigned)rank >= base && (unsigned)rank < incl;
    int digit = 0, below = 0;
    if (mine) {
      unsigned cum = base;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if ((unsigned)rank >= cum + c[i]) cum += c[i];
        else { digit = 4 * lane + i; below = (int)cum; break; }
      }
    }
    const int from = __ffsll((unsigned long long)__ballot(mine)) - 1;
    digit = __shfl(digit, from);
    below = __shfl(below, from);
    prefix |= (u64)(unsigned)digit << shift;
    rank -= below;
  }
  return prefix;
}

// one band of the signature before resampling (SampleAnalyser.cpp:1450-1485): the mean of the source bands
// first..last, a little overscaled, compressed
__device__ __forceinline__ double merged_band(const double* bands, int first, int last) {
  double v = 0.0;
  for (int sb = first; sb <= last; ++sb) v += bands[sb];
  v /= (double)(last - first + 1);
  return pow(v * 1.25, 1.0 / 6.0);
}

__global__ __launch_bounds__(64 * kWaves) void high_level_kernel(HighArgs a) {
  __shared__ u64 keys_all[kWaves * kLdsKeys];
  __shared__ unsigned hist_all[kWaves * 256];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int file = (int)blockIdx.x * kWaves + wave;
  if (file >= a.n_bufs) return;
  u64* keys = keys_all + wave * kLdsKeys;
  unsigned* hist = hist_all + wave * 256;
  const RecordLayout& lay = a.lay;
  const int64_t stride = lay.stride;
  const int64_t row0 = a.frame_offset[file];
  const int n = (int)(a.frame_offset[file + 1] - row0);
  double* scalars = a.scalars + (int64_t)file * kHighScalars;
  double* signature = a.signature + (int64_t)file * (kHighSignatureFrames * kHighSignatureBands);
  if (n <= 0) {
    // no frames (an empty or a refused buffer): zeros.  The reference's resampling loop would read a list without
    // entries here; its result is undefined.
    if (lane < kHighScalars) scalars[lane] = 0.0;
    for (int i = lane; i < kHighSignatureFrames * kHighSignatureBands; i += 64) signature[i] = 0.0;
    return;
  }
  const double* rec = a.rec + row0 * stride;

  // ---- 1. the audible frames' sums, minimum, maxima (SampleAnalyser.cpp:420-440: audible = not silent) ----
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  int n_audible = 0;
  double s_conf = 0.0, s_rolloff = 0.0, mx_centroid = -inf, mn_flat = inf, mx_flat = -inf, s_flat = 0.0, s_acorr = 0.0;
  double s_flux = 0.0, s_contrast = 0.0, s_complexity = 0.0, s_inharm = 0.0;
  for (int p = lane; p < n; p += 64) {
    const double* r = rec + (int64_t)p * stride;
    const bool audible = r[lay.silence] == 0.0;
    const double conf = r[lay.f0_conf], rolloff = r[lay.rolloff], centroid = r[lay.centroid], flat = r[lay.flatness];
    const double acorr = r[lay.autocorr], flux = r[lay.flux], contrast = r[lay.contrast], cplx = r[lay.complexity];
    const double inharm = r[lay.inharm];
    a.peak[row0 + p] = r[lay.amp_peak];   // mHighLevelPeak = mAmplitudePeak (:1606)
    n_audible += audible ? 1 : 0;
    s_conf += audible ? conf : 0.0;
    s_rolloff += audible ? rolloff : 0.0;
    mx_centroid = audible ? fmax(mx_centroid, centroid) : mx_centroid;
    mn_flat = audible ? fmin(mn_flat, flat) : mn_flat;
    mx_flat = audible ? fmax(mx_flat, flat) : mx_flat;
    s_flat += audible ? flat : 0.0;
    s_acorr += audible ? acorr : 0.0;
    s_flux += audible ? flux : 0.0;
    s_contrast += audible ? contrast : 0.0;
    s_complexity += audible ? cplx : 0.0;
    s_inharm += audible ? inharm : 0.0;
  }
  n_audible = wave_sum_i(n_audible);
  s_conf = wave_sum(s_conf);
  s_rolloff = wave_sum(s_rolloff);
  mx_centroid = wave_max(mx_centroid);
  mn_flat = wave_min(mn_flat);
  mx_flat = wave_max(mx_flat);
  s_flat = wave_sum(s_flat);
  s_acorr = wave_sum(s_acorr);
  s_flux = wave_sum(s_flux);
  s_contrast = wave_sum(s_contrast);
  s_complexity = wave_sum(s_complexity);
  s_inharm = wave_sum(s_inharm);
  // TStatistics::Mean (Statistics.cpp:249-266): Sum / Length, the single value itself for Length 1 (the same number)
  const double dn = (double)n_audible;
  const double conf_mean = n_audible ? s_conf / dn : 0.0;                 // AudiblePitchConfidenceMean (:1256-1260)
  const double flat_mean = n_audible ? s_flat / dn : 0.0;

  // ---- 2. the confidence class and the confident pitches (:1262-1292: of ALL frames, not only the audible ones) ----
  const double threshold = (conf_mean >= 0.8) ? 0.8 : (conf_mean >= 0.5) ? 0.5 : 0.2;
  const double quarter_rate = (double)(a.sample_rate / 4);
  const bool in_lds = n <= kLdsKeys;
  int n_pitch = 0, first_audible_pitch = INT_MAX;
  for (int p = lane; p < n; p += 64) {
    const double* r = rec + (int64_t)p * stride;
    const double f0 = r[lay.f0];
    const bool c = confident(f0, r[lay.f0_conf], threshold, quarter_rate);
    if (in_lds) keys[p] = c ? pitch_key(f0) : 0ull;
    n_pitch += c ? 1 : 0;
    if (c && r[lay.silence] == 0.0) first_audible_pitch = min(first_audible_pitch, p);
  }
  n_pitch = wave_sum_i(n_pitch);
  first_audible_pitch = wave_min_i(first_audible_pitch);
  const PitchSource src{in_lds ? keys : nullptr, rec, stride, lay.f0, lay.f0_conf, threshold, quarter_rate};

  // ---- 3. base note and its confidence (:1279-1331) ----
  double base_note = -1.0, base_note_confidence = 0.0;
  if (n_pitch > 0) {
    const double hz = key_pitch(select_key(src, n, (n_pitch - 1) / 2, lane, hist));
    if (hz > 20.0 && hz < quarter_rate) base_note = freq_to_midi(hz);
  }
  if (base_note > 0.0) {
    // TStatistics::StandardDeviation of |base note - note of every confident pitch|: Mean, then Variance around it
    // (Statistics.cpp:270-312: the sum of squares over Length, 0 for a single value)
    double s_off = 0.0;
    for (int p = lane; p < n; p += 64) {
      const u64 k = src.key(p);
      s_off += k ? fabs(base_note - freq_to_midi(key_pitch(k))) : 0.0;
    }
    s_off = wave_sum(s_off);
    const double off_mean = s_off / (double)n_pitch;
    double s_sq = 0.0;
    for (int p = lane; p < n; p += 64) {
      const u64 k = src.key(p);
      const double t = fabs(base_note - freq_to_midi(key_pitch(k))) - off_mean;
      s_sq += k ? t * t : 0.0;
    }
    s_sq = wave_sum(s_sq);
    const double deviation = (n_pitch >= 2) ? sqrt(s_sq / (double)n_pitch) : 0.0;
    const double ratio = deviation / 6.0;
    base_note_confidence = conf_mean * (1.0 - ((1.0 < ratio) ? 1.0 : ratio));
  }

  // ---- 4. the pitch track (:1557-1596) ----
  // look-ahead over frames 0 .. max(1, n / 4) inclusive (files of one frame have none)
  double carried_pitch = 0.0;
  if (n > 1 && first_audible_pitch <= max(1, n / 4)) carried_pitch = rec[(int64_t)first_audible_pitch * stride + lay.f0];
  int carry = -1;
  for (int base = 0; base < n; base += 64) {
    const int p = base + lane;
    const bool inside = p < n;
    const double* r = rec + (int64_t)(inside ? p : 0) * stride;
    const double f0 = r[lay.f0];
    const bool mine = inside && r[lay.silence] == 0.0 && confident(f0, r[lay.f0_conf], threshold, quarter_rate);
    // the last confident audible frame at or before p: inclusive maximum scan of the frame indices
    int last = max(wave_scan_max_i(mine ? p : -1), carry);
    double v = carried_pitch;
    if (last >= 0) v = (last == p) ? f0 : rec[(int64_t)last * stride + lay.f0];
    if (inside) a.pitch[row0 + p] = freq_to_midi(v);
    carry = __builtin_amdgcn_readlane(last, 63);
  }

  // ---- 5. the spectrum signature (:1450-1520): lane = output position ----
  {
    // Step = n / 64 and every multiple of it are exact, so the reference's running sum CurrentPos is lane * Step
    const double pos = (double)lane * ((double)n / (double)kHighSignatureFrames);
    const int ipos = (int)pos;   // TMath::d2i truncates
    const int idx[4] = {max(0, ipos - 1), ipos, min(n - 1, ipos + 1), min(n - 1, ipos + 2)};
    const double x = pos - floor(pos);
    double y[4][kHighSignatureBands];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double* bands = rec + (int64_t)idx[k] * stride + lay.bands;
      // sSpectrumBands = 0, 1, 3, 5, .. 25: a band ends there and starts behind the one before
      y[k][0] = merged_band(bands, 0, 0);
      y[k][1] = merged_band(bands, 1, 1);
#pragma unroll
      for (int b = 2; b < kHighSignatureBands; ++b) y[k][b] = merged_band(bands, 2 * b - 2, 2 * b - 1);
    }
    double* out = signature + lane * kHighSignatureBands;
#pragma unroll
    for (int b = 0; b < kHighSignatureBands; ++b) out[b] = interpolate_cubic(y[0][b], y[1][b], y[2][b], y[3][b], x);
  }

  // ---- the scalars ----
  if (lane == 0) {
    const float* level = a.levels ? a.levels + 2 * (int64_t)file : nullptr;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    scalars[0] = level ? lin_to_db(level[0]) : nan;   // AFX_HL_PEAK_DB (:1336-1339)
    scalars[1] = level ? lin_to_db(level[1]) : nan;   // AFX_HL_RMS_DB
    scalars[2] = base_note;
    scalars[3] = base_note_confidence;
    const double* rhythm = a.rt_scalars + (int64_t)file * 14;
    scalars[4] = quantize_nearest(rhythm[12], 0.5);   // AFX_HL_BPM: the final tempo "made pretty" (:1345-1349)
    scalars[5] = rhythm[13];
    double brightness = 0.0, noisiness = 0.0, harmonicity = 0.0;
    if (n_audible) {
      // MMin(a, b) = a < b ? a : b, MMax(a, b) = a > b ? a : b
      // brightness (:1356-1382)
      double w = freq_to_midi(s_rolloff / dn) / 128.0 * 0.7 + freq_to_midi(mx_centroid) / 128.0 * 0.3;
      w = (1.0 < w) ? 1.0 : w;
      w = (0.0 > w) ? 0.0 : w;
      brightness = pow(w, 4.0);
      // noisiness (:1386-1413)
      w = (1.0 - mn_flat) * 0.2 + (1.0 - flat_mean) * 0.6 + (1.0 - mx_flat) * 0.2;
      w = (1.0 < w) ? 1.0 : w;
      w = (0.0 > w) ? 0.0 : w;
      noisiness = pow(w, 2.0);
      // harmonicity (:1418-1444)
      const double ac = 1.5 * (s_acorr / dn), pc = 2.0 * conf_mean;
      w = ((1.0 < ac) ? 1.0 : ac) * 0.4 + ((1.0 < pc) ? 1.0 : pc) * 0.3 + flat_mean * 0.3;
      w = (1.0 < w) ? 1.0 : w;
      w = (0.0 > w) ? 0.0 : w;
      harmonicity = pow(w, 2.0);
    }
    scalars[6] = brightness;
    scalars[7] = noisiness;
    scalars[8] = harmonicity;
    scalars[9] = flat_mean;                               // the audible means (:1529-1553)
    scalars[10] = n_audible ? s_flux / dn : 0.0;
    scalars[11] = n_audible ? s_complexity / dn : 0.0;
    scalars[12] = n_audible ? s_contrast / dn : 0.0;
    scalars[13] = n_audible ? s_inharm / dn : 0.0;
    scalars[14] = conf_mean;                              // AFX_HL_PITCH_CONFIDENCE (:1601)
  }
}

}  // namespace

hipError_t launch_high_level(const HighArgs& a, hipStream_t stream) {
  if (a.n_bufs <= 0) return hipSuccess;
  const int blocks = (a.n_bufs + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(high_level_kernel, dim3(blocks), dim3(64 * kWaves), 0, stream, a);
  return hipGetLastError();
}

}  // namespace afx
