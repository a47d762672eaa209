// afec_amd/csrc/afx_time.hip -- time-domain neighbours of the spectral loop, gfx950.
//
// Per frame, from the PCM arena (one wave per chunk of consecutive frames, like the frame kernel):
//
//   hop_kernel    amplitude_silence   aubio_silence_detection on the hop, Aubio mathutils.c:345-357, 605-615
//                 amplitude_envelope  TEnvelopeDetector kFast over the hop, SampleAnalyser.cpp (SA) 1787-1804
//   acorr_kernel  auto_correlation    CalcAutoCorrelation, SA:2312-2398 (TAutocorrelation::Calc)
//   pitch_kernel  f0, f0_confidence   aubio yinfast, Aubio pitch/pitchyinfast.c:81-170, pitch.c:399-462,
//                                     SA:876-896 (the fail-safe f0 needs the spectrum: afx_whiten.hip)
//
// The two correlations are computed through the in-register 1024-point complex FFT of afx_fft.h: a real
// 2048-point transform is the complex transform of z[m] = x[2m] + i x[2m+1] plus the even/odd untangle,
// X[k] = E[k] + w^k O[k], X[1024-k] = conj(E[k] - w^k O[k]); the inverse of a Hermitian spectrum runs the
// same steps backwards.  All arithmetic is double whatever the plan's STFT precision.
//
// Layouts: "strided" element = lane + 64 r (FFT in/out), "blocked" element = 16 lane + i (prefix sums,
// first-index searches).  Changes of layout go through the wave's LDS plane with one pad slot per 16.
//
// Each kernel is its chunk loop, its frame loop and the stages called top to bottom; a stage's head comment
// says what it reads and what it leaves.  Resources: tests/golden/kernel_resources.json.

#include <cstddef>
#include <mutex>

#include <hip/hip_runtime.h>

#include "afx_internal.h"
#include "afx_device.h"
#include "afx_fft.h"

namespace afx {
namespace {

constexpr int kTimeWaves = 8;
constexpr int kAcorrSeg = 640;      // acorr_kernel: staged samples per frame, rows start/64 .. start/64 + 9
constexpr int kPadSlots = 1344;     // doubles of a wave's plane
static_assert(kPadSlots >= 1024 + 64, "the blocked layouts: 1024 elements and one pad slot per 16");
static_assert(kPadSlots >= kPlaneSlots, "the transform's exchange (afx_fft.h)");
static_assert(kPadSlots >= 2 * kAcorrSeg, "acorr_kernel stages the segments of two frames");

__device__ __forceinline__ int pad_slot(int e) { return e + (e >> 4); }

// lane constants of the envelope's prefix scan (hop_descriptors): coef^(16 (j + 1)) takes the end value of the last lane
// of the row before to lane j of a row; from lane 31 to lane j of row 2 it is the same power, of row 3 sixteen lanes more
struct EnvelopeScan { double from_row_before, from_lane31; };

// The dynamic LDS of acorr_kernel and pitch_kernel.  The shared tables first (t2, post: 16 KiB each; t1: 1 KiB -- from
// global memory its reads were three exposed cache round trips per transform, the vector-memory path being what the
// frame's own loads wait on), then what pitch_kernel keeps for hop_descriptors, then one plane per wave.
struct TimeLds {
  cx<double> t2[1024];
  cx<double> post[1024];                  // w2048^k at [k]
  cx<double> t1[64];
  double env_pow[32];                     // coef^i, i <= 16
  EnvelopeScan env_scan[64];              // per lane
  double plane[kTimeWaves][kPadSlots];
};
static_assert(offsetof(TimeLds, t2) == 0 && offsetof(TimeLds, post) == 16384 && offsetof(TimeLds, t1) == 32768 &&
              offsetof(TimeLds, env_pow) == 32768 + 1024 && offsetof(TimeLds, env_scan) == 32768 + 1024 + 256 &&
              offsetof(TimeLds, plane) == 32768 + 1024 + 256 + 1024 && sizeof(TimeLds) == 121088,
              "every address of the record is the one the kernels were measured with");
constexpr int kTimeLdsBytes = (int)sizeof(TimeLds);

__device__ __forceinline__ TimeLds& time_lds() {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  return *reinterpret_cast<TimeLds*>(lds_raw);
}

// kPcmScaledF32: the sixteen loaded samples times the buffer's FinalScaling (each product rounded once, like the
// reference's stored doubles: pcm_double, afx_device.h)
template <bool SCALED>
__device__ __forceinline__ void scale16(double (&x)[16], double scale) {
  if (SCALED) {
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = pcm_double<true>(x[i], scale);
  }
}

// sixteen consecutive samples (p 16-byte aligned) held as they were loaded (the conversion to double happens where they
// are used: loads issued early keep 16 / 32 registers, not 32 / 64)
template <typename TIn>
struct Block16;
template <>
struct Block16<float> {
  float4 q[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4* s = reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = s[j];
  }
  __device__ __forceinline__ void get(double (&x)[16]) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[4 * j] = (double)q[j].x; x[4 * j + 1] = (double)q[j].y; x[4 * j + 2] = (double)q[j].z; x[4 * j + 3] = (double)q[j].w;
    }
  }
};
template <>
struct Block16<double> {
  double2 q[8];
  __device__ __forceinline__ void load(const double* p) {
    const double2* s = reinterpret_cast<const double2*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = s[j];
  }
  __device__ __forceinline__ void get(double (&x)[16]) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[2 * j] = q[j].x; x[2 * j + 1] = q[j].y;
    }
  }
};

// Loads of a frame are issued long before they are used where the registers allow it.  Double PCM -- buffers a caller
// normalised itself -- would hold twice the registers in flight (acorr_kernel: 98 of rows): it is loaded where it is used.
template <typename TIn>
constexpr bool kPrefetch = sizeof(TIn) == 4;

// lane 0's value, in every lane
__device__ __forceinline__ float first_lane(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)); }
__device__ __forceinline__ double first_lane(double v) { return read_lane<0>(v); }

using mask64 = unsigned long long;

// aubio_silence_detection: 10 log10(mean x^2) < -48 dB (mathutils.c:605-615, MSilenceThresholdDb).  log10 is
// monotonic, so the test is mean x^2 < 10^-4.8 (they can only disagree for a level within an ulp of the
// threshold); a NaN level is "not silent" in both forms.
__device__ __forceinline__ bool au_silent(double sum_sq, int n) {
  return sum_sq / (double)n < 1.5848931924611134e-05;
}

// ---------------------------------------------------------------------------------------------
// the descriptors of a hop (the first 1024 samples of a frame): hop_kernel's, and pitch_kernel's when it writes them
// ---------------------------------------------------------------------------------------------
// TEnvelopeDetector(kFast, MEnvelopeTimeInMs = 8, rate): mCoef = pow(0.01, 1000 / (ms rate)), Envelopes.cpp:55-70
__device__ __forceinline__ double envelope_coef() { return pow(0.01, 1000.0 / (8.0 * (double)kSampleRate)); }

__device__ __forceinline__ EnvelopeScan envelope_scan(double coef, int lane) {
  const int j = lane & 15;
  EnvelopeScan e;
  e.from_row_before = pow(coef, (double)(16 * (j + 1)));
  e.from_lane31 = (lane >= 48) ? pow(coef, (double)(16 * (j + 17))) : e.from_row_before;
  return e;
}

// the hop's sum of squares, from its samples in the blocked layout
__device__ __forceinline__ double hop_energy(const double (&x)[16]) {
  double e = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) e += x[i] * x[i];
  return wave_sum(e);
}

// The descriptors of a hop from its samples in the blocked layout, x[i] = sample 16 lane + i, and their sum of squares
// e: the silence flag, the envelope maximum (TEnvelopeDetector kFast, reset per frame: SA:1787-1804) and, when
// `amplitude` asks for them, CalcAmplitudePeak / CalcAmplitudeRms (SA:1760-1783).  Leaves them in rec, from lane 0.
// env_i = in_i + c (env_{i-1} - in_i) is affine in env_{i-1} with slope c: a lane runs its 16 samples from 0, the carries
// are an affine scan over the lanes (slope c^16), and env_i = local_i + c^(i+1) carry.
// cpow[i] = coef^i, i <= 16 (registers in hop_kernel, an LDS table in pitch_kernel).
template <typename Pow>
__device__ __forceinline__ void hop_descriptors(const double (&x)[16], double e, double coef, const Pow& cpow, const EnvelopeScan& scan,
                                                uint32_t amplitude, const RecordLayout& lay, double* rec, int lane) {
  if (amplitude) {
    double peak = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) peak = fmax(peak, fabs(x[i]));
    peak = wave_max(peak);
    if (lane == 0) {
      if ((amplitude & (1u << 11)) && lay.amp_peak >= 0) rec[lay.amp_peak] = peak;
      if ((amplitude & (1u << 12)) && lay.amp_rms >= 0) rec[lay.amp_rms] = nan_to_zero(sqrt(e / (double)kHop));
    }
  }
  if (lay.silence < 0 && lay.envelope < 0) return;
  double env = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const double in = fabs(x[i]);
    env = in + coef * (env - in);        // TEnvelopeDetector::Run, Envelopes.inl:14-18
  }
  // The envelope at the end of lane l's sixteen samples is C_l = env_l + s C_(l-1), s = coef^16: a prefix "sum" with a
  // factor per step.  Inside the rows of 16 lanes with DPP row shifts (factors s, s^2, s^4, s^8), then the last lane of
  // row 0 into row 1 and of row 2 into row 3, then lane 31 into rows 2 and 3, each times the power of s that separates the
  // two lanes (EnvelopeScan) -- no LDS round trips (six ds_bpermute steps before).
  double carry = env;
  const double s1 = cpow[16], s2 = s1 * s1, s4 = s2 * s2, s8 = s4 * s4;
  carry = fma(s1, dpp_or_zero<kDppRowShr1>(carry), carry);
  carry = fma(s2, dpp_or_zero<kDppRowShr2>(carry), carry);
  carry = fma(s4, dpp_or_zero<kDppRowShr4>(carry), carry);
  carry = fma(s8, dpp_or_zero<kDppRowShr8>(carry), carry);
  carry = fma(scan.from_row_before, dpp_or_zero<kDppRowBcast15, 0xA>(carry), carry);
  carry = fma(scan.from_lane31, dpp_or_zero<kDppRowBcast31, 0xC>(carry), carry);
  const double in_carry = dpp_or_zero<0x138>(carry);      // wave_shr:1: lane l reads lane l - 1, lane 0 gets 0
  // the lane's sixteen values once more, now from the state the lanes before it leave: the reference's recurrence itself
  // (the first pass, from 0, only gave the scan its per-lane term; its sixteen values are not kept -- 32 registers that
  // the pitch kernel, which calls this with its transforms' registers live, does not have)
  double top = 0.0;
  env = in_carry;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const double in = fabs(x[i]);
    env = in + coef * (env - in);
    top = fmax(top, env);
  }
  top = wave_max(top);
  if (lane == 0) {
    if (lay.silence >= 0) rec[lay.silence] = au_silent(e, kHop) ? 1.0 : 0.0;   // SA:865-868
    if (lay.envelope >= 0) rec[lay.envelope] = top;
  }
}

// ---------------------------------------------------------------------------------------------
// hop kernel: silence flag + envelope maximum of the hop
// ---------------------------------------------------------------------------------------------
template <typename TIn, bool SCALED>
__global__ __launch_bounds__(256) void hop_kernel(const TimeArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave_global = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int wave_stride = gridDim.x * 4;
  const TIn* const pcm = reinterpret_cast<const TIn*>(a.pcm);

  const double coef = envelope_coef();
  double cpow[17];
  cpow[0] = 1.0;
#pragma unroll
  for (int i = 1; i <= 16; ++i) cpow[i] = cpow[i - 1] * coef;
  const EnvelopeScan env_scan = envelope_scan(coef, lane);

  for (int ci = wave_global; ci < a.n_chunks; ci += wave_stride) {
    const Chunk ch = a.chunks[ci];
    const double sc = SCALED ? wave_uniform(ch.scale) : 1.0;
    for (int fi = 0; fi < ch.nframes; ++fi) {
      Block16<TIn> q;
      q.load(pcm + ch.sample_off + (int64_t)fi * kHop + 16 * lane);
      double x[16];
      q.get(x);
      scale16<SCALED>(x, sc);
      double* const rec = a.rec + ((int64_t)ch.frame0 + fi) * a.lay.stride;

      hop_descriptors(x, hop_energy(x), coef, cpow, env_scan, a.amplitude, a.lay, rec, lane);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// FFT plumbing shared by the correlation kernels
// ---------------------------------------------------------------------------------------------
struct TimeCtx {
  const cx<double>* t1;     // LDS, + 16 (lane >> 4)
  const cx<double>* t2;     // LDS, + lane
  const cx<double>* post;   // LDS, + lane: w2048^(lane + 64 r) at [64 r]
  double* plane;            // this wave's
  unsigned plane_rd_addr;
  int lane, partner;
};

template <typename T, int N>
__device__ __forceinline__ void fill_table(T (&dst)[N], const void* src) {
  copy_lds_table(reinterpret_cast<unsigned char*>(dst), src, (int)sizeof(dst), threadIdx.x, kTimeWaves * 64);
}

// fills the record's tables (all threads; ends behind a __syncthreads()) and gives the wave its view of the record
__device__ __forceinline__ TimeCtx time_setup(const TimeArgs& a, TimeLds& lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  fill_table(lds.t2, a.t2);
  fill_table(lds.post, a.post);
  fill_table(lds.t1, a.t1);
  __syncthreads();
  TimeCtx c;
  c.t1 = lds.t1 + 16 * (lane >> 4);
  c.t2 = lds.t2 + lane;
  c.post = lds.post + lane;
  c.plane = lds.plane[wave];
  c.plane_rd_addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double*)c.plane + 8u * lane;
  c.lane = lane;
  c.partner = (64 - lane) & 63;
  return c;
}

__device__ __forceinline__ void fft(cx<double> (&v)[16], const TimeCtx& c) {
  fft1024<double>(v, c.t1, c.t2, reinterpret_cast<unsigned char*>(c.plane), c.plane_rd_addr, c.lane);
}

// Z[1024 - k] for k = lane + 64 r (Z is 1024-periodic)
__device__ __forceinline__ cx<double> partner_of(const cx<double> (&v)[16], int r, const TimeCtx& c) {
  cx<double> p{__shfl(v[15 - r].re, c.partner), __shfl(v[15 - r].im, c.partner)};
  if (c.lane == 0) p = v[(16 - r) & 15];
  return p;
}

// even/odd parts (times 2) of the 2048-point spectrum of the real sequence packed into z:
// 2 E[k] = Z[k] + conj(Z[1024-k]),  2 O[k] = -i (Z[k] - conj(Z[1024-k]))
__device__ __forceinline__ void even_odd(cx<double> z, cx<double> p, cx<double>& e, cx<double>& o) {
  e = {z.re + p.re, z.im - p.im};
  o = {z.im + p.im, p.re - z.re};
}

// ---------------------------------------------------------------------------------------------
// auto_correlation (SA:2312-2398)
// ---------------------------------------------------------------------------------------------
// Two frames per pair of transforms.  TAutocorrelation::Calc (Autocorrelation.cpp:84-104) of a segment of w <= 529
// samples is the inverse transform of its power spectrum.  With circular length N = 1024 the lags k <= N - w come out
// clean (c[k] = r[k] + r[N - k], r[m] = 0 for m >= w); the few lags above that (k in [w - 32, w), at most 32 terms each)
// are summed directly, and the one lag that can still be polluted (k = 496 for w = 529: its alias is r[528]) is
// corrected with the directly summed value.  Two real sequences share one complex transform, z = a + i b:
// 2 A[k] = Z[k] + conj(Z[N-k]), 2 B[k] = -i (Z[k] - conj(Z[N-k])), and since the power spectra are real and even,
// the forward transform of |2A|^2 + i |2B|^2 is 4 N (r_a + i r_b).  (Before: each frame's zero-padded 2048-point real
// transform and its inverse: two complex 1024-point transforms per frame instead of per pair.)

// TAudioMath::MsToSamples(44100, 0.8f) = 35, (44100, 12.0f) = 529 (float maths, AudioMath.inl:127-130)
constexpr int kMinPeriod = 35, kSeekWidth = 529, kMaxSeek = kFft / 2, kAcorrN = 1024, kDirect = 32;
constexpr double kAcorrScale = 1.0 / 4096.0;   // the transforms return 4 N r
constexpr int kRowsFrame = 33, kRowsPair = 49;
constexpr double kNoLag = -1.0e300;

// What the two searches leave of one frame of a pair; wave-uniform.  start: the first rising step; period: the distance
// to the next one behind the minimum period; the correlated segment is x[start .. start + width), staged from the row
// that holds x[start], where it begins at `off`; the lags searched start at `from`.  (width is kSeekWidth for every
// emitted frame: such a frame has remaining >= 2048 and first_rise leaves start <= kMaxSeek - 2, so remaining - start >=
// 1026.  The general form stays: it is the reference's, and costs a scalar min.)
struct AcorrFrame {
  int start, period, width, from, off;
  bool active;      // the frame exists and has a correlation (SA:2358-2362); else its result is 0
};

// Everything the two searches and the correlations of a pair of frames may touch -- samples 0 .. 3135 of the first
// frame, as far as the buffer has them (the arena keeps up to 64 samples past the last frame; zeros behind it) -- is
// loaded in one go: rw[q] = x[64 q + lane]; the second frame's rows are rw[16 ..].  No load depends on a search result.
// x: frame fi of the chunk, remaining: mData.Size() - n at that frame, second: the chunk has frame fi + 1.
template <typename TIn>
__device__ __forceinline__ void load_rows(const TIn* x, int remaining, bool second, int lane, TIn (&rw)[kRowsPair]) {
  // the second frame's row 32 ends its own limit; without a second frame the first frame's row 32 does
  const int lim = min(remaining, second ? kHop + 64 * kRowsFrame : 64 * kRowsFrame);
#pragma unroll
  for (int q = 0; q < kRowsPair; ++q) {
    const int p = 64 * q + lane;
    rw[q] = (q < 32 || p < lim) ? ((q < kRowsFrame || second) ? x[q < kRowsFrame || second ? p : 0] : (TIn)0) : (TIn)0;
  }
}

// bit l: x[64 q + l + 1] > x[64 q + l] of the frame whose rows start at rw[row0].  One ballot per row: the row against
// itself shifted by one lane (wave_shl:1), lane 63 against lane 0 of the next row.
template <typename TIn>
__device__ __forceinline__ mask64 rising_mask(const TIn (&rw)[kRowsPair], int row0, int q) {
  const TIn next0 = (q + 1 < kRowsFrame) ? first_lane(rw[row0 + (q + 1 < kRowsFrame ? q + 1 : q)]) : (TIn)0;
  return __ballot(next_lane(rw[row0 + q], next0) > rw[row0 + q]);
}

// first rising step in [0, min(remaining, 1024) - 1)  (SA:2328-2341), a scalar bit scan; takes it off `remaining` when
// there is one.  -> the step, 0 without one
template <typename TIn>
__device__ __forceinline__ int first_rise(const TIn (&rw)[kRowsPair], int row0, int& remaining) {
  const int bound = min(remaining, kMaxSeek) - 1;
  int st = 0;
  bool found = false;
#pragma unroll
  for (int q = 0; q < kMaxSeek / 64; ++q) {
    if (!found && 64 * q < bound) {
      mask64 m = rising_mask(rw, row0, q);
      const int valid = bound - 64 * q;
      if (valid < 64) m &= ((mask64)1 << valid) - 1;
      if (m) { st = 64 * q + __ffsll((long long)m) - 1; found = true; }
    }
  }
  if (found) remaining -= st;
  return st;
}

// next rising step after the minimum period (SA:2343-2356): positions [lo, hi) of the frame.  -> the period, seek_off
// without a step
template <typename TIn>
__device__ __forceinline__ int rise_after_min_period(const TIn (&rw)[kRowsPair], int row0, int st, int remaining, int seek_off) {
  const int bound = min(remaining - seek_off, kMaxSeek) - 1;
  const int lo = st + seek_off, hi = lo + bound;
  int per = seek_off;
  bool found = false;
#pragma unroll
  for (int q = 0; q < kRowsFrame; ++q) {
    if (!found && 64 * q + 63 >= lo && 64 * q < hi) {
      mask64 m = rising_mask(rw, row0, q);
      if (64 * q < lo) m &= ~(((mask64)1 << (lo - 64 * q)) - 1);
      if (hi - 64 * q < 64) m &= ((mask64)1 << (hi - 64 * q)) - 1;
      if (m) { per = seek_off + (64 * q + __ffsll((long long)m) - 1 - lo); found = true; }
    }
  }
  return per;
}

// the two searches of one frame (`exists`: the chunk has it).  remaining: mData.Size() - n, >= 2048 for an emitted frame
template <typename TIn>
__device__ __forceinline__ AcorrFrame find_segment(const TIn (&rw)[kRowsPair], int row0, int remaining, bool exists) {
  const int st = exists ? first_rise(rw, row0, remaining) : 0;
  const int seek_off = min(remaining, kMinPeriod);
  const int per = exists ? rise_after_min_period(rw, row0, st, remaining, seek_off) : seek_off;
  AcorrFrame f;
  f.start = st;
  f.period = per;
  f.active = exists && remaining != 0 && per < remaining;
  f.width = min(remaining, kSeekWidth);
  f.from = per / 2;
  f.off = st & 63;
  return f;
}

// the segment x[start .. start + width) sits in rows start/64 .. start/64 + 9: through the plane, to seg[0 .. 640) (zeros
// for a frame that has no correlation: its half of the transform's input must be clean)
template <bool SCALED, typename TIn>
__device__ __forceinline__ void stage_segment(const TIn (&rw)[kRowsPair], int row0, const AcorrFrame& f, double sc, double* seg, int lane) {
  const int q0 = f.start >> 6;
#pragma unroll
  for (int q = 0; q < 25; ++q)
    if (q >= q0 && q < q0 + 10) seg[64 * (q - q0) + lane] = f.active ? pcm_double<SCALED>(rw[row0 + q], sc) : 0.0;
}

// the lags the circular transform does not give cleanly, summed directly from the staged segments: lane l' = lane & 31
// of half s = lane >> 5 takes k = w - 32 + l' (32 - l' terms) of frame s.  -> the sum, 0 for a lag below 0
__device__ __forceinline__ double direct_upper_lags(const AcorrFrame (&f)[2], const TimeCtx& c) {
  const int hs = c.lane >> 5, lp = c.lane & 31;
  const int w_h = hs ? f[1].width : f[0].width, off_h = hs ? f[1].off : f[0].off;
  const double* const seg_h = c.plane + kAcorrSeg * hs + off_h;
  const int k_h = w_h - kDirect + lp;
  double direct = 0.0;
  const int kk = k_h >= 0 ? k_h : 0;
#pragma unroll 8
  for (int j = 0; j < kDirect; ++j) {
    const double u = seg_h[j], v2 = seg_h[j + kk];     // (within the staged 640: off + 31 + 528 < 640)
    direct = (j < kDirect - lp) ? fma(u, v2, direct) : direct;
  }
  if (k_h < 0) direct = 0.0;
  return direct;
}

// Reads the staged segments as z = a + i b, m = lane + 64 r (zero from w on), and leaves g[r] = 4 N u^2 (r_a[m] + i r_b[m]):
// transform, |2A|^2 + i |2B|^2, transform.  The two frames share one complex transform, whose rounding errors are
// relative to the larger of the two: each segment is brought to [0.5, 1) by a power of two u first (exact, and the result
// -- a ratio of two of its correlation values -- does not see it); `direct` gets the same factors.  live[s]: frame s is
// active and not all zeros.  A segment of zeros has r[0] = 0 and the result 0 (Autocorrelation.cpp:97-105), not rounding
// noise of its partner over rounding noise.
__device__ __forceinline__ void shared_power_transform(const AcorrFrame (&f)[2], const TimeCtx& c, double& direct, cx<double> (&g)[16],
                                                       bool (&live)[2]) {
  const int lane = c.lane;
  cx<double> v[16];
  double mx[2] = {0.0, 0.0};
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = 64 * r + lane;
    v[r] = {0.0, 0.0};
    if (r < 9) {
      v[r] = {(m < f[0].width) ? c.plane[f[0].off + m] : 0.0, (m < f[1].width) ? c.plane[kAcorrSeg + f[1].off + m] : 0.0};
      mx[0] = fmax(mx[0], fabs(v[r].re));
      mx[1] = fmax(mx[1], fabs(v[r].im));
    }
  }
  wave_lds_fence();
  mx[0] = wave_max(mx[0]);
  mx[1] = wave_max(mx[1]);
  live[0] = f[0].active && mx[0] > 0.0;
  live[1] = f[1].active && mx[1] > 0.0;
  const double ua = ldexp(1.0, -__builtin_amdgcn_frexp_exp(mx[0] > 0.0 ? mx[0] : 1.0));
  const double ub = ldexp(1.0, -__builtin_amdgcn_frexp_exp(mx[1] > 0.0 ? mx[1] : 1.0));
#pragma unroll
  for (int r = 0; r < 9; ++r) v[r] = {v[r].re * ua, v[r].im * ub};
  direct *= (lane >> 5) ? ub * ub : ua * ua;
  fft(v, c);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const cx<double> p = partner_of(v, r, c);
    cx<double> e, o;
    even_odd(v[r], p, e, o);                       // 2 A[k], 2 B[k]
    g[r] = {e.re * e.re + e.im * e.im, o.re * o.re + o.im * o.im};
  }
  fft(g, c);
}

template <typename TIn, bool SCALED>
__global__ __launch_bounds__(kTimeWaves * 64) void acorr_kernel(const TimeArgs a) {
  const TimeCtx c = time_setup(a, time_lds());
  const int lane = c.lane;
  const int wave_global = blockIdx.x * kTimeWaves + (threadIdx.x >> 6);
  const int wave_stride = gridDim.x * kTimeWaves;
  const TIn* const pcm = reinterpret_cast<const TIn*>(a.pcm);

  for (int ci = wave_global; ci < a.n_chunks; ci = next_item(a.queue, ci, min(wave_stride, a.n_chunks), wave_stride, lane)) {
    const Chunk ch = a.chunks[ci];
    const double sc = SCALED ? wave_uniform(ch.scale) : 1.0;
    const int remaining0 = a.remaining[ci];
    const TIn* const chunk_pcm = pcm + ch.sample_off;
    // The rows of the next pair are asked for as soon as this pair has staged its segments: they travel while the two
    // transforms run.
    TIn rw[kRowsPair];
    if (kPrefetch<TIn>) load_rows(chunk_pcm, remaining0, 1 < ch.nframes, lane, rw);
    for (int fi = 0; fi < ch.nframes; fi += 2) {
      if (!kPrefetch<TIn>) load_rows(chunk_pcm + (int64_t)fi * kHop, remaining0 - fi * kHop, fi + 1 < ch.nframes, lane, rw);
      const bool have_b = fi + 1 < ch.nframes;
      AcorrFrame f[2];
      wave_lds_fence();
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        f[s] = find_segment(rw, 16 * s, remaining0 - (fi + s) * kHop, s == 0 || have_b);
        stage_segment<SCALED>(rw, 16 * s, f[s], sc, c.plane + kAcorrSeg * s, lane);
      }
      wave_lds_fence();
      // the rows are dead: the next pair's take their registers (the last pair of a chunk re-reads its own)
      if (kPrefetch<TIn>) {
        __builtin_amdgcn_sched_barrier(0);
        const int fn = fi + 2 < ch.nframes ? fi + 2 : fi;
        load_rows(chunk_pcm + (int64_t)fn * kHop, remaining0 - fn * kHop, fn + 1 < ch.nframes, lane, rw);
        __builtin_amdgcn_sched_barrier(0);
      }
      double best[2] = {0.0, 0.0};
      if (f[0].active || f[1].active) {
        double direct = direct_upper_lags(f, c);
        cx<double> g[16];
        bool live[2];
        shared_power_transform(f, c, direct, g, live);
        // best lag: the largest correlation of each frame over the lags [from, w), over r[0], clipped at 0
        // (Autocorrelation.cpp:97-105): the transform's lags below w - 32 from g, the directly summed ones above.  (Here and
        // not a callee: with both this and the transform as callees the compiler contracts other products of the second
        // transform into fused multiply-adds and results move by an ulp, HISTORY 19.)
        const int hs = lane >> 5, lp = lane & 31;
        const double r0a = read_lane<0>(g[0].re) * kAcorrScale, r0b = read_lane<0>(g[0].im) * kAcorrScale;
        // the alias of lag N - (w - 1) when that lag lies below the directly summed ones: r[w - 1], lane l' = 31's sum
        const double last_a = read_lane<31>(direct), last_b = read_lane<63>(direct);
        double top_a = kNoLag, top_b = kNoLag;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
          const int m = 64 * r + lane;
          const double ca = g[r].re * kAcorrScale - ((m == kAcorrN - (f[0].width - 1)) ? last_a : 0.0);
          const double cb = g[r].im * kAcorrScale - ((m == kAcorrN - (f[1].width - 1)) ? last_b : 0.0);
          if (m >= f[0].from && m < f[0].width - kDirect) top_a = fmax(top_a, ca);
          if (m >= f[1].from && m < f[1].width - kDirect) top_b = fmax(top_b, cb);
        }
        // the directly summed lags of each half
        const int k_h = (hs ? f[1].width : f[0].width) - kDirect + lp;
        const int from_h = hs ? f[1].from : f[0].from;
        const double dtop = (k_h >= 0 && k_h >= from_h) ? direct : kNoLag;
        top_a = fmax(top_a, hs ? kNoLag : dtop);
        top_b = fmax(top_b, hs ? dtop : kNoLag);
        top_a = wave_max(top_a);
        top_b = wave_max(top_b);
        if (r0a != 0.0) top_a /= r0a;                    // Autocorrelation.cpp:97-105
        if (r0b != 0.0) top_b /= r0b;
        best[0] = live[0] ? fmax(0.0, top_a) : 0.0;
        best[1] = live[1] ? fmax(0.0, top_b) : 0.0;
      }
      if (lane == 0) {
        a.rec[((int64_t)ch.frame0 + fi) * a.lay.stride + a.lay.autocorr] = best[0];
        if (have_b) a.rec[((int64_t)ch.frame0 + fi + 1) * a.lay.stride + a.lay.autocorr] = best[1];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// f0 + confidence: aubio yinfast on the 2048-sample frame
// ---------------------------------------------------------------------------------------------
// r_t(tau) = sum_{j<W} x[j] x[j+tau], tau < W, as conj(U) X: U = spectrum of the zero-padded first half, X = spectrum of
// the frame = U + (-1)^k Un with Un the spectrum of the zero-padded second half.  The second half is the next frame's
// first half, so each frame costs one forward transform.
// The loads of a frame are issued long before they are used (two waves per SIMD hide little: every exposed load was ~a
// microsecond of an idle vector ALU): the second half of frame fi + 1 -- the only new samples of a frame -- travels
// during the whole of frame fi (nx), the blocked copies for the squared-difference terms during the inverse transform.
template <typename TIn>
struct PairOf;
template <>
struct PairOf<float> { using type = float2; };
template <>
struct PairOf<double> { using type = double2; };

constexpr int kYinW = kFft / 2;
constexpr double kYinTol = 0.75;                 // MPitchTolerance, SA:62, 801
constexpr int kNoDip = 1 << 30;

// nx[r] = the packed pair m = lane + 64 r of the half frame at p, as loaded
template <typename TIn>
__device__ __forceinline__ void load_half(const TIn* p, int lane, typename PairOf<TIn>::type (&nx)[8]) {
  const typename PairOf<TIn>::type* src = reinterpret_cast<const typename PairOf<TIn>::type*>(p) + lane;
#pragma unroll
  for (int r = 0; r < 8; ++r) nx[r] = src[64 * r];
}

// z = the zero-padded half frame nx as doubles (packed z[m] = x[2m] + i x[2m+1])
template <bool SCALED, typename Pair>
__device__ __forceinline__ void zero_padded(const Pair (&nx)[8], double sc, cx<double> (&z)[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    z[r] = {0.0, 0.0};
    if (r < 8) z[r] = {pcm_double<SCALED>(nx[r].x, sc), pcm_double<SCALED>(nx[r].y, sc)};
  }
}

// chunk prologue: zu = transform of the zero-padded first half of the chunk's first frame; with kPrefetch its second
// half is on its way in nx
template <bool SCALED, typename TIn>
__device__ __forceinline__ void first_half_transform(const TIn* chunk_pcm, double sc, const TimeCtx& c, cx<double> (&zu)[16],
                                                     typename PairOf<TIn>::type (&nx)[8]) {
  {
    typename PairOf<TIn>::type first[8];
    load_half(chunk_pcm, c.lane, first);
    zero_padded<SCALED>(first, sc, zu);
  }
  if (kPrefetch<TIn>) load_half(chunk_pcm + kYinW, c.lane, nx);
  fft(zu, c);
}

// zn = the zero-padded second half of frame fi, from nx (loaded here without kPrefetch); with kPrefetch nx then takes
// the next frame's second half (the last frame of a chunk re-reads its own: no branch, nothing is read beyond what the
// chunk's frames cover)
template <bool SCALED, typename TIn>
__device__ __forceinline__ void next_half(const TIn* chunk_pcm, int fi, int nframes, double sc, int lane,
                                          typename PairOf<TIn>::type (&nx)[8], cx<double> (&zn)[16]) {
  if (!kPrefetch<TIn>) load_half(chunk_pcm + (int64_t)fi * kHop + kYinW, lane, nx);
  zero_padded<SCALED>(nx, sc, zn);
  if (kPrefetch<TIn>) {
    __builtin_amdgcn_sched_barrier(0);
    const int fn = (fi + 1 < nframes) ? fi + 1 : fi;
    load_half(chunk_pcm + (int64_t)fn * kHop + kYinW, lane, nx);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// C = conj(U) X at k and at 1024-k, then the packed spectrum of the inverse: Zc = Ec + i Oc,
// Ec = (C + conj(C'))/2, Oc = (C - conj(C'))/2 conj(w^k).  The factors 1/2 are carried along instead of
// applied (2E, 2O, 2U, 2X, 4C, 8 Zc: exact) and undone with the 1/1024 of the inverse.
// Bins k and 1024 - k share every intermediate (U[k'] = Up, X[k'] = Xp, the roles of C and Cp swap, w[k'] = -conj(w)):
// the output at k' is {ec.re + oc.im, ec.im - oc.re} where the output at k is {ec.re - oc.im, -(ec.im + oc.re)}.
// zu_k, zn_k: the two packed transforms at k, pu, pn: at 1024 - k, w = w2048^k, sign = (-1)^k.
__device__ __forceinline__ void pair_product(double sign, const cx<double>& zu_k, const cx<double>& pu, const cx<double>& zn_k,
                                             const cx<double>& pn, const cx<double>& w, cx<double>& at_k, cx<double>& at_partner) {
  cx<double> e, o, en, on;
  even_odd(zu_k, pu, e, o);
  even_odd(zn_k, pn, en, on);
  const cx<double> wo = cmul(w, o), won = cmul(w, on);
  const cx<double> U{e.re + wo.re, e.im + wo.im};
  const cx<double> Up{e.re - wo.re, -(e.im - wo.im)};                  // U[1024-k] = conj(E - w O)
  const cx<double> X{U.re + sign * (en.re + won.re), U.im + sign * (en.im + won.im)};
  const cx<double> Xp{Up.re + sign * (en.re - won.re), Up.im - sign * (en.im - won.im)};
  const cx<double> C{U.re * X.re + U.im * X.im, U.re * X.im - U.im * X.re};
  const cx<double> Cp{Up.re * Xp.re + Up.im * Xp.im, Up.re * Xp.im - Up.im * Xp.re};
  const cx<double> ec{C.re + Cp.re, C.im - Cp.im};
  const cx<double> d{C.re - Cp.re, C.im + Cp.im};
  const cx<double> oc{d.re * w.re + d.im * w.im, d.im * w.re - d.re * w.im};
  at_k = {ec.re - oc.im, -(ec.im + oc.re)};      // conj(8 Zc)
  at_partner = {ec.re + oc.im, ec.im - oc.re};
}

// pair_product at k = lane + 64 r, r < 8, with the partner bins fetched from lane 64 - lane's registers 15 - r
__device__ __forceinline__ void correlation_at(int r, double sign, const cx<double> (&zu)[16], const cx<double> (&zn)[16], const TimeCtx& c,
                                               cx<double>& at_k, cx<double>& at_partner) {
  const cx<double> pu = partner_of(zu, r, c), pn = partner_of(zn, r, c);
  pair_product(sign, zu[r], pu, zn[r], pn, c.post[64 * r], at_k, at_partner);
}

// g[15 - j] = the partner lane's gp[j]: what it computed for this lane's bin 1024 - k.  Lane 0's bins pair among
// themselves (64 r with 64 (16 - r)): its delivered registers are shifted by one and its bin 512 is its own partner.
__device__ __forceinline__ void deliver_partners(const cx<double> (&gp)[8], const cx<double>& g512, const TimeCtx& c, cx<double> (&g)[16]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    g[15 - j] = {__shfl(gp[j].re, c.partner), __shfl(gp[j].im, c.partner)};
    if (c.lane == 0) g[15 - j] = (j < 7) ? gp[j + 1] : g512;
  }
}

// the frame's samples in the blocked layout (16 consecutive per lane) for the squared-difference terms: asked for in
// front of the inverse transform, used behind it
template <typename TIn>
__device__ __forceinline__ void request_blocked(const TIn* x, int lane, Block16<TIn>& qa, Block16<TIn>& qb) {
  qa.load(x + 16 * lane);
  qb.load(x + kYinW + 16 * lane);
}

// g: the inverse transform's output, c[2m] = Re F[m] / 1024, c[2m+1] = -Im F[m] / 1024 (and the carried factor 8),
// m = lane + 64 r; tau < 1024 <=> r < 8.  Leaves corr[i] = c[16 lane + i], through the plane.
__device__ __forceinline__ void to_blocked(const cx<double> (&g)[16], const TimeCtx& c, double (&corr)[16]) {
  wave_lds_fence();
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int t = 2 * (64 * r + c.lane);
    c.plane[pad_slot(t)] = g[r].re * (1.0 / 8192.0);
    c.plane[pad_slot(t) + 1] = -g[r].im * (1.0 / 8192.0);
  }
  wave_lds_fence();
#pragma unroll
  for (int i = 0; i < 16; ++i) corr[i] = c.plane[17 * c.lane + i];
  wave_lds_fence();
}

// xa, xb = the two halves of the frame in the blocked layout, as doubles (loaded here without kPrefetch)
template <bool SCALED, typename TIn>
__device__ __forceinline__ void blocked_samples(const TIn* x, double sc, int lane, Block16<TIn>& qa, Block16<TIn>& qb,
                                                double (&xa)[16], double (&xb)[16]) {
  if (!kPrefetch<TIn>) request_blocked(x, lane, qa, qb);
  qa.get(xa);
  qb.get(xb);
  scale16<SCALED>(xa, sc);
  scale16<SCALED>(xb, sc);
}

// the squares of the squared-difference terms (pitchyinfast.c:96-117): squares xa, xb in place and leaves the halves'
// sums of squares s0, s1
__device__ __forceinline__ void square_halves(double (&xa)[16], double (&xb)[16], double& s0, double& s1) {
  s0 = 0.0;
  s1 = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    xa[i] *= xa[i];
    xb[i] *= xb[i];
    s0 += xa[i];
    s1 += xb[i];
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
}

// cumulative mean normalisation (pitchyinfast.c:146-153), yin in place
__device__ __forceinline__ void cumulative_mean_normalise(double (&yin)[16], int lane) {
  double cum[16], run = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (16 * lane + i > 0) run += yin[i];
    cum[i] = run;
  }
  const double cum_before = wave_scan_incl(run, lane) - run;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int tau = 16 * lane + i;
    const double tmp2 = cum_before + cum[i];
    // yin[tau] *= tau / tmp2 (pitchyinfast.c:148-150); tmp2 >= 0 is a sum of a^2 + b^2 - ab terms
    yin[i] = (tau == 0) ? 1.0 : ((tmp2 != 0) ? yin[i] * fast_div((double)tau, tmp2) : 1.0);
  }
}

// the (last) global minimum of yin, for a frame without a dip below the tolerance (pitchyinfast.c:161-163).  -> its tau
__device__ __forceinline__ int last_minimum(const double (&yin)[16], int lane) {
  double m = yin[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) m = fmin(m, yin[i]);
  m = wave_min(m);
  int last = -1;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (yin[i] == m) last = 16 * lane + i;
  const int pos = wave_max_i(last);
  return pos < 0 ? 0 : pos;
}

// fvec_quadratic_peak_pos (mathutils.c:494-506) around pos, and the confidence read back from the normalised buffer,
// which goes through the plane for it.  Leaves the period and 1 - yin[(uint) period]
__device__ __forceinline__ void quadratic_peak_and_confidence(const double (&yin)[16], int pos, const TimeCtx& c, double& period,
                                                              double& conf_raw) {
  wave_lds_fence();
#pragma unroll
  for (int i = 0; i < 16; ++i) c.plane[17 * c.lane + i] = yin[i];
  wave_lds_fence();
  period = (double)pos;
  if (pos != 0 && pos != kYinW - 1) {
    const double y0 = c.plane[pad_slot(pos - 1)], y1 = c.plane[pad_slot(pos)], y2 = c.plane[pad_slot(pos + 1)];
    period = (double)pos + 0.5 * (y0 - y2) / (y0 - 2.0 * y1 + y2);
  }
  // o->peak_pos is a uint_t (pitchyinfast.c:38, 160-169); out-of-range casts are undefined there, clamped here
  int at = (period >= 0.0 && period < (double)kYinW) ? (int)period : (period < 0.0 ? 0 : kYinW - 1);
  if (!(period == period)) at = 0;
  conf_raw = 1.0 - c.plane[pad_slot(at)];
  wave_lds_fence();
}

// f0 from the period (pitch.c:450-462), 0 for a silent frame (pitch.c:399-406); the confidence over
// MMaxPitchConfidenceValue clipped to [0, 1] (SA:886-895); from lane 0 into rec
__device__ __forceinline__ void store_pitch(double period, double conf_raw, double s0, double s1, const RecordLayout& lay, double* rec,
                                            int lane) {
  double f0 = (period > 0.0) ? (double)kSampleRate / (period + 0.) : 0.0;
  if (au_silent(s0 + s1, kFft)) f0 = 0.0;
  double conf = conf_raw / 0.25;
  conf = (conf < 0.0) ? 0.0 : (conf > 1.0 ? 1.0 : conf);
  if (!(conf == conf)) conf = 0.0;
  if (lane == 0) {
    rec[lay.f0] = nan_to_zero(f0);
    rec[lay.f0_conf] = conf;
    // hop silence (SA:865-868) parked in the fail-safe slot for afx_whiten.hip, which replaces it
    rec[lay.f0_safe] = au_silent(s0, kHop) ? 1.0 : 0.0;
  }
}

template <typename TIn, bool SCALED>
__global__ __launch_bounds__(kTimeWaves * 64) void pitch_kernel(const TimeArgs a) {
  TimeLds& lds = time_lds();
  const TimeCtx c = time_setup(a, lds);
  const int lane = c.lane;
  const int wave_global = blockIdx.x * kTimeWaves + (threadIdx.x >> 6);
  const int wave_stride = gridDim.x * kTimeWaves;
  const TIn* const pcm = reinterpret_cast<const TIn*>(a.pcm);
  // the envelope's constants in LDS (hop_descriptors)
  const double env_coef = envelope_coef();
  if (a.hop_here && threadIdx.x == 0) {
    double pw = 1.0;
    for (int i = 0; i <= 16; ++i) { lds.env_pow[i] = pw; pw *= env_coef; }
  }
  if (a.hop_here && threadIdx.x < 64) lds.env_scan[threadIdx.x] = envelope_scan(env_coef, threadIdx.x);
  __syncthreads();

  for (int ci = wave_global; ci < a.n_chunks; ci = next_item(a.queue, ci, min(wave_stride, a.n_chunks), wave_stride, lane)) {
    const Chunk ch = a.chunks[ci];
    const double sc = SCALED ? wave_uniform(ch.scale) : 1.0;
    const TIn* const chunk_pcm = pcm + ch.sample_off;
    cx<double> zu[16];                      // transform of the frame's zero-padded first half
    typename PairOf<TIn>::type nx[8];       // second half of the frame in front
    first_half_transform<SCALED>(chunk_pcm, sc, c, zu, nx);
    for (int fi = 0; fi < ch.nframes; ++fi) {
      const TIn* const x = chunk_pcm + (int64_t)fi * kHop;
      double* const rec = a.rec + ((int64_t)ch.frame0 + fi) * a.lay.stride;

      cx<double> zn[16];
      next_half<SCALED>(chunk_pcm, fi, ch.nframes, sc, lane, nx, zn);
      fft(zn, c);
      // correlation spectrum: g = conj(8 Zc), the input of the inverse transform.  A lane works on half of its bins
      // (registers 0..7) and hands the partner lane the other output of each pair -- lane l's register r pairs with lane
      // 64 - l's register 15 - r --, instead of both lanes computing both.  (The loop stands here: as a callee it costs
      // 120 B of scratch, HISTORY 19.)
      const double sign = (lane & 1) ? -1.0 : 1.0;      // (-1)^k, k = lane + 64 r (1024 - k has the same parity)
      cx<double> g[16], gp[8], g512, unused;
#pragma unroll
      for (int r = 0; r < 8; ++r) correlation_at(r, sign, zu, zn, c, g[r], gp[r]);
      pair_product(sign, zu[8], zu[8], zn[8], zn[8], c.post[64 * 8], g512, unused);     // lane 0's bin 512 (the other lanes' result is dropped)
      deliver_partners(gp, g512, c, g);
      // the second half's transform is the next frame's first-half transform
#pragma unroll
      for (int r = 0; r < 16; ++r) zu[r] = zn[r];
      Block16<TIn> qa, qb;
      if (kPrefetch<TIn>) {
        __builtin_amdgcn_sched_barrier(0);
        request_blocked(x, lane, qa, qb);
        __builtin_amdgcn_sched_barrier(0);
      }
      fft(g, c);
      double corr[16], xa[16], xb[16];
      to_blocked(g, c, corr);
      blocked_samples<SCALED>(x, sc, lane, qa, qb, xa, xb);
      // the hop's own descriptors (silence flag, envelope, amplitude: hop_kernel's, SA:865-872, 1760-1804): a batch that
      // computes f0 does not launch a kernel and read the PCM from HBM once more for them; here, where the hop is in
      // registers in the blocked layout anyway
      if (a.hop_here) hop_descriptors(xa, hop_energy(xa), env_coef, lds.env_pow, lds.env_scan[lane], a.amplitude, a.lay, rec, lane);
      double s0, s1, period, conf_raw;
      square_halves(xa, xb, s0, s1);
      // squared differences (pitchyinfast.c:96-117): yin[i] = sqdiff[tau] - r_t[tau], tau = 16 lane + i, with
      // sqdiff[tau] = sum_{j<W} x[j+tau]^2 + sum_{j<W} x[j]^2 = 2 s0 + sum_{j<tau} (x[W+j]^2 - x[j]^2).  (Here and not a
      // callee: that costs nine instructions, HISTORY 19.)
      double yin[16], run = 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        yin[i] = run;
        run += xb[i] - xa[i];
      }
      const double before = wave_scan_incl(run, lane) - run;
      // aubio's Ooura back end returns the inverse transform halved (spectral/fft.c:464-476: scale 1/N where
      // rdft needs 2/N), so "sqdiff - 2 r_t" is sqdiff - r_t in the reference's results
#pragma unroll
      for (int i = 0; i < 16; ++i) yin[i] = (2.0 * s0 + (before + yin[i])) - 2.0 * (0.5 * corr[i]);
      cumulative_mean_normalise(yin, lane);
      // first dip below the tolerance, else the (last) global minimum (pitchyinfast.c:154-163).  (The search stands
      // here: as a callee it costs eleven instructions and a register of <double, false>.)
      const double nxt = next_lane(yin[0], yin[0]);
      int first = kNoDip;
#pragma unroll
      for (int i = 15; i >= 0; --i) {
        const int p = 16 * lane + i;
        const double hi = (i == 15) ? nxt : yin[i + 1];
        if (p >= 2 && p + 3 < kYinW && yin[i] < kYinTol && yin[i] < hi) first = p;
      }
      first = wave_min_i(first);
      int pos = first;
      if (first == kNoDip) pos = last_minimum(yin, lane);
      quadratic_peak_and_confidence(yin, pos, c, period, conf_raw);
      store_pitch(period, conf_raw, s0, s1, a.lay, rec, lane);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
using TimeKernel = void (*)(TimeArgs);

// the <TIn, SCALED> instantiation of a kernel template for the arena's sample type
TimeKernel for_pcm(int pcm_dtype, TimeKernel f32, TimeKernel scaled_f32, TimeKernel f64) {
  return (pcm_dtype == kPcmF32) ? f32 : ((pcm_dtype == kPcmScaledF32) ? scaled_f32 : f64);
}

// Raises the kernel's dynamic LDS limit to kTimeLdsBytes, once per device and kernel: six kernels ask (acorr_kernel and
// pitch_kernel, three sample types each); a device number beyond the record asks every time.
hipError_t raise_lds_limit(TimeKernel kernel) {
  struct Raised { TimeKernel kernel; bool on_device[16]; };
  static Raised raised[6] = {};
  static std::mutex guard;
  int dev = 0;
  (void)hipGetDevice(&dev);
  const bool recorded = dev >= 0 && dev < 16;
  std::lock_guard<std::mutex> lock(guard);
  Raised* r = raised;
  while (r < raised + 5 && r->kernel && r->kernel != kernel) ++r;
  if (recorded && r->kernel == kernel && r->on_device[dev]) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kTimeLdsBytes);
  if (e != hipSuccess) return e;
  if (recorded && (!r->kernel || r->kernel == kernel)) {
    r->kernel = kernel;
    r->on_device[dev] = true;
  }
  return hipSuccess;
}

// hop_kernel: four chunks per workgroup, at most 2048 workgroups
int hop_grid(int n_chunks) { return (n_chunks + 3) / 4 < 2048 ? (n_chunks + 3) / 4 : 2048; }

// acorr_kernel, pitch_kernel: a workgroup per compute unit at most (their waves take further chunks from the queue)
int time_grid(int n_chunks, int waves) {
  int cus = 256;
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
  }
  const int want = (n_chunks + waves - 1) / waves;
  return want < cus ? (want < 1 ? 1 : want) : cus;
}

// a kernel that uses TimeLds
hipError_t launch_with_planes(TimeKernel kernel, const TimeArgs& a, hipStream_t stream) {
  if (a.n_chunks <= 0) return hipSuccess;
  const hipError_t e = raise_lds_limit(kernel);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(time_grid(a.n_chunks, kTimeWaves)), dim3(kTimeWaves * 64), kTimeLdsBytes, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_hop(const TimeArgs& a, hipStream_t stream) {
  if (a.n_chunks <= 0) return hipSuccess;
  const TimeKernel k = for_pcm(a.pcm_dtype, hop_kernel<float, false>, hop_kernel<float, true>, hop_kernel<double, false>);
  hipLaunchKernelGGL(k, dim3(hop_grid(a.n_chunks)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_acorr(const TimeArgs& a, hipStream_t stream) {
  return launch_with_planes(for_pcm(a.pcm_dtype, acorr_kernel<float, false>, acorr_kernel<float, true>, acorr_kernel<double, false>), a, stream);
}

hipError_t launch_pitch(const TimeArgs& a, hipStream_t stream) {
  return launch_with_planes(for_pcm(a.pcm_dtype, pitch_kernel<float, false>, pitch_kernel<float, true>, pitch_kernel<double, false>), a, stream);
}

}  // namespace afx
