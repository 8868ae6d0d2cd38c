// Device vocoder: the codec's STFT pair, Audio2Mel (audio_codecs.py:107-143) and a fast Griffin-Lim phase
// reconstruction over it (Perraudin et al. 2013, the momentum form) -- a stand-in for the reference's mel -> audio
// stage, NOT SoundStream (audio_codecs.py:249-264: a learned vocoder whose artifact is absent).
// Specification: stft / istft / mel_to_linear / griffin_lim of audio_codecs.py (float64 NumPy).
//
// Geometry (audio_codecs.MelGAN): frame 640, hop 320, FFT 1024 -> 513 bins, periodic Hann, pad_end framing
// (frame k = samples [320k, 320k + 640) of the zero-extended signal), F = ceil(n / 320) frames, 128 mel bins.
//
// Both DFTs and both mel products are exact-fp32 GEMMs on gemm_f32_kernel (gemm_f32.h):
//   forward  Y[row][:]  = audio[320 row .. +640) . Bf,  Bf [640, 1088]:  w[n] cos(2 pi k n / 1024) | -w[n] sin(..)
//   inverse  fr[row][:] = X[row][:] . Bi,               Bi [1088, 640]:  c_k / 1024 (cos | -sin) w[n], c_0 = c_512 = 1, else 2
// Framing costs nothing: A is the padded signal itself with lda = 320, K = 640.  Songs are batched in one launch by giving
// each (F + 1) * 320 samples (the last 320 zero): row b (F + 1) + k is frame k of song b, the row k = F straddles two
// songs and is never read back; a launch covers B (F + 1) - 1 rows.
// A spectrum row is 1088 floats: real parts at [0, 513), imaginary parts at [544, 1057), zeros between (the basis
// columns / rows there are zero) -- both halves start 16-byte aligned, so the elementwise kernels move float4s.
// A magnitude row is 544 floats (513 bins, zeros behind).
// One Griffin-Lim iteration is four launches: inverse GEMM, overlap-add, forward GEMM, phase update.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "common.h"
#include "gemm_f32.h"

namespace msd {

constexpr int kVocFrame = 640, kVocHop = 320, kVocFft = 1024, kVocBins = 513, kVocMel = 128;
constexpr int kVocHalf = 544;            // columns of one part (re or im) of a spectrum row; a magnitude row
constexpr int kVocSpec = 2 * kVocHalf;   // 1088 = 17 * 64
constexpr int kVocG4 = kVocHalf / 4;     // float4 groups of one part
constexpr int kVocMelInvN = 576;         // 513 columns of pinv(mel basis), padded to a multiple of 64
constexpr float kVocOlaFloor = 1e-3f;    // istft(floor=): the first samples divide by a vanishing window

// ---- GEMM epilogues ---------------------------------------------------------------------------------------------
// forward DFT -> the public layout [B, F, 2, 513] (re | im); internal row m = b (F + 1) + k
struct EpiVocSpecOut {
  float* out;
  int F;
  __device__ void operator()(int m, int n, float v) const {
    const int b = m / (F + 1), k = m - b * (F + 1);
    const int part = n >= kVocHalf ? 1 : 0, bin = n - part * kVocHalf;
    if (k < F && bin < kVocBins) out[(((size_t)b * F + k) * 2 + part) * kVocBins + bin] = v;
  }
};
// mel product of the encoder -> log(clip(., 1e-5, 1e8)) (audio_codecs.py:141-143), rows compacted to [B, F, 128].
// The logarithm is taken in double and rounded once: half an ulp of a value near log 1e-5 = -11.5 is already 2^-21
// relative on the linear mel, and there are only 128 of them per frame.
struct EpiVocLogMel {
  float* out;
  int F;
  __device__ void operator()(int m, int n, float v) const {
    const int b = m / (F + 1), k = m - b * (F + 1);
    if (k < F) out[((size_t)b * F + k) * kVocMel + n] = (float)log((double)fminf(fmaxf(v, 1e-5f), 1e8f));
  }
};
// mel_to_linear: max(., 0) into the magnitude rows; input row m = b F + k (the caller's [B, F, 128])
struct EpiVocClampMag {
  float* mag;
  int F;
  __device__ void operator()(int m, int n, float v) const {
    const int b = m / F, k = m - b * F;
    if (n < kVocBins) mag[((size_t)b * (F + 1) + k) * kVocHalf + n] = fmaxf(v, 0.f);
  }
};

// ---- elementwise kernels (one float4 per thread and stream; none may spill: build_native.NO_SCRATCH_KERNELS) ------
// [B, n] -> [B, (F + 1) * 320], zero-extended.  grid (ceil(per_song / 1024), B)
__global__ void __launch_bounds__(256) voc_pad_signal_kernel(const float* __restrict__ in, float* __restrict__ out, int n,
                                                             int per_song) {
  const int s = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (s >= per_song) return;
  const float* src = in + (size_t)blockIdx.y * n;
  float4 v;
  v.x = s < n ? src[s] : 0.f;
  v.y = s + 1 < n ? src[s + 1] : 0.f;
  v.z = s + 2 < n ? src[s + 2] : 0.f;
  v.w = s + 3 < n ? src[s + 3] : 0.f;
  *reinterpret_cast<float4*>(out + (size_t)blockIdx.y * per_song + s) = v;
}

__global__ void __launch_bounds__(256) voc_exp_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = reinterpret_cast<const float4*>(in)[i];
  reinterpret_cast<float4*>(out)[i] = make_float4(expf(v.x), expf(v.y), expf(v.z), expf(v.w));
}

// (cos, sin) of the direction of (a, b); (1, 0) for the zero vector.  The pair is scaled by a power of two first so that
// neither square leaves the float range (a bin of a silent frame is denormal, not zero); one rsqrt is the normalisation.
// A vector on an axis has an exact direction and gets it -- the rsqrt is within one ulp, and 0.75 * rsq(0.5625) came out
// as 1 - 2^-24: the DC and Nyquist bins of every frame lie on the real axis (their imaginary parts are exact zeros).
__device__ __forceinline__ void voc_unit(float a, float b, float& c, float& s) {
  const float m = fmaxf(fabsf(a), fabsf(b));
  const int e = (int)((__float_as_uint(m) >> 23) & 0xffu);
  const float sc = __uint_as_float((uint32_t)max(253 - e, 1) << 23);   // 2^(126 - e'): m * sc in [1/4, 4)
  a *= sc;
  b *= sc;
  const float n2 = a * a + b * b;
  const float r = __builtin_amdgcn_rsqf(n2);
  c = n2 > 0.f ? (b == 0.f ? copysignf(1.f, a) : a * r) : 1.f;
  s = n2 > 0.f ? (a == 0.f ? copysignf(1.f, b) : b * r) : 0.f;
}

// src [B, F, 2, 513] (a spectrum, or cos | sin of a phase) -> spectrum rows X [B (F + 1), 1088], times the magnitude
// rows when mag != NULL; normalise: src holds pairs of normal draws, brought to the unit circle first.  The straddling
// rows and the pad columns come out zero.  One thread per float4 group of a part.
__global__ void __launch_bounds__(256) voc_load_spec_kernel(const float* __restrict__ src, const float* __restrict__ mag,
                                                            float* __restrict__ X, int F, int rows, int normalise) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int row = idx / kVocG4, g = idx - row * kVocG4;
  if (row >= rows) return;
  const int b = row / (F + 1), k = row - b * (F + 1);
  float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
  if (k < F) {
    const float* p = src + ((size_t)b * F + k) * 2 * kVocBins;
    float4 mg = make_float4(1.f, 1.f, 1.f, 1.f);
    if (mag != nullptr) mg = *reinterpret_cast<const float4*>(mag + (size_t)row * kVocHalf + 4 * g);
    const float mm[4] = {mg.x, mg.y, mg.z, mg.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int bin = 4 * g + j;
      if (bin < kVocBins) {
        float c = p[bin], s = p[kVocBins + bin];
        if (normalise) voc_unit(c, s, c, s);
        re[j] = mm[j] * c;
        im[j] = mm[j] * s;
      }
    }
  }
  float* x = X + (size_t)row * kVocSpec + 4 * g;
  *reinterpret_cast<float4*>(x) = make_float4(re[0], re[1], re[2], re[3]);
  *reinterpret_cast<float4*>(x + kVocHalf) = make_float4(im[0], im[1], im[2], im[3]);
}

// Overlap-add + normalise: a gather of the two frames that cover a sample (no atomics).  frames [B (F + 1), 640] already
// carry the synthesis window (folded into Bi); inv_norm [2][320] = 1 / max(sum w^2, floor) for the first hop (one tap)
// and for every later one (two).  out: song stride `out_stride`; samples [F * 320, per_song) are written as zeros (the
// zero extension of the padded signal; per_song = F * 320 when out is the caller's).  grid (ceil(per_song / 1024), B)
__global__ void __launch_bounds__(256) voc_ola_kernel(const float* __restrict__ frames, const float* __restrict__ inv_norm,
                                                      float* __restrict__ out, int F, int per_song, size_t out_stride) {
  const int s = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (s >= per_song) return;
  const int k0 = s / kVocHop, o = s - k0 * kVocHop;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (k0 < F) {
    const float* fr = frames + ((size_t)blockIdx.y * (F + 1) + k0) * kVocFrame + o;
    const float4 a = *reinterpret_cast<const float4*>(fr);
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k0 > 0) b = *reinterpret_cast<const float4*>(fr - kVocFrame + kVocHop);
    const float4 w = *reinterpret_cast<const float4*>(inv_norm + (k0 > 0 ? kVocHop : 0) + o);
    v = make_float4((a.x + b.x) * w.x, (a.y + b.y) * w.y, (a.z + b.z) * w.z, (a.w + b.w) * w.w);
  }
  *reinterpret_cast<float4*>(out + (size_t)blockIdx.y * out_stride + s) = v;
}

// Phase update of fast Griffin-Lim: U = Y - alpha Y_prev, X = mag U / |U| ((1, 0) where U = 0).  Y_prev is the other
// half of a ping-pong pair, so nothing is copied.  Pad columns: Y = 0 there and mag = 0, so X = 0.
__global__ void __launch_bounds__(256) voc_phase_kernel(const float* __restrict__ Y, const float* __restrict__ Yprev,
                                                        const float* __restrict__ mag, float* __restrict__ X, int rows,
                                                        float alpha) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int row = idx / kVocG4, g = idx - row * kVocG4;
  if (row >= rows) return;
  const size_t at = (size_t)row * kVocSpec + 4 * g;
  const float4 yr = *reinterpret_cast<const float4*>(Y + at), yi = *reinterpret_cast<const float4*>(Y + at + kVocHalf);
  const float4 pr = *reinterpret_cast<const float4*>(Yprev + at), pi = *reinterpret_cast<const float4*>(Yprev + at + kVocHalf);
  const float4 mg = *reinterpret_cast<const float4*>(mag + (size_t)row * kVocHalf + 4 * g);
  const float ur[4] = {yr.x - alpha * pr.x, yr.y - alpha * pr.y, yr.z - alpha * pr.z, yr.w - alpha * pr.w};
  const float ui[4] = {yi.x - alpha * pi.x, yi.y - alpha * pi.y, yi.z - alpha * pi.z, yi.w - alpha * pi.w};
  const float mm[4] = {mg.x, mg.y, mg.z, mg.w};
  float re[4], im[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float c, s;
    voc_unit(ur[j], ui[j], c, s);
    re[j] = mm[j] * c;
    im[j] = mm[j] * s;
  }
  *reinterpret_cast<float4*>(X + at) = make_float4(re[0], re[1], re[2], re[3]);
  *reinterpret_cast<float4*>(X + at + kVocHalf) = make_float4(im[0], im[1], im[2], im[3]);
}

// |Y| of the encoder: spectrum rows -> magnitude rows (pad columns: sqrt(0) = 0)
__global__ void __launch_bounds__(256) voc_magnitude_kernel(const float* __restrict__ Y, float* __restrict__ mag, int rows) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int row = idx / kVocG4, g = idx - row * kVocG4;
  if (row >= rows) return;
  const size_t at = (size_t)row * kVocSpec + 4 * g;
  const float4 a = *reinterpret_cast<const float4*>(Y + at), b = *reinterpret_cast<const float4*>(Y + at + kVocHalf);
  *reinterpret_cast<float4*>(mag + (size_t)row * kVocHalf + 4 * g) =
      make_float4(sqrtf(a.x * a.x + b.x * b.x), sqrtf(a.y * a.y + b.y * b.y), sqrtf(a.z * a.z + b.z * b.z),
                  sqrtf(a.w * a.w + b.w * b.w));
}

}  // namespace msd

// ---- the handle ---------------------------------------------------------------------------------------------------
namespace msd {
// work buffers, floats per spectrum row (rows = B (F + 1))
enum VocBuf { VB_AUDIO, VB_X, VB_Y0, VB_Y1, VB_FRAMES, VB_MAG, VB_LIN, VB_DRAWS, VB_COUNT };
constexpr size_t kVocPerRow[VB_COUNT] = {kVocHop,     // padded signals
                                         kVocSpec,    // X: the spectrum estimate, A of the inverse GEMM
                                         kVocSpec, kVocSpec,   // Y and Y_prev (ping-pong)
                                         kVocFrame,   // windowed frames
                                         kVocHalf,    // target magnitudes
                                         kVocMel,     // exp(log-mel)
                                         2 * kVocBins};   // phase draws / normalised phases [B, F, 2, 513]
}  // namespace msd

struct msd_vocoder {
  std::string err;
  float* fwd = nullptr;        // Bf [640, 1088]
  float* inv = nullptr;        // Bi [1088, 640]
  float* mel = nullptr;        // mel basis [544, 128] (rows >= 513 zero)
  float* mel_inv = nullptr;    // pinv(mel basis) [128, 576] (columns >= 513 zero)
  float* inv_norm = nullptr;   // [2][320]
  size_t cap_rows = 0;
  size_t last_rows = 0;        // spectrum rows of the last call (msd_vocoder_debug_read)
  float* w[msd::VB_COUNT] = {};
};

namespace msd {

inline void voc_free_work(msd_vocoder* v) {
  for (float*& p : v->w) { if (p) (void)hipFree(p); p = nullptr; }
  v->cap_rows = 0;
}

// grow the work buffers to `rows` spectrum rows; new buffers are cleared on `s`
inline bool voc_reserve(msd_vocoder* v, size_t rows, hipStream_t s) {
  if (rows <= v->cap_rows) return true;
  voc_free_work(v);
  for (int i = 0; i < VB_COUNT; ++i) {
    const size_t bytes = rows * kVocPerRow[i] * sizeof(float);
    if (hipMalloc(reinterpret_cast<void**>(&v->w[i]), bytes) != hipSuccess || hipMemsetAsync(v->w[i], 0, bytes, s) != hipSuccess) {
      voc_free_work(v);
      return false;
    }
  }
  v->cap_rows = rows;
  return true;
}

// the two DFT bases and the overlap-add normalisation, in double, stored as float32
inline void voc_host_tables(std::vector<float>& fwd, std::vector<float>& inv, std::vector<float>& inv_norm) {
  const double two_pi = 6.283185307179586476925286766559;
  std::vector<double> w(kVocFrame), cs(kVocFft), sn(kVocFft);
  for (int n = 0; n < kVocFrame; ++n) w[n] = 0.5 - 0.5 * std::cos(two_pi * n / kVocFrame);
  for (int j = 0; j < kVocFft; ++j) { cs[j] = std::cos(two_pi * j / kVocFft); sn[j] = std::sin(two_pi * j / kVocFft); }
  sn[0] = sn[kVocFft / 2] = 0.0;   // exact zeros: the imaginary parts of the DC and Nyquist bins
  cs[kVocFft / 4] = cs[3 * kVocFft / 4] = 0.0;
  fwd.assign((size_t)kVocFrame * kVocSpec, 0.f);
  inv.assign((size_t)kVocSpec * kVocFrame, 0.f);
  for (int n = 0; n < kVocFrame; ++n)
    for (int k = 0; k < kVocBins; ++k) {
      const int j = (k * n) % kVocFft;
      const double ck = (k == 0 || k == kVocBins - 1) ? 1.0 : 2.0;
      fwd[(size_t)n * kVocSpec + k] = (float)(w[n] * cs[j]);
      fwd[(size_t)n * kVocSpec + kVocHalf + k] = (float)(-w[n] * sn[j]);
      inv[(size_t)k * kVocFrame + n] = (float)(ck / kVocFft * cs[j] * w[n]);
      inv[(size_t)(kVocHalf + k) * kVocFrame + n] = (float)(-ck / kVocFft * sn[j] * w[n]);
    }
  inv_norm.assign(2 * kVocHop, 0.f);
  for (int o = 0; o < kVocHop; ++o) {
    const double one = w[o] * w[o], two = one + w[o + kVocHop] * w[o + kVocHop];
    inv_norm[o] = (float)(1.0 / std::max(one, (double)kVocOlaFloor));
    inv_norm[kVocHop + o] = (float)(1.0 / std::max(two, (double)kVocOlaFloor));
  }
}

inline GemmF32Params voc_gemm(const float* A, int lda, const float* B, int ldb, int M, int N, int K) {
  GemmF32Params p;
  p.A = A; p.B = B; p.lda = lda; p.ldb = ldb; p.M = M; p.N = N; p.K = K;
  return p;
}

constexpr int64_t kVocMaxRows = 1 << 20;   // spectrum rows per call (the elementwise kernels index in 32 bits)
inline bool voc_shape_ok(int batch, int64_t frames) { return batch > 0 && frames > 0 && (int64_t)batch * (frames + 1) <= kVocMaxRows; }

inline dim3 voc_grid_rows(int rows) { return dim3((unsigned)(((size_t)rows * kVocG4 + 255) / 256)); }
inline dim3 voc_grid_samples(int per_song, int batch) { return dim3((unsigned)((per_song / 4 + 255) / 256), (unsigned)batch); }

// caller's [B, n] -> the padded signals
inline void voc_pad(msd_vocoder* v, int batch, int n, int F, const float* audio_dev, hipStream_t s) {
  const int per_song = (F + 1) * kVocHop;
  hipLaunchKernelGGL(voc_pad_signal_kernel, voc_grid_samples(per_song, batch), dim3(256), 0, s, audio_dev, v->w[VB_AUDIO], n, per_song);
}
// padded signals -> spectrum rows through `epi`
template <class Epi>
inline hipError_t voc_forward(msd_vocoder* v, int rows, const Epi& epi, hipStream_t s) {
  return launch_gemm_f32(voc_gemm(v->w[VB_AUDIO], kVocHop, v->fwd, kVocSpec, rows - 1, kVocSpec, kVocFrame), epi, s);
}
// X -> windowed frames -> overlap-added, normalised signal (the padded signals, or the caller's [B, F * 320])
inline hipError_t voc_inverse(msd_vocoder* v, int batch, int F, float* out, bool padded, hipStream_t s) {
  const int rows = batch * (F + 1);
  const hipError_t e = launch_gemm_f32(voc_gemm(v->w[VB_X], kVocSpec, v->inv, kVocFrame, rows - 1, kVocFrame, kVocSpec),
                                       EpiF32Store{v->w[VB_FRAMES], kVocFrame}, s);
  if (e != hipSuccess) return e;
  const int per_song = (padded ? F + 1 : F) * kVocHop;
  hipLaunchKernelGGL(voc_ola_kernel, voc_grid_samples(per_song, batch), dim3(256), 0, s, v->w[VB_FRAMES], v->inv_norm, out, F,
                     per_song, (size_t)per_song);
  return hipGetLastError();
}

}  // namespace msd
