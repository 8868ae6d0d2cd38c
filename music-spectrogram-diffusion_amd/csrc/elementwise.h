// Non-GEMM kernels of the path: fused RMSNorm(+FiLM) -> bf16 planes, the fused
// DDPM/DDIM sampler update, weight packing, embeddings, Philox normal fill.
#pragma once
#include "common.h"

namespace msd {

// ---------------------------------------------------------------------------
// T5 LayerNorm (RMSNorm, eps 1e-6, fp32 statistics; layers.py:632-649) fused
// with the FiLM modulation x*(scale+1)+bias (layers.py:664-665) whose scale/bias
// come from the step-indexed table built at load time, and with the cast to the
// GEMM operand format.  One wave per row, float4 per lane.
//   film == nullptr     -> plain RMSNorm (cross-attention / encoder / final norm)
//   film[(step*slots + slot) * 2D + {0..D-1: scale, D..2D-1: bias}]
// OUT: 0 = bf16 plane, 1 = bf16 hi+lo planes, 2 = fp32
// ---------------------------------------------------------------------------
struct NormParams {
  const float* x;       // [rows, D]
  const float* gamma;   // [D]
  const float* film;    // table or nullptr
  const int* step_ptr;  // device scalar: current scan index i
  int film_slots, film_slot;
  int rows, D;
  h16_t* out[2];
  float* out_f32;
  unsigned* sat = nullptr;   // half-plane range flag (common.h RangeCheck)
  unsigned sat_tag = 1;
};

template <int OUT, int VPL>  // VPL = float4 loads per lane: D <= 256*VPL
__global__ void __launch_bounds__(256) rmsnorm_film_kernel(NormParams p) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.rows) return;
  const float* xr = p.x + (size_t)row * p.D;
  float4 v[VPL];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = (lane + i * 64) * 4;
    if (c < p.D) {
      v[i] = *reinterpret_cast<const float4*>(xr + c);
      ss += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
    }
  }
  ss = wave_sum(ss);
  const float rstd = 1.0f / sqrtf(ss / (float)p.D + 1e-6f);
  const float* fs = nullptr;
  if (p.film) fs = p.film + ((size_t)(*p.step_ptr) * p.film_slots + p.film_slot) * (2 * p.D);
  RangeCheck rc;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = (lane + i * 64) * 4;
    if (c < p.D) {
      const float4 g = *reinterpret_cast<const float4*>(p.gamma + c);
      float y[4] = {v[i].x * rstd * g.x, v[i].y * rstd * g.y, v[i].z * rstd * g.z, v[i].w * rstd * g.w};
      if (fs) {
        const float4 sc = *reinterpret_cast<const float4*>(fs + c);
        const float4 bi = *reinterpret_cast<const float4*>(fs + p.D + c);
        y[0] = y[0] * (sc.x + 1.0f) + bi.x;
        y[1] = y[1] * (sc.y + 1.0f) + bi.y;
        y[2] = y[2] * (sc.z + 1.0f) + bi.z;
        y[3] = y[3] * (sc.w + 1.0f) + bi.w;
      }
      const size_t off = (size_t)row * p.D + c;
      if (OUT == 2) {
        *reinterpret_cast<float4*>(p.out_f32 + off) = make_float4(y[0], y[1], y[2], y[3]);
      } else {
        uint32_t h[2], l[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          rc.see(y[2 * e], y[2 * e + 1]);
          if (OUT == 1) split2_h16(y[2 * e], y[2 * e + 1], h[e], l[e]);
          else h[e] = cvt2_h16(y[2 * e], y[2 * e + 1]);
        }
        *reinterpret_cast<uint2*>(p.out[0] + off) = make_uint2(h[0], h[1]);
        if (OUT == 1) *reinterpret_cast<uint2*>(p.out[1] + off) = make_uint2(l[0], l[1]);
      }
    }
  }
  rc.commit(p.sat, p.sat_tag);
}

// ---------------------------------------------------------------------------
// Philox4x32-10 + Box-Muller standard normals (documented generator shared with
// oracle/philox.py).  key = (seed_lo, seed_hi); counter = (block, subseq,
// stream_lo, stream_hi); element e = 4*block + j, j in 0..3;
//   u = ((x >> 8) + 0.5) * 2^-24 ; (z0, z1) = sqrt(-2 ln u0) * (cos, sin)(2 pi u1)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
    const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += W0; k1 += W1;
  }
}

// The four normals of counter block `blk` of sub-sequence `subseq`: ONE function for the fill kernel below and for the
// sampler's own draw (sampler_step_kernel with no noise buffer), so that both write the same bits.
__device__ __forceinline__ void philox_normal4(uint32_t blk, uint32_t subseq, uint32_t seed_lo, uint32_t seed_hi,
                                               uint32_t stream_lo, uint32_t stream_hi, float (&z)[4]) {
  uint32_t c[4] = {blk, subseq, stream_lo, stream_hi};
  philox4x32_10(c, seed_lo, seed_hi);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u0 = ((float)(c[2 * h] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float u1 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float rad = sqrtf(-2.0f * logf(u0));
    const float ang = 6.283185307179586f * u1;
    z[2 * h] = rad * cosf(ang);
    z[2 * h + 1] = rad * sinf(ang);
  }
}

// grid.y = number of consecutive sub-sequences; row y gets subseq0 + y, offset y * n
__global__ void philox_normal_kernel(float* out, int64_t n, uint32_t seed_lo, uint32_t seed_hi,
                                     uint32_t stream_lo, uint32_t stream_hi, uint32_t subseq0) {
  const int64_t blk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (blk * 4 >= n) return;
  out += (int64_t)blockIdx.y * n;
  float z[4];
  philox_normal4((uint32_t)blk, subseq0 + blockIdx.y, seed_lo, seed_hi, stream_lo, stream_hi, z);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (blk * 4 + j < n) out[blk * 4 + j] = z[j];
}

// ---------------------------------------------------------------------------
// The reference's generator (rng = MSD_RNG_THREEFRY): jax.random.normal for the default, non-partitionable
// Threefry layout, restated on the host in jax_random.py -- this is that file, per element.
//   key = PRNGKey(seed) = (seed >> 32, seed & 0xffffffff);  fold_in(key, d) = threefry(key, (0, d))
//   one draw of n_total values: half = ceil(n_total / 2); element e < half = word 0 of threefry(key, (e, e + half)),
//   element e >= half = word 1 of threefry(key, (e - half, e)); odd n_total: the last counter of the second half is 0
//   u = max(lo, ((bits >> 9 | 0x3f800000) - 1) * scale + lo), lo = nextafter(-1, 0);  normal = sqrt(2) * erfinv(u)
// The host rounds after every operation: the float stages are compiled with contraction OFF (an FMA would change
// the last bit); log1p is the one operation whose rounding neither side controls.
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ void threefry2x32(uint32_t k0, uint32_t k1, uint32_t& x0, uint32_t& x1) {
  const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
  x0 += ks[0];
  x1 += ks[1];
#define MSD_TF_ROUND(r) x0 += x1; x1 = ((x1 << (r)) | (x1 >> (32 - (r)))) ^ x0;
#pragma unroll
  for (int g = 0; g < 5; ++g) {
    if (g % 2 == 0) { MSD_TF_ROUND(13) MSD_TF_ROUND(15) MSD_TF_ROUND(26) MSD_TF_ROUND(6) }
    else { MSD_TF_ROUND(17) MSD_TF_ROUND(29) MSD_TF_ROUND(16) MSD_TF_ROUND(24) }
    x0 += ks[(g + 1) % 3];
    x1 += ks[(g + 2) % 3] + (uint32_t)(g + 1);
  }
#undef MSD_TF_ROUND
}

// bits -> uniform in [nextafter(-1, 0), 1).  The constants are the host code's bit patterns (jax_random.normal):
// lo = 0xBF7FFFFF; scale = float32(1 - lo) = 0x40000000 (the exact 2 - 2^-24 is a tie, rounded to even)
__device__ __forceinline__ float threefry_uniform(uint32_t bits) {
#pragma clang fp contract(off)
  const float lo = __uint_as_float(0xBF7FFFFFu), scale = __uint_as_float(0x40000000u);
  const float f = __uint_as_float((bits >> 9) | 0x3F800000u) - 1.0f;
  const float prod = f * scale;
  const float u = prod + lo;
  return u < lo ? lo : u;   // (no NaN can reach this max)
}

// w = -log1p(-x^2): the one operation of the float stages whose rounding the host does not share.  msd_op_threefry's stage 3
// hands it to the test, which runs everything after it on the host and asks for the device's normal bit for bit.
__device__ __forceinline__ float threefry_log_term(float x) {
#pragma clang fp contract(off)
  const float xx = x * x;
  return -log1pf(-xx);
}

// sqrt(2) * XLA's float32 ErfInv (Giles' single-precision polynomial), every operation rounded on its own
__device__ __forceinline__ float threefry_normal_of_uniform(float x) {
#pragma clang fp contract(off)
  float w = threefry_log_term(x);
  const bool lt = w < 5.0f;
  w = lt ? w - 2.5f : sqrtf(w) - 3.0f;
  float p = lt ? 2.81022636e-08f : -0.000200214257f;
#define MSD_TF_HORNER(a, b) { const float pw = p * w; p = (lt ? (a) : (b)) + pw; }
  MSD_TF_HORNER(3.43273939e-07f, 0.000100950558f)
  MSD_TF_HORNER(-3.5233877e-06f, 0.00134934322f)
  MSD_TF_HORNER(-4.39150654e-06f, -0.00367342844f)
  MSD_TF_HORNER(0.00021858087f, 0.00573950773f)
  MSD_TF_HORNER(-0.00125372503f, -0.0076224613f)
  MSD_TF_HORNER(-0.00417768164f, 0.00943887047f)
  MSD_TF_HORNER(0.246640727f, 1.00167406f)
  MSD_TF_HORNER(1.50140941f, 2.83297682f)
#undef MSD_TF_HORNER
  const float px = p * x;
  const float e = fabsf(x) == 1.0f ? copysignf(__uint_as_float(0x7F800000u), x) : px;
  return __uint_as_float(0x3FB504F3u) * e;   // float32(sqrt(2))
}

__device__ __forceinline__ float threefry_normal_of_bits(uint32_t bits) {
  return threefry_normal_of_uniform(threefry_uniform(bits));
}

// Element e of one draw of n_total values (n_total EVEN: no zero pad) -- what a thread of the sampler computes:
// one Threefry block per element, one of its two words used (jax_random.normal_at is this function on the host).
__device__ __forceinline__ float threefry_normal_at(uint32_t k0, uint32_t k1, uint32_t e, uint32_t half) {
  const bool first = e < half;
  uint32_t x0 = first ? e : e - half, x1 = first ? e + half : e;
  threefry2x32(k0, k1, x0, x1);
  return threefry_normal_of_bits(first ? x0 : x1);
}

// One draw of n values under key (k0, k1): thread t < half takes the counter pair (t, t + half) and writes both words
// of its block (elements t and t + half).  stage: 0 = raw bits (uint32 stored into out), 1 = uniform, 2 = normal,
// 3 = the normal stage's log term of the uniform (threefry_log_term).
// bits_in != nullptr: the caller's words instead of the generator's (the float stages' exhaustive test).
__global__ void __launch_bounds__(256) threefry_normal_kernel(float* out, int64_t n, uint32_t k0, uint32_t k1, int stage,
                                                              const uint32_t* bits_in) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t half = (n + 1) / 2;
  if (t >= half) return;
  const bool second = t + half < n;   // false only for the zero pad of an odd n
  uint32_t x0, x1;
  if (bits_in) {
    x0 = bits_in[t];
    x1 = second ? bits_in[t + half] : 0u;
  } else {
    x0 = (uint32_t)t;
    x1 = second ? (uint32_t)(t + half) : 0u;
    threefry2x32(k0, k1, x0, x1);
  }
  if (stage == 1) { x0 = __float_as_uint(threefry_uniform(x0)); x1 = __float_as_uint(threefry_uniform(x1)); }
  else if (stage == 2) { x0 = __float_as_uint(threefry_normal_of_bits(x0)); x1 = __float_as_uint(threefry_normal_of_bits(x1)); }
  else if (stage == 3) { x0 = __float_as_uint(threefry_log_term(threefry_uniform(x0))); x1 = __float_as_uint(threefry_log_term(threefry_uniform(x1))); }
  uint32_t* o = reinterpret_cast<uint32_t*>(out);   // stored as words: stage 0's bit patterns are not floats
  o[t] = x0;
  if (second) o[t + half] = x1;
}

// ---------------------------------------------------------------------------
// Fused sampler update = everything in eval_step.body after the decoder calls
// (diffusion_utils.py:416-452): CFG combine, x0-from-eps, clip, posterior mean,
// + std * noise (DDPM, diffusion_utils.py:120-163,382-395) or the DDIM update
// (369-379); at scan index 0 returns x0.  Coefficients are per-step scalars from
// the load-time table (row i of `coef`, see msd_api: kCoef*).  Also advances the
// device-side scan index so a captured graph can be replayed N times.
// ---------------------------------------------------------------------------
// Row i of the table (msd_api.hip build_coef_table).  "M*" = the same conversions evaluated at the
// TRAIN schedule's log-SNR, which is where the reference converts the model output
// (diffusion_utils.py:294), while CFG / clip / the sampler use the SAMPLER schedule (:411-412).
enum { kCoefLogsnrT = 0, kCoefLogsnrS, kCoefX0Scale, kCoefX0Eps, kCoefMeanZ, kCoefMeanX0,
       kCoefStd, kCoefEpsScale, kCoefEpsX0, kCoefAlphaS, kCoefSigmaS,
       kCoefMLogsnr, kCoefMX0Scale, kCoefMX0Eps, kCoefMEpsScale, kCoefMEpsX0, kCoefMAlpha, kCoefMSigma,
       kCoefPad0, kCoefPad1, kCoefCount };
enum { kOutEps = 0, kOutX0 = 1, kOutV = 2 };   // = msd_model_output
// words of one row of SamplerParams::rng_key: 0..3 the Philox key and stream, then the generator kind (= MSD_RNG_*), the
// Threefry key PRNGKey(seed) and the mode of the draw: 0 = one draw over the whole [batch, T, n] array under row 0's key
// (every row of the table holds that key then), 1 = every row of the array is a draw of its own under its table row
enum { kRngKind = 4, kRngTfKey0 = 5, kRngTfKey1 = 6, kRngPerRow = 7, kRngWords = 8 };
enum { kRngRowBlock = 1024 };   // elements per block of sampler_step_kernel: a row of a per-row draw is a whole number of them
enum { kRngPhilox = 0, kRngThreefry = 1 };

struct SamplerParams {
  const float* eps;     // [passes][n] decoder outputs (pass 0 = conditional)
  float* z;             // [n] in/out
  const float* const* noise_slot;  // device slot holding the [N][n] per-step draws pointer; a NULL pointer there = draw here
  const uint32_t* rng_key = nullptr;   // [rows][kRngWords] device words, this block's row ALWAYS read (set at every launch): {seed_lo, seed_hi, stream_lo, stream_hi} of the in-kernel draw (round 6):
                                       // step i's noise = sub-sequence 1 + i of the caller's Philox stream, element block =
                                       // this thread -- exactly the row philox_normal_kernel used to write for it (the
                                       // [N][n] buffer: 131 MB x songs at base, a hipMalloc inside msd_sample)
                                       // followed by {generator kind, PRNGKey(seed) word 0, word 1} (kRng*): the kind lives in
                                       // device memory so that ONE captured graph serves both generators
                                       // and {per-row mode} (kRngPerRow): block x reads table row x / row_blocks, so the same
                                       // graph serves the whole-array draw (all rows equal) and the per-row one
  int row_blocks = 1 << 30;            // blocks of kRngRowBlock elements per [T, n] row of z = per row of the key table; the
                                       // default keeps every block on table row 0 (a one-row table, no per-row draw)
  const float* coef;    // [N][kCoefCount]
  int* step_ptr;        // scan index i (device); see step_from_slot1
  int step_from_slot1 = 0;
  int n;                // batch*T*n_dims
  int passes;           // 2 with CFG
  float cond_wt;        // eval_condition_weight
  int clip_x0, ddim;
  int model_output = kOutEps;   // what the network predicts (diffusion_utils.py:288-322)
  h16_t* z_hi;         // optional 16-bit planes of the new z (A operand of the next input projection)
  h16_t* z_lo;
  unsigned* sat = nullptr;   // half-plane range flag (common.h RangeCheck)
  unsigned sat_tag = 1;
};

// The keep form's arguments (msd_sample_keep): frames of the target that are KNOWN.  A struct of its own, so that the
// plain instances' argument block stays at its 120 bytes -- two of the 64-byte lines warm_kernargs counts in, one 128-byte
// cache line; the keep form's 144 bytes take a third 64-byte line.
struct SamplerKeepParams : SamplerParams {
  const float* xk = nullptr;     // [n] the known mel in model units (scale_clip_kernel of the caller's mel)
  const int32_t* keep = nullptr; // [n / n_dims] per frame, a release word v: 0 = free at every step; v >= 1 = known at scan
                                 // indices i >= v - 1 and free below (1 = known throughout: msd_sample_keep's flag)
  int n_dims = 0;                // elements per frame, % 4 == 0: a thread's four elements lie in one frame
};

// The guided form's arguments (msd_sample_guided): the classifier-free guidance weight of this block's row of z comes from a
// device table, indexed as the key table is (block x reads row x / row_blocks), so ONE captured graph serves every weight
// vector.  A struct of its own again: 128 bytes, the plain instances' block stays at its 120.  The launch always carries
// both passes of the model output (passes == 2); a row whose weight is exactly 1 takes the reference's `== 1` branch
// (no combine, pred_x0 not recomputed, the unconditional pass not read) -- block-uniform, a block never straddles rows.
struct SamplerGuidedParams : SamplerParams {
  const float* row_wt = nullptr;   // [rows] eval_condition_weight per row of z
};
// What sampler_update reads in a guided launch: the launch's arguments with the row's weight in cond_wt's place, and one
// pass where that weight is 1.  The update's text, operations and order are untouched: the weight is its operand.
__device__ __forceinline__ SamplerParams with_row_weight(const SamplerParams& p, float w) {
  SamplerParams q = p;
  q.cond_wt = w;
  q.passes = w != 1.0f ? 2 : 1;
  return q;
}

// The update's arithmetic is ONE text, and the operation order is that text: contraction is off, every fused
// multiply-add is an fmaf written here, and every form of the update -- plain, keep, the multistep form's x0 -- is an
// instance of sampler_update below.  ("A zero keep mask is the plain call, bit for bit" is a statement about rounding:
// with contraction left to the compiler the forms fused the DDPM line differently, 26 % of the free elements off by an ulp
// or more on the MI355X)  The order is the one the compiler chose for the first, unpinned text, read off its
// disassembly: every difference of a product fused (fma(-a, b, c)), the CFG combine as two rounded products and a sum,
// the DDPM line as fma(std, nz, (a z) + (b x0)), the DDIM line as fma(sigma, eps, alpha x0).  v mode's alpha z - sigma v
// rounds both products in the conditional pass and fuses the second in the unconditional one: that pass reused the
// first product, so only the other was left to fuse.
//
// model output -> (eps, x0) at the TRAIN schedule's log-SNR (diffusion_utils.py:288-322)
template <int mode>
__device__ __forceinline__ void convert_model_output(const float (&c)[kCoefCount], float z, float o,
                                                     float& eps, float& x0, bool uncond) {
#pragma clang fp contract(off)
  if constexpr (mode == kOutEps) {
    eps = o;
    x0 = c[kCoefMX0Scale] * fmaf(-o, c[kCoefMX0Eps], z);
  } else if constexpr (mode == kOutX0) {
    x0 = o;
    eps = c[kCoefMEpsScale] * fmaf(-o, c[kCoefMEpsX0], z);
  } else {  // v: x0 = alpha z - sigma v
    const float az = c[kCoefMAlpha] * z;
    x0 = uncond ? fmaf(-o, c[kCoefMSigma], az) : az - c[kCoefMSigma] * o;
    eps = c[kCoefMEpsScale] * fmaf(-x0, c[kCoefMEpsX0], z);
  }
}

// one element of eval_step.body after the decoder calls (diffusion_utils.py:416-452):
// o_c / o_u = conditional / unconditional model output, nz = the step's normal draw.
// FORM: kFormPlain = the step; kFormKeep = the step with KNOWN frames (msd_sample_keep): on a kept element (kf, xk = its
// known value in model units), after the CFG combine and the clip, pred_x0 := xk and pred_eps := predict_eps_from_x0(z_t,
// xk, logsnr_t) -- the clip branch's expression -- so the element follows the posterior q(z_s | z_t, x0 = xk) and arrives
// at xk at i == 0; kFormX0 = pred_x0 alone (converted, combined, clipped), what the multistep form steps from; kFormEps =
// pred_eps alone, converted and combined and NOT clipped (p.clip_x0 is not read), what the inversion steps from
// (invert_tail.h).
enum { kFormPlain = 0, kFormKeep, kFormX0, kFormEps };
template <int MODE, int FORM>
__device__ __forceinline__ float sampler_update(const SamplerParams& p, const float (&c)[kCoefCount], int i, float z,
                                                float o_c, float o_u, float nz = 0.f, float xk = 0.f, bool kf = false) {
#pragma clang fp contract(off)
  float eps, x0;
  convert_model_output<MODE>(c, z, o_c, eps, x0, /*uncond=*/false);
  if (p.passes == 2) {
    float eps_u, x0_u;
    convert_model_output<MODE>(c, z, o_u, eps_u, x0_u, /*uncond=*/true);
    eps = p.cond_wt * eps + (1.0f - p.cond_wt) * eps_u;
    x0 = c[kCoefX0Scale] * fmaf(-eps, c[kCoefX0Eps], z);
  }
  if constexpr (FORM == kFormEps) return eps;
  // jnp.clip semantics: a NaN stays a NaN (fminf / fmaxf would turn it into a bound and hide a poisoned input --
  // the half-plane range flag sees Inf but not NaN: v_max3_f32 drops NaN operands)
  if constexpr (FORM == kFormX0) {
    if (p.clip_x0) x0 = x0 < -1.0f ? -1.0f : (x0 > 1.0f ? 1.0f : x0);
    return x0;
  }
  if (p.clip_x0) {
    x0 = x0 < -1.0f ? -1.0f : (x0 > 1.0f ? 1.0f : x0);
    eps = c[kCoefEpsScale] * fmaf(-x0, c[kCoefEpsX0], z);
  }
  if constexpr (FORM == kFormKeep) {
    if (kf) {
      x0 = xk;
      eps = c[kCoefEpsScale] * fmaf(-xk, c[kCoefEpsX0], z);
    }
  }
  float zs;
  if (p.ddim) zs = fmaf(c[kCoefSigmaS], eps, c[kCoefAlphaS] * x0);
  else zs = fmaf(c[kCoefStd], nz, c[kCoefMeanZ] * z + c[kCoefMeanX0] * x0);
  return (i == 0) ? x0 : zs;
}

// What both sampler kernels (this file, multistep_tail.h) share around the update.  (Their third common piece, the store
// of z as operand planes, stays written out in each kernel and in diffuse_to_step_kernel: as a helper, by reference or
// by value, it changed the instructions of all nine sampler instances and of that kernel.)
// Row i of the coefficient table as five 16-byte loads (20 floats, rows 80 bytes apart)
__device__ __forceinline__ void load_coef_row(const float* coef, int i, f32x4 (&cr)[5]) {
  static_assert(kCoefCount == 20, "five 16-byte loads per row");
#pragma unroll
  for (int k = 0; k < 5; ++k) cr[k] = reinterpret_cast<const f32x4*>(coef + (size_t)i * kCoefCount)[k];
}
// The next scan index, published by the launch's last block: every block has read *step_ptr before any kernel of the
// next step can start (kernel boundary); the decrement is ordered by the same boundary.
__device__ __forceinline__ void publish_next_step(const SamplerParams& p, int i) {
  __syncthreads();
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) p.step_ptr[p.step_from_slot1 ? 0 : 1] = i - 1;
}

// MODE = p.model_output as a compile-time constant: with the run-time switch the conversions' two results travelled
// through scratch memory and a maze of scalar branches (885 lines of ISA for an elementwise kernel)
// P = SamplerKeepParams: the keep form -- the frame flag and the known values are loaded with z / eps and handed to
// sampler_update's keep form.  One kernel for both, the difference under `if constexpr`.
template <int MODE, class P = SamplerParams>
__global__ void __launch_bounds__(256) sampler_step_kernel(P p) {
  constexpr bool KEEP = std::is_same<P, SamplerKeepParams>::value;
  constexpr bool GUIDED = std::is_same<P, SamplerGuidedParams>::value;
  static_assert(KEEP || GUIDED || std::is_same<P, SamplerParams>::value, "SamplerParams, SamplerKeepParams or SamplerGuidedParams");
  warm_kernargs<kernarg_lines<P>()>();
  // step_from_slot1: the step's first kernel (in_proj) copied the index to slot 1 and nobody else
  // reads slot 0 any more in this step, so this launch may decrement slot 0 itself
  const int i = p.step_from_slot1 ? p.step_ptr[1] : p.step_ptr[0];
  // The noise slot and the words of the in-kernel draw (generator kind, keys: always valid memory) travel WITH the index:
  // fetched where they are used, inside the branches below, slot -> kind -> key are three dependent round trips to
  // memory in front of the draw (measured: +0.5 % on a segment).  The empty asm pins the loads here (the
  // compiler sinks them into the branches otherwise); it also makes the values per-lane for the compiler, so the two
  // tests below are vector compares whose outcome is the same in every lane.  This is the form that was measured.
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const float* noise = *p.noise_slot;
  // The key row of this block's row of z: its address comes from the block index alone, so the per-row keys are one
  // more address computation in front of the same two loads, not a load behind a load.
  const uint32_t row = blockIdx.x / (uint32_t)p.row_blocks;
  const u32x4* rkp = reinterpret_cast<const u32x4*>(p.rng_key + (size_t)row * kRngWords);
  u32x4 rk0 = rkp[0], rk1 = rkp[1];
  static_assert(kRngKind == 4 && kRngTfKey0 == 5 && kRngTfKey1 == 6 && kRngPerRow == 7, "rk1 = {kind, Threefry key, mode}");
  asm volatile("" : "+v"(noise), "+v"(rk0), "+v"(rk1));
  float wt = 1.0f;   // the guided form: this row's weight, fetched with the key row (the address is the block index's too)
  if constexpr (GUIDED) wt = p.row_wt[row];
  const int idx = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (idx < p.n) {
    // Loads that do not depend on the scan index go out first; the coefficient row (20 floats = five 16-byte loads,
    // rows are 80 bytes apart) and the step's noise follow as soon as the index is here.  The coefficients live in
    // REGISTERS (a pointer into the table made every c[k] of sampler_update a scalar load inside a branch, with a wait
    // each, and pushed the kernel into scratch); native vectors instead of float4 structs copied into arrays.
    const f32x4 zz = *reinterpret_cast<const f32x4*>(p.z + idx);
    const f32x4 ec = *reinterpret_cast<const f32x4*>(p.eps + idx);
    f32x4 eu = {0.f, 0.f, 0.f, 0.f}, nz = {0.f, 0.f, 0.f, 0.f};
    if constexpr (GUIDED) {
      if (wt != 1.0f) eu = *reinterpret_cast<const f32x4*>(p.eps + p.n + idx);   // (the same in every lane)
    } else {
      if (p.passes == 2) eu = *reinterpret_cast<const f32x4*>(p.eps + p.n + idx);
    }
    f32x4 xk = {0.f, 0.f, 0.f, 0.f};
    int kf = 0;
    if constexpr (KEEP) {
      xk = *reinterpret_cast<const f32x4*>(p.xk + idx);
      // the frame's release word -> known in THIS step: one unsigned compare (v == 0 wraps to 2^32 - 1: never known)
      kf = (uint32_t)p.keep[(uint32_t)idx / (uint32_t)p.n_dims] - 1u <= (uint32_t)i;
    }
    f32x4 cr[5];
    load_coef_row(p.coef, i, cr);
    if (!p.ddim && i != 0) {
      // per-row mode (the same in every lane): the draw covers this row's R = row_blocks * kRngRowBlock elements and e is
      // the element inside the row -- what a one-row call under this row's key draws; else the whole array, e = idx
      const bool per_row = rk1[3] != 0u;
      const uint32_t e = per_row ? (uint32_t)idx - row * (uint32_t)p.row_blocks * kRngRowBlock : (uint32_t)idx;
      const uint32_t span = per_row ? (uint32_t)p.row_blocks * kRngRowBlock : (uint32_t)p.n;
      if (noise != nullptr) {   // (the same in every lane)
        nz = *reinterpret_cast<const f32x4*>(noise + (size_t)i * p.n + idx);
      } else if (rk1[0] == kRngThreefry) {   // (the same in every lane) the reference's generator: this thread's four
        // elements of normal(fold_in(PRNGKey(seed), i), [batch, T, n]) ([1, T, n] per row); the folded key is the same
        // for every thread of the draw
        uint32_t f0 = 0u, f1 = (uint32_t)i;
        threefry2x32(rk1[1], rk1[2], f0, f1);
        const uint32_t half = span >> 1;   // span % 4 == 0: no zero pad
#pragma unroll
        for (int k = 0; k < 4; ++k) nz[k] = threefry_normal_at(f0, f1, e + (uint32_t)k, half);
      } else {   // no buffer: this thread's four draws of sub-sequence 1 + i (e / 4 = the counter block)
        float d[4];
        philox_normal4(e >> 2, 1u + (uint32_t)i, rk0[0], rk0[1], rk0[2], rk0[3], d);
        nz = f32x4{d[0], d[1], d[2], d[3]};
      }
    }
    float c[kCoefCount];
#pragma unroll
    for (int k = 0; k < kCoefCount; ++k) c[k] = cr[k >> 2][k & 3];
    f32x4 out;
    if constexpr (GUIDED) {
      const SamplerParams q = with_row_weight(p, wt);
#pragma unroll
      for (int k = 0; k < 4; ++k) out[k] = sampler_update<MODE, kFormPlain>(q, c, i, zz[k], ec[k], eu[k], nz[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        out[k] = sampler_update<MODE, KEEP ? kFormKeep : kFormPlain>(p, c, i, zz[k], ec[k], eu[k], nz[k], xk[k], kf != 0);
    }
    *reinterpret_cast<f32x4*>(p.z + idx) = out;
    if (p.z_hi) {
      uint32_t h[2], l[2];
      RangeCheck rc;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        rc.see(out[2 * k], out[2 * k + 1]);
        split2_h16(out[2 * k], out[2 * k + 1], h[k], l[k]);
      }
      *reinterpret_cast<uint2*>(p.z_hi + idx) = make_uint2(h[0], h[1]);
      if (p.z_lo) *reinterpret_cast<uint2*>(p.z_lo + idx) = make_uint2(l[0], l[1]);
      rc.commit(p.sat, p.sat_tag);
    }
  }
  publish_next_step(p, i);
}

// One launch of a family of sampler kernels, a float4 per thread: sp.model_output picks the instance, and
// kernel_of(ModeTag<MODE>) names the family's kernel of that mode.
template <int MODE> using ModeTag = std::integral_constant<int, MODE>;
template <class P, class F>
static inline void launch_sampler_family(const P& sp, hipStream_t s, F kernel_of) {
  const dim3 grid((sp.n / 4 + 255) / 256), block(256);
  if (sp.model_output == kOutX0) hipLaunchKernelGGL(kernel_of(ModeTag<kOutX0>{}), grid, block, 0, s, sp);
  else if (sp.model_output == kOutV) hipLaunchKernelGGL(kernel_of(ModeTag<kOutV>{}), grid, block, 0, s, sp);
  else hipLaunchKernelGGL(kernel_of(ModeTag<kOutEps>{}), grid, block, 0, s, sp);
}
inline void launch_sampler_step(const SamplerParams& sp, hipStream_t s) {
  launch_sampler_family(sp, s, [](auto m) { return sampler_step_kernel<decltype(m)::value, SamplerParams>; });
}
// the keep form's launches: keep_frames_tail.h, which msd_api.hip includes last (the reason is written there)
void launch_sampler_step(const SamplerKeepParams& sp, hipStream_t s);
void launch_unscale_keep(const float* x0, const float* known, const int32_t* keep, float* out, int n, int n_dims, float fmin,
                         float fmax, hipStream_t s);

// The part-way start of msd_sample_edit (keep_frames_tail.h): the caller's mel -> xk, and z = alpha xk + sigma eps as fp32
// and operand planes.  eps may be z itself (a thread reads its four elements before it writes them).
struct DiffuseParams {
  const float* mel;     // [n] the caller's mel, mel units
  const float* eps;     // [n] the call's initial draw
  float* xk;            // [n] out: scale_features(clip=True) of mel
  float* z;             // [n] out
  h16_t* z_hi;          // out: operand planes of z (z_lo may be null: one-plane precisions)
  h16_t* z_lo;
  int n;                // % 4 == 0
  float fmin, fmax;     // the codec's range
  float alpha, sigma;   // sqrt(sigmoid(+-logsnr_t)) of the start index (host, double, rounded once)
  unsigned* sat = nullptr;   // half-plane range flag (common.h RangeCheck)
  unsigned sat_tag = 1;
};
void launch_diffuse_to_step(const DiffuseParams& dp, hipStream_t s);
// flags[i] = flags[i] != 0: msd_sample_keep's "any non-zero flag = known throughout" as the release word 1
void launch_normalize_flags(const int32_t* in, int32_t* out, int n, hipStream_t s);

// A resampling jump of msd_sample_resample (keep_frames_tail.h): one sample of q(z_t | z_s) from the bottom level of a block
// of steps back to its top, z' = fmaf(b, eps, a * z), as fp32 and operand planes.  z may be z_in (a thread reads its four
// elements before it writes them).  eps == nullptr: drawn here under `keys`, the rows of the pass the jump opens -- what
// that key's initial draw would be (Philox sub-sequence 0; Threefry normal(key, [B | 1, T, n])), per row of z in the
// per-row mode, with sampler_step_kernel's row arithmetic.  The launch's last block then installs those rows in the
// sampler's key table and sets both words of the scan index, so the steps behind it draw under the pass's key from the
// block's top: no host round trip between passes.
struct RenoiseParams {
  const float* z_in;    // [n]
  const float* eps = nullptr;   // [n] the caller's draw (msd_op_renoise), or nullptr
  float* z;             // [n] out
  h16_t* z_hi;          // out: operand planes of z (z_lo may be null: one-plane precisions)
  h16_t* z_lo;
  int n;                // % 4 == 0
  float a, b;           // alpha_t / alpha_s and sqrt(1 - a^2) (host, double, rounded once)
  const uint32_t* keys = nullptr;   // [rows][kRngWords] the pass's key rows (read when eps == nullptr)
  int row_blocks = 1 << 30;         // SamplerParams::row_blocks
  uint32_t* key_table = nullptr;    // the sampler's key table: gets key_words words of `keys`; nullptr = none
  int key_words = 0;
  int* step_ptr = nullptr;          // the device scan index: both words := next_step; nullptr = none
  int next_step = 0;
  unsigned* sat = nullptr;   // half-plane range flag (common.h RangeCheck)
  unsigned sat_tag = 1;
};
void launch_renoise(const RenoiseParams& rp, hipStream_t s);

// The multistep form's arguments (msd_sample_steps with MSD_SAMPLER_DPMPP_2M; kernel and launch: multistep_tail.h).  A
// struct of its own for the keep form's reason: the plain instances' argument block stays at its two 64-byte lines.
// Row i of the side table coef_ms: {sigma_s / sigma_t, -alpha_s expm1(-h), 1 / (2r), 0} (msd_api.hip build_multistep_rows)
enum { kMsZ = 0, kMsD, kMsHist, kMsPad, kMsCount };
struct SamplerMultistepParams : SamplerParams {
  float* x0_prev = nullptr;        // [n] in/out: the previous step's pred_x0; not read at scan index first_step
  const float* coef_ms = nullptr;  // [K][kMsCount]
  int first_step = -1;             // the scan index the call starts at (no history there)
};
void launch_sampler_step(const SamplerMultistepParams& sp, hipStream_t s);
// ... and their guided forms (SamplerGuidedParams above; kernels' instances and launches: guided_tail.h)
struct SamplerMultistepGuidedParams : SamplerMultistepParams {
  const float* row_wt = nullptr;   // [rows], as SamplerGuidedParams::row_wt
};
void launch_sampler_step(const SamplerGuidedParams& sp, hipStream_t s);
void launch_sampler_step(const SamplerMultistepGuidedParams& sp, hipStream_t s);

// The inversion's arguments (msd_invert; kernel and launch: invert_tail.h): one deterministic DDIM step UP the scan, from
// level i to level i + 1.  A struct of its own once more: the plain instances' argument block stays at its 120 bytes.
// Row i of the side table coef_inv: {a, b, 0, 0} of z_up = fmaf(b, eps, a * z) (msd_api.hip build_invert_rows).  The row
// weights are read as SamplerGuidedParams::row_wt is; the form makes no draw: noise_slot and rng_key are not read.
enum { kInvA = 0, kInvB, kInvPad0, kInvPad1, kInvCount };
struct SamplerInvertParams : SamplerParams {
  const float* row_wt = nullptr;     // [rows] eval_condition_weight per row of z; a weight of exactly 1 reads one pass
  const float* coef_inv = nullptr;   // [K][kInvCount]
};
void launch_sampler_invert(const SamplerInvertParams& sp, hipStream_t s);

// The denoising loss (msd_loss; kernels and launches: loss_tail.h).  What changes from call to call -- the caller's buffers,
// the loss form, the time list -- lives in ONE device struct the handle owns, so a captured (diffuse, decoder, loss) graph
// serves every call; `cursor` is the position in the time list, double-buffered like the scan index: loss_diffuse_kernel
// reads word 0 and its last block copies it to word 1, diffusion_loss_kernel reads word 1 and its last block writes
// word 0 := word 1 + 1 -- nobody reads the word a launch writes.
enum { kLossX0 = 0, kLossEps, kLossMaxX0Eps, kLossX0AndEps };   // = MSD_LOSS_X0 ...
enum { kLossL1 = 0, kLossL2 };                                   // = MSD_LOSS_L1, _L2
enum { kLossTimeAlpha = 0, kLossTimeSigma, kLossTimeIndex, kLossTimePad, kLossTimeWords };   // a row of LossCall::times
struct LossCall {
  const float* target;   // [n] the caller's mel, mel units (loss_diffuse_kernel)
  const float* mask;     // [n / n_dims] float, or nullptr = ones
  const float* eps;      // [n_times][n] the caller's draws, or nullptr = drawn in both kernels
  float* out;            // [n_times][passes][n / n_dims]
  const float* times;    // [n_times][kLossTimeWords]: {alpha, sigma, bits of the time index i, 0}
  int32_t type, norm;    // kLoss*
  int32_t cursor[2];
};
static_assert(sizeof(LossCall) == 56, "five pointers and four words");
struct LossDiffuseParams {
  LossCall* call;
  float* x0;            // [n] out: scale_features(clip=True) of the target
  float* z;             // [n] out
  h16_t* z_hi;          // out: operand planes of z (z_lo may be null: one-plane precisions)
  h16_t* z_lo;
  const uint32_t* keys; // [rows][kRngWords] (SamplerParams::rng_key)
  int row_blocks = 1 << 30;   // SamplerParams::row_blocks
  int n;                // % 4 == 0
  float fmin, fmax;     // the codec's range
  int* step_ptr = nullptr;   // the device scan index: both words := i; nullptr = none
  unsigned* sat = nullptr;   // half-plane range flag (common.h RangeCheck)
  unsigned sat_tag = 1;
};
struct LossParams {
  LossCall* call;
  const float* o;       // [passes][n] the model output
  const float* z;       // [n]
  const float* x0;      // [n]
  const float* coef;    // [N][kCoefCount]
  const uint32_t* keys; // as above
  int row_blocks = 1 << 30;
  int n;                // per pass; % n_dims == 0
  int passes;           // 1 or 2
  int n_dims;           // % 4 == 0, 1024 % n_dims == 0: a frame is n_dims / 4 consecutive threads of one block
  int model_output = kOutEps;
};
void launch_loss_diffuse(const LossDiffuseParams& p, hipStream_t s);
void launch_diffusion_loss(const LossParams& p, hipStream_t s);

// g[step][slot][k] = gamma[k] * (film_scale[step][slot][k] + 1): the column multiplier of a
// FiLM-modulated RMSNorm, tabulated for every step (folded-norm GEMM epilogues, gemm_h16.h)
__global__ void build_g_kernel(const float* film, const float* gamma, float* g, int n_steps, int slots,
                               int slot, int D) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_steps * D) return;
  const int step = i / D, k = i % D;
  g[((size_t)step * slots + slot) * D + k] = gamma[k] * (film[((size_t)step * slots + slot) * 2 * D + k] + 1.0f);
}

// step_ptr[0] <- step_ptr[1]  (double-buffered scan index: the sampler writes the
// next index to slot 1 while other blocks of the same launch may still read slot 0)

// scale_to_features (audio_codecs.py:176-183) on the final x0
__global__ void unscale_kernel(const float* x0, float* out, int n, float fmin, float fmax) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (x0[i] + 1.0f) / 2.0f * (fmax - fmin) + fmin;
}

// scale_features(clip=True) (audio_codecs.py:166-174) on the context spectrogram
__global__ void scale_clip_kernel(const float* in, float* out, int n, float fmin, float fmax) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const float f = fminf(fmaxf(in[i], fmin), fmax);
    out[i] = (f - fmin) / (fmax - fmin) * 2.0f + (-1.0f);
  }
}

// ---------------------------------------------------------------------------
// Weight packing: W fp32 [K, N] (reference layout, layers.py:430-431) ->
// W^T bf16 planes [N_out_rows, K]; dst row r takes source column src_col[r]
// (identity, QKV concatenation, or the 16-column wi_0/wi_1 interleave).
// ---------------------------------------------------------------------------
// `ldk` (0 = K) is the row length of the destination and `k0` the first column written: K-concatenated weights
// (the hoisted cross-attention query projection stacks two matrices along K).
__global__ void pack_wt_kernel(const float* w, int K, int N, h16_t* hi, h16_t* lo,
                               int dst_row0, int col_map_mode, int ldk, unsigned* absmax, int k0 = 0) {
  // grid: (ceil(K/64), N) ; block 64: thread = k within chunk
  const int n = blockIdx.y;
  const int k = blockIdx.x * 64 + threadIdx.x;
  int dst = dst_row0 + n;
  if (col_map_mode == 1) dst = dst_row0 + (n / 16) * 32 + (n % 16);        // wi_0 of the gated pair
  else if (col_map_mode == 2) dst = dst_row0 + (n / 16) * 32 + 16 + (n % 16);  // wi_1
  const float w0 = k < K ? w[(size_t)k * N + n] : 0.f;
  if (absmax) {   // largest |w| seen (bits of a non-negative float order like unsigned ints): range check at load
    float mx = fabsf(w0);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (threadIdx.x == 0) atomicMax(absmax, __float_as_uint(mx));
  }
  if (k >= K) return;
  const float v = w0 * kWScale;   // undone on the accumulators (gemm_tile)
  h16_t h, l;
  split_h16(v, h, l);
  const int ld = ldk > 0 ? ldk : K;
  hi[(size_t)dst * ld + k0 + k] = h;
  if (lo) lo[(size_t)dst * ld + k0 + k] = l;
}

// out[k][n] = sum_d a[k][d] g[d] b[d][n]   (a: [K, D], b: [D, N], all fp32 row-major), accumulated in float64 and rounded
// once: Wo_self . diag(gamma_cross) . Wq of the folded cross-attention query projection (msd_api.hip, load time).
// block (16, 16): thread = (n, k)
__global__ void fold_wq_kernel(const float* a, const float* g, const float* b, float* out, int K, int D, int N) {
  const int n = blockIdx.x * 16 + threadIdx.x, k = blockIdx.y * 16 + threadIdx.y;
  if (n >= N || k >= K) return;
  double acc = 0.0;
  for (int d = 0; d < D; ++d) acc += (double)a[(size_t)k * D + d] * (double)g[d] * (double)b[(size_t)d * N + n];
  out[(size_t)k * N + n] = (float)acc;
}

// token embedding (one-hot contraction == row gather, layers.py:556-559) + position
// table rows (network.py:278-287) for the valid positions of one sequence.
//   x[r] = tok_emb[tokens[pos[r]]] + pos_emb[pos[r]]   r < n_valid ; 0 for padding rows
__global__ void embed_tokens_kernel(const int* tokens, const int* pos, int n_valid, int rows,
                                    const float* tok_emb, const float* pos_emb, float* x, int D) {
  const int r = blockIdx.x;
  for (int c = threadIdx.x; c < D; c += blockDim.x) {
    float v = 0.f;
    if (r < n_valid) {
      const int ps = pos[r];
      v = tok_emb[(size_t)tokens[ps] * D + c] + pos_emb[(size_t)ps * D + c];
    }
    x[(size_t)r * D + c] = v;
  }
}

// dst[r] = (r < n_valid) ? src[idx[r]] : 0   (row gather with zero padding)
__global__ void gather_rows_kernel(const float* src, const int* idx, int n_valid, float* dst, int D) {
  const int r = blockIdx.x;
  for (int c = threadIdx.x; c < D; c += blockDim.x)
    dst[(size_t)r * D + c] = (r < n_valid) ? src[(size_t)idx[r] * D + c] : 0.f;
}

// fp32 -> bf16 planes (test helper for the standalone ops)
__global__ void split_planes_kernel(const float* in, h16_t* hi, h16_t* lo, int64_t n, unsigned* sat = nullptr,
                                    unsigned sat_tag = 1) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    h16_t h, l;
    RangeCheck rc;
    rc.see(in[i]);
    split_h16(in[i], h, l);
    hi[i] = h;
    if (lo) lo[i] = l;
    rc.commit(sat, sat_tag);
  }
}
__global__ void merge_planes_kernel(const h16_t* hi, const h16_t* lo, float* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = h2f(hi[i]) + (lo ? h2f(lo[i]) : 0.f);
}

}  // namespace msd
