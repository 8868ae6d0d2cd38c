// The sampler's MULTISTEP form (msd_sample_steps with MSD_SAMPLER_DPMPP_2M): DPM-Solver++(2M) in data-prediction form, one
// kernel per model-output mode, and its launch.  Like keep_frames_tail.h this file belongs to msd_api.hip alone and is
// included LAST, behind keep_frames_tail.h: its instances land behind every kernel the library had before, and the plain
// and keep instances of sampler_step_kernel stay instruction for instruction what they were (elementwise.h, "Why this is
// a second text").  It is a kernel of its own and not a third form of sampler_step_kernel for the same reason.
//
// With the half-log-SNR lambda = logsnr / 2, h = lambda_s - lambda_t and r = h_prev / h (h_prev: the step before this one):
//   D   = x0_t                                      on the first step of a call
//   D   = x0_t + (1 / (2r)) (x0_t - x0_prev)        afterwards          [= (1 + 1/(2r)) x0_t - (1/(2r)) x0_prev]
//   z_s = (sigma_s / sigma_t) z_t + (-alpha_s expm1(-h)) D              i == 0 returns x0_t (the reference's convention)
// x0_t is sampler_update's pred_x0: after the model-output conversion, the CFG combine and the clip.  With D = x0_t the
// last line is ddim_step, rearranged.  No draw: the form is deterministic after init_z.
//
// The three step coefficients come from a [K][4] side table (msd_api.hip build_multistep_rows: {sigma_s / sigma_t,
// -alpha_s expm1(-h), 1 / (2r), 0}), one 16-byte load beside the five of the 20-float row, which stays what the other
// forms load.  x0_prev [n] is read and written in place as 16-byte vectors: a thread owns its four elements.
#pragma once
#include "elementwise.h"
namespace msd {
// pred_x0 of sampler_update, on the pinned conversions of the keep form (contraction off: the operation order is the text)
template <int MODE>
__device__ __forceinline__ float multistep_pred_x0(const SamplerParams& p, const float (&c)[kCoefCount], float z, float o_c,
                                                   float o_u) {
#pragma clang fp contract(off)
  float eps, x0;
  convert_model_output_pinned<MODE>(c, z, o_c, eps, x0, /*uncond=*/false);
  if (p.passes == 2) {
    float eps_u, x0_u;
    convert_model_output_pinned<MODE>(c, z, o_u, eps_u, x0_u, /*uncond=*/true);
    eps = p.cond_wt * eps + (1.0f - p.cond_wt) * eps_u;
    x0 = c[kCoefX0Scale] * fmaf(-eps, c[kCoefX0Eps], z);
  }
  if (p.clip_x0) x0 = x0 < -1.0f ? -1.0f : (x0 > 1.0f ? 1.0f : x0);   // (jnp.clip semantics, as in sampler_update)
  return x0;
}

template <int MODE>
__global__ void __launch_bounds__(256) sampler_multistep_kernel(SamplerMultistepParams p) {
#pragma clang fp contract(off)
  warm_kernargs<kernarg_lines<SamplerMultistepParams>()>();
  const int i = p.step_from_slot1 ? p.step_ptr[1] : p.step_ptr[0];
  const int idx = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (idx < p.n) {
    // as in sampler_step_kernel: what does not depend on the scan index goes out first, the rows behind the index
    const f32x4 zz = *reinterpret_cast<const f32x4*>(p.z + idx);
    const f32x4 ec = *reinterpret_cast<const f32x4*>(p.eps + idx);
    f32x4 eu = {0.f, 0.f, 0.f, 0.f}, xp = {0.f, 0.f, 0.f, 0.f};
    if (p.passes == 2) eu = *reinterpret_cast<const f32x4*>(p.eps + p.n + idx);
    const bool first = i == p.first_step;   // (the same in every lane) no history yet: x0_prev is not read
    if (!first) xp = *reinterpret_cast<const f32x4*>(p.x0_prev + idx);
    static_assert(kCoefCount == 20, "five 16-byte loads per row");
    f32x4 cr[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) cr[k] = reinterpret_cast<const f32x4*>(p.coef + (size_t)i * kCoefCount)[k];
    const f32x4 ms = *reinterpret_cast<const f32x4*>(p.coef_ms + (size_t)i * kMsCount);
    float c[kCoefCount];
#pragma unroll
    for (int k = 0; k < kCoefCount; ++k) c[k] = cr[k >> 2][k & 3];
    f32x4 out, x0v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float x0 = multistep_pred_x0<MODE>(p, c, zz[k], ec[k], eu[k]);
      const float d = first ? x0 : fmaf(ms[kMsHist], x0 - xp[k], x0);
      const float zs = fmaf(ms[kMsZ], zz[k], ms[kMsD] * d);
      x0v[k] = x0;
      out[k] = (i == 0) ? x0 : zs;
    }
    *reinterpret_cast<f32x4*>(p.x0_prev + idx) = x0v;
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
  // the scan index is published as sampler_step_kernel publishes it
  __syncthreads();
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) p.step_ptr[p.step_from_slot1 ? 0 : 1] = i - 1;
}

void launch_sampler_step(const SamplerMultistepParams& sp, hipStream_t s) {
  const dim3 grid((sp.n / 4 + 255) / 256), block(256);
  if (sp.model_output == kOutX0) hipLaunchKernelGGL(sampler_multistep_kernel<kOutX0>, grid, block, 0, s, sp);
  else if (sp.model_output == kOutV) hipLaunchKernelGGL(sampler_multistep_kernel<kOutV>, grid, block, 0, s, sp);
  else hipLaunchKernelGGL(sampler_multistep_kernel<kOutEps>, grid, block, 0, s, sp);
}
}  // namespace msd
