// The sampler's MULTISTEP form (msd_sample_steps with MSD_SAMPLER_DPMPP_2M): DPM-Solver++(2M) in data-prediction form, one
// kernel per model-output mode, and its launch.  Like keep_frames_tail.h this file belongs to msd_api.hip alone and is
// included LAST, behind keep_frames_tail.h: its instances land behind every kernel the library had before (placement
// shows on the clock: keep_frames_tail.h).  It is a kernel of its own and not a third form of sampler_step_kernel, whose
// load order is a measured form: this one makes no draw and has none of that kernel's noise and key loads.
//
// With the half-log-SNR lambda = logsnr / 2, h = lambda_s - lambda_t and r = h_prev / h (h_prev: the step before this one):
//   D   = x0_t                                      on the first step of a call
//   D   = x0_t + (1 / (2r)) (x0_t - x0_prev)        afterwards          [= (1 + 1/(2r)) x0_t - (1/(2r)) x0_prev]
//   z_s = (sigma_s / sigma_t) z_t + (-alpha_s expm1(-h)) D              i == 0 returns x0_t (the reference's convention)
// x0_t is sampler_update's x0-only form (elementwise.h: one text for every form): pred_x0 after the model-output
// conversion, the CFG combine and the clip.  With D = x0_t the
// last line is ddim_step, rearranged.  No draw: the form is deterministic after init_z.
//
// The three step coefficients come from a [K][4] side table (msd_api.hip build_multistep_rows: {sigma_s / sigma_t,
// -alpha_s expm1(-h), 1 / (2r), 0}), one 16-byte load beside the five of the 20-float row, which stays what the other
// forms load.  x0_prev [n] is read and written in place as 16-byte vectors: a thread owns its four elements.
#pragma once
#include "elementwise.h"
namespace msd {
// P = SamplerMultistepGuidedParams: the guided form (guided_tail.h) -- this block's row weight from the device table in
// cond_wt's place, the difference under `if constexpr` as in sampler_step_kernel.
template <int MODE, class P = SamplerMultistepParams>
__global__ void __launch_bounds__(256) sampler_multistep_kernel(P p) {
#pragma clang fp contract(off)
  constexpr bool GUIDED = std::is_same<P, SamplerMultistepGuidedParams>::value;
  static_assert(GUIDED || std::is_same<P, SamplerMultistepParams>::value, "SamplerMultistepParams or SamplerMultistepGuidedParams");
  warm_kernargs<kernarg_lines<P>()>();
  const int i = p.step_from_slot1 ? p.step_ptr[1] : p.step_ptr[0];
  float wt = 1.0f;
  if constexpr (GUIDED) wt = p.row_wt[blockIdx.x / (uint32_t)p.row_blocks];
  const int idx = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (idx < p.n) {
    // as in sampler_step_kernel: what does not depend on the scan index goes out first, the rows behind the index
    const f32x4 zz = *reinterpret_cast<const f32x4*>(p.z + idx);
    const f32x4 ec = *reinterpret_cast<const f32x4*>(p.eps + idx);
    f32x4 eu = {0.f, 0.f, 0.f, 0.f}, xp = {0.f, 0.f, 0.f, 0.f};
    if constexpr (GUIDED) {
      if (wt != 1.0f) eu = *reinterpret_cast<const f32x4*>(p.eps + p.n + idx);   // (the same in every lane)
    } else {
      if (p.passes == 2) eu = *reinterpret_cast<const f32x4*>(p.eps + p.n + idx);
    }
    const bool first = i == p.first_step;   // (the same in every lane) no history yet: x0_prev is not read
    if (!first) xp = *reinterpret_cast<const f32x4*>(p.x0_prev + idx);
    f32x4 cr[5];
    load_coef_row(p.coef, i, cr);
    const f32x4 ms = *reinterpret_cast<const f32x4*>(p.coef_ms + (size_t)i * kMsCount);
    float c[kCoefCount];
#pragma unroll
    for (int k = 0; k < kCoefCount; ++k) c[k] = cr[k >> 2][k & 3];
    f32x4 out, x0v;
    // what sampler_update reads: the launch's own arguments, or -- guided -- those with the row's weight
    const auto& up = [&]() -> decltype(auto) {
      if constexpr (GUIDED) return with_row_weight(p, wt);
      else return (p);
    }();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float x0 = sampler_update<MODE, kFormX0>(up, c, i, zz[k], ec[k], eu[k]);
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
  publish_next_step(p, i);
}

void launch_sampler_step(const SamplerMultistepParams& sp, hipStream_t s) {
  launch_sampler_family(sp, s, [](auto m) { return sampler_multistep_kernel<decltype(m)::value>; });
}
}  // namespace msd
