// The sampler's INVERSION form (msd_invert): deterministic DDIM inversion, one step UP the scan per launch -- from a mel
// and the tokens it was rendered from to the init_z that renders it.  One kernel per model-output mode and its launch.
// msd_api.hip includes this file LAST, behind loss_tail.h: the three instances land behind every kernel the library had
// before (placement shows on the clock: keep_frames_tail.h).
//
// A call of K steps has levels 0 .. K; level l has time l / K, logsnr_l of the SAMPLER schedule, alpha_l =
// sqrt(sigmoid(logsnr_l)), sigma_l = sqrt(sigmoid(-logsnr_l)).  The forward DDIM step at scan index i takes level i + 1 to
// level i: z_i = alpha_i x0 + sigma_i eps with (x0, eps) of eval_step.body at time (i + 1) / K; index 0 returns x0.  The step
// here, at scan index i = 0 .. K - 1, is ONE decoder evaluation of the state it has (level i), at the UPPER level's time
// (i + 1) / K -- so the decoder reads table row i, as the forward step at index i does -- and no draw:
//   eps  = pred_eps(u, time (i + 1) / K)     sampler_update's eps form (elementwise.h, the one text of every form): the model
//                                            output -> eps at the TRAIN schedule, w eps_c + (1 - w) eps_u when w != 1
//   z_up = fmaf(b_i, eps, a_i * u)           the product rounded, then one fused multiply-add; contraction off
//   a_i = alpha_{i+1} / alpha_i, b_i = sigma_{i+1} - a_i sigma_i    (i >= 1)
//   a_0 = alpha_1,               b_0 = sigma_1                       (the mirror of "index 0 returns x0")
// This is the exact inverse of the forward DDIM step with eps FROZEN -- taken at the state below instead of the state
// above -- where the train and the sampler schedule agree at t; with a `linear` sampler schedule, or train != sampler
// schedule, the step is what these lines say and no more.  NO clip: the clip is not invertible where it binds, so the
// inversion ignores sampler.clip_x0.  The result of K steps is z at level K in model units, not unscaled.
//
// a and b come from a [K][4] side table (msd_api.hip build_invert_rows: {a, b, 0, 0}), one 16-byte load beside the five of
// the 20-float row, which stays what the other forms load and gives the train schedule's conversions here.  The weight of
// this block's row of z comes from a device table, read as the guided form reads it; a weight of exactly 1 takes one
// pass and does not read the second.  The launch's last block publishes i + 1: the scan index counts UP.
#pragma once
#include "elementwise.h"
namespace msd {
static_assert(sizeof(SamplerParams) == 120, "the plain instances' argument block: two 64-byte lines");
static_assert(sizeof(SamplerInvertParams) == 136, "the inversion's argument block: three 64-byte lines");

// publish_next_step's mirror: the next scan index UP, published by the launch's last block under the same ordering
__device__ __forceinline__ void publish_step_above(const SamplerParams& p, int i) {
  __syncthreads();
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) p.step_ptr[p.step_from_slot1 ? 0 : 1] = i + 1;
}

template <int MODE>
__global__ void __launch_bounds__(256) sampler_invert_kernel(SamplerInvertParams p) {
#pragma clang fp contract(off)
  warm_kernargs<kernarg_lines<SamplerInvertParams>()>();
  const int i = p.step_from_slot1 ? p.step_ptr[1] : p.step_ptr[0];
  const float wt = p.row_wt[blockIdx.x / (uint32_t)p.row_blocks];
  const int idx = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (idx < p.n) {
    // as in sampler_step_kernel: what does not depend on the scan index goes out first, the rows behind the index
    const f32x4 zz = *reinterpret_cast<const f32x4*>(p.z + idx);
    const f32x4 ec = *reinterpret_cast<const f32x4*>(p.eps + idx);
    f32x4 eu = {0.f, 0.f, 0.f, 0.f};
    if (wt != 1.0f) eu = *reinterpret_cast<const f32x4*>(p.eps + p.n + idx);   // (the same in every lane)
    f32x4 cr[5];
    load_coef_row(p.coef, i, cr);
    const f32x4 iv = *reinterpret_cast<const f32x4*>(p.coef_inv + (size_t)i * kInvCount);
    float c[kCoefCount];
#pragma unroll
    for (int k = 0; k < kCoefCount; ++k) c[k] = cr[k >> 2][k & 3];
    const SamplerParams q = with_row_weight(p, wt);
    f32x4 out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float eps = sampler_update<MODE, kFormEps>(q, c, i, zz[k], ec[k], eu[k]);
      out[k] = fmaf(iv[kInvB], eps, iv[kInvA] * zz[k]);
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
  publish_step_above(p, i);
}

void launch_sampler_invert(const SamplerInvertParams& sp, hipStream_t s) {
  launch_sampler_family(sp, s, [](auto m) { return sampler_invert_kernel<decltype(m)::value>; });
}
}  // namespace msd
