// The launches of the sampler's keep form (msd_sample_keep, msd_sample_edit): the keep instances of sampler_step_kernel,
// the unscale that passes the caller's mel through on kept frames, the part-way start of msd_sample_edit and the resampling
// jump of msd_sample_resample.  msd_api.hip includes this file LAST: the template instances a
// translation unit emits follow the order of their first use, so the keep instances land behind every kernel the
// library had before and those move by 6.4 KB in the code object instead of by 47 KB.  Every one of them is
// instruction for instruction what it was either way, and yet the placement alone shows on the clock: one box, three
// libraries in rotating order, 1000-step segments of base_with_context, three rounds each -- parent commit 941.1 ms (own
// spread 3.1), keep instances emitted beside the plain ones 952.1 ms (1.5), emitted last 947.5 ms (1.9): block B of
// profiles/keep_frames_ab.log, DESIGN 9.  That is why these definitions are not inline and not in elementwise.h; the
// file belongs to msd_api.hip alone.
#pragma once
#include "elementwise.h"
namespace msd {
void launch_sampler_step(const SamplerKeepParams& sp, hipStream_t s) {
  launch_sampler_family(sp, s, [](auto m) { return sampler_step_kernel<decltype(m)::value, SamplerKeepParams>; });
}

// the same on the free frames; a frame known THROUGHOUT (release word 1: msd_sample_keep's kept frame) gets the caller's own
// mel values, whatever they are.  A frame released part-way (word > 1, msd_sample_edit) was sampled: unscaled like a free one.
__global__ void unscale_keep_kernel(const float* x0, const float* known, const int32_t* keep, float* out, int n,
                                    int n_dims, float fmin, float fmax) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = keep[i / n_dims] == 1 ? known[i] : (x0[i] + 1.0f) / 2.0f * (fmax - fmin) + fmin;
}


void launch_unscale_keep(const float* x0, const float* known, const int32_t* keep, float* out, int n, int n_dims, float fmin,
                         float fmax, hipStream_t s) {
  hipLaunchKernelGGL(unscale_keep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x0, known, keep, out, n, n_dims,
                     fmin, fmax);
}

// msd_sample_keep's flags -> release words: any non-zero flag = known throughout = 1
__global__ void normalize_flags_kernel(const int32_t* in, int32_t* out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = in[i] != 0;
}

void launch_normalize_flags(const int32_t* in, int32_t* out, int n, hipStream_t s) {
  hipLaunchKernelGGL(normalize_flags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
}

// The part-way start of msd_sample_edit: a direct sample of q(z_t | x0 = xk) at the start index (the reference's
// diffusion_forward, diffusion_utils.py:109-117: mean alpha x0, std sigma), in ONE pass over [B, T, n]:
//   xk = scale_features(clip=True) of the caller's mel  -- scale_clip_kernel's expression, so its bits
//   z  = fmaf(sigma, eps, alpha * xk)                   -- the product rounded, then one fused multiply-add; contraction off,
//                                                          so that this line is the operation order (tests/edit_spec.py)
// written as fp32 and as operand planes, with the range flag fed as split_z feeds it for the plain start.  eps is the call's
// own initial draw, which the fill kernels (or the init_z copy) have just put into z: a thread reads its float4 of eps
// before it writes its float4 of z, and no other thread touches those elements.  A float4 per lane and step of the
// grid-stride loop; the grid is capped at eight blocks per CU.
__global__ void __launch_bounds__(256) diffuse_to_step_kernel(DiffuseParams p) {
#pragma clang fp contract(off)
  RangeCheck rc;
  const int stride = (int)gridDim.x * 1024;
  for (int idx = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4; idx < p.n; idx += stride) {
    const f32x4 mel = *reinterpret_cast<const f32x4*>(p.mel + idx);
    const f32x4 ep = *reinterpret_cast<const f32x4*>(p.eps + idx);
    f32x4 xk, z;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float f = fminf(fmaxf(mel[k], p.fmin), p.fmax);
      xk[k] = (f - p.fmin) / (p.fmax - p.fmin) * 2.0f + (-1.0f);
      z[k] = fmaf(p.sigma, ep[k], p.alpha * xk[k]);
    }
    *reinterpret_cast<f32x4*>(p.xk + idx) = xk;
    *reinterpret_cast<f32x4*>(p.z + idx) = z;
    uint32_t h[2], l[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      rc.see(z[2 * k], z[2 * k + 1]);
      split2_h16(z[2 * k], z[2 * k + 1], h[k], l[k]);
    }
    *reinterpret_cast<uint2*>(p.z_hi + idx) = make_uint2(h[0], h[1]);
    if (p.z_lo) *reinterpret_cast<uint2*>(p.z_lo + idx) = make_uint2(l[0], l[1]);
  }
  rc.commit(p.sat, p.sat_tag);
}

void launch_diffuse_to_step(const DiffuseParams& dp, hipStream_t s) {
  const int blocks = (dp.n / 4 + 255) / 256;
  hipLaunchKernelGGL(diffuse_to_step_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, dp);
}

// The resampling jump of msd_sample_resample (RePaint, Lugmayr et al. 2022): the state at the bottom level s of a block of
// steps diffused back to the block's top level t, one sample of q(z_t | z_s) in ONE pass over [B, T, n]:
//   z' = fmaf(b, eps, a * z)      a = alpha_t / alpha_s, b = sqrt(1 - a^2)
// the product rounded, then one fused multiply-add; contraction off, so that this line is the operation order
// (tests/resample_spec.py).  Known and free frames alike: a known frame follows q(z_t | xk) before and after.  Written as
// fp32 and as operand planes, the range flag fed as the sampler feeds it.  A float4 per thread and sampler_step_kernel's
// geometry (block x = elements [1024 x, 1024 x + 1024), key row x / row_blocks), because eps is drawn with that kernel's
// functions under the pass's key rows: no grid-stride loop, the element index is the thread's.  The last block installs
// the pass's rows in the sampler's key table and sets the scan index; nobody reads either during this launch (the draw
// above reads p.keys, another buffer), and the kernel boundary orders both in front of the next step.
__global__ void __launch_bounds__(256) renoise_kernel(RenoiseParams p) {
#pragma clang fp contract(off)
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const int idx = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
  if (idx < p.n) {
    const f32x4 zz = *reinterpret_cast<const f32x4*>(p.z_in + idx);
    f32x4 ep;
    if (p.eps != nullptr) {
      ep = *reinterpret_cast<const f32x4*>(p.eps + idx);
    } else {
      const uint32_t row = blockIdx.x / (uint32_t)p.row_blocks;
      const u32x4* rkp = reinterpret_cast<const u32x4*>(p.keys + (size_t)row * kRngWords);
      const u32x4 rk0 = rkp[0], rk1 = rkp[1];
      const bool per_row = rk1[3] != 0u;
      const uint32_t e = per_row ? (uint32_t)idx - row * (uint32_t)p.row_blocks * kRngRowBlock : (uint32_t)idx;
      const uint32_t span = per_row ? (uint32_t)p.row_blocks * kRngRowBlock : (uint32_t)p.n;
      if (rk1[0] == kRngThreefry) {   // normal(key, [B | 1, T, n]) under the row's (already folded) key; span % 4 == 0: no zero pad
        const uint32_t half = span >> 1;
#pragma unroll
        for (int k = 0; k < 4; ++k) ep[k] = threefry_normal_at(rk1[1], rk1[2], e + (uint32_t)k, half);
      } else {   // sub-sequence 0 of the row's Philox key: what msd_fill_normal writes for it (e / 4 = the counter block)
        float d[4];
        philox_normal4(e >> 2, 0u, rk0[0], rk0[1], rk0[2], rk0[3], d);
        ep = f32x4{d[0], d[1], d[2], d[3]};
      }
    }
    f32x4 z;
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = fmaf(p.b, ep[k], p.a * zz[k]);
    *reinterpret_cast<f32x4*>(p.z + idx) = z;
    RangeCheck rc;
    uint32_t h[2], l[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      rc.see(z[2 * k], z[2 * k + 1]);
      split2_h16(z[2 * k], z[2 * k + 1], h[k], l[k]);
    }
    *reinterpret_cast<uint2*>(p.z_hi + idx) = make_uint2(h[0], h[1]);
    if (p.z_lo) *reinterpret_cast<uint2*>(p.z_lo + idx) = make_uint2(l[0], l[1]);
    rc.commit(p.sat, p.sat_tag);
  }
  if (blockIdx.x == gridDim.x - 1) {
    if (p.key_table != nullptr)
      for (int w = (int)threadIdx.x; w < p.key_words; w += 256) p.key_table[w] = p.keys[w];
    if (p.step_ptr != nullptr && threadIdx.x == 0) { p.step_ptr[0] = p.next_step; p.step_ptr[1] = p.next_step; }
  }
}

void launch_renoise(const RenoiseParams& rp, hipStream_t s) {
  hipLaunchKernelGGL(renoise_kernel, dim3((unsigned)((rp.n / 4 + 255) / 256)), dim3(256), 0, s, rp);
}
}  // namespace msd
