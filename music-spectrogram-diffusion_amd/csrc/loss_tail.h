// The two kernels of the denoising loss (msd_loss, msd_op_diffusion_loss): the reference's evaluation loss (models.py
// loss_fn over diffusion_utils.get_diffusion_training_input and calculate_loss) at a time index of the handle's grid.
//   loss_diffuse_kernel        x0 = scale_features(target, clip=True); z_t = fmaf(sigma, eps, alpha x0) at the TRAIN schedule's
//                              (alpha, sigma) of the index; arms the scan index for the decoder pass behind it
//   diffusion_loss_kernel      (eps_hat, x0_hat) = convert_model_output of every pass, the element losses against (eps, x0),
//                              masked, summed per frame
// Dropout is off: this is an evaluation (the reference's loss_fn passes enable_dropout=True even in eval; not restated).
// Both have renoise_kernel's geometry -- block x = elements [1024 x, 1024 x + 1024), key row x / row_blocks, a float4 per
// thread -- because eps is drawn with the sampler's functions under the call's key rows, and drawn AGAIN in the second
// kernel instead of being kept in a second [B, T, n] buffer.  The time list, the position in it and the caller's buffers
// live in device memory (elementwise.h LossCall), so one captured (diffuse, decoder, loss) graph is replayed once per time
// with no host round trip.  msd_api.hip includes this file LAST, behind guided_tail.h: the instances land behind every
// kernel the library had before (placement shows on the clock: keep_frames_tail.h).
#pragma once
#include "elementwise.h"
namespace msd {
// The thread's four draws of the evaluation at time index i: what sampler_step_kernel draws for scan index i (Philox
// sub-sequence 1 + i; Threefry normal(fold_in(key, i), ...)), per row of z in the per-row mode, or the caller's buffer.
__device__ __forceinline__ f32x4 loss_eps4(const float* eps_buf, size_t eps_off, const uint32_t* keys, int row_blocks, int n,
                                           int idx, int i) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  if (eps_buf != nullptr) return *reinterpret_cast<const f32x4*>(eps_buf + eps_off + idx);
  const uint32_t row = blockIdx.x / (uint32_t)row_blocks;
  const u32x4* rkp = reinterpret_cast<const u32x4*>(keys + (size_t)row * kRngWords);
  const u32x4 rk0 = rkp[0], rk1 = rkp[1];
  const bool per_row = rk1[3] != 0u;
  const uint32_t e = per_row ? (uint32_t)idx - row * (uint32_t)row_blocks * kRngRowBlock : (uint32_t)idx;
  const uint32_t span = per_row ? (uint32_t)row_blocks * kRngRowBlock : (uint32_t)n;
  f32x4 ep;
  if (rk1[0] == kRngThreefry) {   // span % 4 == 0: no zero pad
    uint32_t f0 = 0u, f1 = (uint32_t)i;
    threefry2x32(rk1[1], rk1[2], f0, f1);
    const uint32_t half = span >> 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) ep[k] = threefry_normal_at(f0, f1, e + (uint32_t)k, half);
  } else {   // e / 4 = the counter block
    float d[4];
    philox_normal4(e >> 2, 1u + (uint32_t)i, rk0[0], rk0[1], rk0[2], rk0[3], d);
    ep = f32x4{d[0], d[1], d[2], d[3]};
  }
  return ep;
}

// x0 and z_t of the evaluation the cursor points at.  x0 is scale_clip_kernel's expression; z = fmaf(sigma, eps, alpha * x0):
// the product rounded, then one fused multiply-add; contraction off, so that this line is the operation order
// (tests/loss_spec.py).  z is written as fp32 and as operand planes, the range flag fed as the sampler feeds it.  The last
// block copies the cursor to its second word and sets both words of the scan index to the evaluation's time index: nobody
// reads either during this launch, and the kernel boundary orders both in front of the decoder pass.
// (A template for its PLACE alone: a plain kernel is emitted in source order among the plain kernels -- behind renoise_kernel,
// in front of every template instance the library has, which all move by its size --, an instance in the order of first use:
// here, behind everything.  Checked in the code object)
template <int = 0>
__global__ void __launch_bounds__(256) loss_diffuse_kernel(LossDiffuseParams p) {
#pragma clang fp contract(off)
  // (field by field: word 1 of the cursor, which this launch's last block writes, is not read)
  const float* target = p.call->target;
  const float* eps_buf = p.call->eps;
  const int j = p.call->cursor[0];
  const float* tr = p.call->times + (size_t)j * kLossTimeWords;
  const float alpha = tr[kLossTimeAlpha], sigma = tr[kLossTimeSigma];
  const int i = __float_as_int(tr[kLossTimeIndex]);
  const int idx = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
  if (idx < p.n) {
    const f32x4 mel = *reinterpret_cast<const f32x4*>(target + idx);
    const f32x4 ep = loss_eps4(eps_buf, (size_t)j * (size_t)p.n, p.keys, p.row_blocks, p.n, idx, i);
    f32x4 x0, z;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float f = fminf(fmaxf(mel[k], p.fmin), p.fmax);
      x0[k] = (f - p.fmin) / (p.fmax - p.fmin) * 2.0f + (-1.0f);
      z[k] = fmaf(sigma, ep[k], alpha * x0[k]);
    }
    *reinterpret_cast<f32x4*>(p.x0 + idx) = x0;
    *reinterpret_cast<f32x4*>(p.z + idx) = z;
    if (p.z_hi) {
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
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    p.call->cursor[1] = j;
    if (p.step_ptr != nullptr) { p.step_ptr[0] = i; p.step_ptr[1] = i; }
  }
}

void launch_loss_diffuse(const LossDiffuseParams& p, hipStream_t s) {
  hipLaunchKernelGGL(loss_diffuse_kernel<0>, dim3((unsigned)((p.n / 4 + 255) / 256)), dim3(256), 0, s, p);
}

// jnp.maximum: a NaN on either side stays a NaN (fmaxf would drop it)
__device__ __forceinline__ float loss_max(float a, float b) { return (a > b || a != a) ? a : b; }

// One element of calculate_loss (diffusion_utils.py:325-366) times its frame's mask value
__device__ __forceinline__ float loss_element(int type, int norm, float eps_hat, float x0_hat, float eps, float x0, float mask) {
#pragma clang fp contract(off)
  const float d_eps = eps_hat - eps, d_x0 = x0_hat - x0;
  const float l_eps = norm == kLossL2 ? d_eps * d_eps : fabsf(d_eps);
  const float l_x0 = norm == kLossL2 ? d_x0 * d_x0 : fabsf(d_x0);
  float l;
  if (type == kLossX0) l = l_x0;
  else if (type == kLossEps) l = l_eps;
  else if (type == kLossMaxX0Eps) l = loss_max(l_x0, l_eps);
  else l = l_eps + l_x0;
  return l * mask;
}

// The per-frame losses of the evaluation at cursor word 1, every pass of the model output.  A thread converts its four
// elements with convert_model_output (the sampler's text, the train schedule's coefficients of row i, uncond = false for
// every pass), and sums its four masked element losses left to right.  A frame is W = n_dims / 4 consecutive threads of one
// block (W a power of two, W | 256); their sums are added through LDS as a pairwise tree, a fixed order: at level s = 1, 2,
// 4, ... < W thread t with t % 2s == 0 adds the sum of thread t + s to its own, and the frame's first thread stores the
// result.  Threads beyond n hold zeros and store nothing.  The last block advances the cursor (word 0 := word 1 + 1).
template <int MODE>
__global__ void __launch_bounds__(256) diffusion_loss_kernel(LossParams p) {
#pragma clang fp contract(off)
  __shared__ float part[2][256];
  // (field by field: word 0 of the cursor, which this launch's last block writes, is not read)
  const float* mask = p.call->mask;
  const float* eps_buf = p.call->eps;
  float* out = p.call->out;
  const int type = p.call->type, norm = p.call->norm;
  const int j = p.call->cursor[1];
  const int i = __float_as_int(p.call->times[(size_t)j * kLossTimeWords + kLossTimeIndex]);
  const int t = (int)threadIdx.x;
  const int idx = ((int)blockIdx.x * 256 + t) * 4;
  const int frame = idx / p.n_dims;
  float sum[2] = {0.f, 0.f};
  if (idx < p.n) {
    const f32x4 zz = *reinterpret_cast<const f32x4*>(p.z + idx);
    const f32x4 xx = *reinterpret_cast<const f32x4*>(p.x0 + idx);
    const f32x4 ep = loss_eps4(eps_buf, (size_t)j * (size_t)p.n, p.keys, p.row_blocks, p.n, idx, i);
    const float mk = mask != nullptr ? mask[frame] : 1.0f;
    f32x4 cr[5];
    load_coef_row(p.coef, i, cr);
    float c[kCoefCount];
#pragma unroll
    for (int k = 0; k < kCoefCount; ++k) c[k] = cr[k >> 2][k & 3];
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      if (ps < p.passes) {
        const f32x4 oo = *reinterpret_cast<const f32x4*>(p.o + (size_t)ps * (size_t)p.n + idx);
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float eh, xh;
          convert_model_output<MODE>(c, zz[k], oo[k], eh, xh, /*uncond=*/false);
          const float l = loss_element(type, norm, eh, xh, ep[k], xx[k], mk);
          acc = k == 0 ? l : acc + l;
        }
        sum[ps] = acc;
      }
    }
  }
  part[0][t] = sum[0];
  part[1][t] = sum[1];
  const int W = p.n_dims >> 2;
  for (int s = 1; s < W; s <<= 1) {
    __syncthreads();
    if ((t & (2 * s - 1)) == 0) {
      part[0][t] += part[0][t + s];
      part[1][t] += part[1][t + s];
    }
  }
  if (idx < p.n && (t & (W - 1)) == 0) {
    const size_t frames = (size_t)(p.n / p.n_dims);
    for (int ps = 0; ps < p.passes; ++ps) out[((size_t)j * (size_t)p.passes + (size_t)ps) * frames + (size_t)frame] = part[ps][t];
  }
  if (blockIdx.x == gridDim.x - 1 && t == 0) p.call->cursor[0] = j + 1;
}

void launch_diffusion_loss(const LossParams& p, hipStream_t s) {
  const dim3 grid((unsigned)((p.n / 4 + 255) / 256)), block(256);
  if (p.model_output == kOutX0) hipLaunchKernelGGL(diffusion_loss_kernel<kOutX0>, grid, block, 0, s, p);
  else if (p.model_output == kOutV) hipLaunchKernelGGL(diffusion_loss_kernel<kOutV>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(diffusion_loss_kernel<kOutEps>, grid, block, 0, s, p);
}
}  // namespace msd
