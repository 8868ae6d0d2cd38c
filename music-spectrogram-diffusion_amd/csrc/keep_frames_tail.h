// The launches of the sampler's keep form (msd_sample_keep): the keep instances of sampler_step_kernel and the unscale that
// passes the caller's mel through on kept frames.  msd_api.hip includes this file LAST: the template instances a
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
  const dim3 grid((sp.n / 4 + 255) / 256), block(256);
  if (sp.model_output == kOutX0) hipLaunchKernelGGL((sampler_step_kernel<kOutX0, SamplerKeepParams>), grid, block, 0, s, sp);
  else if (sp.model_output == kOutV) hipLaunchKernelGGL((sampler_step_kernel<kOutV, SamplerKeepParams>), grid, block, 0, s, sp);
  else hipLaunchKernelGGL((sampler_step_kernel<kOutEps, SamplerKeepParams>), grid, block, 0, s, sp);
}

// the same on the free frames; a kept frame (msd_sample_keep) gets the caller's own mel values, whatever they are
__global__ void unscale_keep_kernel(const float* x0, const float* known, const int32_t* keep, float* out, int n,
                                    int n_dims, float fmin, float fmax) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = keep[i / n_dims] ? known[i] : (x0[i] + 1.0f) / 2.0f * (fmax - fmin) + fmin;
}


void launch_unscale_keep(const float* x0, const float* known, const int32_t* keep, float* out, int n, int n_dims, float fmin,
                         float fmax, hipStream_t s) {
  hipLaunchKernelGGL(unscale_keep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x0, known, keep, out, n, n_dims,
                     fmin, fmax);
}
}  // namespace msd
