// The sampler's GUIDED form (msd_sample_guided): the classifier-free guidance weight of a row of z is a word of a device
// table, not the handle's msd_config.cfg_weight baked into the launch, so one handle and one set of captured graphs serve
// every weight, a weight per row of a batched call, and guidance limited to an interval of the scan (outside it a step
// is the reference's cond_wt == 1 branch and runs the one-pass plan with the kernels the library always had).
//
// The kernels are instances of sampler_step_kernel (elementwise.h) and sampler_multistep_kernel (multistep_tail.h) on the
// guided argument structs, one per model-output mode each; the update they run is sampler_update, the one text of every
// form, with the row's weight where the other instances read SamplerParams::cond_wt -- so a scalar weight w gives the
// bits of a handle created with cfg_weight = w.  This file belongs to msd_api.hip alone and is included LAST, behind
// multistep_tail.h: the six instances land behind every kernel the library had before (placement shows on the clock:
// keep_frames_tail.h).
#pragma once
#include "elementwise.h"
#include "multistep_tail.h"
namespace msd {
static_assert(sizeof(SamplerParams) == 120, "the plain instances' argument block: two 64-byte lines");
static_assert(sizeof(SamplerGuidedParams) == 128, "the guided instances' argument block: still two 64-byte lines");

void launch_sampler_step(const SamplerGuidedParams& sp, hipStream_t s) {
  launch_sampler_family(sp, s, [](auto m) { return sampler_step_kernel<decltype(m)::value, SamplerGuidedParams>; });
}
void launch_sampler_step(const SamplerMultistepGuidedParams& sp, hipStream_t s) {
  launch_sampler_family(sp, s, [](auto m) { return sampler_multistep_kernel<decltype(m)::value, SamplerMultistepGuidedParams>; });
}
}  // namespace msd
