"""Shared test helpers: product spec -> oracle configs, seeded inputs."""
import dataclasses

import numpy as np
import pytest

import msd_amd
from oracle import backend, fast, net, predict, sampler

T5_FIELDS = ['vocab_size', 'emb_dim', 'num_heads', 'num_encoder_layers', 'num_decoder_layers',
             'head_dim', 'mlp_dim', 'mlp_activations', 'max_decoder_noise_time',
             'decoder_cross_attend_style', 'position_encoding', 'context_positions']


def oracle_configs(spec):
  t5 = net.T5Config(**{k: getattr(spec.t5, k) for k in T5_FIELDS})
  d = spec.diffusion

  def sched(x):
    return sampler.DiffusionSchedule(x.name, start=x.start, stop=x.stop, num_steps=x.num_steps)

  dc = sampler.DiffusionConfig(
      model_output=d.model_output, train_schedule=sched(d.train_schedule),
      classifier_free_guidance=sampler.ClassifierFreeGuidanceConfig(
          eval_condition_weight=d.classifier_free_guidance.eval_condition_weight),
      sampler=sampler.SamplerConfig(
          name=d.sampler.name, clip_x0=d.sampler.clip_x0, logvar_type=d.sampler.logvar_type,
          schedule=sched(d.sampler.schedule)))
  return t5, dc


def make_batch(spec, batch=1, seed=7, ctx_mask='ones', segment0=0):
  """Model features with seeded content.  ctx_mask: 'ones' | 'zeros' | 'ragged'."""
  rng = np.random.default_rng(seed)
  toks = np.concatenate([msd_amd.synthetic.segment_tokens(spec, segment0 + b, min_len=8,
                                                           max_len=spec.task_feature_lengths['inputs'] - 2)
                         for b in range(batch)], 0)
  out = {'encoder_input_tokens': toks}
  n = 128
  if spec.has_context:
    c = spec.task_feature_lengths['targets_context']
    out['encoder_continuous_inputs'] = rng.uniform(-13, 5, (batch, c, n)).astype(np.float32)
    if ctx_mask == 'ones':
      m = np.ones((batch, c), np.int32)
    elif ctx_mask == 'zeros':
      m = np.zeros((batch, c), np.int32)
    else:  # a valid prefix of different length per row (exercises terminal_relative)
      m = np.zeros((batch, c), np.int32)
      for b in range(batch):
        m[b, :int(rng.integers(1, c))] = 1
    out['encoder_continuous_mask'] = m
  out['decoder_target_tokens'] = np.zeros((batch, spec.task_feature_lengths['targets'], n), np.float32)
  return out


def make_noise(spec, batch=1, seed=11):
  rng = np.random.default_rng(seed)
  t, n = spec.task_feature_lengths['targets'], 128
  steps = spec.diffusion.sampler.schedule.num_steps
  return (rng.standard_normal((batch, t, n)).astype(np.float32),
          rng.standard_normal((steps, batch, t, n)).astype(np.float32))


# ---- what the GPU suites of the sampler's forms share (test_gpu_keep_frames, _edit_strength, _few_steps, _sample_forms,
# the sampler cases of test_gpu_fused_ops) ----
@pytest.fixture(scope='module', name='torch')
def gpu_torch():
  """Those modules' `torch` fixture (a module imports this function by name): torch, with the MI355X present and the
  library loaded."""
  import torch
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  msd_amd.native.load()
  return torch


def dev(torch, a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


def bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def round_to_plane(x32, precision):
  """float32 -> the plane type of `precision` (IEEE half via numpy, subnormals kept; bfloat16 via torch on the CPU), round
  to nearest even -> float32."""
  x32 = np.ascontiguousarray(x32, np.float32)
  if precision.startswith('bf16'):
    import torch
    return torch.from_numpy(x32).to(torch.bfloat16).to(torch.float32).numpy()
  with np.errstate(over='ignore'):
    return x32.astype(np.float16).astype(np.float32)


def planes_merged(z32, precision):
  """What the device's operand planes of z merge back to, exactly: hi = P(z), lo = P(z - hi) (split2_h16, common.h) and
  hi + lo in float32 (merge_planes_kernel) -- hi + 0 for the one-plane precisions 'f16' / 'bf16', the kernel's expression
  (it turns a hi of -0 into +0).  z - hi and hi + lo are exact in float32 for both plane types
  (tests/test_planes_merged_host.py holds this function against a nearest-representable search in float64), so the device's
  merged planes must equal this array bit for bit, subnormal lo values included."""
  assert precision in ('f16', 'f16x3', 'bf16', 'bf16x3'), precision
  z32 = np.ascontiguousarray(z32, np.float32)
  hi = round_to_plane(z32, precision)
  if not precision.endswith('x3'):
    return hi + np.float32(0.0)
  with np.errstate(invalid='ignore'):   # (a NaN or Inf in z stays visible: NaN out)
    return hi + round_to_plane(z32 - hi, precision)


# The range cases of the ops whose output is one product plus one fmaf of their arguments (msd_op_invert_step,
# _diffuse_to_step, _renoise): an exact 65504 cannot be constructed there, so one output element is aimed 2^-12 below the
# half-plane limit (must pass) and 2^-12 above it (RangeError on the half-plane build, fine with bfloat16 planes).  The
# margin is ~4000 times the float32 error of those two operations: the float32 specification alone decides the side.
HALF_MAX = 65504.0
RANGE_TARGETS = [('inside', HALF_MAX * (1 - 2.0 ** -12)), ('outside', HALF_MAX * (1 + 2.0 ** -12))]


def check_range_case(call, side, precision, spec32, spec64, target, e):
  """call() -> (z, merged planes) runs the op on inputs whose float64 specification spec64 puts `target` at flat element e:
  asserts on the host that the float32 specification lies on the intended side of 65504 there, then the device's verdict."""
  from msd_amd import native
  v32, v64 = float(np.asarray(spec32).reshape(-1)[e]), float(np.asarray(spec64).reshape(-1)[e])
  assert abs(v64 / target - 1) < 2.0 ** -20, (v64, target)
  assert (v32 < HALF_MAX) if side == 'inside' else (v32 > HALF_MAX), (side, v32)
  others = np.delete(np.abs(np.asarray(spec64)).reshape(-1), e)
  assert others.max() < 100.0   # (the one large element decides)
  if side == 'outside' and not precision.startswith('bf16'):
    with pytest.raises(native.RangeError):
      call()
    return
  z, zp = call()   # no RangeError: the flag word stayed 0
  got = float(z.reshape(-1)[e])
  print('range case %s %s: device %.9g, float32 spec %.9g, float64 spec %.9g' % (side, precision, got, v32, v64))
  assert abs(got / v64 - 1) < 2.0 ** -20 and ((got < HALF_MAX) if side == 'inside' else (got > HALF_MAX)), (side, got)
  np.testing.assert_array_equal(bits(zp), bits(planes_merged(z, precision)))


def known_mel(shape, seed=21):
  """A mel that leaves the codec's range [log 1e-5, 4] at both ends."""
  return np.random.default_rng(seed).uniform(-13.0, 5.0, shape).astype(np.float32)


def sampler_spec(sampler='ddpm', model_output='eps', logvar='large', schedule='cosine', train='cosine',
                 cfg_weight=5.0, clip=True, steps=50):
  """The tiny preset with every switch of the sampler update's arithmetic (the stand-alone sampler ops)."""
  from msd_amd import config as C
  spec = msd_amd.config.preset('tiny', num_steps=steps, cfg_weight=cfg_weight)
  d = spec.diffusion
  ss = C.DiffusionSchedule(schedule, start=1e-4 if schedule == 'linear' else None,
                           stop=2e-2 if schedule == 'linear' else None, num_steps=steps)
  ts = C.DiffusionSchedule(train, start=2e-4 if train == 'linear' else None,
                           stop=3e-2 if train == 'linear' else None, num_steps=80 if train == 'linear' else None)
  d = dataclasses.replace(d, model_output=model_output, train_schedule=ts,
                          sampler=dataclasses.replace(d.sampler, name=sampler, logvar_type=logvar, clip_x0=clip,
                                                      schedule=ss))
  return dataclasses.replace(spec, diffusion=d)


def preset_spec(preset, steps, sampler='ddpm'):
  spec = msd_amd.config.preset(preset, num_steps=steps)
  d = spec.diffusion
  return dataclasses.replace(spec, diffusion=dataclasses.replace(d, sampler=dataclasses.replace(d.sampler, name=sampler)))


def cached_model(cache, preset, steps, sampler='ddpm'):
  """(spec, params, model) -- one two-row handle per configuration in the calling module's `cache`."""
  key = (preset, steps, sampler)
  if key not in cache:
    spec = preset_spec(preset, steps, sampler)
    params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
    cache[key] = (spec, params, msd_amd.InferenceModel(params, spec, batch_size=2, **ALL_PLANES))
  return cache[key]


def attention_ref(q, k, v, heads, valid, rstd=None):
  """float64 oracle attention of [n_q, heads*64] queries on the first `valid` keys; rstd (per query row) scales the
  queries first -- the un-normalised form's algebra."""
  from oracle import ops
  xp = backend.TorchBackend('float64')
  nq = q.shape[0]
  q64 = q.astype(np.float64) if rstd is None else q.astype(np.float64) * rstd[:, None]
  sh = lambda x, n: xp.asarray(np.ascontiguousarray(x, np.float64).reshape(1, n, heads, 64))
  out = ops.dot_product_attention(xp, sh(q64, nq), sh(k[:valid], valid), sh(v[:valid], valid))
  return xp.to_numpy(out).reshape(nq, heads * 64).astype(np.float64)


def rms(a, b):
  a = np.asarray(a, np.float64)
  b = np.asarray(b, np.float64)
  return float(np.sqrt(np.mean((a - b) ** 2)))


# Short DDPM chains (3 - 8 huge steps) are ill-conditioned amplifiers: assert_fp32_class below can tell float32-class
# arithmetic from anything coarser.  Since round 4 the product's default 'f16x3' mode keeps hi + lo planes EVERYWHERE,
# the query side of the decoder's attentions included (round 3's default ran Q and the softmax weights on one half
# plane: 2.5 % faster, fine on O(1) logits, 2.8x the float32 floor on sharp attention -- DESIGN.md 3).  One plane is an
# opt-in (ONE_QUERY_PLANE): its single passes are asserted against the same 2e-4 / 3e-4 bounds as the default's, its
# op-level behaviour on sharp logits in tests/test_gpu_ops.py.
ALL_PLANES = dict(attention_query_planes=2)        # = the library default since round 4 (kept explicit where a test's
                                                    # statistics REQUIRE it, whatever the default becomes)
ONE_QUERY_PLANE = dict(attention_query_planes=1)    # the opt-in: Q and the softmax weights as one half plane each


def assert_fp32_class(got, ref64, ref32, what=''):
  """Short DDPM chains are ill-conditioned by construction: at the first step
  (t = 1, logsnr = -20) x0 = 22026 (z - eps) is clipped to +-1 for all but a few
  marginal elements, where a 1e-6 difference in eps decides the outcome.  Any two valid
  float32-class evaluations (the float32 oracle included) therefore disagree on a
  handful of elements by O(1) while agreeing to ~1e-6 on the rest, and rms is
  dominated by those few.  So the device is compared with the float64 oracle on the
  BULK (median error) and on the COUNT of outliers, using the float32 oracle's own
  deviation from float64 as the yardstick.  (The 1000-step runs use the absolute
  1e-3 rms bar: tests/test_golden.py.)"""
  e_dev = np.abs(np.asarray(got, np.float64) - ref64).ravel()
  e_f32 = np.abs(np.asarray(ref32, np.float64) - ref64).ravel()
  med_dev, med_f32 = np.median(e_dev), np.median(e_f32)
  out_dev, out_f32 = float((e_dev > 1e-2).mean()), float((e_f32 > 1e-2).mean())
  print('%s median |err| device %.2e / f32-oracle %.2e; outliers(>1e-2) device %.4f / f32-oracle %.4f; rms %.2e / %.2e'
        % (what, med_dev, med_f32, out_dev, out_f32, rms(got, ref64), rms(ref32, ref64)))
  assert med_dev <= 1.5 * med_f32 + 1e-6, 'bulk error is not fp32-class'   # (worst over round 4's GPU suite: 1.08)
  # Outliers: at most twice the float32 oracle's own count plus 0.3 % of the elements.  bf16x3 products carry
  # ~2^-17 relative error against float32's 2^-24, so more marginal elements flip at the clip boundary of the
  # first steps, and WHICH ones flip depends on the last bits: two builds of the same kernels whose single
  # decoder passes agree to 4e-6 relative (round 2: a code-generation difference in the attention kernel,
  # DESIGN 11) gave 0.0001 and 0.0020 on the tiny golden, against the float32 oracle's 0.0002.
  assert out_dev <= 2 * out_f32 + 3e-3, 'too many outliers'
  # A third criterion, on the error DISTRIBUTION below the outlier threshold (the two above
  # are nearly blind to a kernel that is moderately wrong everywhere).  A short chain turns one rounding into a
  # spread of errors between 1e-6 and 1e-2 whatever the arithmetic, on different elements for every evaluation -- so an
  # rms over "the elements the float32 oracle gets right" cannot work (measured on the MI355X: the device's rms over
  # those is 3 - 8x the float32 oracle's, simply because its amplified elements are other ones).  What two float32-
  # class evaluations do share is HOW MANY elements end up beyond a given error: on tiny_context the float32 oracle,
  # the half-plane emulation and the bfloat16-plane emulation have 5.4 / 5.5 / 6.5 % of their elements beyond 1e-3 and
  # 27.1 / 27.5 / 30.5 % beyond 1e-4, a single half plane ('f16') 33 % and 35 %.
  # MI355X, 46 short-chain cases (profiles/r03l_tests.log): the device is within +-0.02 of the float32 oracle's fraction at
  # both thresholds (worst ratio 1.07)
  # Round 4 (the bounds of round 3, x1.25 / x1.15 + 0.01, would have passed the bfloat16-plane
  # emulation's 6.5 % against the float32 oracle's 5.4 %): x1.10 / x1.12 + 0.005.  The bfloat16-plane figure is now
  # outside (bound 6.44 %); the worst device case of round 4's suite (profiles/r04z_gpu_tests.log, 32 short-chain cases
  # in both attention modes) is x1.017 / x1.070, +0.003 / +0.0185 absolute.
  for tau, factor, slack in ((1e-3, 1.10, 0.005), (1e-4, 1.12, 0.005)):
    f_dev, f_f32 = float((e_dev > tau).mean()), float((e_f32 > tau).mean())
    print('%s elements beyond %.0e: device %.4f / f32-oracle %.4f' % (what, tau, f_dev, f_f32))
    assert f_dev <= factor * f_f32 + slack, 'too many elements beyond %.0e for float32-class arithmetic' % tau
