"""-m gpu: per-call guidance (msd_sample_guided, msd_op_sampler_step_guided / _multistep_guided, predict(guidance=,
guidance_interval=)) against the specification of tests/guidance_spec.py: eval_step bodies of the oracle configured with
the row's weight inside the interval and with weight 1 outside.

Presets tiny / tiny_context: T = 64, n = 128, so a row of z is 8 of the sampler's 1024-element blocks.  The handle has
N = 96 steps and weight 5 (graph_steps 8): calls of 24 steps are whole graphs at (0, 12) / (12, 24) and graphs plus
singles at (6, 18); a 12-step call of (3, 7) runs singles on both sides of every edge."""
import ctypes
import dataclasses

import numpy as np
import pytest

import msd_amd
from tests import guidance_spec as gs, helpers, multistep_spec as ms
from tests.helpers import gpu_torch  # noqa: F401  (the `torch` fixture)

pytestmark = pytest.mark.gpu

N = 96
ROW_WEIGHTS = [1.0, 5.0, 0.0, 2.5]   # the == 1 branch, an ordinary weight, the unconditional pass alone, a fraction


# --------------------------------------------------------------------------------------------------
# 1. one guided update against the spec
# --------------------------------------------------------------------------------------------------
def _ids(c):
  return ','.join('%s=%s' % kv for kv in c.items()) or 'default'


def _op_inputs(rng, dc, i, shape):
  steps = dc.sampler.schedule.num_steps
  z, oc, ou, nz = (rng.standard_normal(shape).astype(np.float32) for _ in range(4))
  if i > steps // 2 and dc.model_output == 'eps':   # at logsnr ~ -20 only eps ~ z leaves x0 inside [-1, 1]
    oc, ou = z + 1e-5 * oc, z + 1e-5 * ou
  return z, oc, ou, nz


def _criterion(what, got, f64, f32):
  """The single-update criterion of tests/test_gpu_fused_ops.py and tests/test_gpu_few_steps.py."""
  scale = max(1.0, float(np.abs(f64).max()))
  e_dev = np.abs(got.astype(np.float64) - f64).max() / scale
  e_f32 = np.abs(f32 - f64).max() / scale
  print('%s: scaled error device %.3e / float32 %.3e' % (what, e_dev, e_f32))
  assert e_dev <= 1e-6 + 4 * e_f32, (what, e_dev, e_f32)


OP_CASES = [dict(), dict(sampler='ddim'), dict(clip=False), dict(model_output='x0'), dict(model_output='v'),
            dict(schedule='linear', train='linear', model_output='x0')]


@pytest.mark.parametrize('case', OP_CASES, ids=_ids)
def test_op_guided_vs_spec(torch, case):
  """msd_op_sampler_step_guided on four rows of 1024 elements with the weights 1 / 5 / 0 / 2.5 in ONE launch, at the first,
  a middle, the second-to-last and the last scan index: row b against eval_step.body of the oracle configured with
  weight[b], and bit for bit the plain op of a config with cfg_weight = weight[b] on that row."""
  from msd_amd import inference, native
  from oracle import backend, sampler
  spec = helpers.sampler_spec(**case)
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, 'f16x3')
  _, dc = helpers.oracle_configs(spec)
  steps = dc.sampler.schedule.num_steps
  rng = np.random.default_rng(5)
  shape = (4, 8, 128)
  for i in (steps - 1, steps // 2, 1, 0):
    z, oc, ou, nz = _op_inputs(rng, dc, i, shape)
    out = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    native.op_sampler_step_guided(cfg, i, helpers.dev(torch, z), helpers.dev(torch, oc), helpers.dev(torch, ou),
                                  helpers.dev(torch, nz), ROW_WEIGHTS, out)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    for b, w in enumerate(ROW_WEIGHTS):
      row = slice(b, b + 1)
      refs = {}
      for name, xp in (('f32', backend.NumpyBackend('float32')), ('f64', backend.NumpyBackend('float64'))):
        noise = [None] * steps
        noise[i] = xp.asarray(nz[row])
        pred = lambda z, time, include_conditioning, _xp=xp: _xp.asarray((oc if include_conditioning else ou)[row])
        refs[name] = np.asarray(sampler.eval_step(xp, noise, gs.with_weight(dc, w), 1, pred)(xp.asarray(z[row]), i), np.float64)
      _criterion('guided %s i=%d w=%g' % (case, i, w), got[row], refs['f64'], refs['f32'])
      cfg_w = inference._to_native_config(helpers.sampler_spec(**dict(case, cfg_weight=w)), msd_amd.audio_codecs.MelGAN(), 1, 'f16x3')
      plain = torch.empty((1,) + shape[1:], dtype=torch.float32, device='cuda')
      native.op_sampler_step(cfg_w, i, helpers.dev(torch, z[row]), helpers.dev(torch, oc[row]),
                             helpers.dev(torch, ou[row]) if w != 1.0 else None, helpers.dev(torch, nz[row]), plain)
      np.testing.assert_array_equal(helpers.bits(got[row]), helpers.bits(plain.cpu().numpy()))
    assert not np.array_equal(got[0], got[1])


MS_OP_CASES = [dict(), dict(clip=False), dict(model_output='x0'), dict(model_output='v')]


@pytest.mark.parametrize('case', MS_OP_CASES, ids=_ids)
def test_op_multistep_guided_vs_spec(torch, case):
  """The same for msd_op_sampler_step_multistep_guided: z_s and the x0_prev it leaves, per row, against multistep_spec.step
  of the oracle configured with the row's weight, and the plain multistep op's bits."""
  from msd_amd import inference, native
  from oracle import backend
  spec = helpers.sampler_spec(**case)
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, 'f16x3')
  _, dc = helpers.oracle_configs(spec)
  steps = dc.sampler.schedule.num_steps
  rng = np.random.default_rng(5)
  shape = (4, 8, 128)
  for i in (steps - 1, steps // 2, 1, 0):
    first = i == steps - 1
    z, oc, ou, _ = _op_inputs(rng, dc, i, shape)
    prev = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    prev_t = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda') if first else helpers.dev(torch, prev)
    out = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    native.op_sampler_step_multistep_guided(cfg, i, helpers.dev(torch, z), helpers.dev(torch, oc), helpers.dev(torch, ou), prev_t,
                                            first, ROW_WEIGHTS, out)
    got, got_x0 = out.cpu().numpy(), prev_t.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(got_x0).all()
    for b, w in enumerate(ROW_WEIGHTS):
      row = slice(b, b + 1)
      refs = {}
      for name, xp in (('f32', backend.NumpyBackend('float32')), ('f64', backend.NumpyBackend('float64'))):
        pred = lambda z, time, include_conditioning, _xp=xp: _xp.asarray((oc if include_conditioning else ou)[row])
        zs, x0 = ms.step(xp, gs.with_weight(dc, w), xp.asarray(z[row]), i, pred, xp.asarray(prev[row]), first)
        refs[name] = (np.asarray(zs, np.float64), np.asarray(x0, np.float64))
      _criterion('guided 2M %s i=%d w=%g z_s' % (case, i, w), got[row], refs['f64'][0], refs['f32'][0])
      _criterion('guided 2M %s i=%d w=%g x0_prev' % (case, i, w), got_x0[row], refs['f64'][1], refs['f32'][1])
      cfg_w = inference._to_native_config(helpers.sampler_spec(**dict(case, cfg_weight=w)), msd_amd.audio_codecs.MelGAN(), 1, 'f16x3')
      p1 = torch.full((1,) + shape[1:], float('nan'), dtype=torch.float32, device='cuda') if first else helpers.dev(torch, prev[row])
      plain = torch.empty((1,) + shape[1:], dtype=torch.float32, device='cuda')
      native.op_sampler_step_multistep(cfg_w, i, helpers.dev(torch, z[row]), helpers.dev(torch, oc[row]),
                                       helpers.dev(torch, ou[row]) if w != 1.0 else None, p1, first, plain)
      np.testing.assert_array_equal(helpers.bits(got[row]), helpers.bits(plain.cpu().numpy()))
      np.testing.assert_array_equal(helpers.bits(got_x0[row]), helpers.bits(p1.cpu().numpy()))


# --------------------------------------------------------------------------------------------------
# models and references
# --------------------------------------------------------------------------------------------------
_models, _params = {}, {}


def _weights(preset):
  if preset not in _params:
    _params[preset] = msd_amd.synthetic.init_params(helpers.preset_spec(preset, N), 3, norm_scale_jitter=0.1)
  return _params[preset]


def _spec_of(preset, steps, sampler='ddpm', w=5.0):
  spec = helpers.preset_spec(preset, steps, sampler)
  d = spec.diffusion
  return dataclasses.replace(spec, diffusion=dataclasses.replace(d, classifier_free_guidance=dataclasses.replace(
      d.classifier_free_guidance, eval_condition_weight=w)))


def _model(torch, preset='tiny', steps=N, sampler='ddpm', w=5.0):
  """(spec, model): one two-row handle per configuration for the whole module."""
  key = (preset, steps, sampler, w)
  if key not in _models:
    spec = _spec_of(preset, steps, sampler, w)
    _models[key] = (spec, msd_amd.InferenceModel(_weights(preset), spec, batch_size=2, **helpers.ALL_PLANES))
  return _models[key]


def _draws(torch, rng, steps, b, seed, segment, t=64):
  """init_z [B,T,n] and noise [K,B,T,n] of a scalar-key call, made by the fill entry points."""
  from msd_amd import native
  z = torch.empty((b, t, 128), dtype=torch.float32, device='cuda')
  nz = torch.empty((steps, b, t, 128), dtype=torch.float32, device='cuda')
  for i in range(-1, steps):
    dst = z if i < 0 else nz[i]
    if rng == 'philox':
      native.fill_normal(dst, seed, segment, 1 + i)
    else:
      native.fill_normal_threefry(dst, seed, fold=i)
  torch.cuda.synchronize()
  return z.cpu().numpy(), nz.cpu().numpy()


def _references(preset, params, steps, sampler, batch, init_z, noise, weights, lo, hi):
  """[float64, float32] decodes of the specification on the oracle's network configured with `steps` steps."""
  from oracle import backend, fast
  spec = _spec_of(preset, steps, 'ddim' if sampler == 'dpmpp_2m' else sampler)
  cfg, dc = helpers.oracle_configs(spec)
  refs = []
  for dtype in ('float64', 'float32'):
    xp = backend.TorchBackend(dtype)
    fm = fast.FastModel(xp, cfg, dc, params, spec.has_context)
    refs.append(gs.predict(fm, batch, init_z, None if sampler != 'ddpm' else noise, weights, lo, hi,
                           'dpmpp_2m' if sampler == 'dpmpp_2m' else None))
    del fm
  return refs


def _codec_range(model):
  cfg = model._get_native().cfg
  return float(cfg.feature_min), float(cfg.feature_max)


def _assert_class_twice(model, got, ref64, ref32, what):
  """assert_fp32_class on everything, and again on the elements whose float64 specification lies strictly inside the
  codec's range: with most outputs saturated on the clip bounds the float32 oracle's median error is 0 and the first
  application sees little.  Returns the share of outputs on the bounds."""
  fmin, fmax = _codec_range(model)
  helpers.assert_fp32_class(got, ref64, ref32, what)
  inside = (ref64 > fmin) & (ref64 < fmax)
  on_bounds = 1.0 - float(inside.mean())
  print('%s: %.1f %% of the float64 specification on the codec bounds' % (what, 100.0 * on_bounds))
  assert inside.sum() > 1000
  helpers.assert_fp32_class(np.asarray(got)[inside], ref64[inside], ref32[inside], what + ' (inside the codec range)')
  return on_bounds


# --------------------------------------------------------------------------------------------------
# 2. a scalar weight is the handle created with it
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sampler', ['ddpm', 'dpmpp_2m'])
@pytest.mark.parametrize('rng', ['philox', 'threefry'])
def test_scalar_weight_is_a_fresh_handle_created_with_it(torch, rng, sampler):
  """predict(guidance=2.0, steps=24) on the weight-5 handle: the bits of a fresh handle created with cfg_weight = 2.0 under
  the same keys, and float32-class against the oracle configured with 2.0."""
  spec, model = _model(torch)
  _, fresh = _model(torch, 'tiny', 24, sampler, 2.0)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  keys = dict(seed=4, segment=2, rng=rng)
  got, _ = model.predict(batch, guidance=2.0, steps=24, sampler=sampler, **keys)
  want, _ = fresh.predict(batch, **keys)
  np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))
  init_z, noise = _draws(torch, rng, 24, 2, 4, 2)
  ref64, ref32 = _references('tiny', _weights('tiny'), 24, sampler, batch, init_z, noise, [2.0, 2.0], 0, 24)
  _assert_class_twice(model, got, ref64, ref32, 'guidance=2.0, %s, %s' % (rng, sampler))
  plain, _ = model.predict(batch, steps=24, sampler=sampler, **keys)
  assert helpers.rms(plain, got) > 1e-3


# --------------------------------------------------------------------------------------------------
# 3. weight 1: every step is one-pass
# --------------------------------------------------------------------------------------------------
def test_guidance_one_is_the_weight_1_model(torch):
  """guidance=1.0 on the weight-5 handle runs 24 one-pass steps: float32-class against the weight-1 oracle and no farther
  from a fresh handle created with cfg_weight = 1 than the float32 oracle is from float64."""
  spec, model = _model(torch)
  _, fresh = _model(torch, 'tiny', 24, 'ddpm', 1.0)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  keys = dict(seed=4, segment=2)
  got, _ = model.predict(batch, guidance=1.0, steps=24, **keys)
  init_z, noise = _draws(torch, 'philox', 24, 2, 4, 2)
  ref64, ref32 = _references('tiny', _weights('tiny'), 24, 'ddpm', batch, init_z, noise, [1.0, 1.0], 0, 24)
  _assert_class_twice(model, got, ref64, ref32, 'guidance=1.0')
  want, _ = fresh.predict(batch, **keys)
  same = np.array_equal(helpers.bits(got), helpers.bits(want))
  d, yard = np.abs(got.astype(np.float64) - want).max(), np.abs(ref32 - ref64).max()
  print('guidance=1.0: bit-identical to the fresh weight-1 handle: %s (max |diff| %.3e; float32 oracle vs float64 %.3e)' % (same, d, yard))
  assert d <= yard
  assert same   # (observed on the MI355X: bit-identical -- the same one-pass plan and the same kernels on either handle)
  # an interval with weight 1 inside is the same call; a weight-1 row inside a guided interval runs the same branch
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, guidance=1.0, guidance_interval=(0.25, 0.75), steps=24, **keys)[0]),
                                helpers.bits(got))


# --------------------------------------------------------------------------------------------------
# 4. interval chains
# --------------------------------------------------------------------------------------------------
CHAINS = [
    dict(steps=24, g=(6, 18)),                                   # graphs and singles on both sides
    dict(steps=24, g=(12, 24), low_sat=True),                    # no run above the interval
    dict(steps=24, g=(0, 12)),                                   # no run below it
    dict(steps=12, g=(3, 7)),                                    # singles everywhere
    dict(steps=24, g=(6, 18), sampler='dpmpp_2m'),               # x0_prev across both edges
    dict(steps=24, g=(6, 18), sampler='ddim'),
    dict(steps=24, g=(6, 18), preset='tiny_context'),            # ragged context mask
    dict(steps=24, g=(0, 24), w=1.5, low_sat=True),              # a gentle weight through the guided kernels
    dict(steps=24, g=(6, 18), w=[1.0, 5.0], low_sat=True),       # a weight-1 row beside a guided one
]


@pytest.mark.parametrize('case', CHAINS, ids=_ids)
def test_interval_chain_vs_spec(torch, case):
  preset, k, (lo, hi), sampler = case.get('preset', 'tiny'), case['steps'], case['g'], case.get('sampler', 'ddpm')
  w = case.get('w', 5.0)
  spec, model = _model(torch, preset)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  init_z, noise = helpers.make_noise(helpers.preset_spec(preset, k), batch=2)
  call = dict(init_z=init_z, noise=noise if sampler == 'ddpm' else None, steps=k, sampler=sampler)
  got, _ = model.predict(batch, guidance=w, guidance_interval=(lo / k, hi / k), **call)
  assert np.isfinite(got).all()
  weights = w if isinstance(w, list) else [w, w]
  ref64, ref32 = _references(preset, _weights(preset), k, sampler, batch, init_z, noise, weights, lo, hi)
  on_bounds = _assert_class_twice(model, got, ref64, ref32, 'interval %s' % case)
  if case.get('low_sat'):
    assert on_bounds < 0.5
  plain, _ = model.predict(batch, **call)
  diff = helpers.rms(plain, got)
  print('interval %s: rms difference to the plain call %.3f' % (case, diff))
  assert diff > 1e-3   # (a call that ignored the interval or the weight cannot pass)


# --------------------------------------------------------------------------------------------------
# 5. rows
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [dict(w=[1.0, 5.0]), dict(w=[1.5, 3.0]), dict(w=[1.5, 3.0], iv=(0.25, 0.75)),
                                  dict(w=[1.0, 2.5], iv=(0.25, 0.75), sampler='dpmpp_2m', rng='threefry')], ids=_ids)
def test_rows_are_their_one_row_calls(torch, case):
  spec, model = _model(torch)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  seeds, segments = [3, 9], [0, 4]
  kw = dict(rng=case.get('rng', 'philox'), steps=24, sampler=case.get('sampler'), guidance_interval=case.get('iv'))
  got, _ = model.predict(batch, seed=seeds, segment=segments, guidance=case['w'], **kw)
  for b in range(2):
    row = {k: np.ascontiguousarray(v[b:b + 1]) for k, v in batch.items()}
    one, _ = model.predict(row, seed=seeds[b], segment=segments[b], guidance=case['w'][b], **kw)
    np.testing.assert_array_equal(helpers.bits(got[b:b + 1]), helpers.bits(one))


def test_equal_keys_and_tokens_differ_in_guidance_only(torch):
  """A guidance sweep in one call: the same tokens and the same key on both rows, two weights -> two renderings; equal
  weights -> equal rows."""
  spec, model = _model(torch)
  one = helpers.make_batch(spec, batch=1, ctx_mask='ragged')
  batch = {k: np.concatenate([v, v], 0) for k, v in one.items()}
  keys = dict(seed=[3, 3], segment=[1, 1], steps=24)
  got, _ = model.predict(batch, guidance=[1.5, 5.0], **keys)
  assert helpers.rms(got[0], got[1]) > 1e-3
  same, _ = model.predict(batch, guidance=[1.5, 1.5], **keys)
  np.testing.assert_array_equal(helpers.bits(same[0]), helpers.bits(same[1]))
  np.testing.assert_array_equal(helpers.bits(same[0]), helpers.bits(got[0]))


# --------------------------------------------------------------------------------------------------
# 6. identity, graph cache
# --------------------------------------------------------------------------------------------------
def test_none_the_models_weight_and_the_whole_interval_are_the_plain_call(torch):
  spec, model = _model(torch)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  for rng in ('philox', 'threefry'):
    want, _ = model.predict(batch, seed=4, segment=2, rng=rng)
    for kw in (dict(guidance=None), dict(guidance=5.0), dict(guidance_interval=(0, 1)), dict(guidance=5.0, guidance_interval=(0.0, 1.0))):
      got, _ = model.predict(batch, seed=4, segment=2, rng=rng, **kw)
      np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))
  # ... and the model's weight through the guided kernels (a one-element sequence is no scalar): the same bits
  row = {k: np.ascontiguousarray(v[:1]) for k, v in batch.items()}
  np.testing.assert_array_equal(helpers.bits(model.predict(row, seed=4, segment=2, guidance=[5.0])[0]),
                                helpers.bits(model.predict(row, seed=4, segment=2)[0]))


def test_graph_cache_default_graphs_survive_and_seven_entries_leave_room_for_two(torch):
  """A guided-interval call needs two sets of graphs at once.  With seven sets cached neither lookup may invalidate the
  other's: the call gives the bits it gave on an empty cache, and so do the calls around it."""
  spec, model = _model(torch)
  nm = model._get_native()
  batch = helpers.make_batch(spec, batch=1, ctx_mask='ragged')
  keys = dict(seed=4, segment=2)
  guided = dict(guidance=2.0, guidance_interval=(0.25, 0.75), steps=12, **keys)
  nm.reset_graph()
  first, _ = model.predict(batch, **keys)
  want, _ = model.predict(batch, **guided)                      # (three sets cached now)
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, **keys)[0]), helpers.bits(first))
  combos = [(k, s) for s in ('ddim', 'dpmpp_2m') for k in (1, 2, 3)]
  # (a) seven sets, neither of the call's two among them: room is made before the first lookup
  nm.reset_graph()
  runs = [model.predict(batch, **keys)[0]] + [model.predict(batch, steps=k, sampler=s, **keys)[0] for k, s in combos]
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, **guided)[0]), helpers.bits(want))
  # (b) seven sets with the call's one-pass set among them: the guided set is the eighth
  nm.reset_graph()
  model.predict(batch, guidance=1.0, steps=12, **keys)
  for k, s in combos:
    model.predict(batch, steps=k, sampler=s, **keys)
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, **guided)[0]), helpers.bits(want))
  # (c) eight sets, both cached: nothing is captured; then a ninth shape resets the cache and everything still runs
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, **guided)[0]), helpers.bits(want))
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, **keys)[0]), helpers.bits(first))
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, **guided)[0]), helpers.bits(want))
  for (k, s), r in zip(combos, runs[1:]):
    np.testing.assert_array_equal(helpers.bits(model.predict(batch, steps=k, sampler=s, **keys)[0]), helpers.bits(r))


def test_a_weight_1_handle_refuses_and_still_runs(torch):
  from msd_amd import native
  spec, model = _model(torch, 'tiny', 24, 'ddpm', 1.0)
  batch = helpers.make_batch(spec, batch=1, ctx_mask='ragged')
  want, _ = model.predict(batch, seed=4, segment=2)
  with pytest.raises(ValueError, match='weight 1'):
    model.predict(batch, guidance=3.0)
  nm = model._get_native()
  out = torch.empty((1, 64, 128), dtype=torch.float32, device='cuda')
  with pytest.raises(NotImplementedError, match='any weight != 1'):   # (MSD_ERR_UNSUPPORTED)
    nm.sample(1, out, guidance=3.0, stream=model._stream.cuda_stream)
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, seed=4, segment=2)[0]), helpers.bits(want))


# --------------------------------------------------------------------------------------------------
# 7. base-size tiles
# --------------------------------------------------------------------------------------------------
def test_base_size_interval_call(torch):
  """One base_with_context handle of 40 steps, an 8-step call with weight 2 in (2, 6): the one-pass plan's tile family
  (M = 256) inside a chain of graphs and single steps."""
  spec = msd_amd.config.preset('base_with_context', num_steps=40)
  params = msd_amd.synthetic.init_params(spec, 21, norm_scale_jitter=0.1)
  model = msd_amd.InferenceModel(params, spec, batch_size=1, **helpers.ALL_PLANES)
  try:
    batch = helpers.make_batch(spec, batch=1, ctx_mask='ragged')
    init_z, noise = _draws(torch, 'philox', 8, 1, 4, 2, t=256)
    got, _ = model.predict(batch, seed=4, segment=2, steps=8, guidance=2.0, guidance_interval=(0.25, 0.75))
    refs = _references('base_with_context', params, 8, 'ddpm', batch, init_z, noise, [2.0], 2, 6)
    helpers.assert_fp32_class(got, refs[0], refs[1], 'base_with_context, 8 of 40 steps, weight 2 in (2, 6)')
    assert helpers.rms(model.predict(batch, seed=4, segment=2, steps=8)[0], got) > 1e-3
  finally:
    del model
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------------
# 8. errors
# --------------------------------------------------------------------------------------------------
def test_errors(torch):
  from msd_amd import native
  spec, model = _model(torch)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  want, _ = model.predict(batch, seed=4, segment=2, guidance=2.0, steps=12)
  keep, mask = np.zeros((2, 64, 128), np.float32), np.ones((2, 64), np.int32)
  for kw, match in ((dict(guidance=float('nan')), 'finite'), (dict(guidance=float('inf')), 'finite'),
                    (dict(guidance=[1.0, 2.0, 3.0]), 'one per row'), (dict(guidance=2.0, guidance_interval=(0.5, 0.25)), 'guidance_interval'),
                    (dict(guidance=2.0, guidance_interval=(0.0, 1.5)), 'guidance_interval'),
                    (dict(guidance=2.0, keep=keep, keep_mask=mask), 'cannot be combined')):
    with pytest.raises(ValueError, match=match):
      model.predict(batch, **kw)
  nm = model._get_native()
  out = torch.empty((2, 64, 128), dtype=torch.float32, device='cuda')
  stream = model._stream.cuda_stream
  for kw, match in ((dict(guidance=float('nan')), 'finite'), (dict(guidance=[1.0]), 'one per row'),
                    (dict(guidance=2.0, guide_range=(4, 4)), 'guide_range'), (dict(guidance=2.0, guide_range=(0, 97)), 'guide_range'),
                    (dict(guidance=2.0, keep=out, keep_mask=mask), 'cannot be combined')):
    with pytest.raises(ValueError, match=match):
      nm.sample(2, out, stream=stream, **kw)
  # the raw entry point
  seeds = (ctypes.c_uint64 * 2)(4, 4)
  fl = lambda *x: (ctypes.c_float * len(x))(*x)

  def raw(weights, n_weights, lo, hi, steps=12, sampler=-1, batch_rows=2):
    return nm.lib.msd_sample_guided(nm.handle, batch_rows, 0, 0, seeds, None, None, None, steps, sampler, weights, n_weights, lo, hi,
                                    out.data_ptr(), stream)
  for args, word in (((fl(float('nan')), 1, 0, 0), 'finite'), ((fl(2.0, float('inf')), 2, 0, 0), 'finite'),
                     ((fl(2.0, 3.0, 4.0), 3, 0, 0), 'one per row'), ((None, 1, 0, 0), 'one per row'),
                     ((fl(2.0), 1, 4, 4), 'interval'), ((fl(2.0), 1, 6, 2), 'interval'), ((fl(2.0), 1, 0, 13), 'interval'),
                     ((fl(2.0), 1, -1, 4), 'interval')):
    assert raw(*args) == native.MSD_ERR_INVALID_ARGUMENT, args[1:]
    assert word in nm.lib.msd_last_error(nm.handle).decode(), args[1:]
  assert raw(fl(2.0), 1, 0, 0, steps=36) == native.MSD_ERR_INVALID_ARGUMENT
  assert raw(fl(2.0), 1, 0, 0, sampler=7) == native.MSD_ERR_INVALID_ARGUMENT
  assert raw(fl(2.0), 1, 0, 0, batch_rows=3) == native.MSD_ERR_INVALID_ARGUMENT
  # the handle still runs, and gives what it gave
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, seed=4, segment=2, guidance=2.0, steps=12)[0]), helpers.bits(want))
