"""-m gpu: few-step rendering (msd_sample_steps, msd_op_sampler_step_multistep, predict(steps=, sampler=)) against the
specification of tests/multistep_spec.py: the oracle configured with num_steps = K, and DPM-Solver++(2M) written from the
oracle's functions.

Presets tiny / tiny_context: T = 64, n = 128.  The handle has N = 96 steps (graph_steps 8): K = 24 is three step graphs,
K = 12 one graph and four single-step launches, K = 1 a single launch."""
import ctypes

import numpy as np
import pytest

import msd_amd
from tests import helpers, multistep_spec as ms
from tests.helpers import gpu_torch  # noqa: F401  (the `torch` fixture)

pytestmark = pytest.mark.gpu

N = 96


# --------------------------------------------------------------------------------------------------
# 1. one multistep update
# --------------------------------------------------------------------------------------------------
OP_CASES = [dict(), dict(cfg_weight=1.0), dict(clip=False), dict(model_output='x0'), dict(model_output='v')]


@pytest.mark.parametrize('case', OP_CASES, ids=lambda c: ','.join('%s=%s' % kv for kv in c.items()) or 'default')
def test_op_multistep_vs_spec(torch, case):
  """msd_op_sampler_step_multistep at the top index (first: no history), a middle one, 1 and 0 against the spec in float64,
  the spec's float32 evaluation as the yardstick (the sampler ops' criterion, tests/test_gpu_fused_ops.py); x0_prev
  holds the update's pred_x0 afterwards; at i == 0 the output is pred_x0."""
  from msd_amd import inference, native
  from oracle import backend
  spec = helpers.sampler_spec(**case)
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, 'f16x3')
  _, dc = helpers.oracle_configs(spec)
  steps = dc.sampler.schedule.num_steps
  two_pass = dc.classifier_free_guidance.eval_condition_weight != 1
  rng = np.random.default_rng(5)
  shape = (2, 16, 128)
  for i in (steps - 1, steps // 2, 1, 0):
    first = i == steps - 1
    z, oc, ou = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    prev = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    if i > steps // 2 and dc.model_output == 'eps':   # at logsnr ~ -20 only eps ~ z leaves x0 inside [-1, 1]
      oc, ou = z + 1e-5 * oc, z + 1e-5 * ou
    refs = {}
    for name, xp in (('f32', backend.NumpyBackend('float32')), ('f64', backend.NumpyBackend('float64'))):
      pred = lambda z, time, include_conditioning, _xp=xp: _xp.asarray(oc if include_conditioning else ou)
      zs, x0 = ms.step(xp, dc, xp.asarray(z), i, pred, xp.asarray(prev), first)
      refs[name] = (np.asarray(zs, np.float64), np.asarray(x0, np.float64))
    # the history buffer on entry: NaN on the first step -- it must not be read there
    prev_t = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda') if first else helpers.dev(torch, prev)
    out_t = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    native.op_sampler_step_multistep(cfg, i, helpers.dev(torch, z), helpers.dev(torch, oc), helpers.dev(torch, ou) if two_pass else None, prev_t,
                                     first, out_t)
    got, got_x0 = out_t.cpu().numpy(), prev_t.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(got_x0).all()
    for what, dev, k in (('z_s', got, 0), ('x0_prev', got_x0, 1)):
      scale = max(1.0, float(np.abs(refs['f64'][k]).max()))
      e_dev = np.abs(dev.astype(np.float64) - refs['f64'][k]).max() / scale
      e_f32 = np.abs(refs['f32'][k] - refs['f64'][k]).max() / scale
      print('multistep %s i=%d %s: scaled error device %.3e / float32 %.3e' % (case, i, what, e_dev, e_f32))
      assert e_dev <= 1e-6 + 4 * e_f32, (i, what, e_dev, e_f32)
    if i == 0:
      np.testing.assert_array_equal(helpers.bits(got), helpers.bits(got_x0))
      if dc.sampler.clip_x0:
        assert np.abs(got).max() <= 1.0
    else:
      assert not np.array_equal(got, got_x0)
    if not first and 0 < i:   # the history entered: the first-order result differs
      fo_prev, fo_out = helpers.dev(torch, prev), torch.empty(shape, dtype=torch.float32, device='cuda')
      native.op_sampler_step_multistep(cfg, i, helpers.dev(torch, z), helpers.dev(torch, oc), helpers.dev(torch, ou) if two_pass else None,
                                       fo_prev, True, fo_out)
      assert not np.array_equal(fo_out.cpu().numpy(), got)
      np.testing.assert_array_equal(helpers.bits(fo_prev.cpu().numpy()), helpers.bits(got_x0))


# --------------------------------------------------------------------------------------------------
# 2. the closed-form chain on the device
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('steps', [20, 50])
def test_closed_form_chain_on_the_device(torch, steps):
  """The op K times, the host computing the ideal denoiser's eps in float64 between the calls (1024 elements, clip off, one
  pass), and the same with the DDIM op: the device's 2M error against the closed form is below a quarter of the device's
  DDIM error, and the device's 2M chain is within 1e-5 rms of the float64 spec chain (solver errors >= 2e-3, float32
  noise ~1e-6: three orders of magnitude either way)."""
  from msd_amd import inference, native
  from oracle import backend
  shape = (1, 8, 128)
  z1 = np.random.default_rng(3).standard_normal(shape).astype(np.float32)
  exact = ms.exact_end_point(z1)
  xp = backend.NumpyBackend('float64')
  ends = {}
  for sampler in ('dpmpp_2m', 'ddim'):
    spec = helpers.sampler_spec(sampler='ddim', cfg_weight=1.0, clip=False, steps=steps)
    cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, 'f16x3')
    _, dc = helpers.oracle_configs(spec)
    pred = ms.ideal_pred_fn(xp, dc)
    z = helpers.dev(torch, z1)
    prev = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    for i in reversed(range(steps)):
      time = np.full((1,), (i + 1.0) / steps)
      eps = helpers.dev(torch, pred(z.cpu().numpy().astype(np.float64), time, True))
      out = torch.empty_like(z)
      if sampler == 'ddim':
        native.op_sampler_step(cfg, i, z, eps, None, None, out)
      else:
        native.op_sampler_step_multistep(cfg, i, z, eps, None, prev, i == steps - 1, out)
      z = out
    ends[sampler] = z.cpu().numpy().astype(np.float64)
  spec_chain = ms.scan(xp, z1.astype(np.float64), pred, dc)
  e_2m, e_ddim = helpers.rms(ends['dpmpp_2m'], exact), helpers.rms(ends['ddim'], exact)
  d_spec = helpers.rms(ends['dpmpp_2m'], spec_chain)
  print('closed form K = %d: device rms error 2M %.3e, DDIM %.3e (ratio %.2f); device 2M vs float64 spec chain %.3e'
        % (steps, e_2m, e_ddim, e_ddim / e_2m, d_spec))
  assert e_2m < 0.25 * e_ddim
  assert d_spec < 1e-5


# --------------------------------------------------------------------------------------------------
# models
# --------------------------------------------------------------------------------------------------
_models, _params = {}, {}


def _weights(preset):
  if preset not in _params:
    _params[preset] = msd_amd.synthetic.init_params(helpers.preset_spec(preset, N), 3, norm_scale_jitter=0.1)
  return _params[preset]


def _model(torch, preset='tiny', steps=N, sampler='ddpm'):
  """(spec, model) -- one handle per configuration for the whole module; the weights do not depend on the step count."""
  key = (preset, steps, sampler)
  if key not in _models:
    spec = helpers.preset_spec(preset, steps, sampler)
    _models[key] = (spec, msd_amd.InferenceModel(_weights(preset), spec, batch_size=2, **helpers.ALL_PLANES))
  return _models[key]


def _draws(torch, rng, steps, b, seed, segment, t=64):
  """init_z [B,T,n] and noise [K,B,T,n] of a scalar-key call: ONE draw over the whole array per step, made by the fill
  entry points."""
  from msd_amd import native
  z = torch.empty((b, t, 128), dtype=torch.float32, device='cuda')
  nz = torch.empty((steps, b, t, 128), dtype=torch.float32, device='cuda')
  if rng == 'philox':
    native.fill_normal(z, seed, segment, 0)
    for i in range(steps):
      native.fill_normal(nz[i], seed, segment, 1 + i)
  else:
    native.fill_normal_threefry(z, seed, fold=-1)
    for i in range(steps):
      native.fill_normal_threefry(nz[i], seed, fold=i)
  torch.cuda.synchronize()
  return z.cpu().numpy(), nz.cpu().numpy()


def _oracle(preset, steps, sampler, batch, init_z, noise):
  """[float64, float32] decodes of the oracle configured with num_steps = steps ('dpmpp_2m': the spec's scan over the
  oracle's network)."""
  from oracle import backend, fast
  spec = helpers.preset_spec(preset, steps, 'ddim' if sampler == 'dpmpp_2m' else sampler)
  cfg, dc = helpers.oracle_configs(spec)
  refs = []
  for dtype in ('float64', 'float32'):
    xp = backend.TorchBackend(dtype)
    fm = fast.FastModel(xp, cfg, dc, _weights(preset), spec.has_context)
    if sampler == 'dpmpp_2m':
      refs.append(ms.predict(fm, batch, init_z))
    else:
      dec, _ = fm.predict(batch, init_z, None if sampler == 'ddim' else noise)
      refs.append(np.asarray(xp.to_numpy(dec), np.float64))
  return refs


# --------------------------------------------------------------------------------------------------
# 3. strided calls on a handle of 96 steps
# --------------------------------------------------------------------------------------------------
STRIDED = [
    dict(steps=24, rng='philox'),                     # three step graphs
    dict(steps=12, rng='philox', b=2),                # one graph + four single-step launches; two rows
    dict(steps=1, rng='philox'),
    dict(steps=24, rng='threefry'),
    dict(steps=24, rng='philox', sampler='ddim'),
    dict(steps=12, rng='philox', supplied=True),      # a [K,B,T,n] noise tensor
    dict(steps=24, rng='philox', preset='tiny_context'),   # ragged context mask
]


@pytest.mark.parametrize('case', STRIDED, ids=lambda c: ','.join('%s=%s' % kv for kv in c.items()))
def test_strided_call_is_the_k_step_model(torch, case):
  """predict(steps=K) on the 96-step handle against the float64 oracle configured with num_steps = K (assert_fp32_class),
  and against a FRESH handle created with num_steps = K and the same keys: no farther from it than the float32 oracle is
  from float64 on that chain."""
  preset, k, rng, b = case.get('preset', 'tiny'), case['steps'], case['rng'], case.get('b', 1)
  sampler = case.get('sampler')
  spec, model = _model(torch, preset)
  batch = helpers.make_batch(spec, batch=b, ctx_mask='ragged')
  keys = dict(seed=4, segment=2)
  init_z, noise = _draws(torch, rng, k, b, keys['seed'], keys['segment'])
  if case.get('supplied'):
    init_z, noise = helpers.make_noise(helpers.preset_spec(preset, k), batch=b)   # [B,T,n], [K,B,T,n]
    call = dict(init_z=init_z, noise=noise)
  else:
    call = dict(rng=rng, **keys)
  got, _ = model.predict(batch, steps=k, sampler=sampler, **call)
  assert np.isfinite(got).all()
  ref64, ref32 = _oracle(preset, k, sampler or 'ddpm', batch, init_z, noise)
  helpers.assert_fp32_class(got, ref64, ref32, 'strided %s' % case)
  _, fresh_model = _model(torch, preset, k, sampler or 'ddpm')
  fresh, _ = fresh_model.predict(batch, **call)
  same = np.array_equal(helpers.bits(got), helpers.bits(fresh))
  d, yard = np.abs(got.astype(np.float64) - fresh).max(), np.abs(ref32 - ref64).max()
  print('strided %s: bit-identical to the fresh %d-step handle: %s (max |diff| %.3e; float32 oracle vs float64 %.3e)'
        % (case, k, same, d, yard))
  assert d <= yard
  assert same   # (holds on the MI355X in every case: the same kernels on the same table rows)


def test_all_steps_and_none_are_the_default_call(torch):
  spec, model = _model(torch)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  for rng in ('philox', 'threefry'):
    want, _ = model.predict(batch, seed=4, segment=2, rng=rng)
    for kw in (dict(steps=N), dict(steps=None), dict(steps=N, sampler='ddpm'), dict(sampler='ddpm')):
      got, _ = model.predict(batch, seed=4, segment=2, rng=rng, **kw)
      np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))


# --------------------------------------------------------------------------------------------------
# 4. 2M through predict
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('steps', [12, N])
def test_dpmpp_2m_through_predict(torch, steps):
  """sampler='dpmpp_2m' with CFG 5 and the clip, 12 of 96 steps (strided tables) and all 96 (the handle's own tables, the
  other sampler kernel), against the spec's scan over the oracle's network."""
  spec, model = _model(torch)
  assert spec.diffusion.classifier_free_guidance.eval_condition_weight == 5.0 and spec.diffusion.sampler.clip_x0
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  init_z = helpers.make_noise(spec, batch=2)[0]
  got, _ = model.predict(batch, init_z=init_z, steps=steps, sampler='dpmpp_2m')
  ref64, ref32 = _oracle('tiny', steps, 'dpmpp_2m', batch, init_z, None)
  helpers.assert_fp32_class(got, ref64, ref32, 'dpmpp_2m, %d steps' % steps)
  # deterministic after init_z: neither the keys nor a noise tensor enter
  again, _ = model.predict(batch, init_z=init_z, steps=steps, sampler='dpmpp_2m', seed=77, segment=5)
  np.testing.assert_array_equal(helpers.bits(again), helpers.bits(got))
  ddim, _ = model.predict(batch, init_z=init_z, steps=steps, sampler='ddim')
  assert helpers.rms(ddim, got) > 1e-3   # (another solver of the same ODE)


def test_dpmpp_2m_as_the_handles_default(torch):
  """SamplerConfig.name = 'dpmpp_2m': the plain call of such a handle is the 96-step handle's predict(steps=12,
  sampler='dpmpp_2m'), bit for bit."""
  spec, model = _model(torch)
  _, own = _model(torch, 'tiny', 12, 'dpmpp_2m')
  batch = helpers.make_batch(spec, batch=1, ctx_mask='ragged')
  want, _ = model.predict(batch, seed=4, segment=2, steps=12, sampler='dpmpp_2m')
  got, _ = own.predict(batch, seed=4, segment=2)
  np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))


def test_jax_mode_draws_for_the_calls_step_count(torch):
  """rng='jax' with steps=K uploads reference_noise(seed, shape, K): the host draws of a K-step model."""
  from msd_amd import jax_random
  spec, model = _model(torch)
  batch = helpers.make_batch(spec, batch=1, ctx_mask='ragged')
  got, _ = model.predict(batch, seed=5, rng='jax', steps=12)
  z, nz = jax_random.reference_noise(5, (1, 64, 128), 12)
  assert nz.shape == (12, 1, 64, 128)
  want, _ = model.predict(batch, init_z=z, noise=nz, steps=12)
  np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))
  full, _ = model.predict(batch, seed=5, rng='jax')   # ... and the cached draws of another step count are not reused
  z96, nz96 = jax_random.reference_noise(5, (1, 64, 128), N)
  np.testing.assert_array_equal(helpers.bits(full), helpers.bits(model.predict(batch, init_z=z96, noise=nz96)[0]))


# --------------------------------------------------------------------------------------------------
# 5. rows
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sampler', [None, 'dpmpp_2m'])
@pytest.mark.parametrize('rng', ['philox', 'threefry'])
def test_rows_are_their_one_row_calls(torch, rng, sampler):
  spec, model = _model(torch)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  seeds, segments = [3, 9], [0, 4]
  got, _ = model.predict(batch, seed=seeds, segment=segments, rng=rng, steps=24, sampler=sampler)
  for b in range(2):
    row = {k: np.ascontiguousarray(v[b:b + 1]) for k, v in batch.items()}
    one, _ = model.predict(row, seed=seeds[b], segment=segments[b], rng=rng, steps=24, sampler=sampler)
    np.testing.assert_array_equal(helpers.bits(got[b:b + 1]), helpers.bits(one))
  assert helpers.rms(got[0], got[1]) > 0.05


# --------------------------------------------------------------------------------------------------
# 6. graph cache
# --------------------------------------------------------------------------------------------------
def test_graph_cache_keeps_the_default_graphs_and_survives_a_reset(torch):
  spec, model = _model(torch)
  batch = helpers.make_batch(spec, batch=1, ctx_mask='ragged')
  keys = dict(seed=4, segment=2)
  first, _ = model.predict(batch, **keys)
  few, _ = model.predict(batch, steps=24, **keys)
  third, _ = model.predict(batch, **keys)
  np.testing.assert_array_equal(helpers.bits(first), helpers.bits(third))
  assert helpers.rms(first, few) > 1e-3
  # nine distinct (K, sampler) in a row: more than the eight cached sets, so the cache is reset on the way
  combos = [(k, s) for s in ('ddim', 'dpmpp_2m') for k in (1, 2, 3, 4, 6)][:9]
  assert len(set(combos)) == 9
  runs = [model.predict(batch, steps=k, sampler=s, **keys)[0] for k, s in combos]
  again, _ = model.predict(batch, steps=combos[0][0], sampler=combos[0][1], **keys)
  np.testing.assert_array_equal(helpers.bits(again), helpers.bits(runs[0]))
  for (k, s), r in zip(combos, runs):
    assert np.isfinite(r).all(), (k, s)
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, steps=24, **keys)[0]), helpers.bits(few))
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, **keys)[0]), helpers.bits(first))


# --------------------------------------------------------------------------------------------------
# 7. errors
# --------------------------------------------------------------------------------------------------
def test_errors(torch):
  from msd_amd import native
  spec, model = _model(torch)
  batch = helpers.make_batch(spec, batch=1, ctx_mask='ragged')
  divisors = '1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 96'
  with pytest.raises(ValueError, match=divisors):
    model.predict(batch, steps=36)
  model.predict(batch, steps=1)   # (the handle exists and is encoded)
  nm = model._get_native()
  out = torch.empty((1, 64, 128), dtype=torch.float32, device='cuda')
  seeds = (ctypes.c_uint64 * 1)(0)
  stream = model._stream.cuda_stream
  rc = nm.lib.msd_sample_steps(nm.handle, 1, 0, 0, seeds, None, None, None, 36, -1, out.data_ptr(), stream)
  assert rc == native.MSD_ERR_INVALID_ARGUMENT and divisors in nm.lib.msd_last_error(nm.handle).decode()
  rc = nm.lib.msd_sample_steps(nm.handle, 1, 0, 0, seeds, None, None, None, 24, 7, out.data_ptr(), stream)
  assert rc == native.MSD_ERR_INVALID_ARGUMENT and 'sampler' in nm.lib.msd_last_error(nm.handle).decode()
  rc = nm.lib.msd_sample_steps(nm.handle, 1, 0, 0, seeds, None, None, None, -2, -1, out.data_ptr(), stream)
  assert rc == native.MSD_ERR_INVALID_ARGUMENT
  with pytest.raises(ValueError, match='sampler must be one of'):
    model.predict(batch, sampler='euler')
  with pytest.raises(ValueError, match='sampler must be one of'):
    nm.sample(1, out, steps=24, sampler='euler', stream=stream)
  init_z, noise = helpers.make_noise(spec, batch=1)
  with pytest.raises(ValueError, match='noise must be'):
    model.predict(batch, init_z=init_z, noise=noise, steps=24)   # [96, ...] where [24, ...] is due
  with pytest.raises(ValueError, match='noise must be'):
    model.predict(batch, init_z=init_z, noise=noise[:24])        # ... and the other way round
  keep = np.zeros((1, 64, 128), np.float32)
  with pytest.raises(ValueError, match='cannot be combined'):
    model.predict(batch, steps=24, keep=keep, keep_mask=np.ones((1, 64), np.int32))
  with pytest.raises(ValueError, match='cannot be combined'):
    model.predict(batch, sampler='dpmpp_2m', keep=keep, strength=0.5)
  with pytest.raises(ValueError, match='cannot be combined'):
    nm.sample(1, out, steps=24, keep=out, keep_mask=np.ones((1, 64), np.int32), stream=stream)
  # the handle still runs
  model.predict(batch, steps=24)


# --------------------------------------------------------------------------------------------------
# 8. base-size tiles
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def base(torch):
  """One base_with_context handle of 40 steps: the strided bias / gain reads in the 64 x 96 / 64 x 128 / persistent tile
  family, which `tiny` does not launch."""
  spec = msd_amd.config.preset('base_with_context', num_steps=40)
  params = msd_amd.synthetic.init_params(spec, 21, norm_scale_jitter=0.1)
  model = msd_amd.InferenceModel(params, spec, batch_size=1, **helpers.ALL_PLANES)
  yield spec, params, model
  del model
  torch.cuda.empty_cache()


@pytest.mark.parametrize('sampler', ['ddpm', 'dpmpp_2m'])
def test_base_size_strided_call(torch, base, sampler):
  from oracle import backend, fast
  spec, params, model = base
  batch = helpers.make_batch(spec, batch=1, ctx_mask='ragged')
  init_z, noise = _draws(torch, 'philox', 8, 1, 4, 2, t=256)
  got, _ = model.predict(batch, seed=4, segment=2, steps=8, sampler=sampler)
  spec8 = msd_amd.config.preset('base_with_context', num_steps=8)
  cfg, dc = helpers.oracle_configs(spec8)
  refs = []
  for dtype in ('float64', 'float32'):
    xp = backend.TorchBackend(dtype)
    fm = fast.FastModel(xp, cfg, dc, params, True)
    if sampler == 'dpmpp_2m':
      refs.append(ms.predict(fm, batch, init_z))
    else:
      refs.append(np.asarray(xp.to_numpy(fm.predict(batch, init_z, noise)[0]), np.float64))
    del fm
  helpers.assert_fp32_class(got, refs[0], refs[1], 'base_with_context, 8 of 40 steps, %s' % sampler)
