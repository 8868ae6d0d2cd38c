"""-m gpu: known frames in the sampler (msd_sample_keep, msd_op_sampler_step_keep, predict(keep=, keep_mask=),
regenerate) against the specification of tests/keep_spec.py: the reference's eval_step.body with the two replacement
lines, over oracle.fast.FastModel.

Presets tiny / tiny_context: T = 64, n = 128, i.e. eight 1024-element sampler blocks per row, 32 threads per frame."""
import numpy as np
import pytest

import msd_amd
from tests import helpers, keep_spec
from tests.helpers import gpu_torch  # noqa: F401  (the `torch` fixture)

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------------------------------
# 1. one update
# --------------------------------------------------------------------------------------------------
OP_CASES = [
    dict(),
    dict(cfg_weight=1.0),
    dict(sampler='ddim'),
    dict(sampler='ddim', clip=False, cfg_weight=1.0),
    dict(clip=False),
    dict(model_output='x0'),
    dict(model_output='v'),
    dict(logvar='small'),
    dict(schedule='linear', train='linear', model_output='x0'),
    # beyond the issue's list: the remaining forms of the update's arithmetic (v mode's single pass, v mode under DDIM,
    # medium log-variance, eps mode on the linear schedule), for the bit-equality with the plain update
    dict(model_output='v', cfg_weight=1.0, clip=False),
    dict(train='linear', model_output='v', sampler='ddim'),
    dict(logvar='medium:0.3'),
    dict(schedule='linear'),
]


@pytest.mark.parametrize('case', OP_CASES, ids=lambda c: ','.join('%s=%s' % kv for kv in c.items()) or 'default')
def test_op_sampler_step_keep_vs_spec(torch, case):
  """msd_op_sampler_step_keep at the first, a middle, the second-to-last and the last scan index: against the
  specification in float64 with its float32 evaluation as the yardstick (the plain update's criterion,
  tests/test_gpu_fused_ops.py); free elements are msd_op_sampler_step's bits -- the plain and the keep instance of the
  one sampler_update text -- and at i == 0 kept elements are the known values' bits."""
  from msd_amd import inference, native
  from oracle import backend
  spec = helpers.sampler_spec(**case)
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, 'bf16x3')
  _, dc = helpers.oracle_configs(spec)
  steps = dc.sampler.schedule.num_steps
  two_pass = dc.classifier_free_guidance.eval_condition_weight != 1
  xp32, xp64 = backend.NumpyBackend('float32'), backend.NumpyBackend('float64')
  rng = np.random.default_rng(5)
  shape = (2, 16, 128)
  mask = np.zeros(shape[:2], np.int32)   # another pattern in each row: a wrong row or frame index shows
  mask[0, [0, 1, 5, 15]] = 1
  mask[1, 2:10] = 1
  kept = np.broadcast_to(mask[..., None] != 0, shape)
  worst = 0.0
  for i in (steps - 1, steps // 2, 1, 0):
    z = rng.standard_normal(shape).astype(np.float32)
    oc = rng.standard_normal(shape).astype(np.float32)
    ou = rng.standard_normal(shape).astype(np.float32)
    nz = rng.standard_normal(shape).astype(np.float32)
    xk = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    if i > steps // 2 and dc.model_output == 'eps':
      oc = z + 1e-5 * oc   # at logsnr ~ -20 only eps ~ z leaves x0 inside [-1, 1]
      ou = z + 1e-5 * ou
    outs = {}
    for name, xp in (('f32', xp32), ('f64', xp64)):
      noise = [None] * steps
      noise[i] = xp.asarray(nz)
      pred = lambda z, time, include_conditioning, _xp=xp: _xp.asarray(oc if include_conditioning else ou)
      body = keep_spec.eval_step_keep(xp, noise, dc, 2, pred, xp.asarray(xk), keep_spec.frame_mask(xp, mask))
      outs[name] = np.asarray(body(xp.asarray(z), i), np.float64)
    args = (helpers.dev(torch, z), helpers.dev(torch, oc), helpers.dev(torch, ou) if two_pass else None, helpers.dev(torch, nz))
    got_t = torch.empty(shape, dtype=torch.float32, device='cuda')
    native.op_sampler_step_keep(cfg, i, *args, helpers.dev(torch, xk), helpers.dev(torch, mask, np.int32), got_t)
    plain_t = torch.empty(shape, dtype=torch.float32, device='cuda')
    native.op_sampler_step(cfg, i, *args, plain_t)
    got32, plain32 = got_t.cpu().numpy(), plain_t.cpu().numpy()
    np.testing.assert_array_equal(got32[~kept].view(np.uint32), plain32[~kept].view(np.uint32))
    if i == 0:
      np.testing.assert_array_equal(got32[kept].view(np.uint32), xk[kept].view(np.uint32))
    else:
      assert not np.array_equal(got32[kept], plain32[kept])
    got = got32.astype(np.float64)
    scale = max(1.0, float(np.abs(outs['f64']).max()))
    e_dev = np.abs(got - outs['f64']).max() / scale
    e_f32 = np.abs(outs['f32'] - outs['f64']).max() / scale
    print('keep step %s i=%d: scaled error device %.3e / float32 %.3e' % (case, i, e_dev, e_f32))
    worst = max(worst, e_dev)
    assert e_dev <= 1e-6 + 4 * e_f32, (i, e_dev, e_f32)
  print('keep step %s: worst scaled error %.2e' % (case, worst))


# --------------------------------------------------------------------------------------------------
# models
# --------------------------------------------------------------------------------------------------
_models = {}


def _model(torch, preset='tiny_context', steps=8, sampler='ddpm'):
  return helpers.cached_model(_models, preset, steps, sampler)


# --------------------------------------------------------------------------------------------------
# 2. a zero mask changes nothing
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rng', ['philox', 'threefry'])
@pytest.mark.parametrize('sampler, steps', [('ddpm', 16), ('ddpm', 10), ('ddim', 16)])   # 10 = 8 + the remainder graph
def test_zero_mask_is_the_plain_call(torch, sampler, steps, rng):
  spec, _, model = _model(torch, 'tiny_context', steps, sampler)
  for b, keys in ((1, dict(seed=4, segment=2)), (2, dict(seed=[4, 9], segment=[2, 0]))):
    batch = helpers.make_batch(spec, batch=b, ctx_mask='ragged')
    want, _ = model.predict(batch, rng=rng, **keys)
    got, _ = model.predict(batch, rng=rng, keep=helpers.known_mel((b, 64, 128)), keep_mask=np.zeros((b, 64), np.int32), **keys)
    np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))
    again, _ = model.predict(batch, rng=rng, **keys)
    np.testing.assert_array_equal(helpers.bits(again), helpers.bits(want))


# --------------------------------------------------------------------------------------------------
# 3. kept frames come back exactly
# --------------------------------------------------------------------------------------------------
def test_kept_frames_are_returned_exactly(torch):
  spec, _, model = _model(torch)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  known = helpers.known_mel((2, 64, 128))
  mask = keep_spec.parity_masks(2)
  kept = mask.astype(bool)
  assert (known[kept] > 4.0).any() and (known[kept] < np.log(1e-5)).any()   # beyond the codec's range inside kept frames
  plain, _ = model.predict(batch, seed=3)
  for kw in (dict(seed=3), dict(seed=[3, 8], segment=[0, 5]), dict(seed=3, rng='threefry')):
    got, _ = model.predict(batch, keep=known, keep_mask=mask.astype(bool), **kw)
    np.testing.assert_array_equal(helpers.bits(got[kept]), helpers.bits(known[kept]))
    assert np.isfinite(got).all() and np.abs(got[~kept] - known[~kept]).max() > 1.0
  got, _ = model.predict(batch, seed=3, keep=known, keep_mask=mask)
  assert np.abs(got[~kept] - plain[~kept]).max() > 1e-3     # the free frames saw the known ones
  # a device tensor as `keep`, and the all-ones mask: the known mel everywhere
  full, _ = model.predict(batch, seed=3, keep=helpers.dev(torch, known), keep_mask=np.ones((2, 64), np.int64))
  np.testing.assert_array_equal(helpers.bits(full), helpers.bits(known))
  with pytest.raises(ValueError):
    model.predict(batch, keep=known)
  with pytest.raises(ValueError):
    model.predict(batch, keep=known[:, :32], keep_mask=mask)


# --------------------------------------------------------------------------------------------------
# 4. the chain against the specification
# --------------------------------------------------------------------------------------------------
def _spec_refs(spec, params, batch, init_z, noise, known, mask):
  from oracle import backend, fast
  cfg, dc = helpers.oracle_configs(spec)
  refs = []
  for dtype in ('float64', 'float32'):
    fm = fast.FastModel(backend.TorchBackend(dtype), cfg, dc, params, spec.has_context)
    refs.append(keep_spec.predict_keep(fm, batch, init_z, noise, known, mask)[0])
  return refs


@pytest.mark.parametrize('b', [1, 2])
def test_chain_matches_the_spec_on_the_free_frames(torch, b):
  spec, params, model = _model(torch)
  batch = helpers.make_batch(spec, batch=b, ctx_mask='ragged')
  init_z, noise = helpers.make_noise(spec, batch=b)
  known, mask = helpers.known_mel((b, 64, 128)), keep_spec.parity_masks(b)
  got, _ = model.predict(batch, init_z=init_z, noise=noise, keep=known, keep_mask=mask)
  ref64, ref32 = _spec_refs(spec, params, batch, init_z, noise, known, mask)
  kept = mask.astype(bool)
  np.testing.assert_array_equal(helpers.bits(got[kept]), helpers.bits(known[kept]))
  # the free frames only: the kept ones are exact and would dilute the fractions
  helpers.assert_fp32_class(got[~kept], ref64[~kept], ref32[~kept], 'keep b=%d' % b)


def test_chain_matches_the_spec_ddim_without_context(torch):
  spec, params, model = _model(torch, 'tiny', 8, 'ddim')
  batch = helpers.make_batch(spec, batch=2)
  init_z, _ = helpers.make_noise(spec, batch=2)
  known, mask = helpers.known_mel((2, 64, 128)), keep_spec.parity_masks(2)
  got, _ = model.predict(batch, init_z=init_z, keep=known, keep_mask=mask)
  ref64, ref32 = _spec_refs(spec, params, batch, init_z, None, known, mask)
  kept = mask.astype(bool)
  np.testing.assert_array_equal(helpers.bits(got[kept]), helpers.bits(known[kept]))
  helpers.assert_fp32_class(got[~kept], ref64[~kept], ref32[~kept], 'keep ddim')


# --------------------------------------------------------------------------------------------------
# 5. plain and keep graphs live side by side
# --------------------------------------------------------------------------------------------------
def test_plain_and_keep_calls_alternate_on_one_handle(torch):
  spec, params, _ = _model(torch, 'tiny_context', 10)   # (with the remainder graph)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  known, mask = helpers.known_mel((2, 64, 128)), keep_spec.parity_masks(2)
  kw = dict(seed=[6, 7], segment=[1, 2])

  def handle():
    return msd_amd.InferenceModel(params, spec, batch_size=2, **helpers.ALL_PLANES)

  one = handle()
  runs = [one.predict(batch, **kw)[0], one.predict(batch, keep=known, keep_mask=mask, **kw)[0],
          one.predict(batch, **kw)[0], one.predict(batch, keep=known, keep_mask=mask, **kw)[0]]
  fresh_plain = handle().predict(batch, **kw)[0]
  fresh_keep = handle().predict(batch, keep=known, keep_mask=mask, **kw)[0]   # keep first on this one
  np.testing.assert_array_equal(helpers.bits(runs[0]), helpers.bits(runs[2]))
  np.testing.assert_array_equal(helpers.bits(runs[0]), helpers.bits(fresh_plain))
  np.testing.assert_array_equal(helpers.bits(runs[1]), helpers.bits(runs[3]))
  np.testing.assert_array_equal(helpers.bits(runs[1]), helpers.bits(fresh_keep))
  assert not np.array_equal(runs[0], runs[1])


# --------------------------------------------------------------------------------------------------
# 6. regenerate
# --------------------------------------------------------------------------------------------------
def test_regenerate_a_region_across_a_boundary(torch):
  from msd_amd import inference
  spec, _, model = _model(torch)
  toks = [msd_amd.synthetic.segment_tokens(spec, k, min_len=8, max_len=126) for k in range(3)]
  song = helpers.known_mel((1, 192, 128), seed=8)
  new = model.regenerate(song, toks, 40, 100, seed=12)
  assert new.shape == song.shape and new.dtype == np.float32
  np.testing.assert_array_equal(helpers.bits(new[:, :40]), helpers.bits(song[:, :40]))
  np.testing.assert_array_equal(helpers.bits(new[:, 100:]), helpers.bits(song[:, 100:]))   # segment 2 included: untouched
  assert np.abs(new[:, 40:100] - song[:, 40:100]).max() > 1.0
  # the two predict calls the plan names
  plan = inference.plan_region(192, 64, 40, 100)
  assert [k for k, _ in plan] == [0, 1]
  zeros = np.zeros((1, 64, 128), np.float32)
  first, _ = model.predict({'encoder_input_tokens': toks[0].reshape(1, -1), 'encoder_continuous_inputs': zeros,
                            'encoder_continuous_mask': np.zeros((1, 64), np.int32)},
                           seed=12, segment=0, keep=song[:, :64], keep_mask=plan[0][1][None])
  second, _ = model.predict({'encoder_input_tokens': toks[1].reshape(1, -1), 'encoder_continuous_inputs': first,
                             'encoder_continuous_mask': np.ones((1, 64), np.int32)},
                            seed=12, segment=1, keep=song[:, 64:128], keep_mask=plan[1][1][None])
  np.testing.assert_array_equal(helpers.bits(new[:, :64]), helpers.bits(first))
  np.testing.assert_array_equal(helpers.bits(new[:, 64:128]), helpers.bits(second))
