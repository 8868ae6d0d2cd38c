"""-m gpu: deterministic DDIM inversion (msd_invert, msd_op_invert_step, InferenceModel.invert / rerender) against the
specification of tests/invert_spec.py.

Presets tiny / tiny_context: T = 64, n = 128, so a row of z is 8 of the sampler's 1024-element blocks.  The handles have
N = 96 steps and weight 5 (graph_steps 8): an inversion of 24 steps is three graphs, one of 12 a graph and four single
steps, one of 1 a single step."""
import ctypes
import dataclasses

import numpy as np
import pytest

import msd_amd
from tests import helpers, invert_spec as inv, multistep_spec as ms
from tests.helpers import gpu_torch  # noqa: F401  (the `torch` fixture)

pytestmark = pytest.mark.gpu

N = 96


def _ids(c):
  return ','.join('%s=%s' % kv for kv in c.items()) or 'default'


# --------------------------------------------------------------------------------------------------
# 6. one update against the spec
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['eps', 'x0', 'v'])
def test_op_invert_step_vs_spec(torch, mode):
  """msd_op_invert_step on two rows of 1024 elements with the weights (1, 1), (5, 5) and (1, 5), at index 0, a middle one
  and K - 1: the single-update criterion of tests/test_gpu_keep_frames.py (device error <= 1e-6 + 4 x the float32
  restatement's, scaled); the planes merge back to z_out; a per-row call's row b holds the bits of the one-row call."""
  from msd_amd import inference, native
  from oracle import backend
  from tests import guidance_spec as gs
  spec = helpers.sampler_spec(sampler='ddim', model_output=mode, steps=50)   # (clip stays on: the op must not read it)
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, 'f16x3')
  _, dc = helpers.oracle_configs(spec)
  steps = dc.sampler.schedule.num_steps
  rng = np.random.default_rng(5)
  shape = (2, 8, 128)
  for i in (0, steps // 2, steps - 1):
    z, oc, ou = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    rows = {}
    for weights in ([1.0, 1.0], [5.0, 5.0], [1.0, 5.0]):
      one_pass = all(w == 1.0 for w in weights)
      out = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
      planes = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
      native.op_invert_step(cfg, i, helpers.dev(torch, z), helpers.dev(torch, oc), None if one_pass else helpers.dev(torch, ou),
                            weights, out, planes)
      got, zp = out.cpu().numpy(), planes.cpu().numpy()
      assert np.isfinite(got).all()
      for b, w in enumerate(weights):
        row = slice(b, b + 1)
        refs = {}
        for name, xp in (('f32', backend.NumpyBackend('float32')), ('f64', backend.NumpyBackend('float64'))):
          pred = lambda z, time, include_conditioning, _xp=xp: _xp.asarray((oc if include_conditioning else ou)[row])
          refs[name] = np.asarray(inv.step(xp, gs.with_weight(dc, w), xp.asarray(z[row]), i, pred), np.float64)
        scale = max(1.0, float(np.abs(refs['f64']).max()))
        e_dev = np.abs(got[row].astype(np.float64) - refs['f64']).max() / scale
        e_f32 = np.abs(refs['f32'] - refs['f64']).max() / scale
        print('invert step %s i=%d w=%g: scaled error device %.3e / float32 %.3e' % (mode, i, w, e_dev, e_f32))
        assert e_dev <= 1e-6 + 4 * e_f32, (mode, i, w, e_dev, e_f32)
        rows.setdefault(w, []).append(got[row])
      # the planes merge back to exactly what a hi / lo split of z_out holds (tests/helpers.py planes_merged)
      np.testing.assert_array_equal(helpers.bits(zp), helpers.bits(helpers.planes_merged(got, 'f16x3')))
      assert np.abs(zp - got).max() > 0   # (planes, not a copy of z)
    # row b of the (1, 5) call: row 0 of (1, 1)'s bits and row 1 of (5, 5)'s
    np.testing.assert_array_equal(helpers.bits(rows[1.0][2]), helpers.bits(rows[1.0][0]))
    np.testing.assert_array_equal(helpers.bits(rows[5.0][2]), helpers.bits(rows[5.0][1]))
    # ... and a one-row call with the row's weight
    one = torch.empty((1,) + shape[1:], dtype=torch.float32, device='cuda')
    native.op_invert_step(cfg, i, helpers.dev(torch, z[1:]), helpers.dev(torch, oc[1:]), helpers.dev(torch, ou[1:]), [5.0], one,
                          torch.empty_like(one))
    np.testing.assert_array_equal(helpers.bits(one.cpu().numpy()), helpers.bits(rows[5.0][2]))
    assert not np.array_equal(rows[1.0][0], rows[5.0][0])
  # the op refuses a missing unconditional output, and an unconditional output nobody reads
  bad = torch.empty(shape, dtype=torch.float32, device='cuda')
  with pytest.raises(ValueError):
    native.op_invert_step(cfg, 1, bad, bad, None, [1.0, 5.0], bad, torch.empty_like(bad))
  with pytest.raises(ValueError):
    native.op_invert_step(cfg, 1, bad, bad, bad, [1.0, 1.0], bad, torch.empty_like(bad))


@pytest.mark.parametrize('precision', ['f16x3', 'f16', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('side, target', helpers.RANGE_TARGETS, ids=[s for s, _ in helpers.RANGE_TARGETS])
def test_op_invert_step_range_flag(torch, side, target, precision):
  """The range flag of sampler_invert_kernel's tail: eps mode, weight 1 and z = 0 at one element of the launch's last float4
  make its output b * o there; o aims it 2^-12 below 65504 (passes) and 2^-12 above (RangeError with half planes)."""
  from msd_amd import inference, native
  from oracle import backend
  from tests import guidance_spec as gs
  spec = helpers.sampler_spec(sampler='ddim', model_output='eps', steps=50)
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, precision)
  _, dc = helpers.oracle_configs(spec)
  i = dc.sampler.schedule.num_steps // 2
  rng = np.random.default_rng(31)
  shape = (2, 8, 128)
  e = 2 * 1024 - 2
  z, oc = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
  xp64 = backend.NumpyBackend('float64')
  b64 = float(np.asarray(inv.coefficients(xp64, dc, 1, i)[1]).reshape(-1)[0])
  z.reshape(-1)[e] = 0.0
  oc.reshape(-1)[e] = target / b64
  refs = {}
  for name, xp in (('f32', backend.NumpyBackend('float32')), ('f64', xp64)):
    pred = lambda z, time, include_conditioning, _xp=xp: _xp.asarray(oc)
    refs[name] = np.asarray(inv.step(xp, gs.with_weight(dc, 1.0), xp.asarray(z), i, pred), np.float64)

  def call():
    out, planes = (torch.full(shape, float('nan'), dtype=torch.float32, device='cuda') for _ in range(2))
    native.op_invert_step(cfg, i, helpers.dev(torch, z), helpers.dev(torch, oc), None, [1.0, 1.0], out, planes)
    return out.cpu().numpy(), planes.cpu().numpy()
  helpers.check_range_case(call, side, precision, refs['f32'], refs['f64'], target, e)


# --------------------------------------------------------------------------------------------------
# models and references
# --------------------------------------------------------------------------------------------------
_cache, _models = {}, {}


def _spec_of(preset, steps, w=5.0, model_output='eps', clip=True):
  spec = helpers.preset_spec(preset, steps)
  d = spec.diffusion
  return dataclasses.replace(spec, diffusion=dataclasses.replace(
      d, model_output=model_output, sampler=dataclasses.replace(d.sampler, clip_x0=clip),
      classifier_free_guidance=dataclasses.replace(d.classifier_free_guidance, eval_condition_weight=w)))


def _weights(preset):
  return msd_amd.synthetic.init_params(helpers.preset_spec(preset, N), 3, norm_scale_jitter=0.1)


def _model(preset='tiny', steps=N, w=5.0, model_output='eps', clip=True, **kw):
  """(spec, params, model): one two-row handle per configuration for the whole module; the default ones are
  helpers.cached_model's."""
  if (w, model_output, clip) == (5.0, 'eps', True) and not kw:
    return helpers.cached_model(_cache, preset, steps)
  key = (preset, steps, w, model_output, clip, tuple(sorted(kw.items())))
  if key not in _models:
    spec = _spec_of(preset, steps, w, model_output, clip)
    params = _weights(preset)
    _models[key] = (spec, params, msd_amd.InferenceModel(params, spec, batch_size=2, **helpers.ALL_PLANES, **kw))
  return _models[key]


def _batch(spec, rows=2, seed=21):
  batch = helpers.make_batch(spec, batch=rows, ctx_mask='ragged')
  batch['decoder_target_tokens'] = helpers.known_mel((rows, 64, 128), seed)   # (leaves the codec's range at both ends)
  return batch


def _references(preset, params, steps, batch, weights, model_output='eps', clip=True, round_trip=False):
  """[float64, float32] results of the specification on the oracle's network configured with `steps` steps."""
  from oracle import backend, fast
  spec = _spec_of(preset, steps, 5.0, model_output, clip)
  cfg, dc = helpers.oracle_configs(spec)
  refs = []
  for dtype in ('float64', 'float32'):
    fm = fast.FastModel(backend.TorchBackend(dtype), cfg, dc, params, spec.has_context)
    fn = inv.round_trip if round_trip else inv.invert
    refs.append(fn(fm, batch, batch['decoder_target_tokens'], weights))
    del fm
  return refs


# --------------------------------------------------------------------------------------------------
# 7. chains against the spec
# --------------------------------------------------------------------------------------------------
CHAINS = [
    dict(preset='tiny', steps=24, w=1.0),
    dict(preset='tiny', steps=24, w=5.0),
    dict(preset='tiny_context', steps=12, w=1.0),
    dict(preset='tiny_context', steps=12, w=5.0),
    dict(preset='tiny_context', steps=24, w=[1.0, 5.0]),
    dict(preset='tiny', steps=12, w=5.0, model_output='x0'),
]


@pytest.mark.parametrize('case', CHAINS, ids=_ids)
def test_inversion_chain_vs_spec(torch, case):
  """The upward chain has no clip and no x22026 first step: float32-class against the float64 spec with the float32
  oracle run of the same spec as the yardstick."""
  preset, k, w, mode = case['preset'], case['steps'], case['w'], case.get('model_output', 'eps')
  spec, params, model = _model(preset, model_output=mode)
  batch = _batch(spec)
  got = model.invert(batch, steps=k, guidance=w)
  assert got.shape == (2, 64, 128) and got.dtype == np.float32 and np.isfinite(got).all()
  weights = w if isinstance(w, list) else [w, w]
  ref64, ref32 = _references(preset, params, k, batch, weights, mode)
  helpers.assert_fp32_class(got, ref64, ref32, 'inversion %s' % case)
  print('inversion %s: median |err| %.3e, rms of the noise %.3f' % (case, float(np.median(np.abs(got - ref64))), float(np.sqrt(np.mean(ref64 ** 2)))))
  # (a call that ignored the weight, the tokens' mel or the step count cannot pass)
  other = model.invert(batch, steps=k, guidance=2.0)
  assert helpers.rms(other, got) > 1e-3


# --------------------------------------------------------------------------------------------------
# 8. bit identities
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [24, 12, 1])
def test_k_step_inversion_is_a_fresh_handle_created_with_k_steps(torch, k):
  spec, _, model = _model('tiny')
  _, _, fresh = _model('tiny', k)
  batch = _batch(spec)
  for w in (None, 5.0):
    got, want = model.invert(batch, steps=k, guidance=w), fresh.invert(batch, guidance=w)
    np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))
  assert helpers.rms(model.invert(batch, steps=k), model.invert(batch, steps=k, guidance=5.0)) > 1e-3


def test_scalar_weight_rows_repeats_and_single_steps(torch):
  spec, _, model = _model('tiny')
  batch = _batch(spec)
  # a scalar weight w is the handle created with cfg_weight = w; weight 1 the handle created with weight 1 (one-pass plan)
  for w in (2.0, 1.0):
    _, _, fresh = _model('tiny', 24, w=w)
    np.testing.assert_array_equal(helpers.bits(model.invert(batch, steps=24, guidance=w)), helpers.bits(fresh.invert(batch, guidance=w)))
  # None is weight 1 -- not the handle's 5
  np.testing.assert_array_equal(helpers.bits(model.invert(batch, steps=24)), helpers.bits(model.invert(batch, steps=24, guidance=1.0)))
  # the rows of a 2-row call are their one-row calls
  got = model.invert(batch, steps=24, guidance=[1.0, 5.0])
  for b, w in enumerate([1.0, 5.0]):
    row = {key: np.ascontiguousarray(v[b:b + 1]) for key, v in batch.items()}
    np.testing.assert_array_equal(helpers.bits(model.invert(row, steps=24, guidance=w)), helpers.bits(got[b:b + 1]))
  # a second identical call is the first
  np.testing.assert_array_equal(helpers.bits(model.invert(batch, steps=24, guidance=[1.0, 5.0])), helpers.bits(got))
  # graphs + singles (12 steps, 8 per graph) are singles only on a fresh handle
  _, _, singles = _model('tiny', graph_steps=1)
  for w in (1.0, 5.0):
    np.testing.assert_array_equal(helpers.bits(model.invert(batch, steps=12, guidance=w)), helpers.bits(singles.invert(batch, steps=12, guidance=w)))


# --------------------------------------------------------------------------------------------------
# 9. the handle is left intact
# --------------------------------------------------------------------------------------------------
def test_inversions_between_other_calls_leave_the_handle_intact(torch):
  """One 24-step handle: plain predict, invert, keep call, invert with weight 5, guided predict, reset_graph, then the same in
  reverse.  Every predict output is the first call of a fresh handle, every inversion the first one's bits."""
  spec = msd_amd.config.preset('tiny_context', num_steps=24)
  params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
  make = lambda: msd_amd.InferenceModel(params, spec, batch_size=2, **helpers.ALL_PLANES)
  batch = _batch(spec)
  rng = np.random.default_rng(21)
  known = rng.uniform(-11.0, 4.0, (2, 64, 128)).astype(np.float32)
  mask = np.zeros((2, 64), np.int32)
  mask[0, :32] = 1
  mask[1, ::2] = 1
  forms = [('plain', 'predict', dict(seed=4, segment=2)), ('invert', 'invert', dict()),
           ('keep', 'predict', dict(seed=4, segment=2, keep=known, keep_mask=mask)), ('invert w=5', 'invert', dict(guidance=5.0, steps=12)),
           ('guided', 'predict', dict(seed=4, segment=2, guidance=2.0, guidance_interval=(0.25, 0.75), steps=12))]
  run = lambda m, kind, kw: m.predict(batch, **kw)[0] if kind == 'predict' else m.invert(batch, **kw)
  fresh = {}
  for name, kind, kw in forms:   # each form as the FIRST call of a handle of its own
    model = make()
    fresh[name] = run(model, kind, kw)
    assert np.isfinite(fresh[name]).all(), name
    model._get_native().close()
  assert len({helpers.bits(v).tobytes() for v in fresh.values()}) == len(forms)
  model = make()
  first = {name: run(model, kind, kw) for name, kind, kw in forms}
  model._get_native().reset_graph()
  second = {name: run(model, kind, kw) for name, kind, kw in reversed(forms)}
  for name, _, _ in forms:
    np.testing.assert_array_equal(helpers.bits(first[name]), helpers.bits(fresh[name]), err_msg='forward, ' + name)
    np.testing.assert_array_equal(helpers.bits(second[name]), helpers.bits(fresh[name]), err_msg='reverse, ' + name)
  # The make_room hazard: seven sets cached, then an inversion whose set is the eighth / whose set is among them
  nm = model._get_native()
  keys = dict(seed=4, segment=2)
  combos = [(k, s) for s in ('ddim', 'dpmpp_2m') for k in (1, 2, 3)]
  nm.reset_graph()
  runs = [model.predict(batch, **keys)[0]] + [model.predict(batch, steps=k, sampler=s, **keys)[0] for k, s in combos]   # seven sets
  np.testing.assert_array_equal(helpers.bits(model.invert(batch)), helpers.bits(fresh['invert']))                        # the eighth
  np.testing.assert_array_equal(helpers.bits(model.invert(batch, guidance=5.0, steps=12)), helpers.bits(fresh['invert w=5']))   # a ninth: the cache is emptied
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, **keys)[0]), helpers.bits(runs[0]))
  nm.reset_graph()
  model.invert(batch)
  for k, s in combos:   # seven sets, the inversion's among them
    model.predict(batch, steps=k, sampler=s, **keys)
  np.testing.assert_array_equal(helpers.bits(model.invert(batch)), helpers.bits(fresh['invert']))
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, **keys)[0]), helpers.bits(runs[0]))                    # the eighth
  np.testing.assert_array_equal(helpers.bits(model.invert(batch)), helpers.bits(fresh['invert']))
  for (k, s), r in zip(combos, runs[1:]):
    np.testing.assert_array_equal(helpers.bits(model.predict(batch, steps=k, sampler=s, **keys)[0]), helpers.bits(r))


# --------------------------------------------------------------------------------------------------
# 10. the closed form on the device
# --------------------------------------------------------------------------------------------------
def test_ideal_denoiser_chain_through_the_op(torch):
  """The K = 50 ideal-denoiser chain through msd_op_invert_step, the model outputs computed on the host from the device's own
  state: its distance to the float64 spec chain is at most 4 x the distance a float32 NumPy restatement of the same lines
  keeps (two float32 evaluations that differ in operation order)."""
  from msd_amd import inference, native
  from oracle import backend
  steps = 50
  spec = helpers.sampler_spec(sampler='ddim', cfg_weight=1.0, clip=False, steps=steps)
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, 'f16x3')
  _, dc = helpers.oracle_configs(spec)
  xp32, xp64 = backend.NumpyBackend('float32'), backend.NumpyBackend('float64')
  x = (np.sqrt(ms.DATA_VAR) * np.random.default_rng(5).standard_normal((1, 8, 128))).astype(np.float32)
  ref64 = np.asarray(inv.scan(xp64, xp64.asarray(x), ms.ideal_pred_fn(xp64, dc), dc), np.float64)
  ref32 = np.asarray(inv.scan(xp32, xp32.asarray(x), ms.ideal_pred_fn(xp32, dc), dc), np.float64)
  pred32 = ms.ideal_pred_fn(xp32, dc)
  z = x
  for i in range(steps):
    time = xp32.asarray(np.full((1,), (i + 1.0) / steps))
    o = np.asarray(pred32(z=xp32.asarray(z), time=time, include_conditioning=True), np.float32)
    out = torch.empty(z.shape, dtype=torch.float32, device='cuda')
    native.op_invert_step(cfg, i, helpers.dev(torch, z), helpers.dev(torch, o), None, [1.0], out, torch.empty_like(out))
    z = out.cpu().numpy()
  d_dev, d_f32 = helpers.rms(z, ref64), helpers.rms(ref32, ref64)
  print('ideal-denoiser inversion, K = 50: rms distance to the float64 chain device %.3e / float32 NumPy %.3e (ratio %.2f); '
        'distance of the float64 chain to the ODE solution %.3e' % (d_dev, d_f32, d_dev / d_f32, helpers.rms(ref64, inv.exact_top_point(x))))
  assert d_dev <= 4 * d_f32


# --------------------------------------------------------------------------------------------------
# 11. round trip wiring
# --------------------------------------------------------------------------------------------------
def test_round_trip_matches_the_specs_round_trip(torch):
  """invert, then predict(init_z=noise, sampler='ddim', steps=24, guidance=1.0) on a clip-off tiny model: float32-class
  against the spec's own round trip.  How far the round trip lands from the mel is printed, not asserted.
  (What this checks is the WIRING -- the noise is handed over in model units and rendered under the same weight and step
  count.  On synthetic weights the network's eps moves by O(1) between two levels, and the render's first step multiplies
  that by 1 / alpha_K = 22026: measured on the MI355X, the spec's own round trip misses the mel by rms 4e4, the float32
  oracle and the device are both O(10) from the float64 rendering, and the criterion on the rendering is as weak as that.
  The criterion on the noise is the sharp one: median error 4.9e-5 for the device and for the float32 oracle alike.)"""
  spec, params, model = _model('tiny', clip=False)
  batch = _batch(spec)
  batch['decoder_target_tokens'] = np.random.default_rng(2).uniform(-10.0, 3.0, (2, 64, 128)).astype(np.float32)
  noise = model.invert(batch, steps=24, guidance=1.0, return_torch=True)
  got, _ = model.predict(batch, init_z=noise, sampler='ddim', steps=24, guidance=1.0)
  refs = _references('tiny', params, 24, batch, [1.0, 1.0], clip=False, round_trip=True)
  helpers.assert_fp32_class(noise.cpu().numpy(), refs[0][0], refs[1][0], 'round trip: the noise')
  helpers.assert_fp32_class(got, refs[0][1], refs[1][1], 'round trip: the rendering')
  print('round trip, 24 steps, weight 1: rms mel error of the spec %.4f, of the device %.4f (mel rms %.3f)'
        % (helpers.rms(refs[0][1], batch['decoder_target_tokens']), helpers.rms(got, batch['decoder_target_tokens']),
           float(np.sqrt(np.mean(batch['decoder_target_tokens'].astype(np.float64) ** 2)))))


def test_rerender_is_the_hand_written_sequence(torch):
  spec, _, model = _model('tiny_context')
  song = helpers.known_mel((1, 128, 128), 4)
  toks = [msd_amd.synthetic.segment_tokens(spec, k, min_len=8, max_len=spec.task_feature_lengths['inputs'] - 2)[0] for k in range(2)]
  got = model.rerender(song, toks, toks, steps=12, guidance=2.0, render_guidance=2.0)
  assert got.shape == (1, 128, 128) and np.isfinite(got).all()
  outs = []
  for k in range(2):
    ctx = dict(encoder_continuous_inputs=np.zeros((1, 64, 128), np.float32) if k == 0 else None,
               encoder_continuous_mask=(np.zeros if k == 0 else np.ones)((1, 64), np.int32))
    old = dict(ctx, encoder_input_tokens=toks[k].reshape(1, -1), decoder_target_tokens=song[:, k * 64:(k + 1) * 64])
    new = dict(ctx, encoder_input_tokens=toks[k].reshape(1, -1))
    if k:
      old['encoder_continuous_inputs'], new['encoder_continuous_inputs'] = song[:, :64], outs[0]
    noise = model.invert(old, steps=12, guidance=2.0)
    outs.append(model.predict(new, init_z=noise, sampler='ddim', steps=12, guidance=2.0)[0])
  np.testing.assert_array_equal(helpers.bits(got), helpers.bits(np.concatenate(outs, 1)))
  assert helpers.rms(got[:, 64:], model.rerender(song, toks, toks[::-1], steps=12, guidance=2.0, render_guidance=2.0)[:, 64:]) > 1e-3


# --------------------------------------------------------------------------------------------------
# 12. refusals on the device
# --------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_running(torch):
  from msd_amd import native
  spec = _spec_of('tiny', 24, w=1.0)
  params = _weights('tiny')
  model = msd_amd.InferenceModel(params, spec, batch_size=2, **helpers.ALL_PLANES)
  batch = _batch(spec)
  nm = model._get_native()
  stream = model._stream.cuda_stream
  mel = helpers.dev(torch, batch['decoder_target_tokens'])
  out = torch.empty((2, 64, 128), dtype=torch.float32, device='cuda')
  with pytest.raises(RuntimeError, match='msd_encode has not run'):   # before msd_encode
    nm.invert(2, out, mel, stream=stream)
  want, _ = model.predict(batch, seed=4, segment=2)
  usual = model.invert(batch)
  a = native.InvertArgs()
  a.struct_size, a.batch, a.mel_dev, a.out_dev = 8, 2, mel.data_ptr(), out.data_ptr()
  assert nm.lib.msd_invert(nm.handle, ctypes.byref(a), stream) == native.MSD_ERR_INVALID_ARGUMENT
  assert 'struct_size' in nm.lib.msd_last_error(nm.handle).decode()
  with pytest.raises(NotImplementedError, match='any weight != 1'):   # (MSD_ERR_UNSUPPORTED) weights != 1 on a weight-1 handle
    nm.invert(2, out, mel, guidance=3.0, stream=stream)
  with pytest.raises(ValueError, match='weight 1'):
    model.invert(batch, guidance=[1.0, 3.0])
  a.struct_size = ctypes.sizeof(native.InvertArgs)
  for field, value, word in (('num_steps', 7, 'does not divide'), ('batch', 1, 'encoded batch'), ('mel_dev', None, 'null')):
    b = native.InvertArgs.from_buffer_copy(a)
    setattr(b, field, value)
    assert nm.lib.msd_invert(nm.handle, ctypes.byref(b), stream) == native.MSD_ERR_INVALID_ARGUMENT, field
    assert word in nm.lib.msd_last_error(nm.handle).decode(), field
  nan = (ctypes.c_float * 2)(1.0, float('nan'))
  a.weights_host, a.n_weights = nan, 2
  assert nm.lib.msd_invert(nm.handle, ctypes.byref(a), stream) == native.MSD_ERR_INVALID_ARGUMENT
  assert 'finite' in nm.lib.msd_last_error(nm.handle).decode()
  np.testing.assert_array_equal(helpers.bits(model.predict(batch, seed=4, segment=2)[0]), helpers.bits(want))
  np.testing.assert_array_equal(helpers.bits(model.invert(batch)), helpers.bits(usual))


# --------------------------------------------------------------------------------------------------
# 13. range fallback
# --------------------------------------------------------------------------------------------------
def test_range_error_and_fallback(torch):
  """The scaled-norm model of tests/test_gpu_model.py: MSD_ERR_RANGE on 'f16x3'; with range_fallback the call is repeated on
  the bfloat16 planes and matches the spec at their level (that test's bound)."""
  from tests.test_gpu_model import _overflowing_params
  spec = helpers.preset_spec('tiny_context', 8)
  params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
  big = _overflowing_params(params)
  batch = _batch(spec, rows=1)
  strict = msd_amd.InferenceModel(big, spec, range_fallback=False)
  with pytest.raises(msd_amd.native.RangeError, match='bf16x3'):
    strict.invert(batch, guidance=5.0)
  with pytest.raises(msd_amd.native.RangeError):   # the flag was re-armed
    strict.invert(batch)
  model = msd_amd.InferenceModel(big, spec, range_fallback=True)
  with pytest.warns(RuntimeWarning, match='bf16x3'):
    got = model.invert(batch, guidance=5.0)
  assert model.precision == 'bf16x3' and model._get_native().planes == 'bf16' and np.isfinite(got).all()
  from oracle import backend, fast
  cfg, dc = helpers.oracle_configs(dataclasses.replace(spec, diffusion=dataclasses.replace(
      spec.diffusion, sampler=dataclasses.replace(spec.diffusion.sampler, name='ddim'))))
  refs = [inv.invert(fast.FastModel(backend.TorchBackend(dt), cfg, dc, big, spec.has_context), batch, batch['decoder_target_tokens'], [5.0])
          for dt in ('float64', 'float32')]
  e, e32 = helpers.rms(got, refs[0]), helpers.rms(refs[1], refs[0])
  print('[range fallback] inversion rms vs float64 %.3e (float32 oracle %.3e)' % (e, e32))
  assert e <= 4 * e32 + 1e-4


# --------------------------------------------------------------------------------------------------
# 14. base-size tiles
# --------------------------------------------------------------------------------------------------
def test_base_size_inversion(torch):
  """One base_with_context handle of 96 steps, a 3-step inversion with context at weight 1 (the one-pass plan's tile family)
  and at weight 5: float32-class against the spec."""
  from oracle import backend, fast
  spec = msd_amd.config.preset('base_with_context', num_steps=N)
  params = msd_amd.synthetic.init_params(spec, 21, norm_scale_jitter=0.1)
  model = msd_amd.InferenceModel(params, spec, batch_size=1, **helpers.ALL_PLANES)
  try:
    batch = helpers.make_batch(spec, batch=1, ctx_mask='ragged')
    batch['decoder_target_tokens'] = helpers.known_mel((1, 256, 128))
    cfg, dc = helpers.oracle_configs(helpers.preset_spec('base_with_context', 3, 'ddim'))
    got = {w: model.invert(batch, steps=3, guidance=w) for w in (1.0, 5.0)}
    refs = {}
    for dt in ('float64', 'float32'):   # (one oracle network per precision serves both weights)
      fm = fast.FastModel(backend.TorchBackend(dt), cfg, dc, params, True)
      for w in (1.0, 5.0):
        refs[w, dt] = inv.invert(fm, batch, batch['decoder_target_tokens'], [w])
      del fm
    for w in (1.0, 5.0):
      helpers.assert_fp32_class(got[w], refs[w, 'float64'], refs[w, 'float32'], 'base_with_context, 3 of 96 steps, weight %g' % w)
    assert helpers.rms(got[1.0], got[5.0]) > 1e-3
  finally:
    del model
    torch.cuda.empty_cache()
