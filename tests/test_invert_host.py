"""DDIM inversion on the host (no GPU): the identities of the specification (tests/invert_spec.py) in float64, the side
table's Python twin, the planner's and the CLI's refusals, and rerender's call sequence."""
import os
import re

import numpy as np
import pytest

import msd_amd
from msd_amd import inference, native
from oracle import backend, sampler
from tests import guidance_spec as gs, helpers, invert_spec as inv, multistep_spec as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 50


# ---- 1. the exact inverse with frozen eps ----------------------------------------------------------------------------
@pytest.mark.parametrize('w', [1.0, 5.0])
@pytest.mark.parametrize('mode', ['eps', 'x0', 'v'])
def test_inverse_step_with_frozen_eps_returns_the_state_above(mode, w):
  """u = the oracle's own ddim_step result from a random state at index i; the spec's inverse step, fed the eps the forward
  step used, returns that state.  Indices 0, 1 and a middle one: within 1e-12 of the state's scale.  Index K - 1: the forward
  step divides by alpha_t = sqrt(sigmoid(-20)) = 4.5e-5, so the bound is that amplification x 2^-52, computed here."""
  spec = helpers.sampler_spec(sampler='ddim', model_output=mode, cfg_weight=w, clip=False, steps=K)
  _, dc = helpers.oracle_configs(spec)
  xp = backend.NumpyBackend('float64')
  rng = np.random.default_rng(3)
  shape = (2, 8, 128)
  for i in (0, 1, K // 2, K - 1):
    state, oc, ou = (rng.standard_normal(shape) for _ in range(3))
    pred = lambda z, time, include_conditioning: xp.asarray(oc if include_conditioning else ou)
    u = sampler.eval_step(xp, None, dc, shape[0], pred)(xp.asarray(state), i)
    eps = inv.pred_eps(xp, dc, xp.asarray(state), i, pred)   # (clip off: body's pred_eps as the step used it)
    back = np.asarray(inv.step(xp, dc, u, i, pred, eps=eps), np.float64)
    rel = np.abs(back - state).max() / np.abs(state).max()
    bound = 1e-12
    if i == K - 1:
      lt, _ = ms.logsnrs(xp, dc, 1, i)
      amplification = 1.0 / float(np.sqrt(1.0 / (1.0 + np.exp(-np.asarray(lt, np.float64)[0]))))
      assert 2.0e4 < amplification < 2.3e4
      bound = amplification * 2.0 ** -52
    print('%s w=%g i=%d: relative error %.3e (bound %.3e)' % (mode, w, i, rel, bound))
    assert rel <= bound, (mode, w, i, rel, bound)
    # ... and with the eps of the state BELOW (what the inversion has) the step is another one: the identity is about frozen eps
    if i == K // 2:
      assert np.abs(np.asarray(inv.step(xp, dc, u, i, lambda z, time, include_conditioning: xp.asarray(0.5 * oc)), np.float64)
                    - state).max() > 1e-3


# ---- 2. the closed form ------------------------------------------------------------------------------------------------
def _ideal_chain(xp, steps, x):
  spec = helpers.sampler_spec(sampler='ddim', cfg_weight=1.0, clip=False, steps=steps)
  _, dc = helpers.oracle_configs(spec)
  return np.asarray(inv.scan(xp, xp.asarray(x), ms.ideal_pred_fn(xp, dc), dc), np.float64)


def test_ideal_denoiser_chain_approaches_the_probability_flow_solution():
  """Gaussian data and its ideal denoiser: the inversion chain's end point approaches x sqrt(alpha_1^2 v + sigma_1^2) /
  sqrt(v), the probability-flow ODE's solution at t = 1.  An ordering in K, not a figure."""
  xp = backend.NumpyBackend('float64')
  x = np.sqrt(ms.DATA_VAR) * np.random.default_rng(5).standard_normal((1, 8, 128))
  want = inv.exact_top_point(x)
  err = {k: helpers.rms(_ideal_chain(xp, k, x), want) for k in (20, 50, 200)}
  print('ideal-denoiser inversion, rms distance to the ODE solution:', err)
  assert err[200] < err[50] < err[20]
  assert err[20] < 0.5 * float(np.sqrt(np.mean(want ** 2)))   # (and the coarsest is already in the solution's neighbourhood)
  # the exact solutions are each other's inverses
  np.testing.assert_allclose(ms.exact_end_point(want), x, rtol=1e-12)


# ---- 3. the side table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [96, 1000])
def test_side_table_twin_matches_the_spec_for_every_divisor(n):
  """native.invert_rows (the Python twin of build_invert_rows) against the spec's a, b for every K | n.  The twin reads
  float32 log-SNRs: |d logsnr| <= 2^-24 * 20 = 1.2e-6, and d ln(alpha) = sigmoid(-logsnr) d logsnr / 2, likewise sigma, so a
  moves by at most 2 * 6e-7 relative (+ its float32 rounding, 6e-8) and b = sigma_t - a sigma_s, all three <= 1, by at most
  6e-7 + 1.3e-6 + 6e-7 absolute (+ 6e-8)."""
  xp = backend.NumpyBackend('float64')
  _, dc = helpers.oracle_configs(helpers.sampler_spec(steps=n))
  for k in native.divisors(n):
    dck = ms.with_steps(dc, k)
    rows = [ms.logsnrs(xp, dck, 1, i) for i in range(k)]
    lt = np.asarray([np.asarray(r[0], np.float64)[0] for r in rows])
    ls = np.asarray([np.asarray(r[1], np.float64)[0] for r in rows])
    table = native.invert_rows(lt.astype(np.float32), ls.astype(np.float32))
    assert table.dtype == np.float32 and table.shape == (k, 4) and not table[:, 2:].any()
    want = np.asarray([[np.asarray(c, np.float64)[0] for c in inv.coefficients(xp, dck, 1, i)] for i in range(k)])
    assert np.all(np.abs(table[:, 0] - want[:, 0]) <= 2e-6 * np.abs(want[:, 0])), k
    assert np.all(np.abs(table[:, 1] - want[:, 1]) <= 3e-6), k
    # row 0 is (alpha_1, sigma_1): level 1's own values, no quotient
    l1 = np.float64(np.float32(lt[0]))
    assert table[0, 0] == np.float32(np.sqrt(1.0 / (1.0 + np.exp(-l1)))) and table[0, 1] == np.float32(np.sqrt(1.0 / (1.0 + np.exp(l1))))
    if k > 1:   # ... and the rows above it are quotients: a_i alpha_i = alpha_{i+1}
      assert 0.0 < table[1:, 0].max() < 1.0
  with pytest.raises(ValueError):
    native.invert_rows([1.0, 2.0], [1.0])


# ---- 4. planner, bindings and CLI refusals, all before device work ---------------------------------------------------
def test_plan_invert():
  assert inference.plan_invert(None, None, 2, 96, 5.0) == ([1.0], 96)           # None means ONE here, not the model's weight
  assert inference.plan_invert(2.5, 24, 2, 96, 5.0) == ([2.5], 24)
  assert inference.plan_invert([1.0, 5.0], 12, 2, 96, 5.0) == ([1.0, 5.0], 12)
  assert inference.plan_invert(np.asarray([3, 4]), 1, 2, 96, 5.0) == ([3.0, 4.0], 1)
  assert inference.plan_invert(None, 24, 2, 96, 1.0) == ([1.0], 24)             # a weight-1 model inverts at weight 1
  assert inference.plan_invert([1.0, 1.0], 24, 2, 96, 1.0)[0] == [1.0, 1.0]
  for bad in (float('nan'), float('inf'), [1.0, 2.0, 3.0], [[1.0, 2.0]], True, 'loud'):
    with pytest.raises(ValueError, match='guidance'):
      inference.plan_invert(bad, 24, 2, 96, 5.0)
  for bad in (36, 0, -1, 2.5, True, 97):
    with pytest.raises(ValueError, match='1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 96'):
      inference.plan_invert(None, bad, 2, 96, 5.0)
  with pytest.raises(ValueError, match='weight 1'):
    inference.plan_invert(3.0, 24, 2, 96, 1.0)
  with pytest.raises(ValueError, match='weight 1'):
    inference.plan_invert([1.0, 3.0], 24, 2, 96, 1.0)


def _bare_model(cfg_weight=5.0, preset='tiny'):
  m = object.__new__(inference.InferenceModel)
  m.spec = msd_amd.config.preset(preset, num_steps=96, cfg_weight=cfg_weight)
  m.targets_length, m.audio_codec, m.rng = 64, msd_amd.audio_codecs.MelGAN(), 'philox'
  return m


def test_invert_refuses_before_any_device_work():
  """Every ValueError comes from invert's own checks: no handle is built (the object has none)."""
  m = _bare_model()
  toks, mel = np.zeros((2, 8), np.int32), np.zeros((2, 64, 128), np.float32)
  with pytest.raises(ValueError, match='decoder_target_tokens'):
    m.invert({'encoder_input_tokens': toks})
  for bad in (np.zeros((2, 64, 127), np.float32), np.zeros((1, 64, 128), np.float32), np.zeros((2, 64), np.float32)):
    with pytest.raises(ValueError, match='decoder_target_tokens must be'):
      m.invert({'encoder_input_tokens': toks, 'decoder_target_tokens': bad})
  batch = {'encoder_input_tokens': toks, 'decoder_target_tokens': mel}
  for kw, match in ((dict(guidance=float('nan')), 'finite'), (dict(guidance=[1.0, 2.0, 3.0]), 'one per row'),
                    (dict(steps=36), 'divisors'), (dict(steps=0), 'divisors')):
    with pytest.raises(ValueError, match=match):
      m.invert(batch, **kw)
  with pytest.raises(ValueError, match='weight 1'):
    _bare_model(cfg_weight=1.0).invert(batch, guidance=2.0)
  song = np.zeros((1, 128, 128), np.float32)
  segs = [np.zeros((8,), np.int32)] * 2
  with pytest.raises(ValueError, match='segments of tokens'):
    m.rerender(song, segs, segs[:1])
  with pytest.raises(ValueError, match='song must be'):
    m.rerender(song[0], segs, segs)
  with pytest.raises(ValueError, match='divisors'):
    m.rerender(song, segs, segs, steps=36)
  assert 'differs from predict' in inference.InferenceModel.invert.__doc__   # what guidance=None means is documented


class _Lib:
  """Stands in for the loaded library: records the entry point a NativeModel method calls, with its arguments."""

  def __init__(self):
    self.calls = []

  def __getattr__(self, name):
    if not name.startswith('msd_'):
      raise AttributeError(name)

    def entry(*args):
      self.calls.append((name, args))
      return 0
    return entry


def _stub_native(cfg_weight=5.0, num_steps=96):
  nm = object.__new__(native.NativeModel)
  nm.lib, nm.handle = _Lib(), 1
  nm.cfg = native.MsdConfig()
  nm.cfg.cfg_weight, nm.cfg.num_steps, nm.cfg.targets_length, nm.cfg.n_dims = cfg_weight, num_steps, 64, 128
  return nm


def test_native_invert_fills_the_args_and_refuses_before_the_library_is_called():
  mel, out = np.zeros((2, 64, 128), np.float32), np.zeros((2, 64, 128), np.float32)
  nm = _stub_native()
  nm.invert(2, out, mel, steps=24, guidance=[1.0, 2.5], stream=7)
  (name, (handle, ref, stream)), = nm.lib.calls
  a = ref._obj
  assert name == 'msd_invert' and stream == 7
  assert (a.struct_size, a.batch, a.num_steps, a.n_weights) == (native.ctypes.sizeof(native.InvertArgs), 2, 24, 2)
  assert [a.weights_host[0], a.weights_host[1]] == [1.0, 2.5] and a.mel_dev == mel.ctypes.data and a.out_dev == out.ctypes.data
  nm = _stub_native()
  nm.invert(2, out, mel)   # the defaults: the handle's steps, ONE weight of 1
  a = nm.lib.calls[0][1][1]._obj
  assert (a.num_steps, a.n_weights, a.weights_host[0]) == (0, 1, 1.0)
  for kw, match in ((dict(guidance=float('inf')), 'finite'), (dict(guidance=[1.0, 2.0, 3.0]), 'one per row'),
                    (dict(steps=36), 'divisors'), (dict(steps=True), 'divisors')):
    nm = _stub_native()
    with pytest.raises(ValueError, match=match):
      nm.invert(2, out, mel, **kw)
    assert nm.lib.calls == []
  for bad_mel, bad_out in ((mel[:1], out), (mel, out[:, :32]), (None, out)):
    nm = _stub_native()
    with pytest.raises(ValueError, match='must hold'):
      nm.invert(2, bad_out, bad_mel)
    assert nm.lib.calls == []


def test_header_and_binding_declare_the_new_entry_points():
  header = open(os.path.join(ROOT, 'include', 'msd_amd.h')).read()
  assert re.search(r'\bint\s+msd_invert\s*\(\s*msd_model\s*\*\s*m\s*,\s*const\s+msd_invert_args\s*\*', header)
  assert re.search(r'\bint\s+msd_op_invert_step\s*\(\s*const\s+msd_config\s*\*', header)
  assert {'msd_invert', 'msd_op_invert_step'} <= set(native.EXPORTED_SYMBOLS)
  assert callable(native.op_invert_step) and callable(native.NativeModel.invert)
  assert 'MSD_AMD_ABI_VERSION 7' in header   # appended: the version stays
  # the struct, field for field
  body = header[header.index('typedef struct msd_invert_args {'):header.index('} msd_invert_args;')]
  fields = re.findall(r'^\s*(?:const\s+)?(int32_t|float\s*\*)\s*(\w+);', body, flags=re.M)
  assert [n for _, n in fields] == [n for n, _ in native.InvertArgs._fields_]
  assert native.ctypes.sizeof(native.InvertArgs) == 40
  import msd_amd.build_native as bn
  assert 'sampler_invert_kernel' in bn.NO_SCRATCH_KERNELS and 'invert_tail.h' in bn.HEADERS


@pytest.fixture(scope='module')
def midis(tmp_path_factory):
  from msd_amd.frontend import midi_io
  from tests.test_frontend_midi import _random_song
  d = tmp_path_factory.mktemp('invert')
  paths = []
  for name, seed in (('new.mid', 9), ('old.mid', 9), ('long.mid', 10)):   # (seed 10 tokenises to one segment more)
    (d / name).write_bytes(midi_io.note_sequence_to_midi(_random_song(seed, seconds=3.0), ticks_per_quarter=500))
    paths.append(str(d / name))
  np.save(str(d / 'old.npy'), np.zeros((100, 128), np.float32))
  return paths[0], paths[1], str(d / 'old.npy'), paths[2]


def test_cli_rerender_refusals(midis, capsys):
  from msd_amd import synthesize
  new, old, mel, long = midis
  base = [new, '--preset', 'tiny_context', '--num-steps', '96', '--on-too-long', 'truncate', '--dry-run']
  assert synthesize.main([*base, '--rerender', old, '--edit-mel', mel, '--steps', '24', '--guidance', '2']) == 0
  assert 'rerender' in capsys.readouterr().out
  for extra, word in ((['--rerender', old, '--edit-mel', mel, '--regenerate', '0:1'], '--rerender does not go with'),
                      (['--rerender', old, '--edit-mel', mel, '--vary', '0.5'], '--rerender does not go with'),
                      (['--rerender', old, '--score', mel], '--rerender does not go with'),
                      (['--rerender', old], 'needs the old rendering'),
                      (['--rerender', long, '--edit-mel', mel], 'segment by segment'),
                      (['--rerender', old, '--edit-mel', mel, '--sampler', 'ddpm'], 'no --sampler'),
                      (['--rerender', old, '--edit-mel', mel, '--steps', '36'], 'divisors'),
                      (['--rerender', old, '--edit-mel', mel, '--guidance', 'nan'], 'finite'),
                      (['--rerender', old, '--edit-mel', mel, '--guidance', '2', '--cfg-weight', '1'], 'weight 1'),
                      (['--edit-mel', mel], '--rerender OLD.mid')):
    with pytest.raises(SystemExit) as e:
      synthesize.main([*base, *extra])
    assert e.value.code == 2 and word in capsys.readouterr().err, extra


# ---- 5. rerender's call sequence ---------------------------------------------------------------------------------------
def test_rerender_call_sequence():
  """Per segment k: invert(old tokens k, old mel k, context = OLD segment k - 1), then predict(new tokens k, context = NEW
  segment k - 1, init_z = that noise, sampler='ddim', steps=, guidance=render_guidance)."""
  m = _bare_model(preset='tiny_context')
  seen = []

  class T:
    float32 = np.float32

    @staticmethod
    def cat(xs, dim):
      return np.concatenate(xs, axis=dim)

    @staticmethod
    def zeros(shape, dtype=None, device=None):
      return _Arr(np.zeros(shape, np.float32))

  class _Arr(np.ndarray):
    def __new__(cls, a):
      return np.asarray(a).view(cls)

    def clone(self):
      return _Arr(np.array(self))

    def to(self, *_a, **_k):
      return self
  m._torch, m.device, m.targets_context_length = T, None, 64
  inference_to_device = inference._to_device
  song = np.arange(3 * 64 * 128, dtype=np.float32).reshape(1, 3 * 64, 128)
  old_toks = [np.full((8,), 10 + k, np.int32) for k in range(3)]
  new_toks = [np.full((8,), 20 + k, np.int32) for k in range(3)]

  def invert(batch, **kw):
    seen.append(('invert', batch, kw))
    return _Arr(np.full((1, 64, 128), 100.0 + len(seen), np.float32))

  def predict(batch, **kw):
    seen.append(('predict', batch, kw))
    return _Arr(np.full((1, 64, 128), -float(len(seen)), np.float32)), None
  m.invert, m.predict = invert, predict
  try:
    inference._to_device = lambda torch, x, dev, dtype: _Arr(np.asarray(x, np.float32))
    got = m.rerender(song, old_toks, new_toks, steps=24, guidance=2.0, render_guidance=3.0, return_torch=True)
    assert [s[0] for s in seen] == ['invert', 'predict'] * 3
    for k in range(3):
      (_, ib, ikw), (_, pb, pkw) = seen[2 * k], seen[2 * k + 1]
      assert ib['encoder_input_tokens'].tolist() == [old_toks[k].tolist()] and pb['encoder_input_tokens'].tolist() == [new_toks[k].tolist()]
      np.testing.assert_array_equal(ib['decoder_target_tokens'], song[:, k * 64:(k + 1) * 64])
      assert ikw == dict(steps=24, guidance=2.0, return_torch=True)
      assert set(pkw) == {'init_z', 'sampler', 'steps', 'return_torch', 'guidance'}
      assert (pkw['sampler'], pkw['steps'], pkw['guidance'], pkw['return_torch']) == ('ddim', 24, 3.0, True)
      np.testing.assert_array_equal(pkw['init_z'], np.full((1, 64, 128), 100.0 + 2 * k + 1, np.float32))   # THIS segment's noise
      mask = 0 if k == 0 else 1
      assert ib['encoder_continuous_mask'].tolist() == [[mask] * 64] and pb['encoder_continuous_mask'].tolist() == [[mask] * 64]
      if k:
        np.testing.assert_array_equal(ib['encoder_continuous_inputs'], song[:, (k - 1) * 64:k * 64])            # the OLD song
        np.testing.assert_array_equal(pb['encoder_continuous_inputs'], np.full((1, 64, 128), -2.0 * k, np.float32))   # the NEW one
      else:
        assert not np.asarray(ib['encoder_continuous_inputs']).any() and not np.asarray(pb['encoder_continuous_inputs']).any()
    np.testing.assert_array_equal(got, np.concatenate([np.full((1, 64, 128), -2.0 * (k + 1), np.float32) for k in range(3)], 1))
    # render_guidance=None: predict's own default (no keyword); always_mask_context: no segment sees a context
    seen.clear()
    m.rerender(song, old_toks, new_toks, always_mask_context=True, return_torch=True)
    assert all('guidance' not in s[2] or s[0] == 'invert' for s in seen)
    assert all(s[1]['encoder_continuous_mask'].tolist() == [[0] * 64] for s in seen)
    assert seen[0][2] == dict(steps=None, guidance=None, return_torch=True) and seen[1][2]['steps'] is None
  finally:
    inference._to_device = inference_to_device


# ---- the specification's own identities on the oracle's network -----------------------------------------------------
def test_spec_rows_are_their_one_row_specs_and_weights_matter():
  from oracle import fast
  spec = helpers.preset_spec('tiny', 12, 'ddim')
  params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
  cfg, dc = helpers.oracle_configs(spec)
  xp = backend.TorchBackend('float64')
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  mel = helpers.known_mel((2, 64, 128))
  fm = fast.FastModel(xp, cfg, dc, params, spec.has_context)
  both = inv.invert(fm, batch, mel, [1.0, 5.0])
  assert both.shape == (2, 64, 128) and np.isfinite(both).all()
  for b, w in enumerate([1.0, 5.0]):
    row = {k: np.ascontiguousarray(v[b:b + 1]) for k, v in batch.items()}
    np.testing.assert_array_equal(inv.invert(fm, row, mel[b:b + 1], [w]), both[b:b + 1])
  # a scalar weight is the config created with it (weights=None reads the config's)
  dc2 = gs.with_weight(dc, 2.0)
  fm2 = fast.FastModel(xp, cfg, dc2, params, spec.has_context)
  from tests import keep_spec
  keep_spec.encode(fm2, batch)
  x0 = fm2.codec.scale_features(xp, xp.asarray(mel), (-1., 1.), clip=True)
  own = np.asarray(xp.to_numpy(inv.scan(xp, x0, keep_spec.fast_pred_fn(fm2), dc2)), np.float64)
  np.testing.assert_array_equal(inv.invert(fm, batch, mel, [2.0, 2.0]), own)
  assert helpers.rms(own, inv.invert(fm, batch, mel, [1.0, 1.0])) > 1e-3
