"""Per-call guidance on the host (no GPU): plan_guidance, plan_call's combinations and refusals, the routing of "the call
as it was", the CLI, and the identities of the specification (tests/guidance_spec.py) in float64 on `tiny`."""
import dataclasses
import os
import re

import numpy as np
import pytest

import msd_amd
from msd_amd import inference, native
from oracle import backend, fast
from tests import guidance_spec as gs, helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- plan_guidance ---------------------------------------------------------------------------------------------------
def test_plan_guidance_values_and_rounding():
  w, lo, hi = inference.plan_guidance(2.0, None, 3, 24, 5.0)
  assert w.dtype == np.float32 and w.tolist() == [2.0, 2.0, 2.0] and (lo, hi) == (0, 24)
  w, lo, hi = inference.plan_guidance([1.0, 5.0, 0.0], (0.25, 0.75), 3, 24, 5.0)
  assert w.tolist() == [1.0, 5.0, 0.0] and (lo, hi) == (6, 18)
  # an interval alone: the model's weight
  w, lo, hi = inference.plan_guidance(None, (0.0, 0.5), 2, 24, 5.0)
  assert w.tolist() == [5.0, 5.0] and (lo, hi) == (0, 12)
  # floor(x K + 0.5), plan_strength's rounding: 0.3 * 12 = 3.6 -> 4, 0.54 * 12 = 6.48 -> 6, 0.125 * 12 = 1.5 -> 2
  assert inference.plan_guidance(2.0, (0.3, 0.54), 1, 12, 5.0)[1:] == (4, 6)
  assert inference.plan_guidance(2.0, (0.125, 1.0), 1, 12, 5.0)[1:] == (2, 12)
  for s in (0.0, 0.2, 0.37, 0.5, 0.99, 1.0):
    assert inference.plan_guidance(2.0, (0.0, 1.0) if s == 0.0 else (0.0, s), 1, 24, 5.0)[2] == \
        (24 if s == 0.0 else inference.plan_strength([[s]], 24)[1] + 1)
  # NumPy and integer weights
  assert inference.plan_guidance(np.float32(2.5), None, 1, 8, 5.0)[0].tolist() == [2.5]
  assert inference.plan_guidance(np.asarray([3, 4]), None, 2, 8, 5.0)[0].tolist() == [3.0, 4.0]


def test_plan_guidance_the_call_as_it_was():
  """None or the model's own weight as a SCALAR, over the whole scan, plans no guidance at all."""
  for g in (None, 5.0, 5, np.float32(5.0)):
    for iv in (None, (0, 1), (0.0, 1.0), (0.01, 0.99)):   # (24 steps: both round to the ends)
      assert inference.plan_guidance(g, iv, 2, 24, 5.0)[0] is None, (g, iv)
  # ... but not as a sequence, not another weight, not a narrower interval
  assert inference.plan_guidance([5.0, 5.0], None, 2, 24, 5.0)[0] is not None
  assert inference.plan_guidance(5.0 + 1e-6, None, 2, 24, 5.0)[0] is not None
  assert inference.plan_guidance(5.0, (0.0, 0.9), 2, 24, 5.0)[0] is not None
  assert inference.plan_guidance(None, (0.1, 1.0), 2, 24, 5.0)[0] is not None


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), -float('inf'), 1e39, 'loud', True, [1.0], [1.0, 2.0, 3.0],
                                 [[1.0, 2.0]], [1.0, float('nan')], object()])
def test_plan_guidance_refuses_weights(bad):
  with pytest.raises(ValueError, match='guidance'):
    inference.plan_guidance(bad, None, 2, 24, 5.0)


@pytest.mark.parametrize('bad', [(0.5, 0.5), (0.6, 0.4), (-0.1, 0.5), (0.0, 1.1), (float('nan'), 1.0), (0.0,), (0.0, 0.5, 1.0),
                                 0.5, 'a:b', (0.50, 0.51), (0.0, 0.01)])
def test_plan_guidance_refuses_intervals(bad):
  """out of order, outside [0, 1], NaN, not a pair -- and a pair that rounds to no step of the 24."""
  with pytest.raises(ValueError, match='guidance_interval'):
    inference.plan_guidance(2.0, bad, 2, 24, 5.0)


def test_plan_guidance_refuses_step_counts():
  for k in (0, -1, 2.5, True):
    with pytest.raises(ValueError, match='num_steps'):
      inference.plan_guidance(2.0, None, 1, k, 5.0)


# ---- plan_call ---------------------------------------------------------------------------------------------------------
def _plan(**kw):
  args = dict(keep=None, keep_mask=None, strength=None, steps=None, sampler=None, b=2, t=64, n=128, num_steps=96, model_weight=5.0)
  args.update(kw)
  return inference.plan_call(**args)


def test_plan_call_combinations():
  c = _plan(guidance=2.0)
  assert c == inference.SampleCall(guidance=2.0, guide_range=(0, 96))
  c = _plan(guidance=[1.0, 5.0], guidance_interval=(0.25, 0.75), steps=24, sampler='dpmpp_2m')
  assert c == inference.SampleCall(steps=24, sampler='dpmpp_2m', guidance=[1.0, 5.0], guide_range=(6, 18))
  # equal weights travel as ONE weight (no per-row requirement on the shape of a row)
  assert _plan(guidance=[2.0, 2.0]).guidance == 2.0
  # an interval alone: the model's weight inside it
  assert _plan(guidance_interval=(0.0, 0.5), steps=12) == inference.SampleCall(steps=12, guidance=5.0, guide_range=(0, 6))
  # the interval is planned on the CALL's step count
  assert _plan(guidance=2.0, guidance_interval=(0.25, 0.5), steps=8).guide_range == (2, 4)


def test_plan_call_the_call_as_it_was():
  plain = _plan()
  assert plain == inference.SampleCall() and plain.guidance is None and plain.guide_range is None
  for kw in (dict(guidance=5.0), dict(guidance_interval=(0, 1)), dict(guidance=5.0, guidance_interval=(0.0, 1.0))):
    assert _plan(**kw) == plain, kw
    assert _plan(steps=24, sampler='ddim', **kw) == inference.SampleCall(steps=24, sampler='ddim'), kw


def test_plan_call_refusals():
  keep, mask = np.zeros((2, 64, 128), np.float32), np.zeros((2, 64), np.int32)
  for kw in (dict(keep=keep, keep_mask=mask), dict(keep=keep, strength=0.5), dict(keep=keep, keep_mask=mask, resample=(4, 2)),
             dict(strength=0.5), dict(keep_mask=mask)):
    for g in (dict(guidance=2.0), dict(guidance_interval=(0.0, 0.5)), dict(guidance=5.0)):
      with pytest.raises(ValueError, match='guidance.*cannot be combined'):
        _plan(**kw, **g)
  # ... and the refusals of the other forms stay what they were
  with pytest.raises(ValueError, match='few-step edits are not built'):
    _plan(keep=keep, keep_mask=mask, steps=24)
  with pytest.raises(ValueError, match='resample= needs keep'):
    _plan(resample=(4, 2))
  with pytest.raises(ValueError, match='1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 96'):
    _plan(guidance=2.0, steps=36)
  with pytest.raises(ValueError, match='sampler must be one of'):
    _plan(guidance=2.0, sampler='euler')
  with pytest.raises(ValueError, match='weight 1'):
    _plan(guidance=3.0, model_weight=1.0)
  with pytest.raises(ValueError, match='model_weight'):
    _plan(guidance=3.0, model_weight=None)


def test_predict_refuses_before_any_device_work():
  """Every ValueError of the new arguments comes from predict's own checks: no handle is built (the object has none)."""
  m = object.__new__(inference.InferenceModel)
  m.spec = msd_amd.config.preset('tiny', num_steps=96)
  m.targets_length, m.audio_codec, m.rng = 64, msd_amd.audio_codecs.MelGAN(), 'philox'
  batch = {'encoder_input_tokens': np.zeros((2, 8), np.int32)}
  keep = np.zeros((2, 64, 128), np.float32)
  for kw, match in ((dict(guidance=float('nan')), 'finite'), (dict(guidance=[1.0, 2.0, 3.0]), 'one per row'),
                    (dict(guidance=2.0, guidance_interval=(0.5, 0.25)), 'guidance_interval'),
                    (dict(guidance=2.0, guidance_interval=(0.5, 0.5)), 'guidance_interval'),
                    (dict(guidance=2.0, keep=keep, keep_mask=np.zeros((2, 64), np.int32)), 'cannot be combined'),
                    (dict(guidance_interval=(0.0, 0.5), keep=keep, strength=0.5), 'cannot be combined'),
                    (dict(guidance=2.0, keep=keep, keep_mask=np.zeros((2, 64), np.int32), resample=(4, 2)), 'cannot be combined')):
    with pytest.raises(ValueError, match=match):
      m.predict(batch, **kw)
  with pytest.raises(ValueError, match='one guidance weight'):
    m.predict_sequence([np.zeros((8,), np.int32)], guidance=[1.0, 2.0])
  m.spec = msd_amd.config.preset('tiny', num_steps=96, cfg_weight=1.0)
  with pytest.raises(ValueError, match='weight 1'):
    m.predict(batch, guidance=3.0)


# ---- routing: which entry point a call reaches -------------------------------------------------------------------------
class _Lib:
  """Stands in for the loaded library: records the entry point NativeModel.sample calls, with its arguments."""

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
  nm.cfg.cfg_weight, nm.cfg.num_steps, nm.cfg.targets_length = cfg_weight, num_steps, 64
  return nm


def test_the_call_as_it_was_reaches_the_entry_points_it_always_reached():
  """plan_call's plan of None / the model's weight / the whole interval holds no guidance, so NativeModel.sample gets the
  keywords it got before and calls msd_sample / msd_sample_rng / msd_sample_rows / msd_sample_steps."""
  for kw in (dict(), dict(guidance=5.0), dict(guidance_interval=(0, 1)), dict(guidance=5.0, guidance_interval=(0.0, 1.0))):
    call = _plan(**kw)
    for keys, rng, want in ((dict(seed=3, stream_id=1), 'philox', 'msd_sample'), (dict(seed=3, stream_id=1), 'threefry', 'msd_sample_rng'),
                            (dict(seed=[3, 4], stream_id=1), 'philox', 'msd_sample_rows')):
      nm = _stub_native()
      nm.sample(2, None, rng=rng, **keys, **vars(call))
      assert [c[0] for c in nm.lib.calls] == [want], (kw, keys, rng)
    nm = _stub_native()
    nm.sample(2, None, **vars(_plan(steps=24, **kw)))
    assert [c[0] for c in nm.lib.calls] == ['msd_sample_steps']


def test_a_guided_call_reaches_msd_sample_guided():
  nm = _stub_native()
  nm.sample(2, None, seed=[3, 4], stream_id=7, rng='threefry', **vars(_plan(guidance=[1.0, 2.5], guidance_interval=(0.25, 0.75), steps=24,
                                                                            sampler='dpmpp_2m')))
  (name, a), = nm.lib.calls
  assert name == 'msd_sample_guided'
  # (m, batch, rng, per_row, seeds, stream_ids, init_z, noise, num_steps, sampler, weights, n_weights, lo, hi, out, stream)
  assert a[1:4] == (2, native.RNGS['threefry'], 1) and list(a[4]) == [3, 4] and list(a[5]) == [7, 7]
  assert a[8:10] == (24, native.SAMPLERS['dpmpp_2m']) and list(a[10]) == [1.0, 2.5] and a[11:14] == (2, 6, 18)
  nm = _stub_native()
  nm.sample(1, None, guidance=2.0)   # a scalar, the whole scan: ONE weight, range 0, 0, the handle's steps and sampler
  (name, a), = nm.lib.calls
  assert name == 'msd_sample_guided' and a[3] == 0 and a[8:10] == (0, -1) and list(a[10]) == [2.0] and a[11:14] == (1, 0, 0)
  nm = _stub_native()
  nm.sample(1, None, guide_range=(2, 5))   # a range alone: the handle's weight
  assert list(nm.lib.calls[0][1][10]) == [5.0] and nm.lib.calls[0][1][12:14] == (2, 5)


def test_native_sample_refuses_before_the_library_is_called():
  keep = object()
  for kw, match in ((dict(guidance=float('inf')), 'finite'), (dict(guidance=[1.0, 2.0, 3.0]), 'one per row'),
                    (dict(guidance=2.0, guide_range=(5, 5)), 'guide_range'), (dict(guidance=2.0, guide_range=(0, 97)), 'guide_range'),
                    (dict(guidance=2.0, guide_range=(-1, 4)), 'g_lo'), (dict(guidance=2.0, guide_range=(0.0, 4)), 'g_lo'),
                    (dict(guidance=2.0, steps=24, guide_range=(0, 25)), 'guide_range'),
                    (dict(guidance=2.0, keep=keep, keep_mask=np.zeros((2, 64), np.int32)), 'cannot be combined'),
                    (dict(guide_range=(0, 4), keep=keep, release=np.zeros((2, 64), np.int32), start_step=3), 'cannot be combined'),
                    (dict(guidance=2.0, keep=keep, keep_mask=np.zeros((2, 64), np.int32), resample=(4, 2)), 'cannot be combined')):
    nm = _stub_native()
    with pytest.raises(ValueError, match=match):
      nm.sample(2, None, **kw)
    assert nm.lib.calls == []


def test_header_and_binding_declare_the_new_entry_points():
  header = open(os.path.join(ROOT, 'include', 'msd_amd.h')).read()
  assert re.search(r'\bint\s+msd_sample_guided\s*\(\s*msd_model\s*\*', header)
  assert re.search(r'\bint\s+msd_op_sampler_step_guided\s*\(\s*const\s+msd_config\s*\*', header)
  assert re.search(r'\bint\s+msd_op_sampler_step_multistep_guided\s*\(\s*const\s+msd_config\s*\*', header)
  assert {'msd_sample_guided', 'msd_op_sampler_step_guided', 'msd_op_sampler_step_multistep_guided'} <= set(native.EXPORTED_SYMBOLS)
  assert callable(native.op_sampler_step_guided) and callable(native.op_sampler_step_multistep_guided)
  assert 'MSD_AMD_ABI_VERSION 7' in header   # appended: the version stays


# ---- the CLI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def midi(tmp_path_factory):
  from msd_amd.frontend import midi_io
  from tests.test_frontend_midi import _random_song
  path = tmp_path_factory.mktemp('guidance') / 'a.mid'
  path.write_bytes(midi_io.note_sequence_to_midi(_random_song(9, seconds=3.0), ticks_per_quarter=500))
  return str(path)


def test_cli_parses_guidance(midi, capsys):
  from msd_amd import synthesize
  base = ['--preset', 'tiny_context', '--on-too-long', 'truncate', '--dry-run']
  assert synthesize.main([midi, *base, '--guidance', '2.5', '--guidance-interval', '0.2:0.8', '--steps', '50']) == 0
  capsys.readouterr()
  for extra, word in ((['--guidance-interval', '0.8:0.2'], '0 <= LO < HI <= 1'), (['--guidance-interval', '0.5'], 'LO:HI'),
                      (['--guidance-interval', '0:1.5'], '0 <= LO < HI <= 1'), (['--guidance', 'nan'], 'finite'),
                      (['--guidance-interval', '0.5:0.5004'], 'none of the call'),
                      (['--guidance', '2', '--cfg-weight', '1'], 'one pass'),
                      (['--guidance', '2', '--vary', '0.5', '--edit-mel', 'x.npy'], 'guided edits are not built'),
                      (['--guidance-interval', '0:0.5', '--regenerate', '0:1', '--edit-mel', 'x.npy'], 'guided edits are not built')):
    with pytest.raises(SystemExit) as e:
      synthesize.main([midi, *base, *extra])
    assert e.value.code == 2 and word in capsys.readouterr().err, extra


def test_cli_hands_guidance_to_predict_sequence(midi, tmp_path, monkeypatch):
  from msd_amd import synthesize
  seen = {}

  class Model:
    def __init__(self, *a, **k):
      self.targets_context_length = 64

    def check_batch_segments(self, *a):
      pass

    def predict_sequence(self, segments, **kw):
      import torch
      seen.update(kw)
      return torch.zeros((1, 64 * len(segments), 128)), {'prediction_seconds_per_chunk': 1.0,
                                                         'predictions_seconds_per_audio_second': 1.0}
  monkeypatch.setattr(msd_amd, 'InferenceModel', Model)
  args = [midi, '--preset', 'tiny_context', '--num-steps', '96', '--on-too-long', 'truncate', '--out', str(tmp_path / 'o.npy')]
  assert synthesize.main(args + ['--guidance', '2.5', '--guidance-interval', '0.25:0.75']) == 0
  assert seen['guidance'] == 2.5 and seen['guidance_interval'] == (0.25, 0.75)
  seen.clear()
  assert synthesize.main(args + ['--guidance-interval', '0:0.5', '--steps', '24']) == 0
  assert 'guidance' not in seen and seen['guidance_interval'] == (0.0, 0.5) and seen['steps'] == 24
  seen.clear()
  assert synthesize.main(args) == 0
  assert 'guidance' not in seen and 'guidance_interval' not in seen


def test_predict_sequence_passes_guidance_to_every_segment():
  """The hand-off loop and the batch_segments path give predict the song's one weight and its interval."""
  m = object.__new__(inference.InferenceModel)
  seen = []

  class T:
    @staticmethod
    def cat(xs, dim):
      return np.concatenate(xs, axis=dim)
  m._torch, m.device = T, None
  m.audio_codec, m.targets_context_length, m.batch_size = msd_amd.audio_codecs.MelGAN(), None, 2
  m._segment_batch = lambda toks, pred, no_ctx: {'encoder_input_tokens': np.asarray(toks).reshape(1, -1)}

  def predict(batch, **kw):
    seen.append(kw)
    return np.zeros((np.shape(batch['encoder_input_tokens'])[0], 64, 128), np.float32), None
  m.predict = predict
  segs = [np.zeros((8,), np.int32)] * 3
  m.predict_sequence(segs, guidance=2.0, guidance_interval=(0.2, 0.8), return_torch=True)
  assert len(seen) == 3 and all(kw['guidance'] == 2.0 and kw['guidance_interval'] == (0.2, 0.8) for kw in seen)
  seen.clear()
  m.predict_sequence(segs, guidance=2.0, batch_segments=2, return_torch=True)
  assert len(seen) == 2 and all(kw['guidance'] == 2.0 and 'guidance_interval' not in kw for kw in seen)
  seen.clear()
  m.predict_sequence(segs, return_torch=True)
  assert all('guidance' not in kw for kw in seen)


# ---- the specification's identities, float64, tiny ------------------------------------------------------------------------
STEPS = 12


@pytest.fixture(scope='module')
def tiny():
  spec = helpers.preset_spec('tiny', STEPS)
  params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
  cfg, dc = helpers.oracle_configs(spec)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  init_z, noise = helpers.make_noise(spec, batch=2)
  xp = backend.TorchBackend('float64')
  return spec, params, cfg, dc, batch, init_z, noise, xp


def _oracle(tiny, w, sampler='ddpm'):
  spec, params, cfg, dc, batch, init_z, noise, xp = tiny
  dc = dataclasses.replace(gs.with_weight(dc, w), sampler=dataclasses.replace(dc.sampler, name=sampler))
  fm = fast.FastModel(xp, cfg, dc, params, spec.has_context)
  return np.asarray(xp.to_numpy(fm.predict(batch, init_z, noise)[0]), np.float64)


def _spec(tiny, weights, lo, hi, sampler=None, rows=slice(None)):
  spec, params, cfg, dc, batch, init_z, noise, xp = tiny
  if sampler in ('ddim', 'dpmpp_2m'):
    dc = dataclasses.replace(dc, sampler=dataclasses.replace(dc.sampler, name='ddim'))
  fm = fast.FastModel(xp, cfg, dc, params, spec.has_context)
  batch = {k: np.ascontiguousarray(v[rows]) for k, v in batch.items()}
  return gs.predict(fm, batch, init_z[rows], noise[:, rows], weights, lo, hi, 'dpmpp_2m' if sampler == 'dpmpp_2m' else None)


@pytest.mark.parametrize('sampler', ['ddpm', 'ddim'])
def test_spec_full_interval_is_the_oracle_configured_with_w(tiny, sampler):
  for w in (5.0, 2.0):
    np.testing.assert_array_equal(_spec(tiny, [w, w], 0, STEPS, sampler), _oracle(tiny, w, sampler))


def test_spec_empty_guidance_is_the_weight_1_oracle(tiny):
  want = _oracle(tiny, 1.0)
  np.testing.assert_array_equal(_spec(tiny, [5.0, 3.0], 0, 0), want)
  np.testing.assert_array_equal(_spec(tiny, [5.0, 3.0], STEPS, STEPS), want)
  np.testing.assert_array_equal(_spec(tiny, [1.0, 1.0], 0, STEPS), want)   # weight 1 inside the interval: the == 1 branch
  assert helpers.rms(want, _oracle(tiny, 5.0)) > 1e-3


def test_spec_2m_full_interval_is_the_multistep_spec(tiny):
  from tests import multistep_spec as ms
  spec, params, cfg, dc, batch, init_z, noise, xp = tiny
  dc = dataclasses.replace(gs.with_weight(dc, 2.0), sampler=dataclasses.replace(dc.sampler, name='ddim'))
  want = ms.predict(fast.FastModel(xp, cfg, dc, params, spec.has_context), batch, init_z)
  np.testing.assert_array_equal(_spec(tiny, [2.0, 2.0], 0, STEPS, 'dpmpp_2m'), want)


@pytest.mark.parametrize('sampler', ['ddpm', 'dpmpp_2m'])
def test_spec_rows_are_their_one_row_specs(tiny, sampler):
  """Row b of a mixed-weight spec is its one-row spec, weight 1 among them, with and without an interval."""
  for weights, lo, hi in (([1.0, 5.0], 0, STEPS), ([2.5, 0.0], 3, 7)):
    both = _spec(tiny, weights, lo, hi, sampler)
    for b in range(2):
      one = _spec(tiny, weights[b:b + 1], lo, hi, sampler, rows=slice(b, b + 1))
      np.testing.assert_array_equal(both[b:b + 1], one)
  assert helpers.rms(_spec(tiny, [2.5, 0.0], 3, 7, sampler), _spec(tiny, [2.5, 0.0], 0, STEPS, sampler)) > 1e-3
