"""Host-side tests of few-step rendering (no GPU): the specification tests/multistep_spec.py against the oracle, the
solver's order on a case with a closed form, plan_steps, the strided rows of the step tables, the ABI and the CLI."""
import os
import re

import numpy as np
import pytest

from oracle import backend, sampler as du
from tests import multistep_spec as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dc(steps, name='ddim', model_output='eps', cfg_weight=5.0, clip=True):
  return du.DiffusionConfig(
      model_output=model_output,
      classifier_free_guidance=du.ClassifierFreeGuidanceConfig(eval_condition_weight=cfg_weight),
      sampler=du.SamplerConfig(name=name, clip_x0=clip, schedule=du.DiffusionSchedule('cosine', num_steps=steps)))


# (a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('cfg_weight', [1.0, 5.0])
@pytest.mark.parametrize('model_output', ['eps', 'x0', 'v'])
def test_without_history_the_update_is_ddim_step(model_output, cfg_weight, clip):
  """History weight 0 (and the first step of a call, which has none): the spec's update equals the oracle's eval_step with
  sampler 'ddim' to 1e-12 in float64, at the top, a middle, the second-to-last and the last scan index."""
  steps = 40
  dc = _dc(steps, 'ddim', model_output, cfg_weight, clip)
  xp = backend.NumpyBackend('float64')
  rng = np.random.default_rng(8)
  shape = (2, 16, 128)
  for i in (steps - 1, steps // 2, 1, 0):
    z, oc, ou, prev = (rng.standard_normal(shape) for _ in range(4))
    if i > steps // 2 and model_output == 'eps':   # (at logsnr ~ -20 only eps ~ z leaves x0 inside [-1, 1])
      oc, ou = z + 1e-5 * oc, z + 1e-5 * ou
    pred = lambda z, time, include_conditioning: oc if include_conditioning else ou
    want = du.eval_step(xp, None, dc, 2, pred)(z, i)
    scale = max(1.0, float(np.abs(want).max()))
    for kw in (dict(first=False, history_weight=0.0), dict(first=True)):
      got, x0 = ms.step(xp, dc, z, i, pred, prev, **kw)
      assert np.abs(got - want).max() / scale <= 1e-12, (i, kw)
    if i == 0:
      np.testing.assert_array_equal(got, x0)
    # ... and with its own weight the history matters (but not at the last index, which returns x0)
    got2, _ = ms.step(xp, dc, z, i, pred, prev, first=False)
    assert (np.abs(got2 - want).max() > 1e-6) == (0 < i < steps - 1), i


# (b) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('steps', [20, 50, 100])
def test_second_order_on_the_closed_form(steps):
  """Per-element Gaussian data of variance 0.09 and the ideal denoiser: the probability-flow ODE has a closed-form end
  point.  2M's rms error is below a quarter of DDIM's (float64: ratios 7.1, 6.5, 6.3 at 20, 50, 100 steps; DDIM's errors
  3.1e-2, 1.3e-2, 6.5e-3).  1024 elements, clip off."""
  xp = backend.NumpyBackend('float64')
  dc = _dc(steps, 'ddim', 'eps', 1.0, False)
  z1 = np.random.default_rng(3).standard_normal((1, 8, 128))
  exact = ms.exact_end_point(z1)
  pred = ms.ideal_pred_fn(xp, dc)
  e_2m = np.sqrt(np.mean((ms.scan(xp, z1, pred, dc) - exact) ** 2))
  e_ddim = np.sqrt(np.mean((du.eval_scan(xp, z1, None, pred, dc) - exact) ** 2))
  print('K = %d: rms error 2M %.3e, DDIM %.3e, ratio %.2f' % (steps, e_2m, e_ddim, e_ddim / e_2m))
  assert e_2m < 0.25 * e_ddim
  # the spec's own first-order form is the oracle's DDIM scan
  e_1 = np.sqrt(np.mean((ms.scan(xp, z1, pred, dc, history_weight=0.0) - exact) ** 2))
  assert abs(e_1 - e_ddim) <= 1e-12


# (c) ------------------------------------------------------------------------------------------------------------------
def test_plan_steps_times_are_table_rows():
  """For every divisor K of 1000 and every j: float32(j + 1) / float32(K) has the bits of float32(r + 1) / float32(1000),
  r = row_offset + j * stride -- the K-step call's times are a subset of the 1000-step tables'."""
  from msd_amd import inference, native
  assert inference.plan_steps is native.plan_steps
  n = 1000
  divs = [k for k in range(1, n + 1) if n % k == 0]
  assert divs == native.divisors(n) and len(divs) == 16
  for k in divs:
    off, stride = native.plan_steps(n, k)
    assert (off, stride) == (n // k - 1, n // k)
    j = np.arange(k)
    r = off + j * stride
    np.testing.assert_array_equal(r, ms.strided_rows(n, k))
    assert r[-1] == n - 1
    t_k = (j.astype(np.float32) + np.float32(1.0)) / np.float32(k)
    t_n = (r.astype(np.float32) + np.float32(1.0)) / np.float32(n)
    assert t_k.dtype == np.float32 and t_n.dtype == np.float32
    np.testing.assert_array_equal(t_k.view(np.uint32), t_n.view(np.uint32))
  assert native.plan_steps(np.int64(96), np.int32(24)) == (3, 4)


@pytest.mark.parametrize('bad', [0, -1, -50, 3, 30, 999, 2000, True, False, 2.0, '50', None])
def test_plan_steps_refuses_what_does_not_divide(bad):
  from msd_amd import native
  with pytest.raises(ValueError) as e:
    native.plan_steps(1000, bad)
  assert '1, 2, 4, 5, 8, 10, 20, 25, 40, 50, 100, 125, 200, 250, 500, 1000' in str(e.value)
  for n in (0, -3, True, 2.5):
    with pytest.raises(ValueError):
      native.plan_steps(n, 1)


# (d) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_the_k_step_oracle_has_the_log_snrs_of_the_strided_rows(dtype):
  """The oracle configured with cosine num_steps = K: logsnr_t of scan index j is logsnr_t of row (j + 1) N / K - 1 of the
  N-step one, bit for bit (the same time); logsnr_s is NOT a row of the N-step table (s = j / K: the K-row table)."""
  xp = backend.NumpyBackend(dtype)
  n = 1000
  full = du.get_logsnr_t(xp, (xp.arange(n) + 1.0) / float(n), du.DiffusionSchedule('cosine', num_steps=n))
  for k in (1, 8, 20, 50, 250, 1000):
    sched = du.DiffusionSchedule('cosine', num_steps=k)
    lt = du.get_logsnr_t(xp, (xp.arange(k) + 1.0) / float(k), sched)
    np.testing.assert_array_equal(lt, full[ms.strided_rows(n, k)])
    for j in (0, k // 2, k - 1):
      got_t, got_s = ms.logsnrs(xp, _dc(k), 1, j)
      assert got_t[0] == lt[j]
      assert got_s[0] == (lt[j - 1] if j else du.get_logsnr_t(xp, xp.zeros((1,)), sched)[0])


# (e) ------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_entry_points():
  from msd_amd import native
  header = open(os.path.join(ROOT, 'include', 'msd_amd.h')).read()
  assert re.search(r'\bint\s+msd_sample_steps\s*\(\s*msd_model\s*\*', header)
  assert re.search(r'\bint\s+msd_op_sampler_step_multistep\s*\(', header)
  assert re.search(r'MSD_SAMPLER_DPMPP_2M\s*=\s*2\b', header)
  assert native.MSD_SAMPLER_DPMPP_2M == 2 and native.SAMPLERS == {'ddpm': 0, 'ddim': 1, 'dpmpp_2m': 2}
  assert {'msd_sample_steps', 'msd_op_sampler_step_multistep'} <= set(native.EXPORTED_SYMBOLS)
  assert callable(native.op_sampler_step_multistep)


def test_dpmpp_2m_is_a_configurable_default():
  """SamplerConfig.name = 'dpmpp_2m' becomes msd_config.sampler = 2; an unknown name is still the reference's error."""
  import dataclasses
  import msd_amd
  from msd_amd import inference
  spec = msd_amd.config.preset('tiny', num_steps=8)
  d = spec.diffusion
  for name, kind in (('ddpm', 0), ('ddim', 1), ('dpmpp_2m', 2)):
    s = dataclasses.replace(spec, diffusion=dataclasses.replace(d, sampler=dataclasses.replace(d.sampler, name=name)))
    assert inference._to_native_config(s, msd_amd.audio_codecs.MelGAN(), 1, 'f16x3').sampler == kind
  s = dataclasses.replace(spec, diffusion=dataclasses.replace(d, sampler=dataclasses.replace(d.sampler, name='euler')))
  with pytest.raises(ValueError, match='Unknown sampler type'):
    inference._to_native_config(s, msd_amd.audio_codecs.MelGAN(), 1, 'f16x3')


def test_predict_refuses_few_step_edits_before_any_device_work():
  """steps= / sampler= with keep= / strength=, a non-divisor and an unknown sampler are ValueErrors raised by predict's own
  checks: no handle is built (the object below has none)."""
  from msd_amd import inference
  import msd_amd
  m = object.__new__(inference.InferenceModel)
  m.spec = msd_amd.config.preset('tiny', num_steps=96)
  m.targets_length, m.audio_codec, m.rng = 64, msd_amd.audio_codecs.MelGAN(), 'philox'
  batch = {'encoder_input_tokens': np.zeros((1, 8), np.int32)}
  keep = np.zeros((1, 64, 128), np.float32)
  for kw in (dict(steps=24, keep=keep, keep_mask=np.zeros((1, 64), np.int32)), dict(sampler='ddim', keep=keep, strength=0.5),
             dict(steps=24, strength=0.5)):
    with pytest.raises(ValueError, match='cannot be combined'):
      m.predict(batch, **kw)
  with pytest.raises(ValueError, match='1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 96'):
    m.predict(batch, steps=36)
  with pytest.raises(ValueError, match='sampler must be one of'):
    m.predict(batch, sampler='euler')


# (f) ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def midi(tmp_path_factory):
  from msd_amd.frontend import midi_io
  from tests.test_frontend_midi import _random_song
  path = tmp_path_factory.mktemp('few') / 'a.mid'
  path.write_bytes(midi_io.note_sequence_to_midi(_random_song(9, seconds=3.0), ticks_per_quarter=500))
  return str(path)


def test_cli_parses_steps_and_sampler(midi, capsys):
  from msd_amd import synthesize
  base = ['--preset', 'tiny_context', '--on-too-long', 'truncate', '--dry-run']
  assert synthesize.main([midi, *base, '--steps', '50', '--sampler', 'dpmpp_2m']) == 0
  capsys.readouterr()
  with pytest.raises(SystemExit) as e:
    synthesize.main([midi, *base, '--steps', '30'])
  err = capsys.readouterr().err
  assert e.value.code == 2 and '--steps' in err and '1, 2, 4, 5, 8, 10, 20, 25, 40, 50, 100, 125, 200, 250, 500, 1000' in err
  with pytest.raises(SystemExit) as e:
    synthesize.main([midi, *base, '--sampler', 'euler'])
  assert e.value.code == 2
  capsys.readouterr()
  with pytest.raises(SystemExit) as e:
    synthesize.main([midi, *base, '--steps', '50', '--vary', '0.5', '--edit-mel', 'x.npy'])
  assert e.value.code == 2 and 'few-step edits' in capsys.readouterr().err


def test_cli_hands_steps_and_sampler_to_predict_sequence(midi, tmp_path, monkeypatch):
  import msd_amd
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
  assert synthesize.main(args + ['--steps', '24', '--sampler', 'dpmpp_2m']) == 0
  assert seen['steps'] == 24 and seen['sampler'] == 'dpmpp_2m'
  seen.clear()
  assert synthesize.main(args) == 0
  assert 'steps' not in seen and 'sampler' not in seen
