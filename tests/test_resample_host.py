"""Resampling jumps in the known-frame scan (RePaint), the parts that need no device: plan_resample, the jump's coefficients,
the specification (tests/resample_spec.py) against tests/edit_spec.py, the keys of a call's draws, predict's refusals on a
model without a handle, the ABI surface and the command line."""
import dataclasses
import os
import re

import numpy as np
import pytest

import msd_amd
from msd_amd import inference, native
from oracle import backend
from oracle import sampler as du
from tests import edit_spec, helpers, resample_spec
from tests.test_host_logic import _bare_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------------
# the schedule
# --------------------------------------------------------------------------------------------------
def _steps(ops):
  return sum(o[1] - o[2] for o in ops if o[0] == 'steps')


def _jumps(ops):
  return [o for o in ops if o[0] == 'jump']


def test_plan_resample_is_the_binding_s_function():
  assert inference.plan_resample is native.plan_resample


def test_plan_resample_20_steps_jump_8_times_2():
  """S = 20: blocks 8 / 8 / 4, each descended twice: 40 steps and 3 jumps."""
  ops = inference.plan_resample(19, 8, 2)
  assert ops == [('steps', 20, 12), ('jump', 12, 20, 1), ('steps', 20, 12),
                 ('steps', 12, 4), ('jump', 4, 12, 2), ('steps', 12, 4),
                 ('steps', 4, 0), ('jump', 0, 4, 3), ('steps', 4, 0)]
  assert _steps(ops) == 40 and len(_jumps(ops)) == 3


def test_plan_resample_16_steps_jump_4_times_3():
  ops = inference.plan_resample(15, 4, 3)
  want = []
  for k, (top, bottom) in enumerate([(16, 12), (12, 8), (8, 4), (4, 0)]):
    want += [('steps', top, bottom), ('jump', bottom, top, 2 * k + 1), ('steps', top, bottom), ('jump', bottom, top, 2 * k + 2),
             ('steps', top, bottom)]
  assert ops == want
  assert _steps(ops) == 48 and len(_jumps(ops)) == 8


def test_plan_resample_one_short_block():
  """S = 5 below the jump length: one block of five steps."""
  assert inference.plan_resample(4, 8, 2) == [('steps', 5, 0), ('jump', 0, 5, 1), ('steps', 5, 0)]
  assert inference.plan_resample(4, 8, 4)[-2:] == [('jump', 0, 5, 3), ('steps', 5, 0)]
  assert inference.plan_resample(-1, 8, 2) == []   # nothing to sample
  # a jump far beyond the call's steps (the largest C int: "one block") is one block as well
  assert inference.plan_resample(19, 2 ** 31 - 1, 2) == [('steps', 20, 0), ('jump', 0, 20, 1), ('steps', 20, 0)]
  assert resample_spec.n_passes(19, 2 ** 31 - 1, 3) == 3


@pytest.mark.parametrize('s,jump,times', [(20, 8, 2), (16, 4, 3), (5, 8, 2), (1000, 10, 10), (11, 8, 2), (7, 1, 2), (16, 16, 3)])
def test_plan_resample_counts_and_the_spec_s_own_plan(s, jump, times):
  ops = inference.plan_resample(s - 1, jump, times)
  assert _steps(ops) == times * s
  assert len(_jumps(ops)) == (times - 1) * -(-s // jump)
  assert [o[3] for o in _jumps(ops)] == list(range(1, len(_jumps(ops)) + 1))
  assert ops == resample_spec.plan(s - 1, jump, times)
  assert resample_spec.n_passes(s - 1, jump, times) == 1 + len(_jumps(ops))
  # every jump goes from where the steps before it ended back to where they began; the last step ends at level 0
  for a, b in zip(ops, ops[1:]):
    if b[0] == 'jump':
      assert a[0] == 'steps' and (b[1], b[2]) == (a[2], a[1])
    else:
      assert b[1] == (a[2] if a[0] == 'jump' else a[2])
  assert ops[-1][0] == 'steps' and ops[-1][2] == 0 and ops[0][1] == s


@pytest.mark.parametrize('jump', [1, 3, 8, 50])
def test_times_one_is_the_plain_descent(jump):
  for s in (1, 5, 16, 20):
    ops = inference.plan_resample(s - 1, jump, 1)
    assert not _jumps(ops) and _steps(ops) == s
    levels = [lv for o in ops for lv in range(o[1], o[2], -1)]
    assert levels == list(range(s, 0, -1))


@pytest.mark.parametrize('bad', [(15, 0, 2), (15, 8, 0), (15, -1, 2), (15, 8, -3), (15, 2.0, 2), (15, 8, 1.5), (15, True, 2),
                                 (15, 8, True), (15, '8', 2), (15, None, 2), (-2, 8, 2), (1.0, 8, 2)])
def test_plan_resample_refuses(bad):
  with pytest.raises(ValueError):
    inference.plan_resample(*bad)


def test_check_resample():
  assert native.check_resample((8, 2)) == (8, 2) and native.check_resample([np.int64(4), 3]) == (4, 3)
  assert native.check_resample((2 ** 31 - 1, 2 ** 31 - 1)) == (2 ** 31 - 1, 2 ** 31 - 1)   # (the entry point's ints)
  for bad in (8, (8,), (8, 2, 1), (0, 2), (8, 0), (8.0, 2), 'ab', None, (2 ** 31, 2), (8, 2 ** 31)):
    with pytest.raises(ValueError):
      native.check_resample(bad)


# --------------------------------------------------------------------------------------------------
# the jump maps q(z_s | x0) onto q(z_t | x0)
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('schedule', [du.DiffusionSchedule('cosine', num_steps=16),
                                      du.DiffusionSchedule('linear', start=1e-4, stop=2e-2, num_steps=16)], ids=['cosine', 'linear'])
def test_jump_coefficients_compose_the_forward_process(schedule):
  """Every pair of levels s < t, float64: a alpha_s = alpha_t and a^2 sigma_s^2 + b^2 = sigma_t^2 within 1e-12."""
  xp = backend.NumpyBackend('float64')
  n = schedule.num_steps

  def sigma2(level):
    t = (xp.full((1,), 0.0) + float(level)) / float(n)
    return float(xp.sigmoid(-du.get_logsnr_t(xp, t, schedule))[0])

  pairs = 0
  for s in range(n):
    for t in range(s + 1, n + 1):
      a, b = (float(v[0]) for v in resample_spec.jump_coefs(xp, schedule, 1, s, t))
      alpha_s = float(resample_spec.level_alpha(xp, schedule, 1, s)[0])
      alpha_t = float(resample_spec.level_alpha(xp, schedule, 1, t)[0])
      assert 0.0 < a < 1.0 and 0.0 < b <= 1.0
      assert abs(a * alpha_s - alpha_t) <= 1e-12
      assert abs(a * a * sigma2(s) + b * b - sigma2(t)) <= 1e-12
      assert abs(alpha_t * alpha_t + sigma2(t) - 1.0) <= 1e-12
      pairs += 1
  assert pairs == n * (n + 1) // 2


def test_jump_state_is_the_line_of_the_issue():
  xp = backend.NumpyBackend('float64')
  dc = helpers.oracle_configs(msd_amd.config.preset('tiny', num_steps=16))[1]
  rng = np.random.default_rng(2)
  z, eps = rng.standard_normal((2, 4, 8)), rng.standard_normal((2, 4, 8))
  a, b = (float(v[0]) for v in resample_spec.jump_coefs(xp, dc.sampler.schedule, 2, 4, 12))
  np.testing.assert_array_equal(resample_spec.jump_state(xp, dc, z, eps, 4, 12), b * eps + a * z)


# --------------------------------------------------------------------------------------------------
# the specification
# --------------------------------------------------------------------------------------------------
def _fast(sampler, steps=4):
  from oracle import fast
  spec = msd_amd.config.preset('tiny_context', num_steps=steps)
  d = spec.diffusion
  spec = dataclasses.replace(spec, diffusion=dataclasses.replace(d, sampler=dataclasses.replace(d.sampler, name=sampler)))
  params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
  cfg, dc = helpers.oracle_configs(spec)
  return spec, fast.FastModel(backend.NumpyBackend('float64'), cfg, dc, params, True)


@pytest.fixture(scope='module', params=['ddpm', 'ddim'])
def spec_run(request):
  """One float64 model of four steps per sampler: (fm, batch, init_z, noise, known mel)."""
  spec, fm = _fast(request.param)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  init_z, noise = helpers.make_noise(spec, batch=2)
  if request.param == 'ddim':
    noise = None
  return fm, batch, init_z, noise, helpers.known_mel((2, 64, 128))


def _strengths():
  s = np.full((2, 64), 1.0)
  s[0, :20] = 0.0
  s[1, 30:50] = 0.5
  return s


def test_spec_with_times_one_is_the_edit_spec(spec_run):
  fm, batch, init_z, noise, known = spec_run
  for strength in (_strengths(), np.minimum(_strengths(), 0.5)):   # the full scan, and a part-way start
    words, start = inference.plan_strength(strength, 4)
    want = edit_spec.predict_edit(fm, batch, init_z, noise, known, words, start)
    for jump in (1, 3, 8):
      got = resample_spec.predict_resample(fm, batch, init_z, [noise], [None], known, words, start, jump, 1)
      for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_spec_jumps_change_the_free_frames_and_keep_the_known_ones(spec_run):
  fm, batch, init_z, noise, known = spec_run
  words, start = inference.plan_strength(_strengths(), 4)
  rng = np.random.default_rng(13)
  passes = resample_spec.n_passes(start, 2, 2)
  assert passes == 3
  eps = [None] + [rng.standard_normal((2, 64, 128)) for _ in range(passes - 1)]
  nz = [noise] + [None if noise is None else rng.standard_normal(noise.shape) for _ in range(passes - 1)]
  plain = edit_spec.predict_edit(fm, batch, init_z, noise, known, words, start)[0]
  got, x0, xk = resample_spec.predict_resample(fm, batch, init_z, nz, eps, known, words, start, 2, 2)
  assert np.isfinite(got).all()
  np.testing.assert_array_equal(got[0, :20], known[0, :20].astype(np.float64))   # word 1: the caller's values
  np.testing.assert_array_equal(x0[0, :20], xk[0, :20])                          # ... and in model units the scan arrives at xk
  assert np.abs(got[0, 20:] - plain[0, 20:]).max() > 1e-2                        # the jumps happened


# --------------------------------------------------------------------------------------------------
# the keys of the draws
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rng', ['philox', 'threefry'])
@pytest.mark.parametrize('start,jump,times', [(19, 8, 2), (15, 4, 3), (10, 8, 2), (4, 8, 4)])
def test_no_draw_is_keyed_twice_and_pass_zero_is_the_plain_call(rng, start, jump, times):
  n = 20
  keys = resample_spec.draw_keys(rng, 7, 3, n, start, jump, times)
  pairs = [(key, sub) for _, _, key, sub in keys]
  assert len(set(pairs)) == len(pairs)
  # Threefry: what is finally hashed -- the key itself for 'init' / 'jump', fold_in(key, i) for a step -- is distinct too
  if rng == 'threefry':
    from msd_amd import jax_random
    final = [key if sub is None else jax_random.fold_in(key, sub) for key, sub in pairs]
    assert len(set(final)) == len(final)
  plain = resample_spec.draw_keys(rng, 7, 3, n, start, jump, 1)
  # pass 0 -- the first block's first descent -- draws what the plain call draws there: its initial draw and its first steps'
  pass0 = [k for k in keys if k[0] == 0]
  first = min(jump, start + 1)
  assert len(pass0) == 1 + first - (1 if first == start + 1 else 0) and pass0 == plain[:len(pass0)]
  assert [k[1] for k in plain] == ['init'] + ['step'] * start
  if rng == 'philox':
    assert plain[0][2:] == ((7, 3), 0) and [k[3] for k in plain[1:]] == [1 + i for i in range(start, 0, -1)]
  else:
    assert [k[3] for k in plain[1:]] == list(range(start, 0, -1))
  # every pass behind a jump: one jump draw, then its steps' draws under the same key; (times - 1) ceil(S / jump) passes
  jumps = [k for k in keys if k[1] == 'jump']
  assert [k[0] for k in jumps] == list(range(1, 1 + (times - 1) * -(-(start + 1) // jump)))
  for p, _, key, _ in jumps:
    assert all(k[2] == key for k in keys if k[0] == p)
    if rng == 'philox':
      assert key == (7, 3 + (p << 32))
  total_steps = sum(1 for k in keys if k[1] == 'step')
  at_zero = times   # scan index 0 runs `times` times (in the last block) and draws nothing
  assert total_steps == times * (start + 1) - at_zero


def test_philox_passes_need_a_32_bit_stream_id():
  with pytest.raises(ValueError):
    resample_spec.draw_keys('philox', 1, 1 << 32, 16, 15, 8, 2)
  assert resample_spec.draw_keys('philox', 1, 1 << 32, 16, 15, 8, 1)   # no resampling: any stream id


def test_threefry_pass_keys_are_the_first_unused_folds():
  from msd_amd import jax_random
  key = jax_random.prng_key(5)
  assert resample_spec.pass_key('threefry', 5, 0, 16, 0) == key
  assert resample_spec.pass_key('threefry', 5, 0, 16, 1) == jax_random.fold_in(key, 16)
  assert resample_spec.pass_key('threefry', 5, 0, 16, 3) == jax_random.fold_in(key, 18)


def test_a_ddim_call_draws_in_its_jumps_alone():
  keys = resample_spec.draw_keys('philox', 1, 0, 16, 15, 4, 2, draws_noise=False)
  assert [k[1] for k in keys] == ['init'] + ['jump'] * 4


# --------------------------------------------------------------------------------------------------
# predict and NativeModel.sample refuse before any device work
# --------------------------------------------------------------------------------------------------
def test_predict_refuses_before_any_device_work():
  m = _bare_model('tiny_context')   # (no handle: anything past predict's own checks would fail on its missing attributes)
  m.rng = 'philox'
  batch = {'encoder_input_tokens': np.zeros((1, 128), np.int32)}
  keep, mask = np.zeros((1, 64, 128), np.float32), np.zeros((1, 64), np.int32)
  with pytest.raises(ValueError, match='resample= needs keep'):
    m.predict(batch, resample=(8, 2))
  for kw in (dict(steps=2), dict(sampler='ddim'), dict(steps=2, sampler='dpmpp_2m')):
    with pytest.raises(ValueError, match='resample= cannot be combined with steps= / sampler='):
      m.predict(batch, keep=keep, keep_mask=mask, resample=(8, 2), **kw)
  with pytest.raises(ValueError, match='resample= cannot be combined with noise='):
    m.predict(batch, keep=keep, keep_mask=mask, resample=(8, 2), noise=np.zeros((4, 1, 64, 128), np.float32))
  with pytest.raises(ValueError, match="rng='jax'"):
    m.predict(batch, keep=keep, keep_mask=mask, resample=(8, 2), rng='jax')
  m.rng = 'jax'
  with pytest.raises(ValueError, match="rng='jax'"):
    m.predict(batch, keep=keep, strength=0.5, resample=(8, 2))
  m.rng = 'philox'
  for bad in ((0, 2), (8, 0), (8,), (2.5, 2), 8):
    with pytest.raises(ValueError, match='resample|jump|times'):
      m.predict(batch, keep=keep, keep_mask=mask, resample=bad)
  with pytest.raises(ValueError, match='keep and keep_mask go together'):   # the known-frame checks are still plan_call's
    m.predict(batch, keep=keep, resample=(8, 2))


def test_plan_call_carries_the_pair():
  keep, mask = np.zeros((1, 64, 128), np.float32), np.zeros((1, 64), np.int32)
  plain = inference.plan_call(keep, mask, None, None, None, 1, 64, 128, 16)
  call = inference.plan_call(keep, mask, None, None, None, 1, 64, 128, 16, resample=(8, 3))
  assert call.resample == (8, 3) and dataclasses.replace(call, resample=None) == dataclasses.replace(plain, keep_mask=call.keep_mask)
  np.testing.assert_array_equal(call.keep_mask, plain.keep_mask)
  assert inference.plan_call(keep, mask, None, None, None, 1, 64, 128, 16, resample=(8, 1)).resample == (8, 1)
  edit = inference.plan_call(keep, None, 0.5, None, None, 1, 64, 128, 16, resample=(4, 2))
  assert edit.resample == (4, 2) and edit.start_step == 7 and (edit.release == 9).all()
  assert inference.plan_call(None, None, None, None, None, 1, 64, 128, 16).resample is None


def test_vary_and_regenerate_hand_the_pair_to_predict():
  import torch
  m = _bare_model('tiny_context')
  seen = []

  def fake_predict(batch, seed=0, segment=0, return_torch=False, rng=None, keep=None, **kw):
    seen.append(kw)
    return torch.zeros((1, 64, 128)), torch.zeros(1)
  m.predict = fake_predict
  song = helpers.known_mel((1, 192, 128), seed=4)
  toks = [np.full(128, k, np.int32) for k in range(3)]
  m.regenerate(song, toks, 40, 100, resample=(8, 2))
  assert len(seen) == 2 and all(kw['resample'] == (8, 2) and 'keep_mask' in kw for kw in seen)
  seen.clear()
  m.regenerate(song, toks, 40, 100, blend_frames=5, resample=(4, 3))
  assert seen and all(kw['resample'] == (4, 3) and 'strength' in kw for kw in seen)
  seen.clear()
  m.vary(song, toks, 0.5, resample=(4, 2))
  assert len(seen) == 3 and all(kw['resample'] == (4, 2) for kw in seen)
  seen.clear()
  m.vary(song, toks, 0.5)
  m.regenerate(song, toks, 40, 100)
  assert all('resample' not in kw for kw in seen)   # the calls as they were
  for call in (lambda: m.vary(song, toks, 0.5, resample=(0, 2)), lambda: m.regenerate(song, toks, 40, 100, resample=(8, 0))):
    seen.clear()
    with pytest.raises(ValueError):
      call()
    assert not seen


# --------------------------------------------------------------------------------------------------
# ABI surface
# --------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_entry_points():
  header = open(os.path.join(ROOT, 'include', 'msd_amd.h')).read()
  assert re.search(r'\bint\s+msd_sample_resample\s*\(\s*msd_model\s*\*', header)
  assert re.search(r'\bint\s+msd_op_renoise\s*\(\s*const\s+msd_config\s*\*', header)
  assert re.search(r'#define\s+MSD_AMD_ABI_VERSION\s+7\b', header)
  assert {'msd_sample_resample', 'msd_op_renoise'} <= set(native.EXPORTED_SYMBOLS)
  assert callable(native.op_renoise)
  # the entry point has no noise_dev argument
  decl = re.search(r'int\s+msd_sample_resample\s*\(([^;]*)\)\s*;', header).group(1)
  assert 'noise_dev' not in decl and 'int jump' in decl and 'int times' in decl


# --------------------------------------------------------------------------------------------------
# command line
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def midi(tmp_path_factory):
  from msd_amd.frontend import midi_io
  from tests.test_frontend_midi import _random_song
  path = tmp_path_factory.mktemp('resample') / 'a.mid'
  path.write_bytes(midi_io.note_sequence_to_midi(_random_song(9, seconds=3.0), ticks_per_quarter=500))
  return str(path)


@pytest.fixture(scope='module')
def old_mel(tmp_path_factory):
  path = tmp_path_factory.mktemp('resample_mel') / 'old.npy'
  np.save(str(path), helpers.known_mel((100, 128), seed=3))
  return str(path)


def test_cli_parses_resample_under_dry_run(midi, old_mel, capsys):
  from msd_amd import synthesize
  base = [midi, '--preset', 'tiny_context', '--num-steps', '20', '--on-too-long', 'truncate', '--dry-run', '--edit-mel', old_mel]
  # the edit's own report stays what it is without --resample; the resample line follows it
  assert synthesize.main(base + ['--regenerate', '0.2:0.6', '--blend', '3']) == 0
  plain_regen = capsys.readouterr().out
  assert 'regenerate frames [' in plain_regen and '  segment 0: frames [' in plain_regen and '  blend 3, segment 0' in plain_regen
  assert 'resample' not in plain_regen
  assert synthesize.main(base + ['--regenerate', '0.2:0.6', '--blend', '3', '--resample', '8:3']) == 0
  assert capsys.readouterr().out == plain_regen + 'resample 8:3: 60 steps and 6 jumps per full segment\n'
  assert synthesize.main(base + ['--vary', '0.5']) == 0
  plain_vary = capsys.readouterr().out
  assert plain_vary.startswith('vary ') and 'regenerate frames' not in plain_vary and 'sampled again' not in plain_vary
  assert 'resample' not in plain_vary and len(plain_vary.splitlines()) == 1
  assert synthesize.main(base + ['--vary', '0.5', '--resample', '4:2']) == 0
  assert capsys.readouterr().out == plain_vary + 'resample 4:2: 20 steps and 3 jumps per full segment\n'
  for bad in (['--resample', '8:3'],                                              # no edit to go with
              ['--regenerate', '0.2:0.6', '--resample', '8:0'], ['--regenerate', '0.2:0.6', '--resample', '0:2'],
              ['--regenerate', '0.2:0.6', '--resample', '8'], ['--regenerate', '0.2:0.6', '--resample', 'a:b'],
              ['--regenerate', '0.2:0.6', '--resample', '8:2', '--steps', '10'],
              ['--regenerate', '0.2:0.6', '--resample', '8:2', '--rng', 'jax']):
    with pytest.raises(SystemExit) as e:
      synthesize.main((base if '--regenerate' in bad else base[:-2]) + bad)
    assert e.value.code == 2, bad
    capsys.readouterr()
  with pytest.raises(SystemExit) as e:
    synthesize.main([midi, '--preset', 'tiny_context', '--dry-run', '--resample', '8:3', '--steps', '50'])
  assert e.value.code == 2 and '--resample' in capsys.readouterr().err


def test_cli_hands_resample_to_regenerate_and_vary(midi, old_mel, tmp_path, monkeypatch):
  import torch
  from msd_amd import synthesize
  seen = []

  class Model:
    def __init__(self, *a, **k):
      self.targets_context_length = 64
      self._torch, self.device = torch, torch.device('cpu')
      self.audio_codec = msd_amd.audio_codecs.MelGAN()

    def check_batch_segments(self, *a):
      pass

    def regenerate(self, song, segments, start, stop, **kw):
      seen.append(('regenerate', kw))
      return song

    def vary(self, song, segments, strength, **kw):
      seen.append(('vary', kw))
      return song
  monkeypatch.setattr(msd_amd, 'InferenceModel', Model)
  base = [midi, '--preset', 'tiny_context', '--num-steps', '20', '--on-too-long', 'truncate', '--edit-mel', old_mel,
          '--out', str(tmp_path / 'o.npy')]
  assert synthesize.main(base + ['--regenerate', '0.2:0.6', '--resample', '8:3']) == 0
  assert seen[-1][0] == 'regenerate' and seen[-1][1]['resample'] == (8, 3)
  assert synthesize.main(base + ['--vary', '0.5', '--resample', '4:2', '--rng', 'threefry']) == 0
  assert seen[-1][0] == 'vary' and seen[-1][1]['resample'] == (4, 2) and seen[-1][1]['rng'] == 'threefry'
  assert synthesize.main(base + ['--regenerate', '0.2:0.6']) == 0
  assert 'resample' not in seen[-1][1]
