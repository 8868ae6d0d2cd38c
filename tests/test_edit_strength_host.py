"""Edit strength, the parts that need no device: plan_strength / region_strength, the specification (tests/edit_spec.py)
against the oracle's eval_scan and against tests/keep_spec.py, vary / regenerate(blend_frames=) on a stubbed predict, the
ABI surface and the command line."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import msd_amd
from msd_amd import inference, native
from tests import edit_spec, helpers, keep_spec
from tests.test_host_logic import _bare_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------------
# plan_strength
# --------------------------------------------------------------------------------------------------
def test_plan_strength_rounds_half_up_and_names_the_start():
  # N = 20: 0.125 * 20 = 2.5 and 0.375 * 20 = 7.5 are exact in binary -> 3 and 8; 0.55 * 20 = 11.000000000000002 -> 11
  words, start = inference.plan_strength([[0.125, 0.375, 0.55, 0.12, 0.13]], 20)
  assert words.dtype == np.int32 and words.shape == (1, 5) and words.flags['C_CONTIGUOUS']
  assert words.tolist() == [[4, 9, 12, 3, 4]] and start == 10
  # just below a half stays down
  assert inference.plan_strength([[np.nextafter(0.125, 0.0)]], 20)[0].tolist() == [[3]]


def test_plan_strength_ends_of_the_range():
  words, start = inference.plan_strength(np.zeros((2, 3)), 16)
  assert (words == 1).all() and start == -1                   # known throughout, nothing to sample
  words, start = inference.plan_strength(np.ones((2, 3), np.float32), 16)
  assert (words == 0).all() and start == 15                   # free throughout, the full scan
  # a strength that rounds to N is free throughout; one that rounds to 0 is known throughout
  words, start = inference.plan_strength([[0.97, 0.96, 0.03, 0.04]], 16)
  assert words.tolist() == [[0, 16, 1, 2]] and start == 15
  assert inference.plan_strength([[0.5]], 1) == (np.array([[0]], np.int32), 0)
  assert inference.plan_strength([[0.49]], 1)[0].tolist() == [[1]]


def test_plan_strength_mixed_rows_share_the_largest_start():
  s = np.zeros((2, 64))
  s[0] = np.linspace(0.0, 1.0, 64)
  s[1, 10:20] = 0.25
  words, start = inference.plan_strength(s, 16)
  f = edit_spec.free_steps(words, 16)
  np.testing.assert_array_equal(f, np.floor(s * 16 + 0.5).astype(np.int64))
  assert start == 15 and words[0, 0] == 1 and words[0, -1] == 0 and set(words[1].tolist()) == {1, 5}
  words, start = inference.plan_strength(s[1:], 16)
  assert start == 3 and words.max() == 5
  # the rule msd_sample_edit checks: below the full scan every word lies in [1, start_step + 2]
  assert words.min() >= 1 and words.max() <= start + 2


@pytest.mark.parametrize('bad', [[[np.nan]], [[-0.01]], [[1.01]], [[np.inf]], [0.5, 0.5], 0.5, np.zeros((1, 2, 3)), [['a']],
                                 np.zeros((0, 4))])
def test_plan_strength_refuses(bad):
  with pytest.raises(ValueError):
    inference.plan_strength(bad, 16)


def test_plan_strength_refuses_bad_step_counts():
  for n in (0, -1, 2.5, True):
    with pytest.raises(ValueError):
      inference.plan_strength([[0.5]], n)


def test_check_strength_shapes_and_mask():
  flags = np.zeros((2, 4), np.int32)
  flags[1, 2] = 1
  np.testing.assert_array_equal(inference.check_strength(0.5, None, 2, 4), np.full((2, 4), 0.5))
  np.testing.assert_array_equal(inference.check_strength([0.25, 0.75], flags, 2, 4),
                                [[0.25] * 4, [0.75, 0.75, 0.0, 0.75]])
  s = np.arange(8.0).reshape(2, 4) / 8
  got = inference.check_strength(torch.as_tensor(s), None, 2, 4)
  np.testing.assert_array_equal(got, s)
  for bad in (np.zeros(3), np.zeros((2, 3)), np.zeros((4, 2)), np.zeros((2, 4, 1))):
    with pytest.raises(ValueError):
      inference.check_strength(bad, None, 2, 4)


# --------------------------------------------------------------------------------------------------
# region_strength
# --------------------------------------------------------------------------------------------------
def test_region_strength_without_blend_is_plan_region():
  for args in [(192, 64, 40, 100), (192, 64, 70, 100), (256, 64, 64, 192), (64, 64, 0, 64), (192, 64, 10, 65)]:
    hard, soft = inference.plan_region(*args), inference.region_strength(*args, 0)
    assert [k for k, _ in soft] == [k for k, _ in hard]
    for (_, row), (_, s) in zip(hard, soft):
      assert s.dtype == np.float64 and s.shape == row.shape
      np.testing.assert_array_equal(s, 1.0 - row)


def test_region_strength_ramp_crosses_a_segment_boundary():
  # region [60, 70) of three 64-frame segments, 7 frames of ramp: the left ramp [53, 60) lies in segment 0, the right
  # one [70, 77) in segment 1
  plan = inference.region_strength(192, 64, 60, 70, 7)
  assert [k for k, _ in plan] == [0, 1]
  song = np.concatenate([row for _, row in plan])
  np.testing.assert_array_equal(song[60:70], 1.0)
  np.testing.assert_allclose(song[53:60], 1.0 - np.arange(7, 0, -1) / 8.0, rtol=0, atol=1e-15)
  np.testing.assert_allclose(song[70:77], 1.0 - np.arange(1, 8) / 8.0, rtol=0, atol=1e-15)
  assert not song[:53].any() and not song[77:].any()
  # a region that ends on a boundary: only the ramp reaches segment 1, which joins the plan
  plan = inference.region_strength(192, 64, 40, 64, 3)
  assert [k for k, _ in plan] == [0, 1]
  np.testing.assert_allclose(plan[1][1][:4], [0.75, 0.5, 0.25, 0.0], rtol=0, atol=1e-15)
  assert [k for k, _ in inference.plan_region(192, 64, 40, 64)] == [0]
  # the ramp is cut off at the song's ends, and may span more than one segment
  plan = inference.region_strength(192, 64, 2, 5, 100)
  assert [k for k, _ in plan] == [0, 1] and plan[0][1][0] == 1.0 - 2 / 101.0 and plan[1][1][40] == 1.0 - 100 / 101.0
  assert plan[1][1][41] == 0.0


@pytest.mark.parametrize('args', [(192, 64, 100, 100, 2), (200, 64, 0, 10, 2), (192, 64, 10, 20, -1), (192, 64, 10, 20, 1.5),
                                  (192, 64, 10, 193, 0)])
def test_region_strength_refuses(args):
  with pytest.raises(ValueError):
    inference.region_strength(*args)


# --------------------------------------------------------------------------------------------------
# the specification
# --------------------------------------------------------------------------------------------------
def _fast(sampler, steps=4):
  from oracle import backend, fast
  spec = msd_amd.config.preset('tiny_context', num_steps=steps)
  d = spec.diffusion
  spec = dataclasses.replace(spec, diffusion=dataclasses.replace(d, sampler=dataclasses.replace(d.sampler, name=sampler)))
  params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
  cfg, dc = helpers.oracle_configs(spec)
  return spec, fast.FastModel(backend.NumpyBackend('float64'), cfg, dc, params, True)


@pytest.fixture(scope='module', params=['ddpm', 'ddim'])
def spec_run(request):
  """One float64 model per sampler: (fm, batch, init_z, noise, known mel)."""
  spec, fm = _fast(request.param)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  init_z, noise = helpers.make_noise(spec, batch=2)
  if request.param == 'ddim':
    noise = None
  known = np.random.default_rng(21).uniform(-13.0, 5.0, (2, 64, 128)).astype(np.float32)
  return fm, batch, init_z, noise, known


def test_spec_strength_one_everywhere_is_eval_scan(spec_run):
  from oracle import sampler
  fm, batch, init_z, noise, known = spec_run
  words, start = inference.plan_strength(np.ones((2, 64)), 4)
  dec, x0, _ = edit_spec.predict_edit(fm, batch, init_z, noise, known, words, start)
  xp = fm.xp
  want = sampler.eval_scan(xp, xp.asarray(init_z), None if noise is None else xp.asarray(noise), keep_spec.fast_pred_fn(fm), fm.dc)
  assert x0.dtype == np.float64
  np.testing.assert_array_equal(x0, want)


def test_spec_strength_zero_everywhere_returns_the_known_mel(spec_run):
  fm, batch, init_z, noise, known = spec_run
  words, start = inference.plan_strength(np.zeros((2, 64)), 4)
  assert start == -1
  dec, _, _ = edit_spec.predict_edit(fm, batch, init_z, noise, known, words, start)
  np.testing.assert_array_equal(dec, known.astype(np.float64))
  # and with the full scan forced on the same words: every frame known at every step arrives at xk
  dec, x0, xk = edit_spec.predict_edit(fm, batch, init_z, noise, known, words, 3)
  np.testing.assert_array_equal(x0, xk)
  np.testing.assert_array_equal(dec, known.astype(np.float64))


def test_spec_with_flags_at_the_full_scan_is_the_keep_spec(spec_run):
  fm, batch, init_z, noise, known = spec_run
  mask = keep_spec.parity_masks(2)
  words, start = inference.plan_strength(1.0 - mask, 4)
  np.testing.assert_array_equal(words, mask)
  assert start == 3
  got = edit_spec.predict_edit(fm, batch, init_z, noise, known, words, start)
  want = keep_spec.predict_keep(fm, batch, init_z, noise, known, mask)
  for g, w in zip(got, want):
    np.testing.assert_array_equal(g, w)


def test_spec_part_way_start_and_release(spec_run):
  """Half strength: two of four steps from the diffused mel; frames released for the last step only differ from both the
  known mel and the fully free frames' values."""
  fm, batch, init_z, noise, known = spec_run
  s = np.zeros((2, 64))
  s[:, :32] = 0.5
  s[0, 32:40] = 0.25
  words, start = inference.plan_strength(s, 4)
  assert start == 1 and set(words.ravel().tolist()) == {1, 2, 3}
  dec, x0, xk = edit_spec.predict_edit(fm, batch, init_z, noise, known, words, start)
  np.testing.assert_array_equal(dec[words == 1], known.astype(np.float64)[words == 1])
  np.testing.assert_array_equal(x0[words == 1], xk[words == 1])
  assert np.isfinite(dec).all() and np.abs(x0[words > 1] - xk[words > 1]).max() > 1e-3
  # the start state is the diffused mel: alpha^2 + sigma^2 == 1
  alpha, sigma = edit_spec.start_coefs(fm.xp, fm.dc, 2, start)
  np.testing.assert_allclose(alpha ** 2 + sigma ** 2, 1.0, rtol=0, atol=1e-15)
  z = edit_spec.start_state(fm.xp, fm.dc, fm.xp.asarray(xk), fm.xp.asarray(init_z), start)
  np.testing.assert_allclose(z, alpha[0] * xk + sigma[0] * init_z.astype(np.float64), rtol=0, atol=1e-15)


# --------------------------------------------------------------------------------------------------
# predict / vary / regenerate on a stubbed device call
# --------------------------------------------------------------------------------------------------
def test_predict_refuses_strength_without_keep_before_any_device():
  m = _bare_model('tiny_context')
  batch = {'encoder_input_tokens': np.zeros((1, 128), np.int32)}
  with pytest.raises(ValueError, match='strength needs keep'):
    m.predict(batch, strength=0.5)
  with pytest.raises(ValueError):
    m.predict(batch, keep=np.zeros((1, 64, 128), np.float32), strength=1.5)
  with pytest.raises(ValueError):
    m.predict(batch, keep=np.zeros((1, 64, 128), np.float32), strength=np.zeros((1, 63)))


def test_predict_plans_the_strength_and_hands_it_to_the_device_call():
  m = _bare_model('tiny_context')
  m.rng, m.range_fallback, m.precision = 'philox', False, 'f16x3'
  seen = []
  m._predict_once = lambda *a: seen.append(a) or 'out'
  batch = {'encoder_input_tokens': np.zeros((1, 128), np.int32)}
  known = np.zeros((1, 64, 128), np.float32)
  mask = np.zeros((1, 64), bool)
  mask[0, :8] = True
  assert m.predict(batch, keep=known, strength=0.5, keep_mask=mask) == 'out'
  call = seen[0][-1]   # (the one call form predict hands down: inference.SampleCall)
  words = call.release
  assert call.keep is known and call.keep_mask is None and call.start_step == 1            # N = 4: two steps
  assert (words[0, :8] == 1).all() and (words[0, 8:] == 3).all()
  assert call.steps is None and call.sampler is None
  # keep + keep_mask without strength: today's call, untouched
  m.predict(batch, keep=known, keep_mask=mask)
  call = seen[1][-1]
  assert call.release is None and call.start_step is None and call.keep is known
  assert call.keep_mask.dtype == np.int32 and call.keep_mask.sum() == 8


def _stub(m, seen):
  def fake_predict(batch, seed=0, segment=0, return_torch=False, rng=None, keep=None, **kw):
    assert return_torch
    seen.append(dict(batch=batch, seed=seed, segment=segment, rng=rng, keep=keep.clone(), kw=kw))
    return torch.full((1, 64, 128), 1000.0 + 10 * segment + len(seen)), torch.zeros(1)
  m.predict = fake_predict


def _song(k=3):
  return np.random.default_rng(4).uniform(-11, 4, (1, k * 64, 128)).astype(np.float32)


def test_vary_calls_every_segment_with_the_new_context():
  m = _bare_model('tiny_context')
  seen = []
  _stub(m, seen)
  song = _song(3)
  toks = [np.full(128, k, np.int32) for k in range(3)]
  new = m.vary(song, toks, 0.25, seed=5, rng='threefry')
  assert isinstance(new, np.ndarray) and new.shape == song.shape and new.dtype == np.float32
  assert [c['segment'] for c in seen] == [0, 1, 2] and all(c['seed'] == 5 and c['rng'] == 'threefry' for c in seen)
  for k, c in enumerate(seen):
    assert set(c['kw']) == {'strength'} and c['kw']['strength'].shape == (1, 64) and (c['kw']['strength'] == 0.25).all()
    np.testing.assert_array_equal(c['keep'].numpy(), song[:, k * 64:(k + 1) * 64])    # the OLD segment is the known mel
  assert not np.asarray(seen[0]['batch']['encoder_continuous_mask']).any()
  # the context of segment k is the NEW segment k - 1
  assert (torch.as_tensor(seen[1]['batch']['encoder_continuous_inputs']) == 1001.0).all()
  assert (torch.as_tensor(seen[2]['batch']['encoder_continuous_inputs']) == 1012.0).all()
  assert (new[:, :64] == 1001.0).all() and (new[:, 64:128] == 1012.0).all() and (new[:, 128:] == 1023.0).all()
  # one strength per frame, cut per segment
  seen.clear()
  per_frame = np.linspace(0, 1, 192)
  m.vary(torch.as_tensor(song), toks, per_frame, always_mask_context=True, return_torch=True)
  np.testing.assert_array_equal(seen[1]['kw']['strength'], per_frame[None, 64:128])
  assert not np.asarray(seen[1]['batch']['encoder_continuous_mask']).any()
  for bad in (np.zeros(191), np.zeros((2, 192))):
    with pytest.raises(ValueError):
      m.vary(song, toks, bad)
  with pytest.raises(ValueError):
    m.vary(song, toks[:2], 0.5)


def test_regenerate_with_blend_runs_the_ramp_segments_and_keeps_the_rest():
  m = _bare_model('tiny_context')
  seen = []
  _stub(m, seen)
  song = _song(3)
  toks = [np.full(128, k, np.int32) for k in range(3)]
  new = m.regenerate(song, toks, 40, 64, seed=2, blend_frames=3)
  assert [c['segment'] for c in seen] == [0, 1]                    # segment 1: the ramp alone
  want = inference.region_strength(192, 64, 40, 64, 3)
  for c, (_, row) in zip(seen, want):
    assert set(c['kw']) == {'strength'}
    np.testing.assert_array_equal(c['kw']['strength'], row[None])
  assert (new[:, 37:64] == 1001.0).all() and (new[:, 64:67] == 1012.0).all()
  np.testing.assert_array_equal(new[:, :37], song[:, :37])
  np.testing.assert_array_equal(new[:, 67:], song[:, 67:])
  # segment 1 saw segment 0 as it stands
  ctx = torch.as_tensor(seen[1]['batch']['encoder_continuous_inputs']).numpy()
  np.testing.assert_array_equal(ctx[:, :37], song[:, :37])
  assert (ctx[:, 37:] == 1001.0).all()
  # blend_frames = 0 is the call regenerate made before there was a blend: keep_mask, no strength
  seen.clear()
  m.regenerate(song, toks, 40, 64, seed=2, blend_frames=0)
  assert [c['segment'] for c in seen] == [0] and set(seen[0]['kw']) == {'keep_mask'}
  with pytest.raises(ValueError):
    m.regenerate(song, toks, 40, 64, blend_frames=-1)


# --------------------------------------------------------------------------------------------------
# ABI surface
# --------------------------------------------------------------------------------------------------
def test_header_declares_the_three_entries_without_an_abi_bump():
  with open(os.path.join(ROOT, 'include', 'msd_amd.h')) as f:
    header = f.read()
  ws = r'\s*'
  assert re.search(r'\bint\s+msd_sample_edit\s*\(\s*msd_model\s*\*\s*m\s*,\s*int\s+batch\s*,\s*int\s+rng\s*,\s*int\s+per_row\s*,\s*'
                   r'const\s+uint64_t\s*\*\s*seeds\s*,\s*const\s+uint64_t\s*\*\s*stream_ids\s*,\s*const\s+float\s*\*\s*init_z_dev\s*,\s*'
                   r'const\s+float\s*\*\s*noise_dev\s*,\s*const\s+float\s*\*\s*known_dev\s*,\s*const\s+int32_t\s*\*\s*release\s*,\s*'
                   r'int\s+start_step\s*,\s*float\s*\*\s*out_dev\s*,\s*void\s*\*\s*stream\s*\)', header)
  assert re.search(r'\bint\s+msd_op_sampler_step_release\s*\(\s*const\s+msd_config\s*\*\s*cfg\s*,', header)
  assert re.search(r'known_scaled_dev\s*,\s*const\s+int32_t\s*\*\s*release_dev\s*,\s*int\s+n_dims\s*,', header)
  assert re.search(r'\bint\s+msd_op_diffuse_to_step\s*\(\s*const\s+msd_config\s*\*\s*cfg\s*,\s*int\s+step_index\s*,\s*'
                   r'const\s+float\s*\*\s*mel_dev\s*,\s*const\s+float\s*\*\s*eps_dev\s*,', header)
  for name in ('msd_sample_edit', 'msd_op_sampler_step_release', 'msd_op_diffuse_to_step'):
    assert name in native.EXPORTED_SYMBOLS
  assert re.search(r'#define\s+MSD_AMD_ABI_VERSION\s+7\b', header) and native.ABI_VERSION == 7
  assert callable(native.op_sampler_step_release) and callable(native.op_diffuse_to_step)


def test_bindings_declare_the_argument_types():
  import __graft_entry__
  __graft_entry__.build()
  c = ctypes
  vp, i32, i64, u64p = c.c_void_p, c.c_int, c.c_int64, c.POINTER(c.c_uint64)
  cfgp = c.POINTER(native.MsdConfig)
  for planes in ('f16', 'bf16'):
    lib = native.load(planes)
    assert list(lib.msd_sample_edit.argtypes) == [vp, i32, i32, i32, u64p, u64p, vp, vp, vp, vp, i32, vp, vp]
    assert list(lib.msd_op_sampler_step_release.argtypes) == [cfgp, i32, vp, vp, vp, vp, vp, vp, i32, vp, i64, vp]
    assert list(lib.msd_op_diffuse_to_step.argtypes) == [cfgp, i32, vp, vp, vp, vp, vp, i64, vp]
    for name in ('msd_sample_edit', 'msd_op_sampler_step_release', 'msd_op_diffuse_to_step'):
      assert getattr(lib, name).restype is i32
    assert b'abi 7' in lib.msd_version()


# --------------------------------------------------------------------------------------------------
# command line
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def midi(tmp_path_factory):
  from msd_amd.frontend import midi_io
  from tests.test_frontend_midi import _random_song
  path = tmp_path_factory.mktemp('edit') / 'a.mid'
  path.write_bytes(midi_io.note_sequence_to_midi(_random_song(9, seconds=3.0), ticks_per_quarter=500))
  return str(path)


BASE = ['--preset', 'tiny_context', '--num-steps', '8', '--on-too-long', 'truncate']


def _no_model(monkeypatch):
  monkeypatch.setattr(msd_amd, 'InferenceModel', lambda *a, **k: pytest.fail('a model was created'))


def test_cli_dry_run_prints_the_vary_and_blend_plans(midi, tmp_path, capsys, monkeypatch):
  from msd_amd import synthesize
  _no_model(monkeypatch)
  old = tmp_path / 'old.npy'
  np.save(old, np.zeros((240, 128), np.float32))
  assert synthesize.main([midi, *BASE, '--dry-run', '--edit-mel', str(old), '--vary', '0.25']) == 0
  assert 'vary 4 segments at strength 0.25: 2 of 8 steps each' in capsys.readouterr().out
  assert synthesize.main([midi, *BASE, '--dry-run', '--edit-mel', str(old), '--regenerate', '0.8:1.28', '--blend', '7']) == 0
  out = capsys.readouterr().out
  assert 'regenerate frames [40, 64) of 256' in out and 'segment 0: frames [40, 64) sampled again' in out
  assert 'blend 7, segment 0: 7 frames released part-way, 8 of 8 steps' in out
  assert 'blend 7, segment 1: 7 frames released part-way, 7 of 8 steps' in out


@pytest.mark.parametrize('extra, message', [
    (['--vary', '0.5'], 'needs the old rendering'),
    (['--vary', '1.5', '--edit-mel', 'OLD'], 'in [0, 1]'),
    (['--vary', '0.5', '--regenerate', '0.5:1.0', '--edit-mel', 'OLD'], 'give one'),
    (['--blend', '4', '--vary', '0.5', '--edit-mel', 'OLD'], 'goes with --regenerate'),
    (['--blend', '-1', '--regenerate', '0.5:1.0', '--edit-mel', 'OLD'], 'goes with --regenerate'),
    (['--vary', '0.5', '--edit-mel', 'OLD', '--batch-segments', '2'], 'one by one'),
    (['--edit-mel', 'OLD'], '--vary STRENGTH'),
])
def test_cli_usage_errors(midi, tmp_path, capsys, monkeypatch, extra, message):
  from msd_amd import synthesize
  _no_model(monkeypatch)
  old = tmp_path / 'old.npy'
  np.save(old, np.zeros((240, 128), np.float32))
  extra = [str(old) if a == 'OLD' else a for a in extra]
  with pytest.raises(SystemExit) as e:
    synthesize.main([midi, *BASE, '--dry-run', *extra])
  assert e.value.code == 2 and message in capsys.readouterr().err


def test_cli_varies_and_blends_through_the_model(midi, tmp_path, monkeypatch):
  from msd_amd import synthesize
  calls = []

  def fake_model(checkpoint, spec, batch_size=1, **kw):
    m = _bare_model('tiny_context')
    m.vary = lambda song, segments, strength, **kw: calls.append(('vary', strength, kw)) or song + 1.0
    m.regenerate = lambda song, segments, start, stop, **kw: calls.append(('regenerate', (start, stop), kw)) or song + 2.0
    return m

  monkeypatch.setattr(msd_amd, 'InferenceModel', fake_model)
  old, out = tmp_path / 'old.npy', tmp_path / 'new.npy'
  mel = np.random.default_rng(1).uniform(-11, 4, (240, 128)).astype(np.float32)
  np.save(old, mel)
  assert synthesize.main([midi, *BASE, '--edit-mel', str(old), '--vary', '0.3', '--seed', '3', '--out', str(out)]) == 0
  assert calls[0][:2] == ('vary', 0.3) and calls[0][2]['seed'] == 3 and calls[0][2]['return_torch']
  np.testing.assert_array_equal(np.load(out), mel + 1.0)
  assert synthesize.main([midi, *BASE, '--edit-mel', str(old), '--regenerate', '0.8:2.0', '--blend', '5', '--out', str(out)]) == 0
  assert calls[1][:2] == ('regenerate', (40, 100)) and calls[1][2]['blend_frames'] == 5
  assert synthesize.main([midi, *BASE, '--edit-mel', str(old), '--regenerate', '0.8:2.0', '--out', str(out)]) == 0
  assert 'blend_frames' not in calls[2][2]
