"""Known frames in the sampler, the parts that need no device: the specification itself (tests/keep_spec.py) against
the oracle's eval_scan, the segment / mask plan of InferenceModel.regenerate, regenerate on a stubbed predict, the ABI
surface and the command line."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import msd_amd
from msd_amd import inference, native
from tests import helpers, keep_spec
from tests.test_host_logic import _bare_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------------
# the specification
# --------------------------------------------------------------------------------------------------
def _fast(sampler, steps=4, dtype='float64'):
  from oracle import backend, fast
  spec = msd_amd.config.preset('tiny_context', num_steps=steps)
  d = spec.diffusion
  spec = dataclasses.replace(spec, diffusion=dataclasses.replace(d, sampler=dataclasses.replace(d.sampler, name=sampler)))
  params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
  cfg, dc = helpers.oracle_configs(spec)
  fm = fast.FastModel(backend.NumpyBackend(dtype), cfg, dc, params, True)
  return spec, fm


@pytest.fixture(scope='module', params=['ddpm', 'ddim'])
def spec_run(request):
  """One model per sampler, encoded once: (spec, fm, batch, init_z, noise, keep mel)."""
  spec, fm = _fast(request.param)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  init_z, noise = helpers.make_noise(spec, batch=2)
  if request.param == 'ddim':
    noise = None
  keep = np.random.default_rng(21).uniform(-13.0, 5.0, (2, 64, 128)).astype(np.float32)   # beyond both ends of the codec's range
  keep_spec.encode(fm, batch)
  return spec, fm, batch, init_z, noise, keep


def test_spec_with_an_all_zero_mask_is_the_oracles_eval_scan(spec_run):
  from oracle import sampler
  spec, fm, batch, init_z, noise, keep = spec_run
  xp = fm.xp
  z0, nz = xp.asarray(init_z), None if noise is None else xp.asarray(noise)
  pred = keep_spec.fast_pred_fn(fm)
  want = sampler.eval_scan(xp, z0, nz, pred, fm.dc)
  xk = fm.codec.scale_features(xp, xp.asarray(keep), (-1., 1.), clip=True)
  got = keep_spec.eval_scan_keep(xp, z0, nz, pred, fm.dc, xk, keep_spec.frame_mask(xp, np.zeros((2, 64), np.int32)))
  assert got.dtype == np.float64
  np.testing.assert_array_equal(got, want)
  np.testing.assert_array_equal(got, fm.sample(init_z, noise))   # (and FastModel's own loop)


def test_spec_returns_kept_frames_exactly(spec_run):
  spec, fm, batch, init_z, noise, keep = spec_run
  mask = keep_spec.parity_masks(2)
  dec, x0, xk = keep_spec.predict_keep(fm, batch, init_z, noise, keep, mask)
  kept = mask.astype(bool)
  np.testing.assert_array_equal(x0[kept], xk[kept])                       # the scan arrives at xk
  np.testing.assert_array_equal(dec[kept], keep.astype(np.float64)[kept])  # the result holds the caller's values
  assert np.abs(xk).max() <= 1.0 and (keep > 4.0).any() and (keep < np.log(1e-5)).any()
  free = dec[~kept]
  assert np.isfinite(free).all() and not np.array_equal(free, keep.astype(np.float64)[~kept])
  # the free frames are not those of the run without a mask: they saw the known ones
  plain = fm.sample(init_z, noise)
  assert np.abs(x0[~kept] - plain[~kept]).max() > 1e-3


# --------------------------------------------------------------------------------------------------
# plan_region
# --------------------------------------------------------------------------------------------------
def _free(row):
  f = np.nonzero(row == 0)[0]
  assert np.array_equal(f, np.arange(f[0], f[-1] + 1))   # one run of frames
  return int(f[0]), int(f[-1]) + 1


def test_plan_region_inside_one_segment():
  plan = inference.plan_region(192, 64, 70, 100)
  assert [k for k, _ in plan] == [1]
  row = plan[0][1]
  assert row.dtype == np.int32 and row.shape == (64,) and _free(row) == (6, 36) and int(row.sum()) == 64 - 30


def test_plan_region_across_a_boundary():
  plan = inference.plan_region(192, 64, 40, 100)
  assert [k for k, _ in plan] == [0, 1]
  assert _free(plan[0][1]) == (40, 64) and _free(plan[1][1]) == (0, 36)


def test_plan_region_of_whole_segments():
  plan = inference.plan_region(256, 64, 64, 192)
  assert [k for k, _ in plan] == [1, 2]
  assert all(not row.any() for _, row in plan)
  plan = inference.plan_region(64, 64, 0, 64)
  assert [k for k, _ in plan] == [0] and not plan[0][1].any()
  # a region that ends on a boundary does not touch the next segment; one frame past it does
  assert [k for k, _ in inference.plan_region(192, 64, 10, 64)] == [0]
  assert [k for k, _ in inference.plan_region(192, 64, 10, 65)] == [0, 1]


@pytest.mark.parametrize('args', [(192, 64, 100, 100), (192, 64, 100, 40), (192, 64, -1, 10), (192, 64, 10, 193),
                                  (200, 64, 0, 10), (0, 64, 0, 0), (192, 0, 0, 10), (192, 64, 1.5, 10)])
def test_plan_region_refuses_bad_ranges_and_ragged_songs(args):
  with pytest.raises(ValueError):
    inference.plan_region(*args)


def test_check_keep_pairs_and_shapes():
  keep, mask = np.zeros((2, 64, 128), np.float32), np.zeros((2, 64), bool)
  assert inference.check_keep(None, None, 2, 64, 128) == (None, None)
  mask[1, 3] = True
  k, f = inference.check_keep(keep, mask, 2, 64, 128)
  assert k is keep and f.dtype == np.int32 and f.flags['C_CONTIGUOUS'] and f.sum() == 1 and f[1, 3] == 1
  assert inference.check_keep(keep, torch.as_tensor(mask).to(torch.int64) * 7, 2, 64, 128)[1][1, 3] == 1
  for bad in [(keep, None), (None, mask), (keep[:1], mask), (keep, mask[:, :63]), (keep[:, :, :64], mask),
              (keep, mask.astype(np.float32))]:
    with pytest.raises(ValueError):
      inference.check_keep(bad[0], bad[1], 2, 64, 128)
  m = _bare_model('tiny_context')
  with pytest.raises(ValueError, match='go together'):   # before anything touches a device
    m.predict({'encoder_input_tokens': np.zeros((2, 128), np.int32)}, keep=keep)


# --------------------------------------------------------------------------------------------------
# regenerate on a stubbed predict
# --------------------------------------------------------------------------------------------------
def _stub(m, seen):
  """predict stub: every element of row 0 is 1000 + 10 * segment + the call's number (kept frames included: regenerate
  itself must leave them alone)."""
  def fake_predict(batch, seed=0, segment=0, return_torch=False, rng=None, keep=None, keep_mask=None, **kw):
    assert return_torch and not kw
    seen.append(dict(batch=batch, seed=seed, segment=segment, rng=rng, keep=keep.clone(), keep_mask=np.array(keep_mask)))
    return torch.full((1, 64, 128), 1000.0 + 10 * segment + len(seen)), torch.zeros(1)
  m.predict = fake_predict


def _song(k=3):
  return np.random.default_rng(4).uniform(-11, 4, (1, k * 64, 128)).astype(np.float32)


def test_regenerate_calls_keys_masks_and_contexts():
  m = _bare_model('tiny_context')
  seen = []
  _stub(m, seen)
  song = _song(4)
  toks = [np.full(128, k, np.int32) for k in range(4)]
  new = m.regenerate(song, toks, 100, 140, seed=5, rng='threefry')
  assert isinstance(new, np.ndarray) and new.shape == song.shape and new.dtype == np.float32
  assert [c['segment'] for c in seen] == [1, 2] and all(c['seed'] == 5 and c['rng'] == 'threefry' for c in seen)
  assert [int(np.asarray(c['batch']['encoder_input_tokens'])[0, 0]) for c in seen] == [1, 2]
  for c, (lo, hi) in zip(seen, [(36, 64), (0, 12)]):
    assert c['keep_mask'].shape == (1, 64) and _free(c['keep_mask'][0]) == (lo, hi)
    assert np.asarray(c['batch']['encoder_continuous_mask']).tolist() == [[1] * 64]
  # segment 1 keeps the song's frames and sees the ORIGINAL segment 0
  np.testing.assert_array_equal(seen[0]['keep'].numpy(), song[:, 64:128])
  np.testing.assert_array_equal(torch.as_tensor(seen[0]['batch']['encoder_continuous_inputs']).numpy(), song[:, :64])
  # segment 2 sees segment 1 AS IT STANDS: the song outside the region, the first call's result inside
  ctx = torch.as_tensor(seen[1]['batch']['encoder_continuous_inputs']).numpy()
  np.testing.assert_array_equal(ctx[:, :36], song[:, 64:100])
  assert (ctx[:, 36:] == 1011.0).all()
  np.testing.assert_array_equal(seen[1]['keep'].numpy(), song[:, 128:192])
  # the result: the region holds the calls' values, everything else is the input, bit for bit
  assert (new[:, 100:128] == 1011.0).all() and (new[:, 128:140] == 1022.0).all()
  np.testing.assert_array_equal(new[:, :100], song[:, :100])
  np.testing.assert_array_equal(new[:, 140:], song[:, 140:])
  assert len(seen) == 2   # segment 3 is not run again


def test_regenerate_segment_zero_and_always_mask_context_run_without_context():
  m = _bare_model('tiny_context')
  seen = []
  _stub(m, seen)
  song = _song(3)
  toks = [np.full(128, k, np.int32) for k in range(3)]
  out = m.regenerate(torch.as_tensor(song), toks, 10, 70, return_torch=True)
  assert isinstance(out, torch.Tensor) and [c['segment'] for c in seen] == [0, 1]
  assert not np.asarray(seen[0]['batch']['encoder_continuous_mask']).any()
  assert float(torch.as_tensor(seen[0]['batch']['encoder_continuous_inputs']).abs().sum()) == 0.0
  assert np.asarray(seen[1]['batch']['encoder_continuous_mask']).all()
  seen.clear()
  m.regenerate(song, toks, 70, 150, always_mask_context=True)
  assert [c['segment'] for c in seen] == [1, 2]
  for c in seen:
    assert not np.asarray(c['batch']['encoder_continuous_mask']).any()
    assert float(torch.as_tensor(c['batch']['encoder_continuous_inputs']).abs().sum()) == 0.0


def test_regenerate_without_context_model_and_errors():
  m = _bare_model('tiny')
  seen = []
  _stub(m, seen)
  song = _song(2)
  toks = [np.full(128, k, np.int32) for k in range(2)]
  new = m.regenerate(song, toks, 0, 128)
  assert all('encoder_continuous_inputs' not in c['batch'] for c in seen) and [c['segment'] for c in seen] == [0, 1]
  assert (new[:, :64] == 1001.0).all() and (new[:, 64:] == 1012.0).all()
  for bad in [dict(start_frame=0, stop_frame=129), dict(start_frame=5, stop_frame=5)]:
    with pytest.raises(ValueError):
      m.regenerate(song, toks, **bad)
  with pytest.raises(ValueError, match='segments of tokens'):
    m.regenerate(song, toks[:1], 0, 10)
  with pytest.raises(ValueError):
    m.regenerate(song[:, :100], toks, 0, 10)    # not whole segments
  with pytest.raises(ValueError):
    m.regenerate(song[0], toks, 0, 10)          # not [1, frames, n]


# --------------------------------------------------------------------------------------------------
# ABI surface
# --------------------------------------------------------------------------------------------------
def test_header_declares_both_functions_without_an_abi_bump():
  with open(os.path.join(ROOT, 'include', 'msd_amd.h')) as f:
    header = f.read()
  assert re.search(r'\bint\s+msd_sample_keep\s*\(\s*msd_model\s*\*\s*m\s*,\s*int\s+batch\s*,\s*int\s+rng\s*,\s*int\s+per_row\s*,\s*'
                   r'const\s+uint64_t\s*\*\s*seeds\s*,\s*const\s+uint64_t\s*\*\s*stream_ids\s*,\s*const\s+float\s*\*\s*init_z_dev\s*,\s*'
                   r'const\s+float\s*\*\s*noise_dev\s*,\s*const\s+float\s*\*\s*known_dev\s*,\s*const\s+int32_t\s*\*\s*keep_mask\s*,\s*'
                   r'float\s*\*\s*out_dev\s*,\s*void\s*\*\s*stream\s*\)', header)
  assert re.search(r'\bint\s+msd_op_sampler_step_keep\s*\(\s*const\s+msd_config\s*\*\s*cfg\s*,', header)
  assert re.search(r'known_scaled_dev\s*,\s*const\s+int32_t\s*\*\s*keep_mask_dev\s*,\s*int\s+n_dims\s*,', header)
  assert 'msd_sample_keep' in native.EXPORTED_SYMBOLS and 'msd_op_sampler_step_keep' in native.EXPORTED_SYMBOLS
  assert re.search(r'#define\s+MSD_AMD_ABI_VERSION\s+7\b', header) and native.ABI_VERSION == 7
  assert callable(native.op_sampler_step_keep)


# --------------------------------------------------------------------------------------------------
# command line
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def midi(tmp_path_factory):
  from msd_amd.frontend import midi_io
  from tests.test_frontend_midi import _random_song
  path = tmp_path_factory.mktemp('keep') / 'a.mid'
  path.write_bytes(midi_io.note_sequence_to_midi(_random_song(9, seconds=3.0), ticks_per_quarter=500))
  return str(path)


BASE = ['--preset', 'tiny_context', '--num-steps', '4', '--on-too-long', 'truncate']


def _no_model(monkeypatch):
  monkeypatch.setattr(msd_amd, 'InferenceModel', lambda *a, **k: pytest.fail('a model was created'))


def test_region_in_seconds_maps_to_frames_rounded_outward():
  from msd_amd import synthesize
  rate = 16000 / 320   # 50 frames per second
  assert synthesize.region_frames('0.5:1.5', rate) == (25, 75)
  assert synthesize.region_frames('0.51:1.49', rate) == (25, 75)       # outward
  assert synthesize.region_frames('0.1:0.3', rate) == (5, 15)          # 0.1 * 50 and 0.3 * 50 are not exact in binary
  assert synthesize.region_frames('0:0.001', rate) == (0, 1)
  for bad in ['1.0', '2:1', '1:1', 'a:b', '-1:2', '1:2:3']:
    with pytest.raises(ValueError):
      synthesize.region_frames(bad, rate)


def test_cli_dry_run_prints_the_plan_without_a_model(midi, tmp_path, capsys, monkeypatch):
  from msd_amd import synthesize
  _no_model(monkeypatch)
  old = tmp_path / 'old.npy'
  np.save(old, np.zeros((240, 128), np.float32))   # the song lasts 4.8 s: 240 frames, four 64-frame segments
  assert synthesize.main([midi, *BASE, '--dry-run', '--edit-mel', str(old), '--regenerate', '0.8:2.0']) == 0
  out = capsys.readouterr().out
  assert 'regenerate frames [40, 100) of 256' in out and '2 of 4 segments' in out
  assert 'segment 0: frames [40, 64) sampled again, 40 of 64 kept' in out
  assert 'segment 1: frames [0, 36) sampled again, 28 of 64 kept' in out
  assert 'segment 2' not in out


def test_cli_dry_run_with_a_recording(midi, tmp_path, capsys, monkeypatch):
  from msd_amd import synthesize, vocoder
  _no_model(monkeypatch)
  wav = tmp_path / 'old.wav'
  vocoder.write_wav(str(wav), 0.1 * np.sin(np.arange(16000 * 3) / 20.0), 16000)
  assert synthesize.main([midi, *BASE, '--dry-run', '--edit-audio', str(wav), '--regenerate', '1.3:1.4']) == 0
  out = capsys.readouterr().out
  assert 'regenerate frames [65, 70) of 256' in out and 'segment 1: frames [1, 6) sampled again, 59 of 64 kept' in out


@pytest.mark.parametrize('extra, message', [
    (['--regenerate', '0.5:1.0'], 'needs the old rendering'),
    (['--regenerate', '0.5:1.0', '--edit-mel', 'OLD', '--edit-audio', 'x.wav'], 'give one'),
    (['--edit-mel', 'OLD'], '--regenerate START:STOP'),
    (['--regenerate', '4.0:5.5', '--edit-mel', 'OLD'], 'inside the song'),
    (['--regenerate', '2:1', '--edit-mel', 'OLD'], 'START < STOP'),
    (['--regenerate', '0.5:1.0', '--edit-mel', 'OLD', '--batch-segments', '2'], 'one by one'),
    (['--regenerate', '0.5:1.0', '--edit-mel', 'OLD', '--context-audio', 'x.wav'], 'one by one'),
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


def test_cli_pads_the_old_mel_and_edits_the_song(midi, tmp_path, monkeypatch):
  """Without --dry-run: the old mel reaches regenerate padded to whole segments with the codec's pad value, and --out
  gets the edited song cut to the MIDI file's length."""
  from msd_amd import synthesize
  calls = []

  def fake_model(checkpoint, spec, batch_size=1, **kw):
    m = _bare_model('tiny_context')

    def regenerate(song, segments, start, stop, **kw):
      calls.append(dict(song=song.clone(), n=len(segments), start=start, stop=stop, kw=kw))
      new = song.clone()
      new[:, start:stop] = 7.0
      return new
    m.regenerate = regenerate
    return m

  monkeypatch.setattr(msd_amd, 'InferenceModel', fake_model)
  old, out = tmp_path / 'old.npy', tmp_path / 'new.npy'
  mel = np.random.default_rng(1).uniform(-11, 4, (240, 128)).astype(np.float32)
  np.save(old, mel)
  assert synthesize.main([midi, *BASE, '--edit-mel', str(old), '--regenerate', '0.8:2.0', '--seed', '3', '--out', str(out)]) == 0
  c, = calls
  assert (c['n'], c['start'], c['stop']) == (4, 40, 100) and c['kw']['seed'] == 3 and c['kw']['return_torch']
  assert tuple(c['song'].shape) == (1, 256, 128)
  np.testing.assert_array_equal(c['song'][0, :240].numpy(), mel)
  assert (c['song'][0, 240:] == np.float32(np.log(1e-5))).all()
  new = np.load(out)
  assert new.shape == (240, 128) and (new[40:100] == 7.0).all()
  np.testing.assert_array_equal(new[:40], mel[:40])
  np.testing.assert_array_equal(new[100:], mel[100:])
