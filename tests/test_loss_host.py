"""The denoising loss on the host (no GPU): the specification (tests/loss_spec.py) against the reference's own statements
(tests/golden/ref_loss_*.npz, made by tests/golden/make_ref_loss_golden.py), plan_loss_times, the argument errors of
InferenceModel.loss / NativeModel.loss in front of any library call, the binding and the CLI."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import msd_amd
from msd_amd import inference, native
from oracle import backend, fast
from tests import helpers, loss_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def _digest(params, batch, target, mask, eps):
  h = hashlib.sha256()
  for k in sorted(params):
    h.update(k.encode())
    h.update(np.ascontiguousarray(params[k]).tobytes())
  for k in sorted(batch):
    h.update(k.encode())
    h.update(np.ascontiguousarray(batch[k]).tobytes())
  for a in (target, mask, eps):
    h.update(np.ascontiguousarray(a).tobytes())
  return h.hexdigest()[:16]


# ---- the specification against the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', loss_spec.CASES)
def test_spec_reproduces_the_reference(name):
  """loss_spec in float64 == the reference's scale_features / diffusion_forward / module.apply / calculate_loss, per frame,
  for all 4 types x 2 norms at three indices and both conditioning forms: <= 1e-12 relative (the existing reference
  fixtures hold 4e-13)."""
  g = np.load(os.path.join(GOLD, 'ref_loss_%s.npz' % name))
  spec, params, batch, target, mask, eps, idx = loss_spec.case_inputs(name)
  assert _digest(params, batch, target, mask, eps) == str(g['digest']), \
      'seeded inputs changed: regenerate with tests/golden/make_ref_loss_golden.py'
  assert tuple(g['indices']) == tuple(idx) == (0, spec.diffusion.sampler.schedule.num_steps // 2,
                                               spec.diffusion.sampler.schedule.num_steps - 1)
  assert (mask[1, -19:] == 0).all() and mask.sum() == mask.size - 19
  cfg, dc = helpers.oracle_configs(spec)
  xp = backend.TorchBackend('float64', threads=1)
  fm = fast.FastModel(xp, cfg, dc, params, spec.has_context)
  loss_spec.encode(fm, batch)
  worst = 0.0
  for j, i in enumerate(idx):
    out = loss_spec.evaluate(xp, fm, dc, target, mask, eps[j], i)
    for cond in loss_spec.CONDITIONINGS:
      for lt in loss_spec.LOSS_TYPES:
        for ln in loss_spec.LOSS_NORMS:
          want = g[loss_spec.fixture_key(cond, lt, ln)][j]
          got = out[(cond, lt, ln)]
          assert got.shape == want.shape == mask.shape
          assert (got[1, -19:] == 0).all()   # masked frames: exactly zero
          rel = np.abs(got - want).max() / np.abs(want).max()
          worst = max(worst, rel)
          assert rel <= 1e-12, (name, i, cond, lt, ln, rel)
  print('%s: loss_spec float64 vs the reference, worst relative error %.2e' % (name, worst))


def test_spec_max_keeps_a_nan_and_types_relate():
  """max_x0_eps propagates NaN as jnp.maximum does; x0_and_eps is the sum of the two; the maximum is one of the two."""
  spec = msd_amd.config.preset('tiny', num_steps=8)
  _, dc = helpers.oracle_configs(spec)
  r = np.random.default_rng(0)
  z, o, x0, eps = (r.standard_normal((1, 4, 8)) for _ in range(4))
  mask = np.ones((1, 4))
  f = lambda lt, ln, oo=o: loss_spec.op_frame_losses('float64', dc, z, oo, x0, eps, mask, 3, 8, lt, ln)
  for ln in loss_spec.LOSS_NORMS:
    np.testing.assert_allclose(f('x0_and_eps', ln), f('x0', ln) + f('eps', ln), rtol=1e-13)
    assert (f('max_x0_eps', ln) <= f('x0', ln) + f('eps', ln)).all() and (f('max_x0_eps', ln) >= f('eps', ln) / 8).all()
  bad = o.copy()
  bad[0, 2, 5] = np.nan
  got = f('max_x0_eps', 'l1', bad)
  assert np.isnan(got[0, 2]) and np.isfinite(np.delete(got[0], 2)).all()


# ---- plan_loss_times ---------------------------------------------------------------------------------------------------
def test_plan_loss_times_grid():
  assert inference.plan_loss_times is native.plan_loss_times
  for n in (1, 3, 16, 24, 1000):
    assert native.plan_loss_times(n, n) == list(range(n))   # K = N: every index
    for k in {1, min(2, n), min(5, n), min(16, n), n}:
      idx = native.plan_loss_times(n, k)
      assert len(idx) == k and idx == [((2 * j + 1) * n) // (2 * k) for j in range(k)]
      assert all(0 <= i < n for i in idx) and all(b > a for a, b in zip(idx, idx[1:]))   # strictly increasing
  assert native.plan_loss_times(1000, 1) == [500] and native.plan_loss_times(16, 4) == [2, 6, 10, 14]
  assert native.plan_loss_times(16, np.int64(2)) == [4, 12]


def test_plan_loss_times_sequences():
  assert native.plan_loss_times(16, [15, 0, 7, 7]) == [15, 0, 7, 7]   # order and repeats are the caller's
  assert native.plan_loss_times(16, (3,)) == [3] and native.plan_loss_times(16, np.array([1, 2])) == [1, 2]


@pytest.mark.parametrize('bad', [0, -1, 17, True, 2.0, '4', None, [], [16], [-1], [1.0], [True], [0, 16]])
def test_plan_loss_times_refuses(bad):
  with pytest.raises(ValueError):
    native.plan_loss_times(16, bad)


def test_plan_loss_times_refuses_step_counts():
  for n in (0, -3, True, 2.5):
    with pytest.raises(ValueError, match='num_steps'):
      native.plan_loss_times(n, 1)


# ---- argument errors in front of the library ---------------------------------------------------------------------------
class _Lib:
  """Stands in for the loaded library: records the entry points that are called."""

  def __init__(self):
    self.calls = []

  def __getattr__(self, name):
    if not name.startswith('msd_'):
      raise AttributeError(name)

    def entry(*args):
      self.calls.append((name, args))
      return 0
    return entry


def _stub_native(num_steps=16):
  nm = object.__new__(native.NativeModel)
  nm.lib, nm.handle = _Lib(), 1
  nm.cfg = native.MsdConfig()
  nm.cfg.num_steps, nm.cfg.targets_length, nm.cfg.n_dims = num_steps, 64, 128
  return nm


class _T:
  """A tensor stand-in: a shape and a pointer."""

  def __init__(self, *shape):
    self.shape = shape

  def data_ptr(self):
    return 4096


def test_native_loss_fills_the_argument_struct():
  nm = _stub_native()
  nm.loss(2, _T(2, 64, 128), _T(3, 2, 2, 64), [15, 0, 15], seed=[3, 4], stream_id=7, rng='threefry', conditioning='both',
          loss_type='max_x0_eps', loss_norm='l2', mask=_T(2, 64))
  (name, a), = nm.lib.calls
  assert name == 'msd_loss' and a[0] == 1 and a[2] == 0
  s = ctypes.cast(a[1], ctypes.POINTER(native.LossArgs)).contents
  assert s.struct_size == ctypes.sizeof(native.LossArgs) == 88
  assert (s.batch, s.rng, s.per_row, s.n_times) == (2, native.RNGS['threefry'], 1, 3)
  assert [s.seeds[k] for k in range(2)] == [3, 4] and [s.stream_ids[k] for k in range(2)] == [7, 7]
  assert [s.times_host[k] for k in range(3)] == [15, 0, 15]
  assert (s.conditioning, s.loss_type, s.loss_norm) == (2, 2, 1)
  assert s.target_dev == s.mask_dev == s.out_dev == 4096 and s.eps_dev is None
  nm = _stub_native()
  nm.loss(1, _T(1, 64, 128), _T(1, 1, 1, 64), [5])   # the defaults: the spec's eps / l1, the conditional pass, one key
  s = ctypes.cast(nm.lib.calls[0][1][1], ctypes.POINTER(native.LossArgs)).contents
  assert (s.per_row, s.conditioning, s.loss_type, s.loss_norm, s.rng) == (0, 0, native.LOSS_TYPES['eps'], native.LOSS_NORMS['l1'], 0)
  assert s.mask_dev is None


def test_native_loss_refuses_before_the_library_is_called():
  tgt, out = _T(2, 64, 128), _T(2, 1, 2, 64)
  for args, kw, match in (((2, tgt, out, [0, 16]), {}, r'\[0, 16\)'), ((2, tgt, out, []), {}, 'empty'),
                          ((2, tgt, out, 0), {}, r'outside \[1, 16\]'),
                          ((2, tgt, out, [0, 1]), dict(rng='jax'), 'rng'),
                          ((2, tgt, out, [0, 1]), dict(conditioning='neither'), 'conditioning'),
                          ((2, tgt, out, [0, 1]), dict(loss_type='l1'), 'loss_type'),
                          ((2, tgt, out, [0, 1]), dict(loss_norm='eps'), 'loss norm'),
                          ((2, tgt, out, [0, 1]), dict(seed=[1, 2, 3]), 'entries'),
                          ((2, tgt, out, [0, 1]), dict(conditioning='both'), 'out must hold'),
                          ((2, _T(2, 64, 64), out, [0, 1]), {}, 'target must hold'),
                          ((2, tgt, out, [0, 1]), dict(mask=_T(2, 63)), 'mask must hold'),
                          ((2, tgt, out, [0, 1]), dict(eps=_T(1, 2, 64, 128)), 'eps must hold'),
                          ((2, None, out, [0, 1]), {}, 'target must hold')):
    nm = _stub_native()
    with pytest.raises(ValueError, match=match):
      nm.loss(*args, **kw)
    assert nm.lib.calls == [], (args, kw)


def test_inference_loss_refuses_before_any_device_work():
  """Every ValueError comes from loss()'s own checks: no handle is built (the object has none)."""
  m = object.__new__(inference.InferenceModel)
  m.spec = msd_amd.config.preset('tiny', num_steps=16)
  m.targets_length, m.audio_codec, m.rng = 64, msd_amd.audio_codecs.MelGAN(), 'philox'
  mel = np.zeros((2, 64, 128), np.float32)
  batch = {'encoder_input_tokens': np.zeros((2, 8), np.int32), 'decoder_target_tokens': mel}
  for b, kw, match in ((batch, dict(times=0), r'outside \[1, 16\]'), (batch, dict(times=17), r'outside \[1, 16\]'),
                       (batch, dict(times=[3, 16]), r'\[0, 16\)'), (batch, dict(times=True), 'bool'),
                       (batch, dict(rng='jax'), "not 'jax'"), (batch, dict(rng='mt19937'), 'rng'),
                       (batch, dict(conditioning='all'), 'conditioning'), (batch, dict(loss_type='huber'), 'loss_type'),
                       (batch, dict(loss_norm='l3'), 'loss norm'),
                       (batch, dict(eps=np.zeros((15, 2, 64, 128), np.float32)), 'eps must be'),
                       ({'encoder_input_tokens': batch['encoder_input_tokens']}, {}, 'decoder_target_tokens'),
                       (dict(batch, decoder_target_tokens=mel[:, :63]), {}, 'decoder_target_tokens must be'),
                       (dict(batch, decoder_target_mask=np.ones((2, 65))), {}, 'decoder_target_mask')):
    with pytest.raises(ValueError, match=match):
      m.loss(b, **kw)
  with pytest.raises(ValueError, match='song must be'):
    m.score_sequence(np.zeros((64, 128), np.float32), [np.zeros((8,), np.int32)])
  with pytest.raises(ValueError, match='segments of tokens'):
    m.score_sequence(np.zeros((1, 100, 128), np.float32), [np.zeros((8,), np.int32)])
  m.spec = msd_amd.config.preset('tiny', num_steps=16, cfg_weight=1.0)
  with pytest.raises(ValueError, match='weight != 1'):
    m.loss(batch, conditioning='both')


def test_header_and_binding_declare_the_new_entry_points():
  header = open(os.path.join(ROOT, 'include', 'msd_amd.h')).read()
  assert re.search(r'\bint\s+msd_loss\s*\(\s*msd_model\s*\*\s*m\s*,\s*const\s+msd_loss_args\s*\*', header)
  assert re.search(r'\bint\s+msd_op_diffusion_loss\s*\(\s*const\s+msd_config\s*\*', header)
  assert {'msd_loss', 'msd_op_diffusion_loss'} <= set(native.EXPORTED_SYMBOLS)
  assert callable(native.op_diffusion_loss) and callable(native.NativeModel.loss)
  assert 'MSD_AMD_ABI_VERSION 7' in header   # appended: the version stays
  # the struct, field for field: the header's order is the binding's
  body = re.search(r'typedef struct msd_loss_args \{(.*?)\} msd_loss_args;', header, re.S).group(1)
  fields = re.findall(r'(\w+);', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
  assert fields == [f[0] for f in native.LossArgs._fields_]
  for names, table in ((('MSD_LOSS_COND', 'MSD_LOSS_UNCOND', 'MSD_LOSS_BOTH'), native.LOSS_CONDITIONINGS),
                       (('MSD_LOSS_X0', 'MSD_LOSS_EPS', 'MSD_LOSS_MAX_X0_EPS', 'MSD_LOSS_X0_AND_EPS'), native.LOSS_TYPES),
                       (('MSD_LOSS_L1', 'MSD_LOSS_L2'), native.LOSS_NORMS)):
    values = [int(re.search(r'\b%s = (\d+)' % n, header).group(1)) for n in names]
    assert sorted(values) == sorted(table.values()) == list(range(len(names)))


# ---- the CLI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def midi(tmp_path_factory):
  from msd_amd.frontend import midi_io
  from tests.test_frontend_midi import _random_song
  path = tmp_path_factory.mktemp('loss') / 'a.mid'
  path.write_bytes(midi_io.note_sequence_to_midi(_random_song(9, seconds=3.0), ticks_per_quarter=500))
  return str(path)


def test_cli_score_arguments(midi, tmp_path, capsys):
  from msd_amd import synthesize
  base = ['--preset', 'tiny_context', '--num-steps', '16', '--on-too-long', 'truncate', '--dry-run']
  good = str(tmp_path / 'mel.npy')
  np.save(good, np.zeros((40, 128), np.float32))
  assert synthesize.main([midi, *base, '--score', good, '--score-times', '8', '--score-conditioning', 'both']) == 0
  capsys.readouterr()
  narrow, long_ = str(tmp_path / 'narrow.npy'), str(tmp_path / 'long.npy')
  np.save(narrow, np.zeros((40, 64), np.float32))
  np.save(long_, np.zeros((100000, 128), np.float32))
  for extra, word in ((['--score', good, '--score-audio', 'x.wav'], 'give one'),
                      (['--score', good, '--out', 'o.npy'], 'no --out'),
                      (['--score', good, '--wav', 'o.wav'], 'no --out'),
                      (['--score', good, '--vary', '0.5', '--edit-mel', good], 'do not go with'),
                      (['--score', good, '--steps', '8'], 'sample nothing'),
                      (['--score', good, '--guidance', '2'], 'sample nothing'),
                      (['--score', good, '--rng', 'jax'], 'philox or threefry'),
                      (['--score', good, '--score-times', '0'], 'outside [1, 16]'),
                      (['--score', good, '--score-times', '17'], 'outside [1, 16]'),
                      (['--score', good, '--score-conditioning', 'both', '--cfg-weight', '1'], 'one pass'),
                      (['--score-times', '8'], 'go with --score'),
                      (['--score-conditioning', 'uncond'], 'go with --score'),
                      (['--score', narrow], 'must hold mel frames'),
                      (['--score', long_], 'frames, the MIDI file only'),
                      (['--score', str(tmp_path / 'missing.npy')], 'missing.npy')):
    with pytest.raises(SystemExit) as e:
      synthesize.main([midi, *base, *extra])
    assert e.value.code == 2 and word in capsys.readouterr().err, extra


def test_cli_scores_through_score_sequence(midi, tmp_path, monkeypatch, capsys):
  import json
  import torch
  from msd_amd import synthesize
  seen = {}

  class Model:
    def __init__(self, *a, **k):
      self.targets_context_length, self._torch, self.device = 64, torch, 'cpu'
      self.audio_codec = msd_amd.audio_codecs.MelGAN()

    def score_sequence(self, song, segments, **kw):
      seen.update(kw, frames=int(song.shape[1]), segments=len(segments), tail=float(song[0, -1, 0]))
      k = len(segments)
      return {'per_frame': np.ones((1, 64 * k)), 'per_segment': np.arange(k, dtype=np.float64)[None], 'loss': np.array([k * (k - 1) / 2.0]),
              'times': [1, 5, 9, 13]}
  monkeypatch.setattr(msd_amd, 'InferenceModel', Model)
  mel = str(tmp_path / 'mel.npy')
  np.save(mel, np.ones((70, 128), np.float32))
  assert synthesize.main([midi, '--preset', 'tiny_context', '--num-steps', '16', '--on-too-long', 'truncate', '--score', mel,
                          '--score-times', '4', '--score-conditioning', 'uncond', '--seed', '3']) == 0
  out = json.loads(capsys.readouterr().out)
  assert seen['times'] == 4 and seen['conditioning'] == 'uncond' and seen['seed'] == 3
  assert seen['frames'] == 64 * seen['segments'] and seen['tail'] == pytest.approx(msd_amd.audio_codecs.MelGAN().pad_value)
  assert out['frames'] == 70 and out['segments'] == seen['segments'] and out['times'] == [1, 5, 9, 13]
  assert out['loss_given_frames'] == {'uncond': 70.0}   # the sum without the padding's frames
  assert out['per_segment'] == {'uncond': [float(k) for k in range(seen['segments'])]} and list(out['loss']) == ['uncond']
