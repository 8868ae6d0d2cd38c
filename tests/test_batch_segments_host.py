"""Per-row noise keys and predict_sequence(batch_segments=), the parts that need no device: the ABI surface, the
grouping / keying / context rules of the batched segment driver on a stubbed predict, and the provenance of the
four-segment `small` fixture."""
import os
import re

import numpy as np
import pytest
import torch

from msd_amd import native
from tests import helpers
from tests.test_host_logic import _bare_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def test_header_declares_msd_sample_rows_without_an_abi_bump():
  with open(os.path.join(ROOT, 'include', 'msd_amd.h')) as f:
    header = f.read()
  assert re.search(r'\bint\s+msd_sample_rows\s*\(\s*msd_model\s*\*\s*m\s*,\s*int\s+batch\s*,\s*int\s+rng\s*,\s*'
                   r'const\s+uint64_t\s*\*\s*seeds\s*,\s*const\s+uint64_t\s*\*\s*stream_ids\s*,', header)
  assert 'msd_sample_rows' in native.EXPORTED_SYMBOLS
  assert re.search(r'#define\s+MSD_AMD_ABI_VERSION\s+7\b', header) and native.ABI_VERSION == 7


def test_row_keys_broadcasts_scalars_and_checks_lengths():
  assert native.row_keys(3, 5, [0, 1, 2]) == ([5, 5, 5], [0, 1, 2])
  assert native.row_keys(2, np.array([7, 8]), np.int64(4)) == ([7, 8], [4, 4])
  with pytest.raises(ValueError):
    native.row_keys(3, [1, 2], 0)


def _stub(m, seen, t=64):
  """predict stub: row j of the result is filled with its segment index + 1 (scalar or per-row segment alike)."""
  def fake_predict(batch, seed=0, segment=0, return_torch=False, **kw):
    b = np.asarray(batch['encoder_input_tokens']).shape[0]
    seen.append(dict(batch=batch, seed=seed, segment=segment, rows=b, kw=kw))
    segs = [segment] * b if np.isscalar(segment) else list(segment)
    out = torch.stack([torch.full((t, 128), float(s + 1)) for s in segs])
    return out, torch.zeros(b)
  m.predict = fake_predict


def _segments(n=5):
  return [np.full(128, k, np.int32) for k in range(n)]


@pytest.mark.parametrize('first', [0, 7])
def test_batched_groups_rows_keys_and_masked_context(first):
  m = _bare_model('tiny_context')
  m.batch_size = 2
  seen = []
  _stub(m, seen)
  full = m.predict_sequence(_segments(), seed=3, batch_segments=2, always_mask_context=True, first_segment_index=first)
  assert [c['rows'] for c in seen] == [2, 2, 1]
  assert [list(c['segment']) for c in seen] == [[first, first + 1], [first + 2, first + 3], [first + 4]]
  assert all(c['seed'] == 3 for c in seen)
  for g, c in enumerate(seen):
    b = c['rows']
    np.testing.assert_array_equal(np.asarray(c['batch']['encoder_input_tokens'])[:, 0], np.arange(2 * g, 2 * g + b))
    ctx, mask = c['batch']['encoder_continuous_inputs'], np.asarray(c['batch']['encoder_continuous_mask'])
    assert tuple(ctx.shape) == (b, 64, 128) and float(torch.as_tensor(ctx).abs().sum()) == 0.0
    assert mask.shape == (b, 64) and mask.dtype == np.int32 and not mask.any()
  # the same song through the sequential loop of the same stub
  seen_seq = []
  _stub(m, seen_seq)
  want = m.predict_sequence(_segments(), seed=3, always_mask_context=True, first_segment_index=first)
  assert full.shape == want.shape == (1, 5 * 64, 128)
  np.testing.assert_array_equal(full, want)
  np.testing.assert_array_equal(full[0, ::64, 0], first + 1 + np.arange(5))


def test_batch_segments_one_is_the_scalar_loop():
  m = _bare_model('tiny_context')
  seen = []
  _stub(m, seen)
  m.predict_sequence(_segments(3), seed=3, batch_segments=1, first_segment_index=2)
  assert [c['segment'] for c in seen] == [2, 3, 4] and all(np.isscalar(c['segment']) for c in seen)
  assert [c['rows'] for c in seen] == [1, 1, 1]
  assert [int(np.asarray(c['batch']['encoder_continuous_mask']).sum()) for c in seen] == [0, 64, 64]


def test_dependent_segments_are_refused():
  m = _bare_model('tiny_context')
  m.batch_size = 2
  _stub(m, [])
  with pytest.raises(ValueError, match='always_mask_context'):
    m.predict_sequence(_segments(), seed=3, batch_segments=2)
  with pytest.raises(ValueError, match='init_context'):
    m.predict_sequence(_segments(), seed=3, batch_segments=2, always_mask_context=True,
                       init_context=np.zeros((1, 64, 128), np.float32))
  with pytest.raises(ValueError):
    m.predict_sequence(_segments(), batch_segments=0)


def test_model_without_context_needs_no_flag_and_batch_size_bounds_it():
  m = _bare_model('tiny')
  m.batch_size = 3
  seen = []
  _stub(m, seen)
  full, timing = m.predict_sequence(_segments(), seed=1, batch_segments=3, return_timing=True)
  assert [c['rows'] for c in seen] == [3, 2] and full.shape == (1, 5 * 64, 128)
  assert all('encoder_continuous_inputs' not in c['batch'] for c in seen)
  assert timing['prediction_seconds_per_chunk'] >= 0.0   # one timed group (the first is left out)
  with pytest.raises(ValueError, match='batch_size'):
    m.predict_sequence(_segments(), seed=1, batch_segments=4)


def test_cli_refuses_a_dependent_combination_before_sampling(tmp_path, capsys, monkeypatch):
  """--batch-segments on a context preset without --always-mask-context: the ValueError's message, and no predict."""
  import msd_amd
  from msd_amd import synthesize
  from msd_amd.frontend import midi_io
  from tests.test_frontend_midi import _random_song   # the short song of the front-end tests

  path = tmp_path / 'a.mid'
  path.write_bytes(midi_io.note_sequence_to_midi(_random_song(9, seconds=3.0), ticks_per_quarter=500))
  built = []

  def fake_model(checkpoint, spec, batch_size=1, **kw):
    m = _bare_model('tiny_context')
    m.batch_size = batch_size
    built.append(m)
    m.predict = lambda *a, **k: pytest.fail('sampling started')
    return m

  monkeypatch.setattr(msd_amd, 'InferenceModel', fake_model)
  with pytest.raises(SystemExit):
    synthesize.main([str(path), '--preset', 'tiny_context', '--batch-segments', '2', '--num-steps', '4',
                     '--on-too-long', 'truncate'])
  assert built and built[0].batch_size == 2
  assert 'always_mask_context' in capsys.readouterr().err


def test_segment_fixture_continues_the_small_fixture():
  """small_segments_n1000.npz (tests/golden/make_batch_segments_golden.py) is make_golden.py's `small` case continued
  to four segments: its segment 0 is small_n1000.npz's mel."""
  g4 = np.load(os.path.join(GOLD, 'small_segments_n1000.npz'))
  g1 = np.load(os.path.join(GOLD, 'small_n1000.npz'))
  assert int(g4['n_segments']) == 4 and g4['mel'].shape == (1, 4 * 256, 128)
  assert int(g4['weight_seed']) == int(g1['weight_seed']) == 0 and int(g4['noise_seed']) == int(g1['noise_seed']) == 0
  assert helpers.rms(g4['mel'][:, :256], g1['mel']) <= 1e-9
  for k in range(1, 4):   # four different segments
    assert helpers.rms(g4['mel'][:, k * 256:(k + 1) * 256], g1['mel']) > 0.05
