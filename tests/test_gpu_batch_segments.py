"""Per-row noise keys on the device (msd_sample_rows) and the batched segment driver on top of them: row b of a batched
call draws, bit for bit, what the one-row call (seed_b, segment_b) draws; independent segments then share one
msd_encode / msd_sample pair and stay on the float64 fixtures, at the bars the one-row runs are held to."""
import os

import numpy as np
import pytest

import msd_amd
from tests import helpers

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SEEDS, SEGMENTS = [42, 42, 7], [3, 9, 3]


def _twin_batch(spec, nb):
  """nb rows of model features whose rows 0 and 1 are the same segment (same tokens, same context)."""
  batch = helpers.make_batch(spec, batch=nb, ctx_mask='ones')
  for v in batch.values():
    v[1] = v[0]
  return batch


def _explicit_rows(rng, steps, seeds, segments, t):
  """init_z [B,T,n] and noise [N,B,T,n] written ROW BY ROW with the fill entry points over R = T * n elements: what
  the one-row calls (seed_b, segment_b) draw."""
  import torch
  from msd_amd import native
  nb = len(seeds)
  z = torch.empty((nb, t, 128), dtype=torch.float32, device='cuda')
  nz = torch.empty((steps, nb, t, 128), dtype=torch.float32, device='cuda')
  for b in range(nb):
    if rng == 'philox':
      native.fill_normal(z[b], seeds[b], segments[b], 0)
      for i in range(steps):
        native.fill_normal(nz[i, b], seeds[b], segments[b], 1 + i)
    else:
      native.fill_normal_threefry(z[b], seeds[b], fold=-1)
      for i in range(steps):
        native.fill_normal_threefry(nz[i, b], seeds[b], fold=i)
  torch.cuda.synchronize()
  return z, nz


@pytest.mark.parametrize('rng', ['philox', 'threefry'])
@pytest.mark.parametrize('preset,nb', [('tiny_context', 3), ('small', 2)])
def test_rows_draw_what_their_one_row_calls_draw_bit_identical(preset, nb, rng):
  steps = 7
  spec = msd_amd.config.preset(preset, num_steps=steps)
  t = spec.task_feature_lengths['targets']
  batch = _twin_batch(spec, nb)
  seeds, segments = SEEDS[:nb], SEGMENTS[:nb]
  model = msd_amd.InferenceModel('synthetic:1', spec, batch_size=nb)
  scalar_before, _ = model.predict(batch, seed=42, segment=3, rng=rng)   # the whole-array draw; graphs captured here
  got, _ = model.predict(batch, seed=seeds, segment=segments, rng=rng)
  z, nz = _explicit_rows(rng, steps, seeds, segments, t)
  want, _ = model.predict(batch, init_z=z, noise=nz)
  assert np.isfinite(got).all() and np.array_equal(got, want), np.abs(got - want).max()
  # a scalar beside a sequence is broadcast
  if len(set(seeds)) == 1:
    bc, _ = model.predict(batch, seed=seeds[0], segment=segments, rng=rng)
    assert np.array_equal(bc, got)
  # rows 0 and 1: same inputs, same seed, segments 3 and 9 -- Philox keys the stream by the segment, Threefry ignores it
  if rng == 'philox':
    assert helpers.rms(got[0], got[1]) > 0.05
  else:
    assert np.array_equal(got[0], got[1])
  same, _ = model.predict(batch, seed=seeds, segment=[3] * nb, rng=rng)   # equal keys, equal inputs
  assert np.array_equal(same[0], same[1])
  assert np.array_equal(same[0], got[0])                                   # and row 0 does not see its neighbours' keys
  if nb > 2:
    assert helpers.rms(got[0], got[2]) > 0.05                              # another seed (and other inputs)
  # the mode does not stick: the whole-array draw of a scalar call returns the same bits after a row-key call,
  # and is not the per-row draw
  scalar_after, _ = model.predict(batch, seed=42, segment=3, rng=rng)
  assert np.array_equal(scalar_before, scalar_after)
  assert helpers.rms(scalar_after[1], same[1]) > 0.05


def test_ddim_rows_take_their_own_init_z():
  import dataclasses
  import torch
  from msd_amd import native
  spec = msd_amd.config.preset('tiny', num_steps=5)
  d = spec.diffusion
  spec = dataclasses.replace(spec, diffusion=dataclasses.replace(d, sampler=dataclasses.replace(d.sampler, name='ddim')))
  t = spec.task_feature_lengths['targets']
  batch = _twin_batch(spec, 2)
  model = msd_amd.InferenceModel('synthetic:1', spec, batch_size=2)
  for rng in ('philox', 'threefry'):
    got, _ = model.predict(batch, seed=[42, 7], segment=[3, 3], rng=rng)
    z = torch.empty((2, t, 128), dtype=torch.float32, device='cuda')
    for b, sd in enumerate([42, 7]):
      if rng == 'philox':
        native.fill_normal(z[b], sd, 3, 0)
      else:
        native.fill_normal_threefry(z[b], sd, fold=-1)
    torch.cuda.synchronize()
    want, _ = model.predict(batch, init_z=z)
    assert np.isfinite(got).all() and np.array_equal(got, want), rng
    assert helpers.rms(got[0], got[1]) > 0.05


def test_jax_rows_are_the_one_row_host_draws():
  from msd_amd import jax_random
  steps = 3
  spec = msd_amd.config.preset('tiny', num_steps=steps)
  t = spec.task_feature_lengths['targets']
  batch = _twin_batch(spec, 3)
  model = msd_amd.InferenceModel('synthetic:1', spec, batch_size=3)
  got, _ = model.predict(batch, seed=[5, 5, 6], rng='jax')
  draws = {sd: jax_random.reference_noise(sd, (1, t, 128), steps) for sd in (5, 6)}
  z = np.concatenate([draws[sd][0] for sd in (5, 5, 6)], 0)
  nz = np.concatenate([draws[sd][1] for sd in (5, 5, 6)], 1)
  want, _ = model.predict(batch, init_z=z, noise=nz)
  assert np.array_equal(got, want) and np.array_equal(got[0], got[1])


def test_bad_row_key_arguments():
  import ctypes
  import torch
  spec = msd_amd.config.preset('tiny', num_steps=2)
  batch = _twin_batch(spec, 2)
  model = msd_amd.InferenceModel('synthetic:1', spec, batch_size=2)
  with pytest.raises(ValueError):
    model.predict(batch, seed=[1, 2, 3])
  nm = model._get_native()
  out = torch.empty((2, 64, 128), dtype=torch.float32, device='cuda')
  rc = nm.lib.msd_sample_rows(nm.handle, 2, 0, None, None, None, None, out.data_ptr(), 0)
  assert rc == 1   # MSD_ERR_INVALID_ARGUMENT: seeds is NULL
  seeds = (ctypes.c_uint64 * 2)(1, 2)
  assert nm.lib.msd_sample_rows(nm.handle, 2, 5, seeds, None, None, None, out.data_ptr(), 0) == 1   # unknown rng
  assert nm.lib.msd_sample_rows(nm.handle, 1, 0, seeds, None, None, None, out.data_ptr(), 0) == 1   # batch != encoded batch
  assert nm.lib.msd_sample_rows(nm.handle, 2, 1, seeds, None, None, None, out.data_ptr(), 0) == 0   # NULL stream_ids: Threefry


def test_small_four_segments_in_one_call_1000_steps():
  """`small`, the 4 fixture segments as ONE batched call with per-row keys against the float64 oracle's one-row runs:
  every row <= 1e-4 rms, the bar test_small_1000_steps_within_1e3_rms holds this model to at B = 1.  The sequential
  loop (batch_segments=1, the explicit-free path of the same keys) runs beside it."""
  g = np.load(os.path.join(GOLD, 'small_segments_n1000.npz'))
  n_seg, t = int(g['n_segments']), 256
  spec = msd_amd.config.preset('small', num_steps=1000)
  segs = [msd_amd.synthetic.segment_tokens(spec, k) for k in range(n_seg)]
  model = msd_amd.InferenceModel('synthetic:0', spec, batch_size=4)
  errs = {}
  for bs in (4, 1):
    got = model.predict_sequence(segs, seed=int(g['noise_seed']), batch_segments=bs)
    assert got.shape == (1, n_seg * t, 128)
    errs[bs] = [helpers.rms(got[:, k * t:(k + 1) * t], g['mel'][:, k * t:(k + 1) * t]) for k in range(n_seg)]
    print('small, 4 segments, 1000 steps, batch_segments=%d: rms vs float64 oracle per segment: %s'
          % (bs, ' '.join('%.3e' % e for e in errs[bs])))
  assert np.isfinite(errs[1]).all()
  assert max(errs[4]) <= 1e-4, errs


def test_base_with_context_four_rows_1000_steps():
  """base_with_context, segments (0, 1, 5, 11) of the 12-segment float64 fixture as ONE B = 4 call (128-row tiles, the
  persistent MLP-in loop, non-consecutive stream ids), each row on the fixture's previous segment as context and keyed
  (noise_seed, its segment): every row <= 1e-3 rms (north_star's bar; the B = 1 runs of
  test_base_with_context_every_segment_on_the_reference_context measure 0.57e-4 .. 0.87e-4)."""
  g = np.load(os.path.join(GOLD, 'base_chain_n1000.npz'))
  rows, t = (0, 1, 5, 11), 256
  assert int(g['n_segments']) >= 12
  spec = msd_amd.config.preset('base_with_context', num_steps=1000)
  mel = g['mel'].astype(np.float32)
  ctx = np.stack([np.zeros((t, 128), np.float32) if k == 0 else mel[0, (k - 1) * t:k * t] for k in rows])
  mask = np.stack([(np.zeros if k == 0 else np.ones)((t,), np.int32) for k in rows])
  batch = {'encoder_input_tokens': np.concatenate([msd_amd.synthetic.segment_tokens(spec, k) for k in rows], 0),
           'encoder_continuous_inputs': np.ascontiguousarray(ctx), 'encoder_continuous_mask': mask}
  model = msd_amd.InferenceModel('synthetic:0', spec, batch_size=4)
  got, _ = model.predict(batch, seed=int(g['noise_seed']), segment=list(rows))
  errs = [helpers.rms(got[j], g['mel'][0, k * t:(k + 1) * t]) for j, k in enumerate(rows)]
  print('base_with_context, segments %s in one B = 4 call, rms vs float64 oracle: %s (B = 1: 0.57e-4 .. 0.87e-4)'
        % (rows, ' '.join('%.2e' % e for e in errs)))
  assert max(errs) <= 1e-3, errs


def test_cli_batch_segments_writes_the_same_shape(tmp_path):
  from msd_amd import synthesize
  from msd_amd.frontend import midi_io
  from tests.test_frontend_midi import _random_song
  path = tmp_path / 'cli.mid'
  path.write_bytes(midi_io.note_sequence_to_midi(_random_song(9, seconds=12.0), ticks_per_quarter=500))
  shapes = {}
  for name, extra in (('loop', []), ('batched', ['--batch-segments', '3'])):
    out = tmp_path / (name + '.npy')
    assert synthesize.main([str(path), '--preset', 'small', '--num-steps', '4', '--out', str(out)] + extra) == 0
    shapes[name] = np.load(out).shape
    assert np.isfinite(np.load(out)).all()
  assert shapes['batched'] == shapes['loop'] and shapes['loop'][1] == 128 and shapes['loop'][0] > 2 * 256
