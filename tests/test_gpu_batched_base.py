"""-m gpu: batched CFG steps at the base model's real shapes against the float64 oracle.

One CFG step of base_with_context (num_steps = 1: predict runs exactly one step on the given init_z) for 2, 3, 4 and 8
songs per call.  Afterwards the handle's `eps` debug buffer holds the raw model outputs of both passes, [2][B][T][128]
(conditional rows first: sampler_step_kernel reads eps[idx] and eps[n + idx]); every song's two passes are held to
the float64 oracle (3e-4 max-rel: the bar tests/test_ref_golden.py holds the one-song base pass to) and to the same
song run alone on the same library (float32 rounding).  By the host's launch rules (msd_api.hip pick_tile,
cross_split, plan_step; attention.h attention_query_blocks) the batch sizes reach:
  B = 2   M = 1024  the folded cross-attention query projection on a CFG step (its upper limit), narrow tiles
  B = 3   M = 1536  fold off, narrow tiles, 128-row attention blocks for the cross- (key split 2) and the
                    self-attention of layers >= 1 (both passes in one launch)
  B = 4   M = 2048  128-row GEMM tiles, the persistent gated-MLP-in loop, 128-row attention blocks with key split 2
                    and the in-launch merge
  B = 8   M = 4096  the bench's batched configuration: 128-row attention blocks unsplit, several persistent tiles per CU
The songs mix the extreme cross key counts in every launch: the full 2046 tokens with a full context (2303 keys), 8
tokens without context (every key in the first part of a key split) and an all-padding song without context (no key
at all: the all-masked -> 0 rule inside a batched launch)."""
import time

import numpy as np
import pytest

import msd_amd
from tests import helpers

pytestmark = pytest.mark.gpu

N_SONGS = 8
F16_BAR = 3e-4        # against float64 (tests/test_ref_golden.py's one-song base pass)
BATCH_BAR = 2e-5      # against the same song alone (test_base_size_decoder_pass_does_not_depend_on_the_batch)


def _songs(spec):
  """8 fixed songs: [0] 2046 tokens + full context, [1] 8 tokens + no context, [2] all padding + no context, [3:] random
  lengths with ragged context masks."""
  rng = np.random.default_rng(2046)
  n_in, c, t = spec.task_feature_lengths['inputs'], spec.task_feature_lengths['targets_context'], \
      spec.task_feature_lengths['targets']
  toks = np.zeros((N_SONGS, n_in), np.int32)
  mask = np.zeros((N_SONGS, c), np.int32)
  toks[0, :n_in - 2] = rng.integers(3, 1391, n_in - 2)
  toks[0, n_in - 2] = 1
  mask[0] = 1
  toks[1, :8] = rng.integers(3, 1391, 8)
  toks[1, 8] = 1
  for j, ctx_len in zip(range(3, N_SONGS), (1, 255, 100, 17, 200)):
    toks[j] = msd_amd.synthetic.segment_tokens(spec, 300 + j, min_len=8, max_len=n_in - 2)[0]
    mask[j, :ctx_len] = 1
  batch = {'encoder_input_tokens': toks,
           'encoder_continuous_inputs': rng.uniform(-13, 5, (N_SONGS, c, 128)).astype(np.float32),
           'encoder_continuous_mask': mask,
           'decoder_target_tokens': np.zeros((N_SONGS, t, 128), np.float32)}
  init_z = rng.standard_normal((N_SONGS, t, 128)).astype(np.float32)
  return batch, init_z


def _first(batch, b):
  return {k: np.ascontiguousarray(v[:b]) for k, v in batch.items()}


@pytest.fixture(scope='module')
def base():
  """Spec, weights, songs and the float64 oracle's two passes per song (once for every batch size below)."""
  from oracle import backend, fast
  t0 = time.perf_counter()
  spec = msd_amd.config.preset('base_with_context', num_steps=1)
  params = msd_amd.synthetic.init_params(spec, 21, norm_scale_jitter=0.1)
  batch, init_z = _songs(spec)
  cfg, dc = helpers.oracle_configs(spec)
  xp = backend.TorchBackend('float64')
  fm = fast.FastModel(xp, cfg, dc, params, True)
  fm.encode(batch['encoder_input_tokens'], batch['encoder_continuous_inputs'], batch['encoder_continuous_mask'])
  ref = np.stack([xp.to_numpy(fm.decoder_pass(xp.asarray(init_z), 0, cond)).astype(np.float64) for cond in (True, False)])
  del fm
  print('\n[batched base] oracle: %d songs, both passes, %.1f s' % (N_SONGS, time.perf_counter() - t0))
  return spec, params, batch, init_z, ref   # ref [2 passes][song][T][128]


def _cfg_step(base, b, **kw):
  """One CFG step of songs [:b] in a handle of b songs -> its raw outputs [2 passes][b][T][128]."""
  import torch
  spec, params, batch, init_z, _ = base
  model = msd_amd.InferenceModel(params, spec, batch_size=b, **kw)
  out = []
  for j0 in range(0, N_SONGS if b == 1 else b, b):   # b = 1: every song alone, one after the other
    sub = {k: np.ascontiguousarray(v[j0:j0 + b]) for k, v in batch.items()}
    model.predict(sub, init_z=init_z[j0:j0 + b], noise=np.zeros((1, b, 256, 128), np.float32))
    out.append(model._get_native().debug_read('eps', 2 * b * 256 * 128).reshape(2, b, 256, 128))
  precision = model.precision
  del model
  torch.cuda.empty_cache()
  return np.concatenate(out, 1).astype(np.float64), precision


def _rel(got, want):
  return np.abs(got - want).max() / np.abs(want).max()


_alone = {}


def _alone_run(base, precision):
  """Every song alone (B = 1), same library, same step: the yardstick of the batched runs' float32 rounding."""
  if precision not in _alone:
    got, prec = _cfg_step(base, 1, precision=precision)
    assert prec == precision
    ref = base[4]
    errs = [[_rel(got[p, j], ref[p, j]) for j in range(N_SONGS)] for p in range(2)]
    print('[batched base] %s B = 1: max rel err vs float64 per song, cond: %s | uncond: %s'
          % (precision, ' '.join('%.1e' % e for e in errs[0]), ' '.join('%.1e' % e for e in errs[1])))
    _alone[precision] = got, max(max(e) for e in errs)
  return _alone[precision]


def test_eps_buffer_layout_is_both_passes_in_song_order(base):
  """The layout the tests below read: after a one-step predict at B = 1 the `eps` buffer holds the conditional pass in
  rows [0, T) and the unconditional one in [T, 2T) -- the same function as msd_decoder_pass of the same step."""
  import torch
  spec, params, batch, init_z, ref = base
  model = msd_amd.InferenceModel(params, spec, batch_size=1)
  nm = model._get_native()
  sub = _first(batch, 1)
  model.predict(sub, init_z=init_z[:1], noise=np.zeros((1, 1, 256, 128), np.float32))
  eps = nm.debug_read('eps', 2 * 256 * 128).reshape(2, 256, 128).astype(np.float64)
  z = torch.as_tensor(init_z[:1]).cuda()
  for p, cond in ((0, True), (1, False)):
    out = torch.zeros_like(z)
    nm.decoder_pass(1, 0, z, cond, out)
    torch.cuda.synchronize()
    single = out.cpu().numpy()[0].astype(np.float64)
    d = _rel(eps[p], single)
    print('[batched base] B = 1, %s pass: CFG step vs single decoder pass max rel %.1e, vs float64 %.1e'
          % ('cond' if cond else 'uncond', d, _rel(eps[p], ref[p, 0])))
    assert d < BATCH_BAR, (cond, d)
    assert _rel(eps[p], ref[p, 0]) < F16_BAR
  assert _rel(eps[0], eps[1]) > 1e-2   # the passes differ (song 0 has tokens and context)
  del model, nm
  torch.cuda.empty_cache()


@pytest.mark.parametrize('b', [2, 3, 4, 8])
def test_batched_cfg_step_matches_float64_and_the_song_alone(base, b):
  t0 = time.perf_counter()
  ref = base[4]
  alone, _ = _alone_run(base, 'f16x3')
  got, prec = _cfg_step(base, b)
  assert prec == 'f16x3'
  for p, name in enumerate(('cond', 'uncond')):
    e64 = [_rel(got[p, j], ref[p, j]) for j in range(b)]
    e1 = [_rel(got[p, j], alone[p, j]) for j in range(b)]
    print('[batched base] B = %d, %s: per song max rel err vs float64 %s | vs the song alone %s'
          % (b, name, ' '.join('%.1e' % e for e in e64), ' '.join('%.1e' % e for e in e1)))
    assert max(e64) < F16_BAR, (b, name, e64)
    assert max(e1) < BATCH_BAR, (b, name, e1)
  print('[batched base] B = %d: %.1f s' % (b, time.perf_counter() - t0))


def test_batched_variants_match_float64(base):
  """The other launch forms of the same songs: B = 8 with the per-tile 128 x 128 MLP-in launch (mlp_in_persistent
  off); B = 4 with the separate merge launch, BIT-identical to the in-launch merge (one merge function, as
  test_exact_launch_shortcuts_are_bit_identical asserts at <= 2 songs); B = 8 on bfloat16 planes ('bf16x3', the other
  library build: twice the rounding error of half planes), bounded by its own one-song error and never looser than
  twice the half-plane bar."""
  t0 = time.perf_counter()
  ref = base[4]
  default4, _ = _cfg_step(base, 4)
  runs = {'B = 8, per-tile MLP-in': _cfg_step(base, 8, mlp_in_persistent=False)[0],
          'B = 4, merge launch': _cfg_step(base, 4, cross_merge_in_launch=False)[0]}
  assert np.array_equal(runs['B = 4, merge launch'], default4), np.abs(runs['B = 4, merge launch'] - default4).max()
  alone_bf, bf_one = _alone_run(base, 'bf16x3')
  bf_bar = min(2 * F16_BAR, max(F16_BAR, 2 * bf_one))
  got, prec = _cfg_step(base, 8, precision='bf16x3')
  assert prec == 'bf16x3'
  runs['B = 8, bf16x3'] = got
  for name, got in runs.items():
    bar = bf_bar if 'bf16' in name else F16_BAR
    for p, pname in enumerate(('cond', 'uncond')):
      b = got.shape[1]
      e64 = [_rel(got[p, j], ref[p, j]) for j in range(b)]
      print('[batched base] %s, %s: per song max rel err vs float64 %s (bar %.1e)'
            % (name, pname, ' '.join('%.1e' % e for e in e64), bar))
      assert max(e64) < bar, (name, pname, e64)
  e1 = max(_rel(runs['B = 8, bf16x3'][p, j], alone_bf[p, j]) for p in range(2) for j in range(N_SONGS))
  print('[batched base] B = 8, bf16x3: max rel diff to the song alone %.1e; %.1f s' % (e1, time.perf_counter() - t0))
  assert e1 < 2 * BATCH_BAR, e1
