"""-m gpu: the whole path through the C-ABI (encode, tables, one decoder pass,
the sampler loop, predict, predict_sequence) against the oracle on seeded inputs.

Tolerances.  Integer/byte data (schedule indices, masks) are exact.  Floating
point follows BASELINE.json's bar -- mel frames within 1e-3 rms -- read this way:
short DDPM chains are ill-conditioned (helpers.assert_fp32_class explains why), so
they compare bulk error and outlier count against the float32 oracle's own deviation
from float64; the 1000-step runs (tests/test_golden.py) use the absolute 1e-3 rms bar."""
import numpy as np
import pytest

import msd_amd
from tests import helpers

pytestmark = pytest.mark.gpu


def _oracle(spec, params, batch, init_z, noise, dtype='float64', precision='f32', trace=None):
  from oracle import backend, fast
  cfg, dc = helpers.oracle_configs(spec)
  xp = backend.TorchBackend(dtype)
  fm = fast.FastModel(xp, cfg, dc, params, spec.has_context, precision=precision)
  out = fm.predict(batch, init_z, noise, trace=trace)[0]
  return xp.to_numpy(out).astype(np.float64), fm


@pytest.fixture(scope='module')
def tiny_ctx():
  import torch
  assert torch.cuda.is_available()
  spec = msd_amd.config.preset('tiny_context', num_steps=6)
  params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
  model = msd_amd.InferenceModel(params, spec, batch_size=2, **helpers.ALL_PLANES)   # short-chain statistics: helpers.ALL_PLANES
  return spec, params, model


def test_schedule_table_matches_oracle(tiny_ctx):
  spec, params, model = tiny_ctx
  from oracle import backend, sampler
  sched = model._get_native().schedule()
  n = spec.diffusion.sampler.schedule.num_steps
  xp = backend.NumpyBackend('float32')
  i = np.arange(n, dtype=np.float32)
  cos = sampler.DiffusionSchedule('cosine', num_steps=n)
  lt = sampler.get_logsnr_t(xp, (i + 1) / np.float32(n), cos)
  ls = sampler.get_logsnr_t(xp, i / np.float32(n), cos)
  np.testing.assert_allclose(sched[:, 0], lt, atol=3e-5)
  np.testing.assert_allclose(sched[:, 1], ls, atol=3e-5)
  rev = sampler.diffusion_reverse(backend.NumpyBackend('float64'), x0=np.ones(n), z_t=np.zeros(n),
                                  logsnr_s=ls.astype(np.float64), logsnr_t=lt.astype(np.float64),
                                  logvar_type='large')
  np.testing.assert_allclose(sched[:, 5], rev['mean'], rtol=2e-4, atol=1e-7)   # (1-r) alpha_s
  np.testing.assert_allclose(sched[:, 6], rev['std'], rtol=2e-4, atol=1e-7)


def test_film_table_matches_oracle(tiny_ctx):
  """FiLM scale/bias table = sinusoid(t*2e4) -> Dense -> swish -> Dense -> swish -> Dense, all fp32
  (network.py:377-392, layers.py:660-665).  The float32 time signal is intrinsically
  implementation-sensitive: scaled_time reaches 2e4 rad, so one ulp of exp() in
  inv_timescales moves sin/cos by ~1e-3 in the highest-frequency channels (true of the
  reference across XLA backends as well) -- hence the looser bound on this table."""
  spec, params, model = tiny_ctx
  from oracle import backend, fast
  cfg, dc = helpers.oracle_configs(spec)
  n, ld, d = dc.sampler.schedule.num_steps, cfg.num_decoder_layers, cfg.emb_dim
  film = model._get_native().debug_read('film').reshape(n, 2 * ld, 2 * d)
  for dt, tol in (('float32', 2e-3), ('float64', 5e-3)):
    fm = fast.FastModel(backend.NumpyBackend(dt), cfg, dc, params, True)
    worst = max(float(np.abs(film[:, 2 * l + k] - fm.film[l][k]).max())
                for l in range(ld) for k in range(2))
    print('film table max abs diff vs %s oracle: %.3e' % (dt, worst))
    assert worst < tol


@pytest.fixture(scope='module')
def tiny_ctx_default(tiny_ctx):
  """The same model with the OPT-IN single query-side plane (Q and the softmax weights of the decoder's attentions as
  one half plane each: round 3's default); `tiny_ctx` is the product's default = all planes."""
  spec, params, _ = tiny_ctx
  return msd_amd.InferenceModel(params, spec, batch_size=2, **helpers.ONE_QUERY_PLANE)


@pytest.mark.parametrize('attention', ['default', 'one query-side plane'])
@pytest.mark.parametrize('mask', ['ones', 'zeros', 'ragged'])
def test_encode_and_single_decoder_pass(tiny_ctx, tiny_ctx_default, mask, attention):
  import torch
  spec, params, model = tiny_ctx
  if attention != 'default':
    model = tiny_ctx_default
  nm = model._get_native()
  batch = helpers.make_batch(spec, batch=2, ctx_mask=mask)
  ref_out, fm = None, None
  from oracle import backend, fast
  cfg, dc = helpers.oracle_configs(spec)
  xp = backend.NumpyBackend('float64')
  fm = fast.FastModel(xp, cfg, dc, params, True)
  fm.encode(batch['encoder_input_tokens'], batch['encoder_continuous_inputs'],
            batch['encoder_continuous_mask'])
  ctx = torch.as_tensor(batch['encoder_continuous_inputs']).cuda()
  nm.encode(2, batch['encoder_input_tokens'], ctx, batch['encoder_continuous_mask'])
  z = np.random.default_rng(0).standard_normal((2, 64, 128)).astype(np.float32)
  zd = torch.as_tensor(z).cuda()
  for step, cond in [(5, True), (2, True), (0, False), (3, False)]:
    eps = torch.zeros_like(zd)
    nm.decoder_pass(2, step, zd, cond, eps)
    torch.cuda.synchronize()
    want = fm.decoder_pass(z.astype(np.float64), step, cond)
    err = np.abs(eps.cpu().numpy() - want).max() / np.abs(want).max()
    assert err < 2e-4, (mask, step, cond, err)  # fp32-class (bf16 operands would give ~1e-2)


def test_predict_explicit_noise_matches_oracle(tiny_ctx):
  spec, params, model = tiny_ctx
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  init_z, noise = helpers.make_noise(spec, batch=2)
  got, scores = model.predict(batch, init_z=init_z, noise=noise)
  ref64, _ = _oracle(spec, params, batch, init_z, noise, 'float64')
  ref32, _ = _oracle(spec, params, batch, init_z, noise, 'float32')
  assert got.dtype == np.float32 and got.shape == (2, 64, 128)
  assert scores.shape == (2,) and not scores.any()
  helpers.assert_fp32_class(got, ref64, ref32, 'predict')


def test_predict_seed_uses_documented_philox(tiny_ctx):
  spec, params, model = tiny_ctx
  from oracle import philox
  batch = helpers.make_batch(spec, batch=1)
  got, _ = model.predict(batch, seed=42, segment=3)
  init_z, noise = philox.segment_noise((1, 64, 128), 6, seed=42, segment=3)
  again, _ = model.predict(batch, init_z=init_z, noise=noise)
  # same Philox bits in; the draws differ by transcendental ulps (device vs NumPy log/sin/cos, 1e-6
  # level: tests/test_gpu_ops.py pins that), which a 6-step chain amplifies on the few clip-marginal
  # elements only: the bulk must agree to 1e-5 and fewer than 0.1 % of the elements may move by > 1e-2
  e = np.abs(got.astype(np.float64) - again).ravel()
  print('philox seed vs explicit draws: median %.2e, >1e-2: %.5f, rms %.2e' % (np.median(e), (e > 1e-2).mean(), helpers.rms(got, again)))
  assert np.median(e) < 1e-5 and (e > 1e-2).mean() < 1e-3
  same, _ = model.predict(batch, seed=42, segment=3)
  np.testing.assert_array_equal(got, same)                       # deterministic
  other, _ = model.predict(batch, seed=43, segment=3)
  assert helpers.rms(got, other) > 0.1


def test_cfg_weight_one_and_ddim_and_no_context_model():
  import torch
  for preset, kw in [('tiny_context', dict(cfg_weight=1.0)), ('tiny', dict(cfg_weight=5.0))]:
    spec = msd_amd.config.preset(preset, num_steps=5, **kw)
    params = msd_amd.synthetic.init_params(spec, 9, norm_scale_jitter=0.1)
    model = msd_amd.InferenceModel(params, spec, **helpers.ALL_PLANES)
    batch = helpers.make_batch(spec)
    init_z, noise = helpers.make_noise(spec)
    got, _ = model.predict(batch, init_z=init_z, noise=noise)
    ref64, _ = _oracle(spec, params, batch, init_z, noise, 'float64')
    ref32, _ = _oracle(spec, params, batch, init_z, noise, 'float32')
    helpers.assert_fp32_class(got, ref64, ref32, preset)
  # DDIM switch (diffusion_utils.py:369-379)
  import dataclasses
  spec = msd_amd.config.preset('tiny_context', num_steps=5)
  d = spec.diffusion
  spec = dataclasses.replace(spec, diffusion=dataclasses.replace(
      d, sampler=dataclasses.replace(d.sampler, name='ddim')))
  params = msd_amd.synthetic.init_params(spec, 9)
  model = msd_amd.InferenceModel(params, spec, **helpers.ALL_PLANES)
  batch = helpers.make_batch(spec)
  init_z, _ = helpers.make_noise(spec)
  got, _ = model.predict(batch, init_z=init_z)
  ref64, _ = _oracle(spec, params, batch, init_z, None, 'float64')
  ref32, _ = _oracle(spec, params, batch, init_z, None, 'float32')
  helpers.assert_fp32_class(got, ref64, ref32, 'ddim')


@pytest.mark.parametrize('prec,tol', [('f16', 5e-3), ('bf16', 3e-2)])
def test_single_plane_mode_is_close_to_its_emulation(tiny_ctx, prec, tol):
  """The fast non-parity mode (one half plane per operand): checked against the oracle's 'f16'
  emulation on one decoder pass (a full chain in it is chaotic by design of the test config)."""
  import torch
  spec, params, _ = tiny_ctx
  model = msd_amd.InferenceModel(params, spec, precision=prec)
  nm = model._get_native()
  batch = helpers.make_batch(spec)
  from oracle import backend, fast
  cfg, dc = helpers.oracle_configs(spec)
  xp = backend.TorchBackend('float32')
  fm = fast.FastModel(xp, cfg, dc, params, True, precision=prec)
  fm.encode(batch['encoder_input_tokens'], batch['encoder_continuous_inputs'],
            batch['encoder_continuous_mask'])
  nm.encode(1, batch['encoder_input_tokens'], torch.as_tensor(batch['encoder_continuous_inputs']).cuda(),
            batch['encoder_continuous_mask'])
  z = np.random.default_rng(0).standard_normal((1, 64, 128)).astype(np.float32)
  eps = torch.zeros((1, 64, 128), device='cuda')
  nm.decoder_pass(1, 3, torch.as_tensor(z).cuda(), True, eps)
  torch.cuda.synchronize()
  want = xp.to_numpy(fm.decoder_pass(xp.asarray(z), 3, True))
  assert np.abs(eps.cpu().numpy() - want).max() / np.abs(want).max() < tol


def test_predict_sequence_matches_oracle_song(tiny_ctx):
  spec, params, model = tiny_ctx
  from oracle import backend, philox, predict
  cfg, dc = helpers.oracle_configs(spec)
  segs = [msd_amd.synthetic.segment_tokens(spec, k, min_len=8, max_len=100) for k in range(3)]
  got = model.predict_sequence(segs, seed=5)
  assert got.shape == (1, 192, 128)
  zs, ns = zip(*[philox.segment_noise((1, 64, 128), 6, seed=5, segment=k) for k in range(3)])
  outs = {}
  for dt in ('float64', 'float32'):
    xp = backend.TorchBackend(dt)
    outs[dt] = predict.predict_song(xp, cfg, dc, params, segs, zs, ns, context_length=64)
  # (device Philox vs NumPy Philox differ by transcendental ulps; chained through 3 segments)
  helpers.assert_fp32_class(got, outs['float64'], outs['float32'], 'song (3 chained segments)')
  masked = model.predict_sequence(segs, seed=5, always_mask_context=True)
  np.testing.assert_array_equal(masked[:, :64], got[:, :64])   # segment 0 identical
  assert helpers.rms(masked[:, 64:], got[:, 64:]) > 1e-3        # context matters afterwards


def test_error_paths(tiny_ctx):
  spec, params, model = tiny_ctx
  nm = model._get_native()
  batch = helpers.make_batch(spec)
  bad = dict(batch)
  bad['encoder_input_tokens'] = batch['encoder_input_tokens'][:, :5]
  with pytest.raises(ValueError):
    model.predict(bad)
  bad = dict(batch)
  bad['encoder_input_tokens'] = batch['encoder_input_tokens'].astype(np.float32)
  with pytest.raises(ValueError, match='Input type must be an integer'):   # layers_test.py:392-401
    model.predict(bad)
  bad = dict(batch)
  bad['encoder_input_tokens'] = batch['encoder_input_tokens'] + 100000
  with pytest.raises(ValueError):
    model.predict(bad)
  with pytest.raises(KeyError):
    nm.set_weight('decoder/not_a_weight', np.zeros(3, np.float32))
  with pytest.raises(ValueError):
    nm.set_weight('decoder/decoder_norm/scale', np.zeros(7, np.float32))
  fresh = msd_amd.native.NativeModel(msd_amd.inference._to_native_config(
      spec, model.audio_codec, 1, 'bf16x3'))
  with pytest.raises(RuntimeError):
    fresh.encode(1, batch['encoder_input_tokens'])
  # half-precision operand planes hold |w| < 128: a projection weight outside fails loudly at load time
  big = dict(params)
  k = 'decoder/layers_0/mlp/wo/kernel'
  big[k] = params[k].copy()
  big[k][3, 5] = 200.0
  with pytest.raises(NotImplementedError, match='magnitude'):
    msd_amd.InferenceModel(big, spec)._get_native()


def test_empty_inputs_give_unconditional_result(tiny_ctx):
  """All-PAD tokens + masked context: no key anywhere -> cross-attention is exactly
  zero for the conditional pass too (layers.py:882-902), so CFG collapses."""
  spec, params, model = tiny_ctx
  batch = helpers.make_batch(spec, ctx_mask='zeros')
  batch['encoder_input_tokens'] = np.zeros_like(batch['encoder_input_tokens'])
  init_z, noise = helpers.make_noise(spec)
  got, _ = model.predict(batch, init_z=init_z, noise=noise)
  ref64, _ = _oracle(spec, params, batch, init_z, noise, 'float64')
  ref32, _ = _oracle(spec, params, batch, init_z, noise, 'float32')
  assert np.isfinite(got).all()
  helpers.assert_fp32_class(got, ref64, ref32, 'empty')


def test_batched_songs_use_big_tiles_and_match_oracle():
  """16 songs per handle: M = 2*16*64 = 2048 rows -> the 128-row GEMM tiles of the batched
  path (msd_api.hip big_m_threshold).  emb 192 / 3 heads / mlp 256 make every N a multiple of the
  96/128-column tiles so all big instantiations run; checked per song against the oracle.
  (The rejected alternative tiles of the experiments build run the same test: tests/frozen/gpu_experiments_r04.py.)"""
  import dataclasses
  base = msd_amd.config.preset('tiny_context', num_steps=4)
  spec = dataclasses.replace(base, t5=dataclasses.replace(base.t5, emb_dim=192, num_heads=3))
  params = msd_amd.synthetic.init_params(spec, 5, norm_scale_jitter=0.1)
  B = 16
  model = msd_amd.InferenceModel(params, spec, batch_size=B, **helpers.ALL_PLANES)
  batch = helpers.make_batch(spec, batch=B, ctx_mask='ragged')
  init_z, noise = helpers.make_noise(spec, batch=B)
  got, _ = model.predict(batch, init_z=init_z, noise=noise)
  ref64, _ = _oracle(spec, params, batch, init_z, noise, 'float64')
  ref32, _ = _oracle(spec, params, batch, init_z, noise, 'float32')
  helpers.assert_fp32_class(got, ref64, ref32, what='batched B=16')
  # round 6: the gated-MLP input projection of that run was the PERSISTENT tile loop with the register epilogue
  # (msd_config.mlp_in_persistent, gemm_h16.h gemm_h16_geglu_persist_kernel: M = 2048 rows of 128 x 128 tiles, several per
  # block at this size); the per-tile launch it replaces must land in the same class -- same function, another
  # contraction of the epilogue's multiply-adds
  plain = msd_amd.InferenceModel(params, spec, batch_size=B, mlp_in_persistent=False, **helpers.ALL_PLANES)
  got_plain, _ = plain.predict(batch, init_z=init_z, noise=noise)
  helpers.assert_fp32_class(got_plain, ref64, ref32, what='batched B=16, per-tile MLP-in launch')
  d = np.asarray(got, np.float64) - np.asarray(got_plain, np.float64)
  print('batched B=16: persistent vs per-tile MLP-in: median |diff| %.2e, max %.2e' % (np.median(np.abs(d)), np.abs(d).max()))
  assert np.median(np.abs(d)) < 1e-5
  del plain
  # and one decoder pass, elementwise (no chaotic amplification)
  import torch
  from oracle import backend, fast
  cfg, dc = helpers.oracle_configs(spec)
  fm = fast.FastModel(backend.NumpyBackend('float64'), cfg, dc, params, True)
  fm.encode(batch['encoder_input_tokens'], batch['encoder_continuous_inputs'], batch['encoder_continuous_mask'])
  nm = model._get_native()
  z = np.random.default_rng(1).standard_normal((B, 64, 128)).astype(np.float32)
  zd = torch.as_tensor(z).cuda()
  for step, cond in [(3, True), (1, False)]:
    eps = torch.zeros_like(zd)
    nm.decoder_pass(B, step, zd, cond, eps)
    torch.cuda.synchronize()
    want = fm.decoder_pass(z.astype(np.float64), step, cond)
    err = np.abs(eps.cpu().numpy() - want).max() / np.abs(want).max()
    assert err < 2e-4, (step, cond, err)


def test_midi_in_synthesis(tiny_ctx, tmp_path):
  """MIDI file -> tokens (front end) -> chained segments on the device; equal to
  feeding the same tokens by hand, and to the oracle song on those tokens."""
  import dataclasses
  from msd_amd.frontend import midi_io, note_sequences
  base = tiny_ctx[0]                        # tiny shapes, but the real 1536-entry MT3 vocabulary
  spec = dataclasses.replace(base, t5=dataclasses.replace(base.t5, vocab_size=1536))
  params = msd_amd.synthetic.init_params(spec, 4, norm_scale_jitter=0.1)
  model = msd_amd.InferenceModel(params, spec, **helpers.ALL_PLANES)
  ns = note_sequences.NoteSequence()
  for k, (p, prog) in enumerate([(60, 0), (64, 0), (67, 40), (72, 40), (55, 0)]):
    ns.add_note(pitch=p, velocity=90, start_time=0.3 * k, end_time=0.3 * k + 1.1, program=prog)
  ns.add_note(pitch=36, velocity=100, start_time=2.0, end_time=2.1, is_drum=True)
  ns.total_time = 2.4                      # tiny model: 64 frames = 1.28 s per segment -> 2 segments
  path = tmp_path / 'tiny.mid'
  path.write_bytes(midi_io.note_sequence_to_midi(ns, ticks_per_quarter=500))
  toks = model.tokenize_note_sequence(midi_io.midi_file_to_note_sequence(str(path)))
  assert len(toks) == 2 and toks[0].shape == (1, spec.task_feature_lengths['inputs'])
  a = model.synthesize_midi(str(path), seed=3)
  b = model.predict_sequence(toks, seed=3)
  assert a.shape == (1, 2 * 64, 128) and np.array_equal(a, b)
  assert np.isfinite(a).all() and a.std() > 0.1


def test_rng_jax_mode_uses_reference_draws(tiny_ctx):
  """rng='jax': the draws of jax.random for PRNGKey(seed) (jax_random.py), independent of `segment`."""
  from msd_amd import jax_random
  spec, params, model = tiny_ctx
  batch = helpers.make_batch(spec, batch=1)
  got, _ = model.predict(batch, seed=5, segment=0, rng='jax')
  z, nz = jax_random.reference_noise(5, (1, 64, 128), spec.diffusion.sampler.schedule.num_steps)
  want, _ = model.predict(batch, init_z=z, noise=nz)
  assert np.array_equal(got, want)
  again, _ = model.predict(batch, seed=5, segment=3, rng='jax')       # the reference ignores the segment
  assert np.array_equal(got, again)
  other, _ = model.predict(batch, seed=6, rng='jax')
  assert not np.array_equal(got, other)
  with pytest.raises(ValueError):
    model.predict(batch, rng='mt19937')


@pytest.mark.parametrize('split', [0, 1, 2, 4, 8])
@pytest.mark.parametrize('valid', [1, 130, 1022])
def test_key_split_cross_attention_edge_lengths(valid, split):
  """inputs 1024 + context 64 -> S_pad >= 1024 -> the key-split cross-attention (`split` blocks per query
  group + merge; 0 = the library's per-segment choice, the others through msd_config.cross_key_split: every split the
  launcher can choose is tested, round 5).  Key counts at the extremes: blocks with NO stage of their own (1 valid
  token, with and without context keys), a ragged last stage, a full key axis.  Single decoder passes against the
  float64 oracle, elementwise (a short sampling chain would only add its own chaos, helpers.py)."""
  import dataclasses
  import torch
  from oracle import backend, fast
  base = msd_amd.config.preset('tiny_context', num_steps=3)
  spec = dataclasses.replace(base, task_feature_lengths={'inputs': 1024, 'targets': 64, 'targets_context': 64})
  params = msd_amd.synthetic.init_params(spec, 6, norm_scale_jitter=0.1)
  model = msd_amd.InferenceModel(params, spec, cross_key_split=split, **helpers.ALL_PLANES)
  nm = model._get_native()
  cfg, dc = helpers.oracle_configs(spec)
  z = np.random.default_rng(0).standard_normal((1, 64, 128)).astype(np.float32)
  zd = torch.as_tensor(z).cuda()
  for mask in ('ragged', 'zeros', 'ones'):
    batch = helpers.make_batch(spec, batch=1, ctx_mask=mask)
    toks = batch['encoder_input_tokens']
    toks[0, valid:] = 0
    toks[0, :valid] = np.maximum(toks[0, :valid], 3)
    toks[0, valid - 1] = 1
    fm = fast.FastModel(backend.NumpyBackend('float64'), cfg, dc, params, True)
    fm.encode(toks, batch['encoder_continuous_inputs'], batch['encoder_continuous_mask'])
    nm.encode(1, toks, torch.as_tensor(batch['encoder_continuous_inputs']).cuda(), batch['encoder_continuous_mask'])
    for step in (2, 0):
      eps = torch.zeros_like(zd)
      nm.decoder_pass(1, step, zd, True, eps)
      torch.cuda.synchronize()
      want = fm.decoder_pass(z.astype(np.float64), step, True)
      err = np.abs(eps.cpu().numpy() - want).max() / np.abs(want).max()
      assert err < 2e-4, (valid, mask, step, err)


@pytest.mark.parametrize('preset,mask', [('tiny_context', 'ragged'), ('tiny_context', 'zeros'), ('tiny', 'ones')])
def test_sum_cross_attends_style(preset, mask):
  """decoder_cross_attend_style='sum_cross_attends' (the T5Config dataclass default, network.py:199-216): one
  cross-attention module per encoding (own q/k/v/out kernels, own key region and key count in the cache),
  outputs summed into the residual.  Single decoder passes elementwise against the float64 oracle, then a
  sampled segment with the float32 oracle as yardstick."""
  import dataclasses
  import torch
  from oracle import backend, fast
  spec = msd_amd.config.preset(preset, num_steps=6)
  spec = dataclasses.replace(spec, t5=dataclasses.replace(spec.t5, decoder_cross_attend_style='sum_cross_attends'))
  params = msd_amd.synthetic.init_params(spec, 8, norm_scale_jitter=0.1)
  model = msd_amd.InferenceModel(params, spec, batch_size=2, **helpers.ALL_PLANES)
  nm = model._get_native()
  batch = helpers.make_batch(spec, batch=2, ctx_mask=mask)
  cfg, dc = helpers.oracle_configs(spec)
  fm = fast.FastModel(backend.NumpyBackend('float64'), cfg, dc, params, spec.has_context)
  if spec.has_context:
    fm.encode(batch['encoder_input_tokens'], batch['encoder_continuous_inputs'], batch['encoder_continuous_mask'])
    nm.encode(2, batch['encoder_input_tokens'], torch.as_tensor(batch['encoder_continuous_inputs']).cuda(),
              batch['encoder_continuous_mask'])
  else:
    fm.encode(batch['encoder_input_tokens'])
    nm.encode(2, batch['encoder_input_tokens'])
  z = np.random.default_rng(0).standard_normal((2, 64, 128)).astype(np.float32)
  zd = torch.as_tensor(z).cuda()
  for step, cond in [(5, True), (1, True), (2, False)]:
    eps = torch.zeros_like(zd)
    nm.decoder_pass(2, step, zd, cond, eps)
    torch.cuda.synchronize()
    want = fm.decoder_pass(z.astype(np.float64), step, cond)
    err = np.abs(eps.cpu().numpy() - want).max() / np.abs(want).max()
    assert err < 2e-4, (preset, mask, step, cond, err)
  init_z, noise = helpers.make_noise(spec, batch=2)
  got, _ = model.predict(batch, init_z=init_z, noise=noise)
  ref64, _ = _oracle(spec, params, batch, init_z, noise, 'float64')
  ref32, _ = _oracle(spec, params, batch, init_z, noise, 'float32')
  helpers.assert_fp32_class(got, ref64, ref32, 'sum_cross_attends %s/%s' % (preset, mask))


# ---- half-plane range: loud, never silent (VERDICT r02 item 4 / ADVICE r02) ---------------------------------
def _overflowing_params(params):
  """A model the float32 reference runs without any trouble and the half planes cannot hold: the first decoder
  norm's scale times 1e5, its consumers (q / k / v kernels) times 1e-5.  The folded-norm planes hold
  y = x (.) gamma (.) (film_scale + 1) BEFORE the 1/rms, i.e. ~1e5 |x| > 65504, while every
  float32 / bfloat16-plane evaluation is scale-invariant there."""
  big = dict(params)
  lp = 'decoder/layers_0/'
  big[lp + 'pre_self_attention_layer_norm/scale'] = params[lp + 'pre_self_attention_layer_norm/scale'] * 1e5
  for k in ('query', 'key', 'value'):
    big[lp + 'self_attention/%s/kernel' % k] = params[lp + 'self_attention/%s/kernel' % k] * 1e-5
  return big


def test_activation_beyond_the_half_range_fails_the_call(tiny_ctx):
  spec, params, _ = tiny_ctx
  model = msd_amd.InferenceModel(_overflowing_params(params), spec, range_fallback=False)   # default precision f16x3; the fallback (on by default) would hide the error
  batch = helpers.make_batch(spec)
  init_z, noise = helpers.make_noise(spec)
  with pytest.raises(msd_amd.native.RangeError, match="bf16x3"):
    model.predict(batch, init_z=init_z, noise=noise)
  with pytest.raises(msd_amd.native.RangeError):                              # the flag was re-armed
    model.predict(batch, init_z=init_z, noise=noise)
  ok = msd_amd.InferenceModel(params, spec)                                   # and an in-range model is untouched
  got, _ = ok.predict(batch, init_z=init_z, noise=noise)
  assert np.isfinite(got).all()


def test_range_fallback_switches_to_bfloat16_planes_and_matches_the_oracle(tiny_ctx):
  spec, params, _ = tiny_ctx
  big = _overflowing_params(params)
  model = msd_amd.InferenceModel(big, spec, range_fallback=True)
  batch = helpers.make_batch(spec)
  init_z, noise = helpers.make_noise(spec)
  with pytest.warns(RuntimeWarning, match='bf16x3'):
    got, _ = model.predict(batch, init_z=init_z, noise=noise)
  assert model.precision == 'bf16x3' and model._get_native().planes == 'bf16'
  ref64, _ = _oracle(spec, big, batch, init_z, noise, 'float64')
  ref32, _ = _oracle(spec, big, batch, init_z, noise, 'float32')
  assert np.isfinite(got).all()
  # bfloat16 planes: float32-class with twice the rounding error of the half planes
  e, e32 = helpers.rms(got, ref64), helpers.rms(ref32, ref64)
  print('[range fallback] rms vs float64 %.3e (float32 oracle %.3e)' % (e, e32))
  assert e <= 4 * e32 + 1e-4


def test_range_fallback_fires_in_the_middle_of_a_song():
  """predict_sequence with the (default) range fallback when the overflow only shows up from segment 1 on.
  sum_cross_attends gives the context its own cross-attention module: the context encoder's final norm scale times
  3e5 and that module's key / value kernels divided by 3e5 are the same function in exact arithmetic, but the
  encodings of an UNMASKED context (segments >= 1) leave the half-plane range.  Segment 0 (context masked: the context
  encoder does not run) stays on 'f16x3'; segment 1 raises MSD_ERR_RANGE inside msd_encode, the model switches to
  'bf16x3' with a warning, repeats that segment and finishes the song there."""
  import dataclasses
  spec = msd_amd.config.preset('tiny_context', num_steps=4)
  spec = dataclasses.replace(spec, t5=dataclasses.replace(spec.t5, decoder_cross_attend_style='sum_cross_attends'))
  params = dict(msd_amd.synthetic.init_params(spec, 21, norm_scale_jitter=0.1))
  params['continuous_encoder/encoder_norm/scale'] = (params['continuous_encoder/encoder_norm/scale'] * 3e5).astype(np.float32)
  for name in list(params):
    if 'MultiHeadDotProductAttention_1/key/' in name or 'MultiHeadDotProductAttention_1/value/' in name:
      params[name] = (params[name] / 3e5).astype(np.float32)
  segs = [msd_amd.synthetic.segment_tokens(spec, k) for k in range(3)]
  model = msd_amd.InferenceModel(params, spec)                       # range_fallback defaults to True
  with pytest.warns(RuntimeWarning, match='bf16x3'):
    song = model.predict_sequence(segs, seed=3)
  assert model.precision == 'bf16x3' and np.isfinite(song).all()
  t = spec.task_feature_lengths['targets']
  # segment 0 is what a model that never fell back computes; segments 1, 2 are what a bfloat16-plane model computes
  # when resumed on segment 0's prediction
  strict = msd_amd.InferenceModel(params, spec, range_fallback=False)
  np.testing.assert_array_equal(strict.predict_sequence(segs[:1], seed=3), song[:, :t])
  with pytest.raises(msd_amd.native.RangeError):
    strict.predict_sequence(segs, seed=3)
  other = msd_amd.InferenceModel(params, spec, precision='bf16x3')
  rest = other.predict_sequence(segs[1:], seed=3, init_context=song[:, :t], first_segment_index=1)
  np.testing.assert_array_equal(rest, song[:, t:])


def test_a_precision_of_the_other_library_build_is_refused(tiny_ctx):
  """MSD_PREC_BF16X3 used to alias MSD_PREC_F16X3 and ran whatever planes the loaded library had."""
  spec, _, model = tiny_ctx
  cfg = msd_amd.inference._to_native_config(spec, model.audio_codec, 1, 'bf16x3')
  with pytest.raises(NotImplementedError, match='libmsd_amd_bf16.so'):
    msd_amd.native.NativeModel(cfg, planes='f16')
  cfg = msd_amd.inference._to_native_config(spec, model.audio_codec, 1, 'f16x3')
  with pytest.raises(NotImplementedError, match='libmsd_amd.so'):
    msd_amd.native.NativeModel(cfg, planes='bf16')
  assert msd_amd.native.NativeModel(msd_amd.inference._to_native_config(spec, model.audio_codec, 1, 'bf16')).planes == 'bf16'


def test_base_size_decoder_pass_does_not_depend_on_the_batch():
  """base_with_context shapes at 1, 2 and 3 songs per handle: M = 512 / 1024 / 1536 decoder rows pick different tiles
  (one song: 32 x 48 MLP-out at one tile per CU and 64 x 32 attention-out; 2 - 3 songs: two / three rounds of the same
  tiles, key split 2 instead of 4 -- msd_api.hip pick_tile, cross_ksplit_for), all below the 128-row tiles of the
  batched path.  An output element's K order does not depend on its tile, so a song's decoder pass must come out the
  same whichever batch it sits in (up to the key-split grouping of the cross-attention: float32 rounding), and equal
  songs in one batch must be BIT-identical.  (The single-song pass itself is pinned to the reference by
  tests/test_ref_golden.py's full-size fixture.)"""
  import torch
  spec = msd_amd.config.preset('base_with_context', num_steps=4)
  params = msd_amd.synthetic.init_params(spec, 0)
  one = helpers.make_batch(spec, batch=1, ctx_mask='ragged')
  z1 = np.random.default_rng(5).standard_normal((1, 256, 128)).astype(np.float32)
  outs = {}
  for B in (1, 2, 3):
    model = msd_amd.InferenceModel(params, spec, batch_size=B)
    nm = model._get_native()
    toks = np.repeat(one['encoder_input_tokens'], B, 0)
    ctx = torch.as_tensor(np.repeat(one['encoder_continuous_inputs'], B, 0)).cuda()
    mask = np.repeat(one['encoder_continuous_mask'], B, 0)
    nm.encode(B, toks, ctx, mask)
    z = torch.as_tensor(np.repeat(z1, B, 0)).cuda()
    for step, cond in ((3, True), (0, False)):
      eps = torch.zeros_like(z)
      nm.decoder_pass(B, step, z, cond, eps)
      torch.cuda.synchronize()
      outs[B, step] = eps.cpu().numpy()
    del model, nm
    torch.cuda.empty_cache()
  for step in (3, 0):
    ref = outs[1, step][0]
    for B in (2, 3):
      for j in range(1, B):
        np.testing.assert_array_equal(outs[B, step][j], outs[B, step][0])
      rel = np.abs(outs[B, step][0] - ref).max() / np.abs(ref).max()
      print('base size, %d songs, step %d: max rel diff to the one-song pass %.2e' % (B, step, rel))
      assert rel < 2e-5, (B, step, rel)


@pytest.mark.parametrize('preset,steps', [('tiny_context', 8), ('small', 3), ('base_with_context', 3)])
def test_exact_launch_shortcuts_are_bit_identical(preset, steps):
  """Rounds 5 - 6's launch-level shortcuts change WHEN and WHERE work runs, never the arithmetic; each is a msd_config knob
  and the sampled segment must be BIT-identical with it on (library default) and off (the folded cross-attention query
  projection is the exception -- another rounding order: test_folded_cross_query_projection_is_the_same_function):
    dedup_layer0        S5: in a CFG step decoder layer 0's QKV / self-attention / attention-out run on the conditional
                        pass's rows only and the attention-out epilogue writes every row twice -- both passes hold the
                        same rows up to the first cross-attention (models/diffusion/models.py:373-386, network.py:174-193)
    kv_touch_ahead      the cross-attention's prefetch wave touches K / V^T lines ahead of their LDS-DMA (attention.h)
  One and two songs per handle."""
  from oracle import philox
  spec = msd_amd.config.preset(preset, num_steps=steps)
  params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
  t = spec.task_feature_lengths['targets']
  for nb in (1, 2):
    batch = helpers.make_batch(spec, batch=nb, ctx_mask='ones') if spec.has_context else \
        {'encoder_input_tokens': np.concatenate([msd_amd.synthetic.segment_tokens(spec, 40 + b) for b in range(nb)], 0)}
    init_z, noise = philox.segment_noise((nb, t, 128), steps, seed=5, segment=0)
    outs = {}
    # weight_prefetch=True: the K / V touches ride on the launch's weight-prefetch wave, which the library turns OFF by
    # itself for models whose step fits the 256 MB cache (tiny_context, small) -- without forcing it the touch variants
    # of those presets would compare identical code paths
    for name, kw in (('default', {}), ('dedup_layer0 off', dict(dedup_layer0=False)),
                     ('merge launch', dict(cross_merge_in_launch=False)),
                     ('merge launch, split 2', dict(cross_merge_in_launch=False, cross_key_split=2)),
                     ('merge in launch, split 2', dict(cross_merge_in_launch=True, cross_key_split=2)),
                     ('kv_touch_ahead off', dict(kv_touch_ahead=0, weight_prefetch=True)),
                     ('kv_touch_ahead 2', dict(kv_touch_ahead=2, weight_prefetch=True)),
                     ('kv_touch_ahead 5', dict(kv_touch_ahead=5, weight_prefetch=True))):
      model = msd_amd.InferenceModel(params, spec, batch_size=nb, **kw, **helpers.ALL_PLANES)
      got, _ = model.predict(batch, init_z=init_z, noise=noise)
      outs[name] = np.asarray(got)
      del model
    assert np.isfinite(outs['default']).all()
    # Round 6: ONE reference for every variant.  The touch variants force the weight-prefetch wave on, i.e. run the PF = 1
    # instantiations of the kernels where the small presets run PF = 0 by default; until round 6 those rounded differently
    # in the last bit (the attention kernel's multiply-adds were contracted per instantiation: at two songs even
    # dedup_layer0 changed the bits, through the self-attention's block shape -- tools/diag/bitwise_matrix.py).  Every
    # intended multiply-add of that kernel is an explicit fma now, so the families agree.  (A key split of 2 sums the keys
    # in another order than the library's own choice: those two variants are compared with each other.)
    for name, got in outs.items():
      ref = 'merge launch, split 2' if 'split 2' in name else 'default'
      assert np.array_equal(got, outs[ref]), (preset, nb, name, np.abs(got - outs[ref]).max())


@pytest.mark.parametrize('preset,style,nb', [('tiny_context', 'concat', 2), ('tiny_context', 'sum', 2), ('tiny', 'concat', 1),
                                             ('small', 'concat', 1), ('base_with_context', 'concat', 1),
                                             ('base_with_context', 'concat', 2), ('base_with_context', 'concat', 3),
                                             ('base_with_context', 'sum', 1)])
def test_folded_cross_query_projection_is_the_same_function(preset, style, nb):
  """S6 (round 6; msd_config.cross_q_fold): the cross-attention's query projection has no launch of its own.  With
  x1 = x0 + ao . Wo (network.py:174-193) the projection's input is rstd(x1) (x1 (.) gamma) (network.py:196-198, layers.py:632-666), so
    (x1 (.) gamma) . Wq = (x0 (.) gamma) . Wq + ao . (Wo diag(gamma) Wq):
  the first term rides on the QKV launch, the second runs beside the self-attention output projection, the 1/rms scales
  the logits inside the attention kernel.  Exact algebra, another rounding order: single decoder passes with the fold on
  (library default) and off must agree to float32 rounding AND both must sit on the float64 oracle like every other
  pass (2e-4 max-rel: tests above); a CFG segment of a few steps must stay in the float32 class.  Both cross-attention
  styles (one and two modules), the duplicating layer 0 (CFG), 1 - 3 songs.  The fold takes launches of up to 1024
  decoder rows (msd_api.hip plan_step): every single pass here folds (M = nb T <= 768), a CFG step only up to 2 songs
  at base (M = 2 nb T: 1024 at 2 songs; at 3, M = 1536, both handles run the unfolded order and the segment comparison
  is of that order with itself).  Asserted per case: the folded handle's single conditional pass writes the `qp` buffer
  (the QKV launch's half of the folded queries; zero in a fresh handle), and a CFG step launches no cross-attention
  query projection when folded, one per decoder layer and module otherwise (msd_profile_steps' eager steps)."""
  import dataclasses
  import torch
  from oracle import backend, fast
  steps = 4
  spec = msd_amd.config.preset(preset, num_steps=steps)
  if style == 'sum':
    spec = dataclasses.replace(spec, t5=dataclasses.replace(spec.t5, decoder_cross_attend_style='sum_cross_attends'))
  params = msd_amd.synthetic.init_params(spec, 5, norm_scale_jitter=0.1)
  t = spec.task_feature_lengths['targets']
  batch = helpers.make_batch(spec, batch=nb, ctx_mask='ragged') if spec.has_context else \
      {'encoder_input_tokens': np.concatenate([msd_amd.synthetic.segment_tokens(spec, 70 + b) for b in range(nb)], 0)}
  cfg, dc = helpers.oracle_configs(spec)
  small_enough = preset.startswith('tiny')
  fm = None
  if small_enough:
    fm = fast.FastModel(backend.NumpyBackend('float64'), cfg, dc, params, spec.has_context)
    if spec.has_context:
      fm.encode(batch['encoder_input_tokens'], batch['encoder_continuous_inputs'], batch['encoder_continuous_mask'])
    else:
      fm.encode(batch['encoder_input_tokens'])
  z = np.random.default_rng(1).standard_normal((nb, t, 128)).astype(np.float32)
  zd = torch.as_tensor(z).cuda()
  init_z, noise = helpers.make_noise(spec, batch=nb)
  eps, seg = {}, {}
  cfg_folds = 2 * nb * t <= 1024   # (every single pass of these cases folds: nb t <= 768)
  n_cross = 2 if style == 'sum' else 1
  for fold in (True, False):
    model = msd_amd.InferenceModel(params, spec, batch_size=nb, cross_q_fold=fold, **helpers.ALL_PLANES)
    nm = model._get_native()
    if spec.has_context:
      nm.encode(nb, batch['encoder_input_tokens'], torch.as_tensor(batch['encoder_continuous_inputs']).cuda(),
                batch['encoder_continuous_mask'])
    else:
      nm.encode(nb, batch['encoder_input_tokens'])
    if fold:
      assert not nm.debug_read('qp').any()
    for step, cond in ((steps - 1, True), (1, True), (0, False)):
      out = torch.zeros_like(zd)
      nm.decoder_pass(nb, step, zd, cond, out)
      torch.cuda.synchronize()
      eps[fold, step] = out.cpu().numpy()
      if fold and step == steps - 1:   # the single conditional pass ran folded
        assert np.abs(nm.debug_read('qp', nb * t * n_cross * spec.t5.num_heads * 64)).max() > 0, (preset, style, nb)
      if fm is not None:
        want = fm.decoder_pass(z.astype(np.float64), step, cond)
        err = np.abs(eps[fold, step] - want).max() / np.abs(want).max()
        assert err < 2e-4, (preset, style, fold, step, cond, err)
    got, _ = model.predict(batch, init_z=init_z, noise=noise)   # CFG steps: the duplicating layer 0 + the fold
    seg[fold] = np.asarray(got)
    cross_q = nm.profile_steps(nb, 1)['gemm_cross_q'][1]
    print('%s/%s, %d song(s), fold %s: cross-q launches per CFG step %d' % (preset, style, nb, fold, cross_q))
    assert cross_q == (0 if fold and cfg_folds else spec.t5.num_decoder_layers * n_cross), (preset, style, nb, fold, cross_q)
    del model, nm
    torch.cuda.empty_cache()
  for step in (steps - 1, 1, 0):
    rel = np.abs(eps[True, step] - eps[False, step]).max() / np.abs(eps[False, step]).max()
    print('%s/%s, %d song(s), step %d: folded vs unfolded decoder pass, max rel %.2e' % (preset, style, nb, step, rel))
    assert rel < (2e-5 if step else 1e-30), (preset, style, step, rel)   # (step 0 ran unconditional: no cross-attention, same bits)
  assert np.isfinite(seg[True]).all()
  if small_enough:
    # a few huge steps amplify rounding (helpers.assert_fp32_class): both orders must show the float32 oracle's error
    # distribution -- the folded one no worse than the unfolded one (tests/diag/fold_stats.py, profiles/r06d_fold_stats.log:
    # the fractions beyond 1e-3 / 1e-4 agree to 0.003 over 16 cases)
    ref64, _ = _oracle(spec, params, batch, init_z, noise, 'float64')
    ref32, _ = _oracle(spec, params, batch, init_z, noise, 'float32')
    e32 = np.abs(ref32 - ref64).ravel()
    for tau in (1e-3, 1e-4):
      f = {k: float((np.abs(seg[k].astype(np.float64) - ref64).ravel() > tau).mean()) for k in (True, False)}
      f32 = float((e32 > tau).mean())
      print('%s/%s beyond %.0e: folded %.4f unfolded %.4f float32 oracle %.4f' % (preset, style, tau, f[True], f[False], f32))
      assert f[True] <= 1.05 * f[False] + 0.003, (preset, style, tau, f)
      assert f[True] <= 1.30 * f32 + 0.01, (preset, style, tau, f, f32)
    med = {k: float(np.median(np.abs(seg[k].astype(np.float64) - ref64))) for k in (True, False)}
    assert med[True] <= 1.5 * float(np.median(e32)) + 1e-6, med
  else:   # the two orders stay together to that class
    d = seg[True] - seg[False]
    print('%s/%s: folded vs unfolded %d-step segment: rms %.2e, max %.2e' % (preset, style, steps, np.sqrt((d ** 2).mean()), np.abs(d).max()))
    assert np.sqrt((d ** 2).mean()) < 1e-3, (preset, style)


@pytest.mark.parametrize('preset,nb', [('tiny_context', 1), ('tiny_context', 3), ('small', 1)])
def test_sampler_draws_the_step_noise_itself_bit_identical(preset, nb):
  """msd_sample with noise == NULL (round 6): sampler_step_kernel draws step i's noise from sub-sequence 1 + i of the
  (seed, segment) Philox stream -- the [N][batch T n] buffer philox_normal_kernel used to fill up front (131 MB x songs at
  base, a hipMalloc inside msd_sample) is gone.  Same generator function, same counters: the segment must be
  BIT-identical to a run that is handed exactly those rows (msd_fill_normal) as explicit noise."""
  import torch
  from msd_amd import native
  steps = 7
  spec = msd_amd.config.preset(preset, num_steps=steps)
  t = spec.task_feature_lengths['targets']
  batch = helpers.make_batch(spec, batch=nb, ctx_mask='ones') if spec.has_context else \
      {'encoder_input_tokens': np.concatenate([msd_amd.synthetic.segment_tokens(spec, 60 + b) for b in range(nb)], 0)}
  model = msd_amd.InferenceModel('synthetic:1', spec, batch_size=nb)
  model.predict(batch, init_z=np.zeros((nb, t, 128), np.float32), noise=np.zeros((steps, nb, t, 128), np.float32))   # graphs captured, tables built
  got, _ = model.predict(batch, seed=42, segment=3)
  z = torch.empty((nb, t, 128), dtype=torch.float32, device='cuda')
  nz = torch.empty((steps, nb, t, 128), dtype=torch.float32, device='cuda')
  native.fill_normal(z, 42, 3, 0)
  for i in range(steps):
    native.fill_normal(nz[i], 42, 3, 1 + i)
  torch.cuda.synchronize()
  want, _ = model.predict(batch, init_z=z, noise=nz)
  assert np.isfinite(got).all() and np.array_equal(np.asarray(got), np.asarray(want)), np.abs(np.asarray(got) - np.asarray(want)).max()
  other, _ = model.predict(batch, seed=42, segment=4)
  assert helpers.rms(got, other) > 0.05                     # the segment index keys the stream


def test_staging_copies_of_packed_weights_are_freed():
  """msd_finalize_weights frees the float32 staging copy of every matrix it packed (round 5: 1.5 of 1.65 GB per handle
  at base_with_context; msd_config.keep_raw_weights = 1 keeps them): the device memory a handle holds drops by about
  the size of its matrices, the result does not change, and a late msd_set_weight is refused with a clear message."""
  import torch
  spec = msd_amd.config.preset('small', num_steps=2)
  params = msd_amd.synthetic.init_params(spec, 1)
  batch = {'encoder_input_tokens': msd_amd.synthetic.segment_tokens(spec, 3)}
  matrices = sum(v.size for k, v in params.items() if v.ndim == 2 and 'embedding' not in k and 'Embed_0' not in k) * 4
  used, outs = {}, {}
  for keep in (True, False):
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    model = msd_amd.InferenceModel(params, spec, keep_raw_weights=keep)
    outs[keep], _ = model.predict(batch, seed=1)
    torch.cuda.synchronize()
    used[keep] = free0 - torch.cuda.mem_get_info()[0]
    if not keep:
      nm = model._get_native()
      name = 'decoder/layers_0/mlp/wo/kernel'
      with pytest.raises(RuntimeError, match='loaded once per handle'):
        nm.set_weight(name, params[name])
    # ... and so is a weight whose float32 copy is still resident (a norm scale; every weight with keep_raw_weights):
    # accepting it used to clear `finalized` while a second msd_finalize_weights refuses -- a dead handle
    nm = model._get_native()
    with pytest.raises(RuntimeError, match='loaded once per handle'):
      nm.set_weight('decoder/decoder_norm/scale', params['decoder/decoder_norm/scale'])
    again, _ = model.predict(batch, seed=1)
    assert np.array_equal(np.asarray(again), np.asarray(outs[keep]))   # the handle is still usable
    del model
  assert np.array_equal(np.asarray(outs[True]), np.asarray(outs[False]))
  assert used[True] - used[False] > 0.6 * matrices, (used, matrices)   # (the allocator returns whole 2 MiB blocks: measured 0.77)


def test_two_handles_from_two_threads_on_one_device():
  """Handles are independent: two threads may create, load and run one each on the SAME device at the same time
  (include/msd_amd.h "Threading").  Round 5: the library's synchronous copies / fills go through the handle's own
  non-blocking stream -- through the legacy stream, a second handle that loaded its weights while the first captured its
  step graph failed both ("operation would make the legacy stream depend on a capturing blocking stream").  Results
  equal the same work done one after the other, bit for bit."""
  import threading
  spec = msd_amd.config.preset('tiny_context', num_steps=16)
  params = [msd_amd.synthetic.init_params(spec, 20 + i, norm_scale_jitter=0.1) for i in range(2)]
  batches = [helpers.make_batch(spec, batch=1, seed=30 + i, ctx_mask='ones') for i in range(2)]

  def run(i, out):
    model = msd_amd.InferenceModel(params[i], spec)
    a, _ = model.predict(batches[i], seed=i, segment=0)
    b, _ = model.predict(batches[i], seed=i, segment=1)
    out[i] = (np.asarray(a), np.asarray(b))

  want = {}
  for i in range(2):
    run(i, want)
  for _ in range(3):                       # a few times: the race is a matter of timing
    got, errs = {}, []

    def guarded(i):
      try:
        run(i, got)
      except Exception as e:               # noqa: BLE001 -- reported below, from the main thread
        errs.append(repr(e))

    threads = [threading.Thread(target=guarded, args=(i,)) for i in range(2)]
    for t in threads:
      t.start()
    for t in threads:
      t.join()
    assert not errs, errs
    for i in range(2):
      assert np.array_equal(got[i][0], want[i][0]) and np.array_equal(got[i][1], want[i][1])
