"""-m gpu: the denoising loss (msd_loss, msd_op_diffusion_loss, InferenceModel.loss) against the specification of
tests/loss_spec.py and the reference's own statements (tests/golden/ref_loss_*.npz).

Presets tiny / tiny_context: T = 64, n = 128, two rows -- a 1024-element block of the two kernels holds 8 frames, a row is
8 blocks; the mask of row 1 is zero on its last 19 frames, which cuts inside a block."""
import os

import numpy as np
import pytest

import msd_amd
from msd_amd import inference, native
from oracle import backend, fast
from tests import helpers, loss_spec, ref_cases
from tests.helpers import gpu_torch  # noqa: F401  (the `torch` fixture)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
N = 16
_models = {}


def _model(preset='tiny_context'):
  return helpers.cached_model(_models, preset, N)


def _batch(spec, b=2):
  batch = helpers.make_batch(spec, batch=b, seed=5, ctx_mask='ragged')
  batch['decoder_target_tokens'] = helpers.known_mel((b, 64, 128))
  mask = np.ones((b, 64), np.float32)
  mask[-1, -19:] = 0.0
  batch['decoder_target_mask'] = mask
  return batch


def _fill(torch, rng, seed, segment, i, shape):
  """The eps of time index i under one key over `shape`: what the fill entry points write."""
  buf = torch.empty(shape, dtype=torch.float32, device='cuda')
  if rng == 'philox':
    native.fill_normal(buf, seed, segment, 1 + i)
  else:
    native.fill_normal_threefry(buf, seed, fold=i)
  torch.cuda.synchronize()
  return buf


def _alpha_sigma(nm, i):
  """diffuse_coefs' formula on the train log-SNR of row i (msd_get_schedule word 7): double, rounded once."""
  l = float(nm.schedule()[i, 7])
  return np.float32(np.sqrt(1.0 / (1.0 + np.exp(-l)))), np.float32(np.sqrt(1.0 / (1.0 + np.exp(l))))


def _fma32(a, b, c):
  """fmaf(a, b, c) on float32 arrays: the exact product (48 bits: exact in float64), the sum rounded TO ODD in float64
  (TwoSum's error decides), then rounded once to float32 -- the correctly rounded a * b + c."""
  a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
  a, b, c = np.broadcast_arrays(a, b, c)
  p = a * b
  s = p + c
  bb = s - p
  e = (p - (s - bb)) + (c - bb)
  bits = s.copy().view(np.int64)
  adjust = (e != 0) & ((bits & 1) == 0)
  grow = (e > 0) == (s > 0)
  bits = np.where(adjust, np.where(grow, bits + 1, bits - 1), bits)
  return bits.view(np.float64).astype(np.float32)


def _x0_bits(mel):
  """scale_clip_kernel's expression in NumPy float32."""
  codec = msd_amd.audio_codecs.MelGAN()
  fmin, fmax = np.float32(codec.min_value), np.float32(codec.max_value)
  return (np.clip(mel, fmin, fmax) - fmin) / (fmax - fmin) * np.float32(2.0) + np.float32(-1.0)


# --------------------------------------------------------------------------------------------------
# 1. bit for bit
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rng', ['philox', 'threefry'])
def test_z_is_the_diffused_target_and_given_eps_is_the_drawn_call(torch, rng):
  spec, params, model = _model()
  batch = _batch(spec)
  nm = model._get_native()
  for i in (0, 7, N - 1):
    drawn = model.loss(batch, times=[i], seed=11, segment=3, rng=rng)
    z = nm.debug_read('z')[:2 * 64 * 128].reshape(2, 64, 128)
    x0_dev = nm.debug_read('loss_x0')[:2 * 64 * 128].reshape(2, 64, 128)
    eps = _fill(torch, rng, 11, 3, i, (2, 64, 128))
    alpha, sigma = _alpha_sigma(nm, i)
    x0 = _x0_bits(batch['decoder_target_tokens'])
    assert np.array_equal(helpers.bits(x0_dev), helpers.bits(x0))
    want = _fma32(sigma, eps.cpu().numpy(), alpha * x0)
    assert np.array_equal(helpers.bits(z), helpers.bits(want)), (rng, i, np.abs(z - want).max())
    given = model.loss(batch, times=[i], seed=99, segment=0, rng=rng, eps=eps[None])
    assert np.array_equal(given['per_frame'], drawn['per_frame']) and np.isfinite(drawn['per_frame']).all()
    assert drawn['loss'].shape == (1,) and drawn['loss'][0] > 0 and drawn['target_frames'] == 2 * 64 - 19


@pytest.mark.parametrize('preset', ['tiny', 'tiny_context'])
def test_per_frame_is_the_loss_op_on_the_decoder_pass(torch, preset):
  """cond / uncond: per_frame == msd_op_diffusion_loss applied to msd_decoder_pass(i, z)'s output, bit for bit; masked
  frames are exactly 0."""
  spec, params, model = _model(preset)
  batch = _batch(spec)
  nm = model._get_native()
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 2, 'f16x3')
  mask = helpers.dev(torch, batch['decoder_target_mask'])
  for i, lt, ln in ((0, 'eps', 'l1'), (9, 'max_x0_eps', 'l2'), (N - 1, 'x0_and_eps', 'l1'), (5, 'x0', 'l2')):
    for cond in ('cond', 'uncond'):
      got = model.loss(batch, times=[i], seed=4, segment=1, conditioning=cond, loss_type=lt, loss_norm=ln)['per_frame'][0]
      z = helpers.dev(torch, nm.debug_read('z')[:2 * 64 * 128].reshape(2, 64, 128))
      x0 = helpers.dev(torch, nm.debug_read('loss_x0')[:2 * 64 * 128].reshape(2, 64, 128))
      eps = _fill(torch, 'philox', 4, 1, i, (2, 64, 128))
      o = torch.empty_like(z)
      nm.decoder_pass(2, i, z, cond == 'cond', o)
      out = torch.full((2, 64), float('nan'), dtype=torch.float32, device='cuda')
      native.op_diffusion_loss(cfg, i, lt, ln, o, z, x0, eps, mask, out, 128)
      want = out.cpu().numpy()
      assert np.array_equal(got.astype(np.float32), want), (preset, i, cond, lt, ln)
      assert (got[1, -19:] == 0).all() and (got[0] > 0).all() and (got[1, :-19] > 0).all()


def test_times_permute_and_repeat_and_calls_repeat(torch):
  spec, params, model = _model()
  batch = _batch(spec)
  a = model.loss(batch, times=[2, 9, 15], seed=1, conditioning='both')
  b = model.loss(batch, times=[15, 2, 2, 9], seed=1, conditioning='both')
  assert a['per_time'].shape == (3, 2, 2) and b['per_time'].shape == (4, 2, 2)
  assert np.array_equal(b['per_time'], a['per_time'][[2, 0, 0, 1]])   # a repeated index draws the same eps: equal rows
  again = model.loss(batch, times=[2, 9, 15], seed=1, conditioning='both')
  assert np.array_equal(again['per_frame'], a['per_frame']) and np.array_equal(again['per_time'], a['per_time'])
  grid = model.loss(batch, times=3, seed=1, conditioning='both')
  assert grid['times'] == [2, 8, 13] and np.array_equal(grid['per_time'][0], a['per_time'][0])
  # the two passes of `both` are the single forms up to a batched launch's rounding
  for k, cond in enumerate(('cond', 'uncond')):
    one = model.loss(batch, times=[2, 9, 15], seed=1, conditioning=cond)
    np.testing.assert_allclose(a['per_frame'][k], one['per_frame'][0], rtol=2e-4, atol=1e-6)
  assert np.abs(a['per_frame'][0] - a['per_frame'][1]).max() > 1e-3   # conditioning matters


@pytest.mark.parametrize('conditioning', ['cond', 'both'])
@pytest.mark.parametrize('rng', ['philox', 'threefry'])
def test_rows_are_their_one_row_calls(torch, rng, conditioning):
  """Per-row keys: row b of the call equals the one-row call (seed_b, segment_b), bit for bit -- its per-frame losses at
  every entry of `times`, their per-time sums and its z --, and the call equals the one whose eps was filled row by row
  under those keys."""
  spec, params, model = _model()
  batch = _batch(spec)
  nm = model._get_native()
  seeds, segments, times = [7, 8], [3, 9], [1, 12]
  kw = dict(rng=rng, conditioning=conditioning)
  got = model.loss(batch, times=times, seed=seeds, segment=segments, **kw)
  got_t = [model.loss(batch, times=[i], seed=seeds, segment=segments, **kw)['per_frame'] for i in times]   # [passes, B, T] each
  z_rows = nm.debug_read('z')[:2 * 64 * 128].reshape(2, 64, 128).copy()   # the state of the LAST time
  assert np.array_equal(np.stack(got_t, 0).sum(axis=3), got['per_time'])
  eps = torch.stack([torch.cat([_fill(torch, rng, seeds[b], segments[b], i, (1, 64, 128)) for b in range(2)], 0) for i in times], 0)
  want = model.loss(batch, times=times, eps=eps, conditioning=conditioning)
  assert np.array_equal(got['per_frame'], want['per_frame']) and np.array_equal(got['per_time'], want['per_time'])
  for b in range(2):
    one = {k: v[b:b + 1] for k, v in batch.items()}
    row = model.loss(one, times=times, seed=seeds[b], segment=segments[b], **kw)
    assert np.array_equal(row['per_frame'][:, 0], got['per_frame'][:, b]), (rng, b)
    assert np.array_equal(row['per_time'][:, :, 0], got['per_time'][:, :, b]), (rng, b)
    for j, i in enumerate(times):   # ... and frame by frame at every entry of `times`
      row_i = model.loss(one, times=[i], seed=seeds[b], segment=segments[b], **kw)['per_frame']
      assert np.array_equal(row_i[:, 0], got_t[j][:, b]), (rng, b, i)
    assert np.array_equal(helpers.bits(nm.debug_read('z')[:64 * 128].reshape(64, 128)), helpers.bits(z_rows[b])), (rng, b)
  whole = model.loss(batch, times=times, seed=7, segment=3, **kw)   # the mode does not stick: one draw over both rows
  assert np.abs(whole['per_frame'][0, 1] - got['per_frame'][0, 1]).max() > 1e-3


def _fresh(spec, params):
  return msd_amd.InferenceModel(params, spec, batch_size=2, **helpers.ALL_PLANES)


def test_order_independence_with_predict(torch):
  """predict then loss == a fresh handle's first loss; loss then predict == a fresh handle's first mel; likewise with
  reset_graph between the calls.  Bit for bit."""
  spec, params, _ = _model()
  batch = _batch(spec)
  kw = dict(times=[3, 14], seed=2, segment=5, conditioning='both')
  first_loss = _fresh(spec, params).loss(batch, **kw)['per_frame']
  first_mel, _ = _fresh(spec, params).predict(batch, seed=2, segment=5)
  for reset in (False, True):
    m = _fresh(spec, params)
    mel, _ = m.predict(batch, seed=2, segment=5)
    if reset:
      m._get_native().reset_graph()
    assert np.array_equal(mel, first_mel)
    assert np.array_equal(m.loss(batch, **kw)['per_frame'], first_loss), reset
    m = _fresh(spec, params)
    assert np.array_equal(m.loss(batch, **kw)['per_frame'], first_loss)
    if reset:
      m._get_native().reset_graph()
    mel, _ = m.predict(batch, seed=2, segment=5)
    assert np.array_equal(mel, first_mel), reset
    assert np.array_equal(m.loss(batch, **kw)['per_frame'], first_loss)   # and the cached graphs of both still serve


# --------------------------------------------------------------------------------------------------
# 2. against float64
# --------------------------------------------------------------------------------------------------
def _rel(got, ref):
  """per-frame errors relative to the frame's float64 loss, over the frames that have one"""
  live = ref != 0
  assert (np.asarray(got)[~live] == 0).all()
  return np.abs(np.asarray(got, np.float64)[live] - ref[live]) / ref[live]


@pytest.mark.parametrize('train', ['cosine', 'linear'])
@pytest.mark.parametrize('mode', ['eps', 'x0', 'v'])
def test_op_against_float64(torch, mode, train):
  """msd_op_diffusion_loss on random o, z, x0, eps over all (type, norm) of this mode and train schedule at indices
  {0, 1, N // 2, N - 1}, a ragged mask that cuts inside a block: the largest per-frame error relative to the frame's float64
  loss is at most 4x that of the same specification run in float32 (the margin: another summation order, and the fused
  multiply-adds of the pinned conversion text)."""
  spec = helpers.sampler_spec(model_output=mode, train=train, steps=N)
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, 'f16x3')
  _, dc = helpers.oracle_configs(spec)
  r = np.random.default_rng(17)
  shape = (2, 67, 128)   # 16.75 blocks: the last block is partial
  o, z, x0, eps = (r.standard_normal(shape).astype(np.float32) for _ in range(4))
  mask = np.ones(shape[:2], np.float32)
  mask[0, 30:35] = 0.0
  mask[1, -19:] = 0.0
  dev = [helpers.dev(torch, a) for a in (o, z, x0, eps, mask)]
  worst = 0.0
  for i in (0, 1, N // 2, N - 1):
    for lt in loss_spec.LOSS_TYPES:
      for ln in loss_spec.LOSS_NORMS:
        f64 = loss_spec.op_frame_losses('float64', dc, z, o, x0, eps, mask, i, N, lt, ln)
        f32 = loss_spec.op_frame_losses('float32', dc, z, o, x0, eps, mask, i, N, lt, ln)
        out = torch.full(shape[:2], float('nan'), dtype=torch.float32, device='cuda')
        native.op_diffusion_loss(cfg, i, lt, ln, *dev, out, 128)
        e_dev, e_f32 = _rel(out.cpu().numpy(), f64).max(), _rel(f32, f64).max()
        worst = max(worst, e_dev / e_f32)
        print('op loss %s/%s %s %s i=%d: largest relative frame error device %.3e / float32 %.3e (ratio %.2f)'
              % (mode, train, lt, ln, i, e_dev, e_f32, e_dev / e_f32))
        assert e_dev <= 4 * e_f32, (mode, train, lt, ln, i, e_dev, e_f32)
  print('op loss %s/%s: worst ratio %.2f' % (mode, train, worst))
  # jnp.maximum keeps a NaN: one poisoned element of the model output makes its frame's max_x0_eps loss a NaN on the device
  # as in the specification (either operand of the maximum may be the poisoned one: eps_hat in mode eps, x0_hat in mode x0,
  # both in mode v), and no other frame's; a masked frame's NaN stays a NaN too (NaN * 0)
  bad = o.copy()
  bad[0, 3, 5] = np.nan
  bad[1, -1, 77] = np.nan
  for ln in loss_spec.LOSS_NORMS:
    want = loss_spec.op_frame_losses('float32', dc, z, bad, x0, eps, mask, N // 2, N, 'max_x0_eps', ln)
    out = torch.full(shape[:2], 0.0, dtype=torch.float32, device='cuda')
    native.op_diffusion_loss(cfg, N // 2, 'max_x0_eps', ln, helpers.dev(torch, bad), *dev[1:], out, 128)
    got = out.cpu().numpy()
    assert np.isnan(want[0, 3]) and np.isnan(want[1, -1]) and np.isnan(want).sum() == 2
    assert np.array_equal(np.isnan(got), np.isnan(want)), (mode, train, ln)


_refs = {}


def _case(name):
  """(spec, params, batch, target, mask, eps, idx, fixture, float32-oracle frames) of a fixture case, computed once."""
  if name not in _refs:
    spec, params, batch, target, mask, eps, idx = loss_spec.case_inputs(name)
    cfg, dc = helpers.oracle_configs(spec)
    xp = backend.TorchBackend('float32', threads=1)
    fm = fast.FastModel(xp, cfg, dc, params, spec.has_context)
    loss_spec.encode(fm, batch)
    f32 = [loss_spec.evaluate(xp, fm, dc, target, mask, eps[j], i) for j, i in enumerate(idx)]
    _refs[name] = (spec, params, batch, target, mask, eps, idx, np.load(os.path.join(GOLD, 'ref_loss_%s.npz' % name)), f32)
  return _refs[name]


def _assert_frames_in_the_float32_class(got, ref64, ref32, what):
  e_dev, e_f32 = _rel(got, ref64), _rel(ref32, ref64)
  print('%s: per-frame relative error, largest device %.3e / float32 oracle %.3e (ratio %.2f); median %.3e / %.3e (ratio %.2f)'
        % (what, e_dev.max(), e_f32.max(), e_dev.max() / e_f32.max(), np.median(e_dev), np.median(e_f32),
           np.median(e_dev) / np.median(e_f32)))
  assert e_dev.max() <= 2 * e_f32.max(), what
  assert np.median(e_dev) <= 2 * np.median(e_f32), what


@pytest.mark.parametrize('form', ['cond', 'uncond', 'both'])
@pytest.mark.parametrize('name', loss_spec.CASES)
def test_call_against_the_reference(torch, name, form):
  """Every fixture case and conditioning form: the device's per-frame losses (three indices, all types and norms) against the
  reference's, with loss_spec over the float32 oracle decoder as the yardstick: largest and median per-frame relative error
  at most 2x the float32 oracle's."""
  spec, params, batch, target, mask, eps, idx, g, f32 = _case(name)
  key = ('case', name)
  if key not in _models:
    _models[key] = msd_amd.InferenceModel(params, spec, batch_size=2, **helpers.ALL_PLANES)
  model = _models[key]
  b = dict(batch, decoder_target_tokens=target, decoder_target_mask=mask)
  for lt in loss_spec.LOSS_TYPES:
    for ln in loss_spec.LOSS_NORMS:
      got = np.stack([model.loss(b, times=[i], eps=eps[j:j + 1], conditioning=form, loss_type=lt, loss_norm=ln)['per_frame']
                      for j, i in enumerate(idx)], 1)   # [passes, 3, B, T]
      for k, cond in enumerate(('cond', 'uncond') if form == 'both' else (form,)):
        ref64 = g[loss_spec.fixture_key(cond, lt, ln)]
        ref32 = np.stack([f[(cond, lt, ln)] for f in f32], 0)
        _assert_frames_in_the_float32_class(got[k], ref64, ref32, '%s %s/%s %s %s' % (name, form, cond, lt, ln))


def test_full_size_against_float64(torch):
  """base_with_context (ref_cases base_with_context_n3's inputs, N = 3, all three indices, both passes) against loss_spec in
  float64 under the call-level criterion."""
  spec, params, batch, init_z, noise = ref_cases.inputs('base_with_context_n3')
  target = helpers.known_mel(init_z.shape)
  mask = np.ones(init_z.shape[:2], np.float32)
  mask[0, -19:] = 0.0
  cfg, dc = helpers.oracle_configs(spec)
  refs = {}
  for dtype in ('float64', 'float32'):
    xp = backend.TorchBackend(dtype)
    fm = fast.FastModel(xp, cfg, dc, params, spec.has_context)
    loss_spec.encode(fm, batch)
    refs[dtype] = [loss_spec.evaluate(xp, fm, dc, target, mask, noise[i], i, combos=[('eps', 'l1')]) for i in range(3)]
  model = msd_amd.InferenceModel(params, spec, batch_size=1)
  got = model.loss(dict(batch, decoder_target_tokens=target, decoder_target_mask=mask), times=[0, 1, 2], eps=noise,
                   conditioning='both')
  assert got['per_time'].shape == (3, 2, 1)
  frames = np.stack([model.loss(dict(batch, decoder_target_tokens=target, decoder_target_mask=mask), times=[i], eps=noise[i:i + 1],
                                conditioning='both')['per_frame'] for i in range(3)], 1)
  np.testing.assert_allclose(frames.sum(axis=3), np.moveaxis(got['per_time'], 0, 1), rtol=1e-12)
  for k, cond in enumerate(('cond', 'uncond')):
    _assert_frames_in_the_float32_class(frames[k], np.stack([r[(cond, 'eps', 'l1')] for r in refs['float64']], 0),
                                        np.stack([r[(cond, 'eps', 'l1')] for r in refs['float32']], 0), 'base_with_context ' + cond)


# --------------------------------------------------------------------------------------------------
# 3. refusals
# --------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(torch):
  import ctypes
  spec = msd_amd.config.preset('tiny_context', num_steps=N, cfg_weight=1.0)
  params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
  model = msd_amd.InferenceModel(params, spec, batch_size=2, **helpers.ALL_PLANES)
  batch = _batch(spec)
  nm = model._get_native()
  tgt = helpers.dev(torch, batch['decoder_target_tokens'])
  out = torch.zeros((1, 2, 2, 64), dtype=torch.float32, device='cuda')
  with pytest.raises(RuntimeError, match='msd_encode has not run'):   # before encode
    nm.loss(2, tgt, out[:, :1], [3])
  good = model.loss(batch, times=[3])['per_frame']
  with pytest.raises(NotImplementedError, match='cfg_weight 1'):   # both passes on a weight-1 handle
    nm.loss(2, tgt, out, [3], conditioning='both')
  with pytest.raises(ValueError, match='batch 1 != encoded batch 2'):
    nm.loss(1, tgt[:1], out[:, :1, :1], [3])
  # what the Python layers refuse themselves, handed to the entry point directly: each names the offending value
  def raw(**kw):
    a = native.LossArgs()
    seeds = (ctypes.c_uint64 * 2)(1, 2)
    times = (ctypes.c_int32 * 2)(*kw.pop('times', (3, 4)))
    a.struct_size, a.batch, a.rng, a.per_row, a.seeds, a.n_times, a.times_host = ctypes.sizeof(a), 2, 0, 0, seeds, 2, times
    a.target_dev, a.out_dev, a.loss_type = tgt.data_ptr(), out.data_ptr(), 1
    for k, v in kw.items():
      setattr(a, k, v)
    rc = nm.lib.msd_loss(nm.handle, ctypes.byref(a), 0)
    return rc, nm.lib.msd_last_error(nm.handle).decode()
  for kw, rc_want, word in ((dict(times=(3, N)), 1, 'time index %d' % N), (dict(times=(-1, 3)), 1, 'time index -1'),
                            (dict(n_times=0), 1, 'n_times 0'), (dict(rng=5), 1, 'unknown rng 5'),
                            (dict(conditioning=3), 1, 'unknown conditioning 3'), (dict(loss_type=4), 1, 'loss_type: 4'),
                            (dict(loss_norm=2), 1, 'loss norm: 2'), (dict(struct_size=80), 1, 'struct_size 80')):
    rc, msg = raw(**kw)
    assert rc == rc_want and word in msg, (kw, rc, msg)
  assert raw()[0] == 0
  assert np.array_equal(model.loss(batch, times=[3])['per_frame'], good)   # the handle works afterwards


# --------------------------------------------------------------------------------------------------
# 4. range fallback
# --------------------------------------------------------------------------------------------------
def test_range_error_and_fallback(torch):
  """The scaled-norm model of tests/test_gpu_model.py at the two ends of the time grid: MSD_ERR_RANGE on 'f16x3'; with
  range_fallback the call is repeated on the bfloat16 planes, as predict's and invert's are."""
  from tests.test_gpu_model import _overflowing_params
  spec = msd_amd.config.preset('tiny_context', num_steps=N)
  big = _overflowing_params(msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1))
  batch = _batch(spec, b=1)
  strict = msd_amd.InferenceModel(big, spec, range_fallback=False)
  with pytest.raises(native.RangeError, match='bf16x3'):
    strict.loss(batch, times=[0, N - 1])
  assert strict.precision == 'f16x3'
  model = msd_amd.InferenceModel(big, spec, range_fallback=True)
  with pytest.warns(RuntimeWarning, match='bf16x3'):
    got = model.loss(batch, times=[0, N - 1])
  assert model.precision == 'bf16x3' and model._get_native().planes == 'bf16'
  assert got['times'] == [0, N - 1] and got['per_frame'].shape == (1, 1, 64)
  for key in ('loss', 'per_row', 'per_frame', 'per_time'):
    assert np.isfinite(got[key]).all(), key
