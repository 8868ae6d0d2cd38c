"""-m gpu: resampling jumps in the known-frame scan (msd_sample_resample, msd_op_renoise, predict(keep=, resample=),
regenerate / vary(resample=)) against the specification of tests/resample_spec.py: tests/edit_spec.py's scan with RePaint's
schedule -- blocks of `jump` steps descended `times` times, the state diffused back up in between -- and one generator key
per pass.

Presets tiny / tiny_context: T = 64, n = 128, i.e. eight 1024-element blocks per row of the jump kernel and the sampler."""
import ctypes

import numpy as np
import pytest

import msd_amd
from tests import helpers, keep_spec, resample_spec
from tests.helpers import gpu_torch  # noqa: F401  (the `torch` fixture)

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------------------------------
# 1. the jump on its own
# --------------------------------------------------------------------------------------------------
# 14208 elements = 13 blocks of 1024 and a partial one (the kernel has no grid-stride loop: one float4 per thread)
@pytest.mark.parametrize('precision', ['f16x3', 'f16'])
def test_op_renoise_vs_spec(torch, precision):
  """msd_op_renoise against the specification's jump in float64 with its float32 evaluation as the yardstick
  (test_op_diffuse_to_step_vs_spec's criterion); the planes merge back to z."""
  from msd_amd import inference, native
  from oracle import backend
  n = 3 * 37 * 128
  shape = (1, n // 4, 4)
  spec = helpers.sampler_spec()
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, precision)
  _, dc = helpers.oracle_configs(spec)
  steps = dc.sampler.schedule.num_steps
  rng = np.random.default_rng(9)
  for lo, hi in ((0, 8), (6, 14), (steps - 4, steps), (steps - 1, steps)):
    z_in = rng.standard_normal(shape).astype(np.float32)
    eps = rng.standard_normal(shape).astype(np.float32)
    refs = {}
    for name, xp in (('f32', backend.NumpyBackend('float32')), ('f64', backend.NumpyBackend('float64'))):
      refs[name] = np.asarray(resample_spec.jump_state(xp, dc, xp.asarray(z_in), xp.asarray(eps), lo, hi), np.float64)
    z_t, zp_t = (torch.full(shape, float('nan'), dtype=torch.float32, device='cuda') for _ in range(2))
    native.op_renoise(cfg, lo, hi, helpers.dev(torch, z_in), helpers.dev(torch, eps), z_t, zp_t)
    z, zp = z_t.cpu().numpy(), zp_t.cpu().numpy()
    scale = max(1.0, float(np.abs(refs['f64']).max()))
    e_dev = np.abs(z.astype(np.float64) - refs['f64']).max() / scale
    e_f32 = np.abs(refs['f32'] - refs['f64']).max() / scale
    print('renoise %s %d -> %d: scaled error device %.3e / float32 %.3e' % (precision, lo, hi, e_dev, e_f32))
    assert e_dev <= 1e-6 + 4 * e_f32, (lo, hi, e_dev, e_f32)
    # the planes merge back to exactly what a hi / lo split of z holds (tests/helpers.py planes_merged); one plane: hi alone
    np.testing.assert_array_equal(helpers.bits(zp), helpers.bits(helpers.planes_merged(z, precision)))
    assert np.abs(zp - z).max() > 0   # (planes, not a copy of z)


@pytest.mark.parametrize('precision', ['f16x3', 'f16', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('side, target', helpers.RANGE_TARGETS, ids=[s for s, _ in helpers.RANGE_TARGETS])
def test_op_renoise_range_flag(torch, side, target, precision):
  """The range flag of renoise_kernel's tail: eps = 0 at one element of the launch's last float4, in a partial block, makes
  its output a * z there; z aims it 2^-12 below 65504 (passes) and 2^-12 above (RangeError with half planes)."""
  from msd_amd import inference, native
  from oracle import backend
  n = 3 * 37 * 128
  shape = (1, n // 4, 4)
  e = n - 2
  spec = helpers.sampler_spec()
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, precision)
  _, dc = helpers.oracle_configs(spec)
  lo, hi = 6, 14
  rng = np.random.default_rng(35)
  z_in = rng.standard_normal(shape).astype(np.float32)
  eps = rng.standard_normal(shape).astype(np.float32)
  xp64 = backend.NumpyBackend('float64')
  a64 = float(np.asarray(resample_spec.jump_coefs(xp64, dc.sampler.schedule, 1, lo, hi)[0]).reshape(-1)[0])
  eps.reshape(-1)[e] = 0.0
  z_in.reshape(-1)[e] = target / a64
  refs = {name: np.asarray(resample_spec.jump_state(xp, dc, xp.asarray(z_in), xp.asarray(eps), lo, hi), np.float64)
          for name, xp in (('f32', backend.NumpyBackend('float32')), ('f64', xp64))}

  def call():
    z_t, zp_t = (torch.full(shape, float('nan'), dtype=torch.float32, device='cuda') for _ in range(2))
    native.op_renoise(cfg, lo, hi, helpers.dev(torch, z_in), helpers.dev(torch, eps), z_t, zp_t)
    return z_t.cpu().numpy(), zp_t.cpu().numpy()
  helpers.check_range_case(call, side, precision, refs['f32'], refs['f64'], target, e)


def test_op_renoise_refuses_bad_levels(torch):
  from msd_amd import inference, native
  cfg = inference._to_native_config(helpers.sampler_spec(), msd_amd.audio_codecs.MelGAN(), 1, 'f16x3')
  t = [torch.zeros((1, 16, 4), dtype=torch.float32, device='cuda') for _ in range(4)]
  for lo, hi in ((-1, 4), (4, 4), (8, 4), (0, 51)):
    with pytest.raises(ValueError):
      native.op_renoise(cfg, lo, hi, *t)
  native.op_renoise(cfg, 0, 50, *t)


# --------------------------------------------------------------------------------------------------
# models and draws
# --------------------------------------------------------------------------------------------------
_models = {}


def _handle(spec, params):
  return msd_amd.InferenceModel(params, spec, batch_size=2, **helpers.ALL_PLANES)


def _model(torch, preset='tiny_context', steps=16, sampler='ddpm'):
  return helpers.cached_model(_models, preset, steps, sampler)


def _rows(b, seed, segment):
  """The (seed, stream id) of every fill of a draw and the rows each covers: one over all b rows for scalar keys, one per
  row for per-row keys."""
  if np.isscalar(seed) and np.isscalar(segment):
    return [(int(seed), int(segment), slice(0, b))]
  from msd_amd import native
  seeds, segments = native.row_keys(b, seed, segment)
  return [(seeds[r], segments[r], slice(r, r + 1)) for r in range(b)]


def _pass_draws(torch, rng, steps, b, seed, segment, passes, draws_noise=True, t=64):
  """(pass_noise, pass_eps) for the specification, under the keys of resample_spec.pass_key: 'philox' read back with
  msd_fill_normal, 'threefry' from the host's jax_random.  pass_eps[0] is the call's own initial draw."""
  from msd_amd import jax_random, native
  pass_noise, pass_eps = [], []
  for p in range(passes):
    eps = np.empty((b, t, 128), np.float32)
    nz = np.zeros((steps, b, t, 128), np.float32) if draws_noise else None
    for sd, sg, rows in _rows(b, seed, segment):
      key = resample_spec.pass_key(rng, sd, sg, steps, p)
      shape = (rows.stop - rows.start, t, 128)
      if rng == 'philox':
        buf = torch.empty(shape, dtype=torch.float32, device='cuda')
        native.fill_normal(buf, key[0], key[1], 0)
        eps[rows] = buf.cpu().numpy()
        for i in range(1, steps if draws_noise else 0):   # (scan index 0 draws nothing)
          native.fill_normal(buf, key[0], key[1], 1 + i)
          nz[i, rows] = buf.cpu().numpy()
      else:
        eps[rows] = jax_random.normal(key, shape)
        for i in range(1, steps if draws_noise else 0):
          nz[i, rows] = jax_random.normal(jax_random.fold_in(key, i), shape)
    pass_noise.append(nz)
    pass_eps.append(eps)
  return pass_noise, pass_eps


def _spec_refs(spec, params, batch, init_z, pass_noise, pass_eps, known, words, start, jump, times):
  from oracle import backend, fast
  cfg, dc = helpers.oracle_configs(spec)
  refs = []
  for dtype in ('float64', 'float32'):
    fm = fast.FastModel(backend.TorchBackend(dtype), cfg, dc, params, spec.has_context)
    refs.append(resample_spec.predict_resample(fm, batch, init_z, pass_noise, pass_eps, known, words, start, jump, times)[0])
  return refs


def _chain(torch, model_key, b, strength, want_start, jump, times, what, rng='philox', seed=4, segment=2, model=None,
           give_init_z=False, keep_mask=None):
  """One call with resampling against the specification.  Returns (got, known, words, (ref64, ref32), batch, call kwargs)."""
  from msd_amd import inference
  spec, params, shared = _model(torch, *model_key)
  model = model or shared
  steps = spec.diffusion.sampler.schedule.num_steps
  ddim = spec.diffusion.sampler.name == 'ddim'
  batch = helpers.make_batch(spec, batch=b, ctx_mask='ragged')
  known = helpers.known_mel((b, 64, 128))
  if keep_mask is not None:
    words, start = np.ascontiguousarray(keep_mask, np.int32), steps - 1
    kw = dict(keep=known, keep_mask=keep_mask)
  else:
    strength = np.broadcast_to(np.asarray(strength, np.float64), (b, 64))
    words, start = inference.plan_strength(strength, steps)
    kw = dict(keep=known, strength=strength)
  assert start == want_start
  passes = resample_spec.n_passes(start, jump, times)
  pass_noise, pass_eps = _pass_draws(torch, rng, steps, b, seed, segment, passes, draws_noise=not ddim)
  init_z = pass_eps[0]
  if give_init_z:
    init_z = helpers.make_noise(spec, batch=b)[0]
    kw['init_z'] = init_z
  kw.update(seed=seed, segment=segment, rng=rng)
  got, _ = model.predict(batch, resample=(jump, times), **kw)
  ref64, ref32 = _spec_refs(spec, params, batch, init_z, pass_noise, pass_eps, known, words, start, jump, times)
  verbatim = words == 1
  np.testing.assert_array_equal(helpers.bits(got[verbatim]), helpers.bits(known[verbatim]))
  assert np.isfinite(got).all()
  helpers.assert_fp32_class(got[~verbatim], ref64[~verbatim], ref32[~verbatim], what)
  return got, known, words, (ref64, ref32), batch, kw


# --------------------------------------------------------------------------------------------------
# 2. times = 1 is the call without resample
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rng', ['philox', 'threefry'])
@pytest.mark.parametrize('steps', [16, 20])   # 20 = two graphs and four singles
def test_times_one_is_the_call_without_resample(torch, steps, rng):
  """Through msd_sample_resample (predict hands (jump, 1) down): the bits of msd_sample_keep / msd_sample_edit."""
  spec, _, model = _model(torch, 'tiny_context', steps)
  for b, keys in ((1, dict(seed=4, segment=2)), (2, dict(seed=[4, 9], segment=[2, 0]))):
    batch = helpers.make_batch(spec, batch=b, ctx_mask='ragged')
    known, mask = helpers.known_mel((b, 64, 128)), keep_spec.parity_masks(b)
    strength = np.full((b, 64), 0.55)
    strength[0, :9] = 0.0
    for form in (dict(keep_mask=mask), dict(strength=strength), dict(strength=strength, init_z=helpers.make_noise(spec, batch=b)[0])):
      want, _ = model.predict(batch, rng=rng, keep=known, **form, **keys)
      for jump in (8, 3):
        got, _ = model.predict(batch, rng=rng, keep=known, resample=(jump, 1), **form, **keys)
        np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))


# --------------------------------------------------------------------------------------------------
# 3. chains against the specification
# --------------------------------------------------------------------------------------------------
_case_a = {}


def _run_case_a(torch, b, rng='philox'):
  """Case (a), run once per batch size and generator and shared (the references are the expensive part)."""
  if (b, rng) not in _case_a:
    keys = dict(seed=4, segment=2) if b == 1 else dict(seed=[4, 9], segment=[2, 0])
    _case_a[b, rng] = _chain(torch, ('tiny_context', 20), b, None, 19, 8, 2, 'resample (a) b=%d %s' % (b, rng), rng=rng,
                             keep_mask=keep_spec.parity_masks(b), **keys)
  return _case_a[b, rng]


@pytest.mark.parametrize('b,rng', [(1, 'philox'), (2, 'philox'), (2, 'threefry')])
def test_chain_graph_singles_and_a_short_last_block(torch, b, rng):
  """(a) N = 20, jump 8, times 2: blocks 8 / 8 / 4 = the 8-step graph and four single-step launches, 40 steps and 3 jumps.
  B = 1 under one key, B = 2 under per-row keys and both generators (the draws of the specification are made row by row,
  [1, T, n] each under its row's key: what the one-row calls draw)."""
  got, known, words, refs, batch, kw = _run_case_a(torch, b, rng)
  _, _, model = _model(torch, 'tiny_context', 20)
  plain, _ = model.predict(batch, resample=(8, 1), **kw)
  free = words == 0
  assert np.abs(got[free] - plain[free]).max() > 1e-2   # the jumps happened


def test_chain_singles_only_on_a_handle_without_the_single_step_graph(torch):
  """(b) N = 16, jump 4, times 3: 48 steps, all through the single-step graph, which a handle of N = 16 (two whole graphs)
  never captured before: a fresh handle whose first call is this one.  init_z given: it starts pass 0."""
  spec, params, _ = _model(torch, 'tiny_context', 16)
  _chain(torch, ('tiny_context', 16), 2, None, 15, 4, 3, 'resample (b)', model=_handle(spec, params), give_init_z=True,
         keep_mask=keep_spec.parity_masks(2))


def test_chain_part_way_start(torch):
  """(c) N = 20, strength 0.55: the call starts at scan index 10 -- level 11: blocks 8 / 3."""
  s = np.full((2, 64), 0.55)
  s[0, :12] = 0.0
  s[1, 40:] = 0.0
  got, known, _, _, _, _ = _chain(torch, ('tiny_context', 20), 2, s, 10, 8, 2, 'resample (c)')
  assert np.abs(got - known).max() > 1e-2


def test_chain_ramps_released_inside_resampled_blocks(torch):
  """(d) strengths 0 .. 1 across the frames: every frame is released at its own scan index, in every descent of its block."""
  s = np.stack([np.linspace(0.0, 1.0, 64), np.linspace(0.9, 0.05, 64) ** 2])
  s[1, 7] = 0.0
  got, known, words, _, _, _ = _chain(torch, ('tiny_context', 16), 2, s, 15, 8, 2, 'resample (d)', seed=[6, 7], segment=[1, 2])
  assert words[0, 0] == 1 and words[1, 7] == 1 and words[0, -1] == 0 and len(set(words.ravel().tolist())) >= 15


def test_chain_ddim_draws_in_its_jumps_alone(torch):
  """(e) DDIM, no context, N = 8, jump 4, times 2: the jumps draw, the steps do not."""
  got, known, words, _, _, _ = _chain(torch, ('tiny', 8, 'ddim'), 2, None, 7, 4, 2, 'resample (e) ddim',
                                      keep_mask=keep_spec.parity_masks(2))


def test_chain_threefry(torch):
  """(f) as (a) with B = 2 under one Threefry key: one draw over the whole [2, T, n] array per jump and step."""
  _chain(torch, ('tiny_context', 20), 2, None, 19, 8, 2, 'resample (f) threefry', rng='threefry', seed=5, segment=0,
         keep_mask=keep_spec.parity_masks(2))


# --------------------------------------------------------------------------------------------------
# 4. rows of a per-row-keyed call
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rng', ['philox', 'threefry'])
def test_rows_draw_under_their_own_keys_in_every_pass(torch, rng):
  """Twin rows (equal inputs) under keys (k0, k1) and (k1, k0): row 0 of one call is row 1 of the other, bit for bit -- a
  row's draws, the jumps' included, follow its key and not its position; equal keys give equal rows."""
  spec, _, model = _model(torch, 'tiny_context', 20)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ones')
  for v in batch.values():
    v[1] = v[0]
  known = helpers.known_mel((2, 64, 128))
  known[1] = known[0]
  mask = np.stack([keep_spec.parity_masks(1)[0]] * 2)
  kw = dict(keep=known, keep_mask=mask, resample=(8, 2), rng=rng)
  ab, _ = model.predict(batch, seed=[4, 9], segment=[2, 0], **kw)
  ba, _ = model.predict(batch, seed=[9, 4], segment=[0, 2], **kw)
  aa, _ = model.predict(batch, seed=[4, 4], segment=[2, 2], **kw)
  np.testing.assert_array_equal(helpers.bits(ab[0]), helpers.bits(ba[1]))
  np.testing.assert_array_equal(helpers.bits(ab[1]), helpers.bits(ba[0]))
  np.testing.assert_array_equal(helpers.bits(aa[0]), helpers.bits(aa[1]))
  np.testing.assert_array_equal(helpers.bits(aa[0]), helpers.bits(ab[0]))
  assert helpers.rms(ab[0], ab[1]) > 0.05


@pytest.mark.parametrize('rng', ['philox', 'threefry'])
def test_one_row_calls_are_the_rows_of_the_batched_call(torch, rng):
  """The one-row calls under (seed_b, segment_b), against row b of case (a)'s two-row specification, whose draws were
  made row by row: float32-class like the batched call itself (a batched launch rounds differently, so the two are not
  compared bit for bit).  Under both generators."""
  got2, _, words, (ref64, ref32), batch, kw = _run_case_a(torch, 2, rng)
  _, _, model = _model(torch, 'tiny_context', 20)
  for r in range(2):
    row = {k: v[r:r + 1] for k, v in batch.items()}
    one, _ = model.predict(row, keep=kw['keep'][r:r + 1], keep_mask=kw['keep_mask'][r:r + 1], seed=kw['seed'][r],
                           segment=kw['segment'][r], rng=kw['rng'], resample=(8, 2))
    free = words[r] != 1
    helpers.assert_fp32_class(one[0][free], ref64[r][free], ref32[r][free], 'one-row call of row %d, %s' % (r, rng))
    np.testing.assert_array_equal(helpers.bits(one[0][~free]), helpers.bits(got2[r][~free]))


# --------------------------------------------------------------------------------------------------
# 5. alternating calls on one handle
# --------------------------------------------------------------------------------------------------
def test_resample_calls_alternate_with_the_other_forms(torch):
  spec, params, _ = _model(torch, 'tiny_context', 16)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  known, mask = helpers.known_mel((2, 64, 128)), keep_spec.parity_masks(2)
  kw = dict(seed=[6, 7], segment=[1, 2])
  strength = np.full((2, 64), 0.25)
  strength[1, :10] = 0.0
  forms = [dict(), dict(keep=known, keep_mask=mask), dict(keep=known, strength=strength)]
  one = _handle(spec, params)
  before = [one.predict(batch, **kw, **c)[0] for c in forms]
  res = one.predict(batch, **kw, keep=known, keep_mask=mask, resample=(4, 2))[0]
  after = [one.predict(batch, **kw, **c)[0] for c in forms]
  for a, b in zip(before, after):
    np.testing.assert_array_equal(helpers.bits(a), helpers.bits(b))
  assert not np.array_equal(res, before[1])
  np.testing.assert_array_equal(helpers.bits(one.predict(batch, **kw, keep=known, keep_mask=mask, resample=(4, 2))[0]), helpers.bits(res))
  one._get_native().reset_graph()
  np.testing.assert_array_equal(helpers.bits(one.predict(batch, **kw, keep=known, keep_mask=mask, resample=(4, 2))[0]), helpers.bits(res))
  # a part-way call with resampling between them, and a fresh handle returns the same bits for it
  part = one.predict(batch, **kw, keep=known, strength=strength, resample=(3, 2))[0]
  np.testing.assert_array_equal(helpers.bits(_handle(spec, params).predict(batch, **kw, keep=known, strength=strength, resample=(3, 2))[0]),
                                helpers.bits(part))
  np.testing.assert_array_equal(helpers.bits(one.predict(batch, **kw)[0]), helpers.bits(before[0]))


# --------------------------------------------------------------------------------------------------
# 6. regenerate and vary
# --------------------------------------------------------------------------------------------------
def test_regenerate_and_vary_with_resampling_on_a_song(torch):
  from msd_amd import inference
  spec, _, model = _model(torch, 'tiny_context', 16)
  toks = [msd_amd.synthetic.segment_tokens(spec, k, min_len=8, max_len=126) for k in range(3)]
  song = helpers.known_mel((1, 192, 128), seed=8)
  got = model.regenerate(song, toks, 40, 100, seed=12, resample=(8, 2))
  assert got.shape == song.shape and got.dtype == np.float32 and np.isfinite(got).all()
  np.testing.assert_array_equal(helpers.bits(got[:, :40]), helpers.bits(song[:, :40]))
  np.testing.assert_array_equal(helpers.bits(got[:, 100:]), helpers.bits(song[:, 100:]))
  assert np.abs(got[:, 40:100] - song[:, 40:100]).max() > 1e-2
  assert np.abs(got[:, 40:100] - model.regenerate(song, toks, 40, 100, seed=12)[:, 40:100]).max() > 1e-2
  # composed by hand: segments 0 and 1, each with the song as it stands as context
  new = song.copy()
  for k, row in inference.plan_region(192, 64, 40, 100):
    batch = model._segment_batch(toks[k], None if k == 0 else torch.as_tensor(new[:, (k - 1) * 64:k * 64]).cuda(), k == 0)
    out, _ = model.predict(batch, seed=12, segment=k, keep=new[:, k * 64:(k + 1) * 64].copy(), keep_mask=row[None], resample=(8, 2))
    new[0, k * 64:(k + 1) * 64][row == 0] = out[0][row == 0]
  np.testing.assert_array_equal(helpers.bits(got), helpers.bits(new))
  # vary
  s = np.full(192, 0.5)
  s[50:80] = 0.0
  got = model.vary(song, toks, s, seed=12, resample=(4, 2))
  np.testing.assert_array_equal(helpers.bits(got[:, 50:80]), helpers.bits(song[:, 50:80]))
  assert np.abs(got - model.vary(song, toks, s, seed=12)).max() > 1e-2
  new = song.copy()
  for k in range(3):
    batch = model._segment_batch(toks[k], None if k == 0 else torch.as_tensor(new[:, (k - 1) * 64:k * 64]).cuda(), k == 0)
    out, _ = model.predict(batch, seed=12, segment=k, keep=new[:, k * 64:(k + 1) * 64].copy(), strength=s[None, k * 64:(k + 1) * 64],
                           resample=(4, 2))
    new[:, k * 64:(k + 1) * 64] = out
  np.testing.assert_array_equal(helpers.bits(got), helpers.bits(new))


# --------------------------------------------------------------------------------------------------
# 7. errors
# --------------------------------------------------------------------------------------------------
def test_errors(torch):
  from msd_amd import native
  spec, _, model = _model(torch, 'tiny_context', 16)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  known, mask = helpers.known_mel((2, 64, 128)), keep_spec.parity_masks(2)
  good, _ = model.predict(batch, keep=known, keep_mask=mask, resample=(4, 2))   # (encoded, buffers allocated)
  for bad in ((0, 2), (4, 0)):
    with pytest.raises(ValueError):
      model.predict(batch, keep=known, keep_mask=mask, resample=bad)
  with pytest.raises(ValueError, match='stream_id < 2\\^32'):
    model.predict(batch, keep=known, keep_mask=mask, resample=(4, 2), segment=1 << 32)
  with pytest.raises(ValueError, match='stream_id < 2\\^32'):
    model.predict(batch, keep=known, keep_mask=mask, resample=(4, 2), segment=[0, 1 << 32])
  model.predict(batch, keep=known, keep_mask=mask, resample=(4, 1), segment=1 << 32)          # no jump: any stream id
  model.predict(batch, keep=known, keep_mask=mask, resample=(4, 2), segment=1 << 32, rng='threefry')   # no stream id in the key
  # NativeModel.sample and the raw C call
  nm = model._get_native()
  out = torch.empty((2, 64, 128), dtype=torch.float32, device='cuda')
  known_t = helpers.dev(torch, known)
  words = np.ascontiguousarray(mask, np.int32)
  s = model._stream.cuda_stream
  for bad in ((0, 2), (4, 0), (4,), 4):
    with pytest.raises(ValueError):
      nm.sample(2, out, seed=1, keep=known_t, keep_mask=mask, resample=bad, stream=s)
  with pytest.raises(ValueError, match='resample needs keep'):
    nm.sample(2, out, seed=1, resample=(4, 2), stream=s)
  with pytest.raises(ValueError):
    nm.sample(2, out, seed=1, keep=known_t, keep_mask=mask, resample=(4, 2), steps=8, stream=s)
  with pytest.raises(ValueError):
    nm.sample(2, out, seed=1, keep=known_t, keep_mask=mask, resample=(4, 2), noise=torch.zeros((16, 2, 64, 128), device='cuda'), stream=s)
  lib, h = nm.lib, nm.handle
  one = (ctypes.c_uint64 * 1)(1)
  zero = (ctypes.c_uint64 * 1)(0)
  big = (ctypes.c_uint64 * 1)(1 << 32)
  wp = words.ctypes.data

  def raw(seeds=one, streams=zero, known_p=known_t.data_ptr(), words_p=wp, start=15, jump=4, times=2, out_p=out.data_ptr()):
    return lib.msd_sample_resample(h, 2, native.MSD_RNG_PHILOX, 0, seeds, streams, None, known_p, words_p, start, jump, times, out_p, s)

  assert raw() == 0
  model._stream.synchronize()
  first = out.cpu().numpy().copy()
  inval = native.MSD_ERR_INVALID_ARGUMENT
  assert raw(jump=0) == inval and b'jump' in lib.msd_last_error(h)
  assert raw(times=0) == inval and raw(jump=-3) == inval and raw(times=-1) == inval
  assert raw(streams=big) == inval and b'2^32' in lib.msd_last_error(h)
  assert raw(streams=big, times=1) == 0
  assert raw(seeds=None) == inval and raw(known_p=None) == inval and raw(words_p=None) == inval and raw(out_p=None) == inval
  assert raw(start=16) == inval and raw(start=-2) == inval
  assert lib.msd_sample_resample(None, 2, 0, 0, one, zero, None, known_t.data_ptr(), wp, 15, 4, 2, out.data_ptr(), s) == inval
  # a jump beyond the call's steps -- INT_MAX, the natural "one block" -- is the one-block call, bit for bit; beyond an int it
  # is refused before the entry point
  assert raw(jump=16) == 0
  model._stream.synchronize()
  one_block = out.cpu().numpy().copy()
  assert not np.array_equal(one_block, first)
  assert raw(jump=2 ** 31 - 1) == 0
  model._stream.synchronize()
  np.testing.assert_array_equal(helpers.bits(out.cpu().numpy()), helpers.bits(one_block))
  part_way = np.full((2, 64), 3, np.int32)   # (a part-way start wants every frame known at the steps it skips)
  assert raw(jump=2 ** 31 - 1, times=3, start=4, words_p=part_way.ctypes.data) == 0   # ... and with more passes than the call before
  model._stream.synchronize()
  wide, _ = model.predict(batch, keep=known, keep_mask=mask, resample=(2 ** 31 - 1, 2))
  np.testing.assert_array_equal(helpers.bits(wide), helpers.bits(model.predict(batch, keep=known, keep_mask=mask, resample=(16, 2))[0]))
  for bad in ((2 ** 31, 2), (4, 2 ** 31)):
    with pytest.raises(ValueError, match='32-bit'):
      model.predict(batch, keep=known, keep_mask=mask, resample=bad)
  # a handle whose sampler is dpmpp_2m refuses known frames, with or without jumps: through predict, NativeModel.sample and
  # the raw C call; its plain call still runs afterwards
  spec_ms, _, model_ms = _model(torch, 'tiny_context', 16, 'dpmpp_2m')
  plain_ms, _ = model_ms.predict(batch, seed=3)
  with pytest.raises(NotImplementedError):
    model_ms.predict(batch, keep=known, keep_mask=mask, resample=(4, 2))
  nm_ms, s_ms = model_ms._get_native(), model_ms._stream.cuda_stream
  with pytest.raises(NotImplementedError):
    nm_ms.sample(2, out, seed=1, keep=known_t, keep_mask=mask, resample=(4, 2), stream=s_ms)
  assert nm_ms.lib.msd_sample_resample(nm_ms.handle, 2, native.MSD_RNG_PHILOX, 0, one, zero, None, known_t.data_ptr(), wp, 15, 4, 2,
                                       out.data_ptr(), s_ms) == 6   # MSD_ERR_UNSUPPORTED
  assert b'known frames' in nm_ms.lib.msd_last_error(nm_ms.handle)
  np.testing.assert_array_equal(helpers.bits(model_ms.predict(batch, seed=3)[0]), helpers.bits(plain_ms))
  # the handle still runs, and returns the same bits
  assert raw() == 0
  model._stream.synchronize()
  np.testing.assert_array_equal(helpers.bits(out.cpu().numpy()), helpers.bits(first))
  again, _ = model.predict(batch, keep=known, keep_mask=mask, resample=(4, 2))
  np.testing.assert_array_equal(helpers.bits(again), helpers.bits(good))


# --------------------------------------------------------------------------------------------------
# 8. base-size tiles
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def base(torch):
  """One base_with_context handle of 4 steps: T = 256, 32 blocks per row in the jump kernel, the base tile family."""
  spec = msd_amd.config.preset('base_with_context', num_steps=4)
  params = msd_amd.synthetic.init_params(spec, 21, norm_scale_jitter=0.1)
  model = msd_amd.InferenceModel(params, spec, batch_size=1, **helpers.ALL_PLANES)
  yield spec, params, model
  del model
  torch.cuda.empty_cache()


def test_base_size_call(torch, base):
  """N = 4, jump 8, times 2: one short block of four steps, descended twice with the jump from level 0 (x0) back to level 4
  between the descents, float32-class against the specification.  (Few steps: the two references of 8 steps each are
  nearly all of this test's time, as in test_gpu_few_steps.py's base-size case.)"""
  from oracle import backend, fast
  spec, params, model = base
  batch = helpers.make_batch(spec, batch=1, ctx_mask='ragged')
  known = helpers.known_mel((1, 256, 128))
  mask = np.zeros((1, 256), np.int32)
  mask[0, :100] = 1
  mask[0, 200:] = 1
  pass_noise, pass_eps = _pass_draws(torch, 'philox', 4, 1, 4, 2, resample_spec.n_passes(3, 8, 2), t=256)
  got, _ = model.predict(batch, seed=4, segment=2, keep=known, keep_mask=mask, resample=(8, 2))
  cfg, dc = helpers.oracle_configs(spec)
  refs = []
  for dtype in ('float64', 'float32'):
    fm = fast.FastModel(backend.TorchBackend(dtype), cfg, dc, params, True)
    refs.append(resample_spec.predict_resample(fm, batch, pass_eps[0], pass_noise, pass_eps, known, mask, 3, 8, 2)[0])
    del fm
  free = mask == 0
  np.testing.assert_array_equal(helpers.bits(got[~free]), helpers.bits(known[~free]))
  helpers.assert_fp32_class(got[free], refs[0][free], refs[1][free], 'base_with_context, resample (8, 2) of 4 steps')
