"""-m gpu: edit strength (msd_sample_edit, msd_op_sampler_step_release, msd_op_diffuse_to_step, predict(strength=), vary,
regenerate(blend_frames=)) against the specification of tests/edit_spec.py: tests/keep_spec.py's x0-replacement with
keep := (i >= f) per step, a scan from start_step down and the known mel diffused to the start index.

Presets tiny / tiny_context: T = 64, n = 128, i.e. eight 1024-element sampler blocks per row, 32 threads per frame."""
import numpy as np
import pytest

import msd_amd
from tests import edit_spec, helpers, keep_spec
from tests.helpers import gpu_torch  # noqa: F401  (the `torch` fixture)

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------------------------------
# 1. one update with release words
# --------------------------------------------------------------------------------------------------
OP_CASES = [dict(), dict(sampler='ddim'), dict(model_output='v'), dict(model_output='x0'), dict(cfg_weight=1.0),
            dict(sampler='ddim', clip=False, cfg_weight=1.0), dict(logvar='small')]


@pytest.mark.parametrize('case', OP_CASES, ids=lambda c: ','.join('%s=%s' % kv for kv in c.items()) or 'default')
def test_op_release_is_the_keep_op_or_the_plain_op_per_frame(torch, case):
  """msd_op_sampler_step_release at the first, a middle, the second-to-last and the last scan index, words 0, 1, i, i + 1
  and i + 2 in another pattern per row: a frame with i >= v - 1 (v >= 1) holds msd_op_sampler_step_keep's bits with flag
  1, every other frame msd_op_sampler_step's; at i == 0 only v == 1 frames are the known values' bits."""
  from msd_amd import inference, native
  spec = helpers.sampler_spec(**case)
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, 'f16x3')
  steps = spec.diffusion.sampler.schedule.num_steps
  two_pass = spec.diffusion.classifier_free_guidance.eval_condition_weight != 1
  rng = np.random.default_rng(5)
  shape = (2, 16, 128)
  for i in (steps - 1, steps // 2, 1, 0):
    kinds = np.array([0, 1, i, i + 1, i + 2], np.int32)
    words = np.stack([kinds[np.arange(16) % 5], kinds[(3 * np.arange(16) + 2) % 5]])   # two row patterns, every word in each
    known_now = (words >= 1) & (i >= words - 1)
    assert known_now.any() and (~known_now).any() and (words[known_now] > 1).any() == (i > 0)
    z, oc, ou, nz = (rng.standard_normal(shape).astype(np.float32) for _ in range(4))
    xk = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    args = (helpers.dev(torch, z), helpers.dev(torch, oc), helpers.dev(torch, ou) if two_pass else None, helpers.dev(torch, nz))
    xk_t = helpers.dev(torch, xk)
    outs = {}
    for name in ('release', 'keep', 'plain'):
      outs[name] = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    native.op_sampler_step_release(cfg, i, *args, xk_t, helpers.dev(torch, words, np.int32), outs['release'])
    native.op_sampler_step_keep(cfg, i, *args, xk_t, helpers.dev(torch, 7 * np.ones((2, 16)), np.int32), outs['keep'])   # (any non-zero flag)
    native.op_sampler_step(cfg, i, *args, outs['plain'])
    got, keep, plain = (outs[k].cpu().numpy() for k in ('release', 'keep', 'plain'))
    kn = np.broadcast_to(known_now[..., None], shape)
    np.testing.assert_array_equal(helpers.bits(got[kn]), helpers.bits(keep[kn]))
    np.testing.assert_array_equal(helpers.bits(got[~kn]), helpers.bits(plain[~kn]))
    assert not np.array_equal(keep[kn], plain[kn])   # (the two differ where it matters)
    if i == 0:
      np.testing.assert_array_equal(known_now, words == 1)
      np.testing.assert_array_equal(helpers.bits(got[kn]), helpers.bits(xk[kn]))
      assert not np.array_equal(got[~kn], xk[~kn])


# --------------------------------------------------------------------------------------------------
# 2. the part-way start on its own
# --------------------------------------------------------------------------------------------------
# 14208 elements = 13 blocks of 1024 and a partial one; 2048 * 1024 + 4 * 333: past the launch's grid cap of 2048 blocks (the
# grid-stride loop's second trip, partial)
@pytest.mark.parametrize('precision', ['f16x3', 'f16'])
@pytest.mark.parametrize('n', [3 * 37 * 128, 2048 * 1024 + 4 * 333], ids=['odd', 'past_the_grid_cap'])
def test_op_diffuse_to_step_vs_spec(torch, n, precision):
  """msd_op_diffuse_to_step against the specification's start state in float64 with its float32 evaluation as the
  yardstick (the sampler ops' criterion); xk holds the bits of scale_clip_kernel's expression; the planes merge back to z."""
  from msd_amd import inference, native
  from oracle import backend, predict
  shape = (1, n // 4, 4)
  spec = helpers.sampler_spec()
  codec = predict.MelGANCodec()
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, precision)
  _, dc = helpers.oracle_configs(spec)
  steps = dc.sampler.schedule.num_steps
  rng = np.random.default_rng(9)
  mel = rng.uniform(-13.0, 5.0, shape).astype(np.float32)
  assert (mel > 4.0).any() and (mel < np.log(1e-5)).any()   # beyond the codec's range at both ends
  eps = rng.standard_normal(shape).astype(np.float32)
  # scale_clip_kernel's expression, every operation rounded to float32 (IEEE on both sides)
  fmin, fmax = np.float32(cfg.feature_min), np.float32(cfg.feature_max)
  xk_bits = (np.clip(mel, fmin, fmax) - fmin) / (fmax - fmin) * np.float32(2.0) + np.float32(-1.0)
  assert xk_bits.dtype == np.float32 and xk_bits.min() == -1.0 and xk_bits.max() == 1.0
  for i in (steps - 2, steps // 2, 1, 0):
    refs = {}
    for name, xp in (('f32', backend.NumpyBackend('float32')), ('f64', backend.NumpyBackend('float64'))):
      xk = codec.scale_features(xp, xp.asarray(mel), (-1., 1.), clip=True)
      refs[name] = np.asarray(edit_spec.start_state(xp, dc, xk, xp.asarray(eps), i), np.float64)
    z_t, zp_t, xk_t = (torch.full(shape, float('nan'), dtype=torch.float32, device='cuda') for _ in range(3))
    native.op_diffuse_to_step(cfg, i, helpers.dev(torch, mel), helpers.dev(torch, eps), z_t, zp_t, xk_t)
    z, zp, xk_dev = z_t.cpu().numpy(), zp_t.cpu().numpy(), xk_t.cpu().numpy()
    np.testing.assert_array_equal(helpers.bits(xk_dev), helpers.bits(xk_bits))
    scale = max(1.0, float(np.abs(refs['f64']).max()))
    e_dev = np.abs(z.astype(np.float64) - refs['f64']).max() / scale
    e_f32 = np.abs(refs['f32'] - refs['f64']).max() / scale
    print('diffuse n=%d %s i=%d: scaled error device %.3e / float32 %.3e' % (n, precision, i, e_dev, e_f32))
    assert e_dev <= 1e-6 + 4 * e_f32, (i, e_dev, e_f32)
    # the planes merge back to exactly what a hi / lo split of z holds (tests/helpers.py planes_merged); one plane: hi alone
    np.testing.assert_array_equal(helpers.bits(zp), helpers.bits(helpers.planes_merged(z, precision)))
    assert np.abs(zp - z).max() > 0   # (planes, not a copy of z)


@pytest.mark.parametrize('precision', ['f16x3', 'f16', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('side, target', helpers.RANGE_TARGETS, ids=[s for s, _ in helpers.RANGE_TARGETS])
def test_op_diffuse_to_step_range_flag(torch, side, target, precision):
  """The range flag of diffuse_to_step_kernel's tail (xk is clipped to [-1, 1], so the large value comes through eps): one
  element of the launch's last float4, in a partial block, aimed 2^-12 below 65504 (passes) and 2^-12 above (RangeError
  with half planes)."""
  from msd_amd import inference, native
  from oracle import backend, predict
  n = 3 * 37 * 128
  shape = (1, n // 4, 4)
  e = n - 2
  spec = helpers.sampler_spec()
  codec = predict.MelGANCodec()
  cfg = inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, precision)
  _, dc = helpers.oracle_configs(spec)
  i = dc.sampler.schedule.num_steps // 2
  rng = np.random.default_rng(33)
  mel = rng.uniform(-13.0, 5.0, shape).astype(np.float32)
  eps = rng.standard_normal(shape).astype(np.float32)

  def spec_of(xp):
    xk = codec.scale_features(xp, xp.asarray(mel), (-1., 1.), clip=True)
    return np.asarray(edit_spec.start_state(xp, dc, xk, xp.asarray(eps), i), np.float64)
  xp64 = backend.NumpyBackend('float64')
  eps.reshape(-1)[e] = 0.0
  mean64 = spec_of(xp64).reshape(-1)[e]   # alpha * xk there
  sigma64 = float(np.asarray(edit_spec.start_coefs(xp64, dc, 1, i)[1]).reshape(-1)[0])
  eps.reshape(-1)[e] = (target - mean64) / sigma64

  def call():
    z_t, zp_t, xk_t = (torch.full(shape, float('nan'), dtype=torch.float32, device='cuda') for _ in range(3))
    native.op_diffuse_to_step(cfg, i, helpers.dev(torch, mel), helpers.dev(torch, eps), z_t, zp_t, xk_t)
    return z_t.cpu().numpy(), zp_t.cpu().numpy()
  helpers.check_range_case(call, side, precision, spec_of(backend.NumpyBackend('float32')), spec_of(xp64), target, e)


# --------------------------------------------------------------------------------------------------
# models
# --------------------------------------------------------------------------------------------------
_models = {}


def _handle(spec, params):
  return msd_amd.InferenceModel(params, spec, batch_size=2, **helpers.ALL_PLANES)


def _model(torch, preset='tiny_context', steps=16, sampler='ddpm'):
  return helpers.cached_model(_models, preset, steps, sampler)


# --------------------------------------------------------------------------------------------------
# 3. strength = 1 - mask is the keep call
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rng', ['philox', 'threefry'])
@pytest.mark.parametrize('steps', [16, 10])   # 10 = 8 + the remainder graph
def test_strength_one_minus_mask_is_the_keep_call(torch, steps, rng):
  spec, _, model = _model(torch, 'tiny_context', steps)
  for b, keys in ((1, dict(seed=4, segment=2)), (2, dict(seed=4, segment=2)), (2, dict(seed=[4, 9], segment=[2, 0]))):
    batch = helpers.make_batch(spec, batch=b, ctx_mask='ragged')
    known, mask = helpers.known_mel((b, 64, 128)), keep_spec.parity_masks(b)
    want, _ = model.predict(batch, rng=rng, keep=known, keep_mask=mask, **keys)
    got, _ = model.predict(batch, rng=rng, keep=known, strength=1.0 - mask, **keys)
    np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))
    # ... and strength 1 with the mask beside it: the mask's frames get strength 0
    got, _ = model.predict(batch, rng=rng, keep=known, strength=1.0, keep_mask=mask, **keys)
    np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))


# --------------------------------------------------------------------------------------------------
# 4. part-way chains against the specification
# --------------------------------------------------------------------------------------------------
def _spec_refs(spec, params, batch, init_z, noise, known, words, start):
  from oracle import backend, fast
  cfg, dc = helpers.oracle_configs(spec)
  refs = []
  for dtype in ('float64', 'float32'):
    fm = fast.FastModel(backend.TorchBackend(dtype), cfg, dc, params, spec.has_context)
    refs.append(edit_spec.predict_edit(fm, batch, init_z, noise, known, words, start)[0])
  return refs


def _chain(torch, model_key, b, strength, want_start, what, model=None):
  from msd_amd import inference
  spec, params, shared = _model(torch, *model_key)
  model = model or shared
  steps = spec.diffusion.sampler.schedule.num_steps
  batch = helpers.make_batch(spec, batch=b, ctx_mask='ragged')
  init_z, noise = helpers.make_noise(spec, batch=b)
  if spec.diffusion.sampler.name == 'ddim':
    noise = None
  known = helpers.known_mel((b, 64, 128))
  strength = np.broadcast_to(np.asarray(strength, np.float64), (b, 64))
  words, start = inference.plan_strength(strength, steps)
  assert start == want_start
  got, _ = model.predict(batch, init_z=init_z, noise=noise, keep=known, strength=strength)
  ref64, ref32 = _spec_refs(spec, params, batch, init_z, noise, known, words, start)
  verbatim = words == 1
  np.testing.assert_array_equal(helpers.bits(got[verbatim]), helpers.bits(known[verbatim]))
  assert np.isfinite(got).all()
  helpers.assert_fp32_class(got[~verbatim], ref64[~verbatim], ref32[~verbatim], what)
  return got, known, words


@pytest.mark.parametrize('b', [1, 2])
def test_chain_one_graph_and_three_singles(torch, b):
  """N = 20, strength 0.55: 11 steps from scan index 10 = one 8-step graph and three single-step launches."""
  got, known, _ = _chain(torch, ('tiny_context', 20), b, 0.55, 10, 'edit N=20 s=0.55 b=%d' % b)
  assert np.abs(got - known).max() > 1e-2


def test_chain_singles_only_on_a_handle_without_the_single_step_graph(torch):
  """N = 16, strength 0.25: 4 steps, all through the single-step graph, which a handle of N = 16 (two whole graphs)
  never captured before: a fresh handle whose first call is this one."""
  spec, params, _ = _model(torch, 'tiny_context', 16)
  _chain(torch, ('tiny_context', 16), 2, 0.25, 3, 'edit N=16 s=0.25', model=_handle(spec, params))


def test_chain_the_graph_alone(torch):
  """N = 16, strength 0.5: 8 steps = one launch of the 8-step graph."""
  _chain(torch, ('tiny_context', 16), 2, 0.5, 7, 'edit N=16 s=0.5')


def test_chain_ramps_from_the_full_scan(torch):
  """Strengths 0 .. 1 across row 0's frames and another ramp in row 1: the call starts at N - 1 from init_z and every
  frame is released at its own step; strength-0 frames are the caller's bits."""
  s = np.stack([np.linspace(0.0, 1.0, 64), np.linspace(0.9, 0.05, 64) ** 2])
  s[1, 7] = 0.0
  got, known, words = _chain(torch, ('tiny_context', 16), 2, s, 15, 'edit ramps')
  assert words[0, 0] == 1 and words[1, 7] == 1 and words[0, -1] == 0 and len(set(words.ravel().tolist())) >= 15
  np.testing.assert_array_equal(helpers.bits(got[0, 0]), helpers.bits(known[0, 0]))
  np.testing.assert_array_equal(helpers.bits(got[1, 7]), helpers.bits(known[1, 7]))


def test_chain_ddim_without_context(torch):
  """DDIM, no context, N = 8: a part-way start (5 steps: singles only) with strength-0 frames in both rows."""
  s = np.full((2, 64), 0.6)
  s[0, :9] = 0.0
  s[1, 30:41] = 0.0
  s[1, 50:] = 0.3
  got, known, words = _chain(torch, ('tiny', 8, 'ddim'), 2, s, 4, 'edit ddim')
  assert (words == 1).sum() == 20
  np.testing.assert_array_equal(helpers.bits(got[0, :9]), helpers.bits(known[0, :9]))
  np.testing.assert_array_equal(helpers.bits(got[1, 30:41]), helpers.bits(known[1, 30:41]))


def test_generated_draws_start_the_part_way_call(torch):
  """Without init_z the part-way start's eps is the draw the full call starts from: the Philox / Threefry fill, per row under
  per-row keys -- the call with that draw given explicitly returns the same bits."""
  from msd_amd import native
  spec, _, model = _model(torch, 'tiny_context', 16)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  known = helpers.known_mel((2, 64, 128))
  rows = [torch.empty((64, 128), dtype=torch.float32, device='cuda') for _ in range(2)]
  for b, (seed, segment) in enumerate([(4, 2), (9, 0)]):
    native.fill_normal(rows[b], seed, segment, 0)
  z_rows = torch.stack(rows)
  got, _ = model.predict(batch, seed=[4, 9], segment=[2, 0], keep=known, strength=0.5)
  # (the step noise is keyed by the same rows: sub-sequence 1 + i, drawn in the kernel either way)
  want, _ = model.predict(batch, seed=[4, 9], segment=[2, 0], keep=known, strength=0.5, init_z=z_rows)
  np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))
  whole = torch.empty((2, 64, 128), dtype=torch.float32, device='cuda')
  native.fill_normal_threefry(whole, 4)
  got, _ = model.predict(batch, seed=4, rng='threefry', keep=known, strength=0.5)
  want, _ = model.predict(batch, seed=4, rng='threefry', keep=known, strength=0.5, init_z=whole)
  np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))
  assert np.abs(got - known).max() > 1e-2


# --------------------------------------------------------------------------------------------------
# 5. plain, keep and edit calls on one handle
# --------------------------------------------------------------------------------------------------
def test_plain_keep_and_edit_calls_alternate_on_one_handle(torch):
  """N = 16 has no single-step graph until the part-way call needs it: the plain call after that capture returns the bits
  of the plain call before it, and every call the bits a fresh handle returns."""
  spec, params, _ = _model(torch, 'tiny_context', 16)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  known, mask = helpers.known_mel((2, 64, 128)), keep_spec.parity_masks(2)
  kw = dict(seed=[6, 7], segment=[1, 2])
  strength = np.full((2, 64), 0.25)
  strength[1, :10] = 0.0
  calls = [dict(), dict(keep=known, keep_mask=mask), dict(keep=known, strength=strength), dict()]
  one = _handle(spec, params)
  runs = [one.predict(batch, **kw, **c)[0] for c in calls]
  fresh = [_handle(spec, params).predict(batch, **kw, **c)[0] for c in calls[:3]]
  for k in range(3):
    np.testing.assert_array_equal(helpers.bits(runs[k]), helpers.bits(fresh[k]))
  np.testing.assert_array_equal(helpers.bits(runs[3]), helpers.bits(runs[0]))
  assert not np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[1], runs[2])
  # and once more round: the cached graphs of all three forms replay
  again = [one.predict(batch, **kw, **c)[0] for c in calls[1:3]]
  np.testing.assert_array_equal(helpers.bits(again[0]), helpers.bits(runs[1]))
  np.testing.assert_array_equal(helpers.bits(again[1]), helpers.bits(runs[2]))


# --------------------------------------------------------------------------------------------------
# 6. vary and regenerate(blend_frames=)
# --------------------------------------------------------------------------------------------------
def test_vary_and_blended_regenerate_on_a_song(torch):
  from msd_amd import inference
  spec, _, model = _model(torch, 'tiny_context', 8)
  toks = [msd_amd.synthetic.segment_tokens(spec, k, min_len=8, max_len=126) for k in range(3)]
  song = helpers.known_mel((1, 192, 128), seed=8)
  # vary at full strength is predict_sequence
  want = model.predict_sequence(toks, seed=12)
  got = model.vary(song, toks, 1.0, seed=12)
  assert got.shape == song.shape and got.dtype == np.float32
  np.testing.assert_array_equal(helpers.bits(got), helpers.bits(want))
  # a variation: strength 0.5 but for a stretch of strength 0, which is the input's
  s = np.full(192, 0.5)
  s[50:80] = 0.0
  got = model.vary(song, toks, s, seed=12)
  assert got.shape == song.shape and np.isfinite(got).all()
  np.testing.assert_array_equal(helpers.bits(got[:, 50:80]), helpers.bits(song[:, 50:80]))
  assert np.abs(got[:, :50] - song[:, :50]).max() > 1e-2 and np.abs(got[:, :50] - want[:, :50]).max() > 1e-2
  np.testing.assert_array_equal(helpers.bits(model.vary(song, toks, 0.0, seed=12)), helpers.bits(song))
  # regenerate: blend_frames = 0 is the call as it was
  hard = model.regenerate(song, toks, 40, 100, seed=12)
  np.testing.assert_array_equal(helpers.bits(model.regenerate(song, toks, 40, 100, seed=12, blend_frames=0)), helpers.bits(hard))
  # a ramp of 15 frames: strengths 15/16 .. 1/16; at N = 8 the outermost (1/16 -> 0.5 -> one step) is still released
  soft = model.regenerate(song, toks, 40, 100, seed=12, blend_frames=15)
  assert soft.shape == song.shape and np.isfinite(soft).all()
  np.testing.assert_array_equal(helpers.bits(soft[:, :25]), helpers.bits(song[:, :25]))
  np.testing.assert_array_equal(helpers.bits(soft[:, 115:]), helpers.bits(song[:, 115:]))
  assert np.abs(soft[:, 25:40] - song[:, 25:40]).max() > 1e-3 and np.abs(soft[:, 100:115] - song[:, 100:115]).max() > 1e-3
  plan = inference.region_strength(192, 64, 40, 100, 15)
  assert [k for k, _ in plan] == [0, 1]
  # a region whose ramp alone reaches segment 2: that segment is sampled too, its frames beyond the ramp untouched
  soft = model.regenerate(song, toks, 100, 128, seed=12, blend_frames=3)
  assert np.abs(soft[:, 128:131] - song[:, 128:131]).max() > 1e-3
  np.testing.assert_array_equal(helpers.bits(soft[:, 131:]), helpers.bits(song[:, 131:]))
  np.testing.assert_array_equal(helpers.bits(soft[:, :97]), helpers.bits(song[:, :97]))


# --------------------------------------------------------------------------------------------------
# 7. errors
# --------------------------------------------------------------------------------------------------
def test_errors(torch):
  spec, _, model = _model(torch, 'tiny_context', 16)
  batch = helpers.make_batch(spec, batch=2, ctx_mask='ragged')
  known = helpers.known_mel((2, 64, 128))
  with pytest.raises(ValueError, match='strength needs keep'):
    model.predict(batch, strength=0.5)
  with pytest.raises(ValueError):
    model.predict(batch, keep=known, strength=np.full((2, 64), 1.25))
  # the library's own checks, through native directly
  good, _ = model.predict(batch, keep=known, strength=0.25)   # (encoded, buffers allocated)
  nm = model._get_native()
  out = torch.empty((2, 64, 128), dtype=torch.float32, device='cuda')
  known_t = helpers.dev(torch, known)
  words = np.full((2, 64), 3, np.int32)
  s = model._stream.cuda_stream

  def call(words, start):
    nm.sample(2, out, seed=1, keep=known_t, release=words, start_step=start, stream=s)

  call(words, 3)   # 1 <= v <= start + 2
  for bad_word, start in ((0, 3), (6, 3), (17, 15), (-1, 15)):   # free at a skipped step (twice); beyond N; negative
    bad = words.copy()
    bad[1, 5] = bad_word
    with pytest.raises(ValueError, match='release word %d of row 1, frame 5' % bad_word):
      call(bad, start)
  for start in (16, -2):
    with pytest.raises(ValueError, match='start_step'):
      call(words, start)
  with pytest.raises(ValueError, match='release word 3'):
    call(words, -1)                                  # no step runs only where every frame is known throughout
  call(np.ones((2, 64), np.int32), -1)
  model._stream.synchronize()
  np.testing.assert_array_equal(helpers.bits(out.cpu().numpy()), helpers.bits(known))
  with pytest.raises(ValueError):
    nm.sample(2, out, seed=1, keep=known_t, release=words[:1], start_step=3, stream=s)
  with pytest.raises(ValueError):
    nm.sample(2, out, seed=1, start_step=3, stream=s)
  # the handle still works
  again, _ = model.predict(batch, keep=known, strength=0.25)
  np.testing.assert_array_equal(helpers.bits(again), helpers.bits(good))
