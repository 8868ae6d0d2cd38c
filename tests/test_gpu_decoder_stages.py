"""-m gpu: the WIRED decoder step (csrc/msd_api.hip in_proj, self_attention_block, cross_attention_block, mlp_block,
final_projection under plan_step -- the argument fillers the product uses, not standalone_ops.h's), buffer by buffer
against float64.  The cases, the layouts and the reference are tests/decoder_stage_cases.py's (proven without a GPU in
tests/test_decoder_stage_cases_host.py).

Bounds.  The reference is FastModel(float64), the yardstick FastModel(float32, precision = the handle's), and BOTH run
on the device's own FiLM table (set_film(debug_read('film'))): the float32 time signal of a table puts 5e-5 between any
two evaluations that build their own, a hundred times the arithmetic's 5e-7 (the table itself is held by
test_film_table_matches_oracle and the load-time table tests).  Asserted per buffer, pass and song:
  device statistic <= FACTOR x yardstick statistic      (encode_cases.stats: rms and largest error over the reference's rms)
FACTOR: twice the worst ratio measured on the MI355X (profiles/decoder_stages.log: the worst ratio per spec, kind of call,
precision and buffer), rounded up to one digit and never above 4.  One activation operand of ONE launch on one plane is
150 .. 800 x the yardstick at the buffer the launch writes (test_decoder_stage_cases_host.py), the next arithmetic class 10 x (bf16x3) and 500 x (f16)."""
import time

import numpy as np
import pytest

import msd_amd
from tests import decoder_stage_cases as dc
from tests import helpers
from tests.helpers import gpu_torch  # noqa: F401 -- the `torch` fixture

pytestmark = pytest.mark.gpu

# device statistic <= FACTOR x yardstick statistic (rule above).  Worst measured ratios (profiles/decoder_stages.log,
# condensed from 2094 figures; each the largest-error statistic of one buffer of one song):
#   f16x3 2.57 (W depth 2, single pass) -> 5.14, capped at 4   bf16x3 1.78 (N depth 1) -> 3.56 -> 4   f16 1.81 (N depth 1) -> 3.62 -> 4
FACTOR = {'f16x3': 4.0, 'bf16x3': 4.0, 'f16': 4.0}
BATCH_BAR = 2e-5   # a song in a batch against the same song alone (tests/test_gpu_batched_base.py)

_oracles, _expected, _songs, _alone = {}, {}, {}, {}
_wall = {'oracle': 0.0, 'device': 0.0}


class _timed:
  def __init__(self, what):
    self.what = what

  def __enter__(self):
    self.t0 = time.perf_counter()

  def __exit__(self, *a):
    _wall[self.what] += time.perf_counter() - self.t0


def _wall_line(what):
  print('[stage-wall] after %s: oracle %.1f s, device %.1f s (cumulative over the module)' % (what, _wall['oracle'], _wall['device']))


def songs(name):
  if name not in _songs:
    _songs[name] = dc.songs(name)
  return _songs[name]


def _exp(call, j, p, dtype, precision, film):
  """decoder_stage_cases.expected of song j in pass p of `call`, in the arithmetic (dtype, precision) on the table
  `film`; computed once per module and left unchanged."""
  cond = call.pass_cond(p)
  key = (call.name, call.depth, j, call.step, cond, dtype, precision, film.tobytes())
  if key not in _expected:
    with _timed('oracle'):
      okey = (call.name, call.depth, dtype, precision)
      if okey not in _oracles:
        fm = dc.make_oracle(call.name, call.depth, dtype, precision, torch_backend=True)
        dc.encode_songs(fm, songs(call.name)[0], range(dc.N_SONGS))
        _oracles[okey] = fm
      fm = _oracles[okey]
      fm.set_film(film)
      tr = dc.trace_song(fm, songs(call.name)[1][j], call.step, cond, j)
      if fm.kv[j] is None or not cond:
        assert tr['x2'][call.depth - 1] is tr['x1'][call.depth - 1]   # no valid key: the cross update is exactly zero
      _expected[key] = dc.expected(fm, tr, call.depth - 1)
  return _expected[key]


def _model(call, batch=None):
  spec = dc.build_spec(call.name, call.depth, call.num_steps)
  model = msd_amd.InferenceModel(dc.build_params(call.name, call.depth), spec, batch_size=batch or call.batch,
                                 precision=call.precision, **call.model_kw)
  return model, model._get_native()


def _read(nm, call):
  return {n: nm.debug_read(n) for n in dc.buffer_names(call)}


def _ratio(got, want, yard):
  dev, yd = dc.stats(got, want), dc.stats(yard, want)
  r = tuple((d / y) if y > 0 else (0.0 if d == 0 else np.inf) for d, y in zip(dev, yd))
  return dev, yd, r


def _check(call, bufs, film, song_ids, yard_precision=None):
  """Every stage_items entry of every (pass, song) of the call against float64 -> (failures, worst ratio, rows); prints
  every ratio."""
  prec = yard_precision or call.precision
  failures, worst, rows = [], 0.0, []
  for p in range(call.passes):
    for b, j in enumerate(song_ids):
      ref, yard = _exp(call, j, p, 'float64', 'f32', film), _exp(call, j, p, 'float32', prec, film)
      for label, got, key in dc.stage_items(call, bufs, p, b, ref):
        dev, yd, r = _ratio(got, dc.pick(ref, key), dc.pick(yard, key))
        print('[stage-ratio] %-34s layer %d %-14s pass %d song %d  rms %.3e / %.3e = %6.2f   max %.3e / %.3e = %6.2f' %
              (call.tag, call.depth - 1, label, p, j, dev[0], yd[0], r[0], dev[1], yd[1], r[1]))
        rows.append((label, p, j, dev, yd, r))
        worst = max(worst, *r)
        if not max(r) <= FACTOR[prec]:
          failures.append('%s: layer %d buffer %s pass %d (%s) song %d: ratios %.2f / %.2f (bound %.0f)' %
                          (call.tag, call.depth - 1, label, p, 'cond' if call.pass_cond(p) else 'uncond', j, r[0], r[1], FACTOR[prec]))
  return failures, worst, rows


def _rel(got, want):
  return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


# ---- 1. single passes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,depth,prec', dc.SINGLE_HANDLES, ids=['%s-%d-%s' % h for h in dc.SINGLE_HANDLES])
def test_single_pass_stages_against_float64(torch, name, depth, prec):
  """msd_decoder_pass on a 5-step handle at step indices 0, 2, 4, conditional and unconditional: every buffer the pass
  leaves (decoder_stage_cases: 'What survives') of every song; the returned eps IS the eps buffer's rows."""
  calls = dc.single_calls(name, depth, prec)
  with _timed('device'):
    model, nm = _model(calls[0])
    assert model.precision == prec
    batch, z = songs(name)
    B = calls[0].batch
    sub = dc.sub_batch(batch, range(B))
    nm.encode(B, sub['encoder_input_tokens'], helpers.dev(torch, sub['encoder_continuous_inputs']), sub['encoder_continuous_mask'])
    film = nm.debug_read('film')
    zd = helpers.dev(torch, z[:B])
    reads = []
    for call in calls:
      eps = torch.zeros_like(zd)
      nm.decoder_pass(B, call.step, zd, call.cond, eps)
      torch.cuda.synchronize()
      reads.append((_read(nm, call), eps.cpu().numpy()))
  failures, worst = [], 0.0
  for call, (bufs, eps) in zip(calls, reads):
    assert np.array_equal(helpers.bits(bufs['eps'][:eps.size]), helpers.bits(eps.ravel())), call.tag
    f, w, _ = _check(call, bufs, film, range(B))
    failures += f
    worst = max(worst, w)
  print('[stage-ratio] worst single %s/d%d/%s: %.2f' % (name, depth, prec, worst))
  _wall_line('single %s-%d-%s' % (name, depth, prec))
  del model, nm
  torch.cuda.empty_cache()
  assert not failures, '\n'.join(failures[:30])


# ---- 2. CFG steps ---------------------------------------------------------------------------------------------------
def _cfg_run(torch, call, song_ids):
  """One CFG step of the songs on a 1-step handle of len(song_ids) rows -> (buffers, film)."""
  with _timed('device'):
    model, nm = _model(call, batch=len(song_ids))
    assert model.precision == call.precision
    batch, z = songs(call.name)
    T = dc.SPECS[call.name].T
    model.predict(dc.sub_batch(batch, song_ids), init_z=np.ascontiguousarray(z[list(song_ids)]),
                  noise=np.zeros((1, len(song_ids), T, dc.N_MEL), np.float32))
    out = _read(nm, call), nm.debug_read('film'), nm.debug_read('touch_blocks')
    del model, nm
    torch.cuda.empty_cache()
  return out


def _alone_run(torch, name, depth, j):
  """Song j's CFG step alone (B = 1, the default plan): x and eps of both passes."""
  key = (name, depth, j)
  if key not in _alone:
    bufs, _, _ = _cfg_run(torch, dc.cfg_call(name, depth, 1, 'default'), (j,))
    _alone[key] = {k: bufs[k].astype(np.float64) for k in ('x', 'eps')}
  return _alone[key]


@pytest.mark.parametrize('name,depth,b,variant', dc.CFG_CASES, ids=['%s-%d-%d-%s' % c for c in dc.CFG_CASES])
def test_cfg_step_stages_against_float64(torch, name, depth, b, variant):
  """One CFG step (plan_cfg_step) of b songs: every buffer of both passes of every song against float64; every song's x
  and eps against the same song's one-song step (a batched launch must not mix songs); a song without a valid key:
  from the cross block on its conditional pass IS its unconditional pass, bit for bit (g, x, ssq, y, eps)."""
  call = dc.cfg_call(name, depth, b, variant)
  sc = dc.SPECS[name]
  bufs, film, touch = _cfg_run(torch, call, range(b))
  if variant == 'prefetch':
    assert touch.min() > 0, touch   # the attention launches of this case carry touch blocks
  failures, worst, _ = _check(call, bufs, film, range(b))
  print('[stage-ratio] worst cfg %s: %.2f' % (call.tag, worst))
  BT = b * sc.T
  for j in range(b):
    alone = _alone_run(torch, name, depth, j)
    for p in range(2):
      for k, width in (('x', sc.emb), ('eps', dc.N_MEL)):
        got = dc.read_rows(bufs[k], width, dc.song_rows(p, j, b, sc.T))
        want = dc.read_rows(alone[k], width, dc.song_rows(p, 0, 1, sc.T))
        d = _rel(got, want)
        print('[stage-ratio] %-34s %-3s pass %d song %d against the song alone: max rel %.1e' % (call.tag, k, p, j, d))
        if not d < BATCH_BAR:
          failures.append('%s: %s pass %d song %d differs from the song alone by %.1e' % (call.tag, k, p, j, d))
    if not _exp(call, j, 0, 'float64', 'f32', film)['has_cross']:
      # no valid key: the cross update is EXACTLY zero (x2 == x1), so everything behind it in the conditional pass is the
      # unconditional pass bit for bit -- the same x1 (one self block, or the same rows' arithmetic), x1 + 0, and then the
      # same MLP launches on both row ranges
      for k, width in (('g', sc.mlp), ('x', sc.emb), ('ssq', sc.emb // 32), ('y', sc.emb), ('eps', dc.N_MEL)):
        c, u = (dc.read_rows(bufs[k], width, dc.song_rows(p, j, b, sc.T)) for p in range(2))
        same = np.array_equal(helpers.bits(c), helpers.bits(u))
        print('[stage-ratio] %-34s %-3s song %d (no key): conditional against unconditional %s' %
              (call.tag, k, j, 'bit-identical' if same else 'DIFFERS, max abs %.3e' % np.abs(c.astype(np.float64) - u).max()))
        if not same:
          failures.append('%s: song %d has no key, yet its conditional %s is not its unconditional %s bit for bit' % (call.tag, j, k, k))
  assert b < 3 or not _exp(call, 2, 0, 'float64', 'f32', film)['has_cross']   # the all-padding song is in the batch
  _wall_line('cfg %s' % call.tag)
  assert not failures, '\n'.join(failures[:30])


# ---- 3. the whole pass ----------------------------------------------------------------------------------------------
def test_eps_of_a_full_depth_pass_is_float32_class(torch):
  """eps of one conditional and one unconditional pass of spec N at depth 2 and of the full tiny_context preset (two
  encoder layers) under the stage bound with the shared table: about 1e-6 where the suite's single-pass bars (2e-4 / 3e-4,
  unchanged) are set by the FiLM table's float32 time signal."""
  from oracle import backend, fast
  failures = []
  for which in ('N', 'tiny_context'):
    with _timed('device'):
      if which == 'N':
        spec, params = dc.build_spec('N', 2), dc.build_params('N', 2)
        batch, z = dc.sub_batch(songs('N')[0], (0, 1)), songs('N')[1][:2]
      else:
        spec = msd_amd.config.preset('tiny_context', num_steps=5)
        params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
        batch, z = helpers.make_batch(spec, batch=2, ctx_mask='ragged'), helpers.make_noise(spec, batch=2)[0]
      model = msd_amd.InferenceModel(params, spec, batch_size=2)
      nm = model._get_native()
      assert model.precision == 'f16x3'
      nm.encode(2, batch['encoder_input_tokens'], helpers.dev(torch, batch['encoder_continuous_inputs']), batch['encoder_continuous_mask'])
      film = nm.debug_read('film')
      zd, got = helpers.dev(torch, z), {}
      for cond in (True, False):
        eps = torch.zeros_like(zd)
        nm.decoder_pass(2, 2, zd, cond, eps)
        torch.cuda.synchronize()
        got[cond] = eps.cpu().numpy()
    with _timed('oracle'):
      cfg, dcfg = helpers.oracle_configs(spec)
      out = {}
      for dtype, prec in (('float64', 'f32'), ('float32', 'f16x3')):
        fm = fast.FastModel(backend.NumpyBackend(dtype), cfg, dcfg, params, True, precision=prec, in_proj_planes=True)
        fm.set_film(film)
        fm.encode(batch['encoder_input_tokens'], batch['encoder_continuous_inputs'], batch['encoder_continuous_mask'])
        out[dtype] = {cond: np.asarray(fm.decoder_pass(fm.xp.asarray(z), 2, cond), np.float64) for cond in (True, False)}
    for cond in (True, False):
      for j in range(2):
        dev, yd, r = _ratio(got[cond][j], out['float64'][cond][j], out['float32'][cond][j])
        print('[stage-ratio] full depth %-12s eps %-6s song %d  rms %.3e / %.3e = %6.2f   max %.3e / %.3e = %6.2f' %
              (which, 'cond' if cond else 'uncond', j, dev[0], yd[0], r[0], dev[1], yd[1], r[1]))
        assert dev[0] < 1e-5   # (float32 class in absolute terms too: 20 x below the 2e-4 bar)
        if not max(r) <= FACTOR['f16x3']:
          failures.append('%s eps %s song %d: ratios %.2f / %.2f' % (which, 'cond' if cond else 'uncond', j, r[0], r[1]))
    del model, nm
  _wall_line('full depth')
  assert not failures, '\n'.join(failures)


# ---- 4. the comparison resolves the class ---------------------------------------------------------------------------
GEMM_OUTPUTS = ('qk.q', 'qk.k', 'vt', 'ao(cross 0)', 'cq', 'g', 'x', 'ssq(sum)', 'y', 'eps')


def test_one_plane_handle_is_told_apart(torch):
  """A precision = 'f16' handle (one half plane everywhere) against the f16x3 yardstick: every buffer a GEMM or its epilogue writes (and the cross-attention output) is
  beyond FACTOR x the yardstick by at least a factor 10 -- the device counterpart of the host test's separation."""
  call = dc.Call('N', 2, 2, 'single', 2, True, 'default', 'f16')
  with _timed('device'):
    model, nm = _model(call)
    assert model.precision == 'f16'
    batch, z = songs('N')
    sub = dc.sub_batch(batch, range(2))
    nm.encode(2, sub['encoder_input_tokens'], helpers.dev(torch, sub['encoder_continuous_inputs']), sub['encoder_continuous_mask'])
    film = nm.debug_read('film')
    zd = helpers.dev(torch, z[:2])
    eps = torch.zeros_like(zd)
    nm.decoder_pass(2, 2, zd, True, eps)
    torch.cuda.synchronize()
    bufs = _read(nm, call)
  # (the f16x3 emulation saw no f16-encoded keys: the cached K / V are one class apart too, as on a real one-plane handle)
  _, _, rows = _check(call, bufs, film, range(2), yard_precision='f16x3')
  seen = set()
  for label, p, j, dev, yd, r in rows:
    if label in GEMM_OUTPUTS:
      seen.add(label)
      assert r[0] >= 10 * FACTOR['f16x3'], (label, j, r)
  assert seen == set(GEMM_OUTPUTS)
  _wall_line('one plane')


# ---- 5. the debug read's names --------------------------------------------------------------------------------------
def test_debug_read_names(torch):
  """ao2 / cq2 exist on a handle with a second cross-attention module (spec M), with that module's [Bmax T, J]; on spec N
  they are refused as unknown buffers and the handle stays usable."""
  sc = dc.SPECS['M']
  model, nm = _model(dc.cfg_call('M', 1, 2, 'default'))
  for name in ('ao2', 'cq2'):
    assert nm.debug_read(name).shape == (2 * sc.T * sc.J,), name
  assert nm.debug_read('cq').shape == (2 * 2 * sc.T * sc.J,) and nm.debug_read('ao').shape == (2 * 2 * sc.T * sc.J,)
  del model, nm
  call = dc.Call('N', 1, 2, 'single', 2, True)
  model, nm = _model(call)
  for name in ('ao2', 'cq2'):
    with pytest.raises(Exception, match="unknown debug buffer '%s'" % name):
      nm.debug_read(name)
  batch, z = songs('N')
  sub = dc.sub_batch(batch, range(2))
  nm.encode(2, sub['encoder_input_tokens'], helpers.dev(torch, sub['encoder_continuous_inputs']), sub['encoder_continuous_mask'])
  zd = helpers.dev(torch, z[:2])
  eps = torch.zeros_like(zd)
  nm.decoder_pass(2, 2, zd, True, eps)
  torch.cuda.synchronize()
  got = nm.debug_read('eps')[:eps.numel()]
  assert np.isfinite(got).all() and np.array_equal(helpers.bits(got), helpers.bits(eps.cpu().numpy().ravel()))
