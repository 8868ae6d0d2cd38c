"""-m gpu: every GEMM tile and epilogue the decoder launches, one instance at a time, against float64.

msd_op_gemm_site runs ONE launch site (GemmSites / DualSites of csrc/msd_api.hip) on the caller's operands through the
product's own dispatch; msd_op_gemm_site_tiles lists a site's tiles from the tile table itself, so a tile added later is
tested here (or fails for lack of a shape) without anyone remembering to.  The references are the float64 restatements
of tests/gemm_site_refs.py (checked on the CPU by tests/test_gemm_site_refs.py).

Bars, relative to max |reference| (the existing op tests' bars for the same epilogue; bf16x3 = twice f16x3):
  stored / accumulated GEMM outputs 1e-5, folded-norm consumer outputs 4e-5, x (and y = x (.) g) of the producers 2e-5,
  GEGLU 3e-5, QKV 2e-5.  The rows' sums of squares get twice the producers' bar: d(x^2) = 2 x dx.
One-plane modes: linear outputs 3e-3 (f16) / 2e-2 (bf16), from test_gemm_h16.  Everything else is held against a NumPy
emulation -- operands rounded to one plane as csrc/common.h does (weights times 2^9 in the half build), results the
product stores as planes rounded likewise (they are the next launch's one-plane operands), product and epilogue in
float64: the device adds only float32 accumulation, so it has to stay within 2 x the emulation's own error against
float64 + the two-plane bar of that epilogue.

Every buffer an epilogue only stores to starts as NaN (plane results inside the entry, float32 ones here) and every one
it accumulates into as a known x: a tile no block ran stays NaN, a tile two blocks ran has its update applied twice.
"""
import math

import numpy as np
import pytest

from tests import gemm_site_refs as R

pytestmark = pytest.mark.gpu

PRECISIONS = ['f16x3', 'bf16x3', 'f16', 'bf16']
TWO_PLANE = ['f16x3', 'bf16x3']
BARS = {'gemm': 1e-5, 'folded': 4e-5, 'x': 2e-5, 'geglu': 3e-5, 'qkv': 2e-5, 'ssq': 4e-5}   # f16x3; bf16x3: twice
ONE_PLANE_LINEAR = {'f16': 3e-3, 'bf16': 2e-2}
SINGLE_SITES = ['qkv', 'mlp_in', 'residual_square', 'residual_tall', 'resnorm_tall', 'resnorm_tall_dup', 'resnorm_square',
                'store_h16', 'store_f32', 'in_proj', 'resnorm_tall_y2']
DUAL_SITES = ['dual_qkv', 'dual_out', 'dual_out_dup']
STEPS, STEP = 3, 2   # step-indexed tables have 3 rows with different values and are read at row 2
SEG = 32             # QKV: rows per V^T segment (a 64-row tile holds two segments)
T_POS = 40           # in-projection: rows of the position table (no multiple of a tile)


def _fmt(prec):
  return 'bf16' if prec.startswith('bf16') else 'f16'


def _kind(site):
  for k in ('qkv', 'mlp_in', 'residual', 'resnorm', 'store', 'in_proj'):
    if site.startswith(k):
      return k
  return {'dual_qkv': 'qkv', 'dual_out': 'resnorm', 'dual_out_dup': 'resnorm'}[site]


@pytest.fixture(scope='module')
def env():
  import torch
  import msd_amd
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  yield torch, msd_amd.native
  # for the record: the worst error of this run per (precision, site, tile, output), beside its bar
  for key in sorted(WORST):
    print('GEMMSITE-WORST %s %s %s %s: %.2e (bar %.2e)' % (key + WORST[key]))


# ---- inputs (those of the existing op tests) -------------------------------------------------------------------------
def _residual_like(rng, m, n):
  x = (3.0 * rng.standard_normal((m, n))).astype(np.float32)
  x[:, ::7] *= 20.0   # a few dominant channels, like a trained residual stream
  return x


def _gains(rng, n):   # gamma (.) (1 + FiLM scale), one row per step
  gamma = 1.0 + 0.3 * rng.standard_normal(n)
  return (gamma[None, :] * (1.0 + 0.5 * rng.standard_normal((STEPS, n)))).astype(np.float32)


def make(site, m, n, k, seed=0, rowscale=False, bias=True, split=None, null_hi=False, null_lo=False, y2_rows=None, passes=1, with_y2=False):
  """The operands of one problem of `site` as float32 arrays (+ integer fields), by msd_gemm_site_args field name."""
  rng = np.random.default_rng([seed, m, n, k])
  kind = _kind(site)
  p = dict(m=m, n=n, k=k, step=STEP, steps=STEPS)
  p['a'] = rng.standard_normal((m, k)).astype(np.float32)
  p['w'] = (rng.standard_normal((k, n if kind != 'mlp_in' else n // 2)) / np.sqrt(k)).astype(np.float32)
  if kind == 'mlp_in':
    p['w'] *= np.float32(4.0)   # wide pre-activations: both GELU tails
    p['w_gate'] = (rng.standard_normal((k, n // 2)) / np.sqrt(k)).astype(np.float32)
  if rowscale:   # a consumer of the folded norm: a = x (.) g, the partial sums of x, the tabulated bias . W
    xr = _residual_like(rng, m, k)
    p['a'] = (xr * _gains(rng, k)[STEP]).astype(np.float32)
    p['ssq'] = R.partial_ssq(xr).astype(np.float32)
    if bias:
      film = 0.5 * rng.standard_normal((STEPS, k))
      wfull = p['w'] if kind != 'mlp_in' else np.concatenate([p['w'], p['w_gate']], axis=1)
      p['bias'] = (film @ wfull.astype(np.float64)).astype(np.float32)
  if kind == 'qkv':
    p['seg_len'] = SEG
  if kind == 'residual':
    p['x'] = _residual_like(rng, m, n)
  if kind == 'resnorm':
    dup = site.endswith('_dup')
    p['x'] = _residual_like(rng, 2 * m if dup else m, n)
    p['g_lo'], p['g_hi'] = _gains(rng, n), _gains(rng, n)
    p['split_row'] = m // 2 if split is None else split
    if null_hi:
      del p['g_hi']
    if null_lo:   # the folded attention-out launch: the conditional rows' y has no reader
      del p['g_lo']
    if dup:
      p['dup_rows'] = m
      p['x'][m:] = np.float32(5.0)   # overwritten by the second copy
    if site.endswith('_y2'):
      p['g2'] = (1.0 + 0.3 * rng.standard_normal(n)).astype(np.float32)
      p['y2_rows'] = m if y2_rows is None else y2_rows
  if kind == 'in_proj':
    p['pos'] = rng.standard_normal((T_POS, n)).astype(np.float32)
    p['g_lo'] = _gains(rng, n)
    p['seg_len'], p['passes'] = T_POS, passes
    if with_y2:
      p['g2'] = (1.0 + 0.3 * rng.standard_normal(n)).astype(np.float32)
  return p


def evaluate(site, p, fmt=None):
  """{output: (float64 array, bar class)} of problem p.  fmt: None = float64 on the float32 inputs (the reference);
  'f16' / 'bf16' = the one-plane emulation of the module docstring."""
  ra = (lambda v: v) if fmt is None else (lambda v: R.round_plane(v, fmt))
  rw = (lambda v: v) if fmt is None else (lambda v: R.round_weight(v, fmt))
  ro = (lambda v: v) if fmt is None else (lambda v: None if v is None else R.round_plane(v.astype(np.float32), fmt).astype(np.float64))
  kind, step = _kind(site), p['step']
  a, w = ra(p['a']), rw(p['w'])
  scaled = 'ssq' in p
  if kind == 'qkv':
    return {'out': (ro(R.linear(a, w, p.get('ssq'), p.get('bias'), step)), 'folded' if scaled else 'qkv')}
  if kind == 'store':
    out = R.linear(a, w, p.get('ssq'), p.get('bias'), step)
    return {'out': (out if site == 'store_f32' else ro(out), 'folded' if scaled else 'gemm')}
  if kind == 'mlp_in':
    return {'out': (ro(R.mlp_in(a, w, rw(p['w_gate']), p.get('ssq'), p.get('bias'), step)), 'geglu')}
  if kind == 'residual':
    return {'x': (R.residual(p['x'], a, w), 'gemm')}
  if kind == 'resnorm':
    x, ssq, y, y2 = R.residual_norm(p['x'], a, w, p.get('g_lo'), p.get('g_hi'), p['split_row'], step, p.get('dup_rows'),
                                    p.get('g2'), p.get('y2_rows', 0))
    out = {'x': (x, 'x'), 'ssq_out': (ssq, 'ssq'), 'y': (ro(y), 'x')}
    if y2 is not None:
      out['y2'] = (ro(y2), 'x')
    return out
  x, ssq, y, y2 = R.in_proj(a, w, p['pos'], p['g_lo'], step, p['passes'], p.get('g2'))
  out = {'x': (x, 'x'), 'ssq_out': (ssq, 'ssq'), 'y': (ro(y), 'x')}
  if y2 is not None:
    out['y2'] = (ro(y2), 'x')
  return out


def evaluate_second(site, p, fmt=None):
  """The second problem of a dual site: {'out2': ...}."""
  a, w = p['a2'], p['w2']
  if fmt is not None:
    a, w = R.round_plane(a, fmt), R.round_weight(w, fmt)
  if site == 'dual_qkv':
    return {'out2': (R.linear(a, w), 'gemm')}
  return {'out2': (R.add_store(a, w, p['addend2']), 'gemm')}


# ---- running one problem ---------------------------------------------------------------------------------------------
_INT_FIELDS = ('m', 'n', 'k', 'step', 'steps', 'seg_len', 'split_row', 'dup_rows', 'y2_rows', 'passes', 'm2', 'n2', 'k2')
_IN_PTRS = ('a', 'w', 'w_gate', 'ssq', 'bias', 'g_lo', 'g_hi', 'g2', 'pos', 'a2', 'w2', 'addend2')


def launch(env, prec, site, p, **opts):
  """Runs problem p; returns ({output: float32 array}, the entry's ran_* report).  ssq_out comes back as the rows' sums."""
  torch, native = env
  kind = _kind(site)
  m, n = p['m'], p['n']
  dev = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float32)).cuda()
  nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
  fields = {f: p[f] for f in _INT_FIELDS if f in p}
  fields.update({f: dev(p[f]) for f in _IN_PTRS if f in p})
  outs = {}
  if kind in ('qkv', 'store'):
    outs['out'] = nan(m, n)
  elif kind == 'mlp_in':
    outs['out'] = nan(m, n // 2)
  elif kind == 'residual':
    outs['x'] = dev(p['x'])
  elif kind == 'resnorm':
    rows = p['x'].shape[0]
    outs.update(x=dev(p['x']), y=nan(rows, n), ssq_out=nan(rows, n // 32))
    if 'g2' in p:
      outs['y2'] = nan(m, n)
  else:
    rows = p['passes'] * m
    outs.update(x=nan(rows, n), y=nan(rows, n), ssq_out=nan(rows, n // 32))
    if 'g2' in p:
      outs['y2'] = nan(m, n)
  if 'a2' in p:
    outs['out2'] = nan(p['m2'], p['n2'])
  fields.update(outs)
  fields.update(opts)
  ran = native.op_gemm_site(prec, site, **fields)
  torch.cuda.synchronize()
  got = {k: v.cpu().numpy() for k, v in outs.items()}
  if 'ssq_out' in got:
    got['ssq_out'] = got['ssq_out'].astype(np.float64).sum(axis=1)
  return got, ran


def _err(got, ref):
  """max |got - ref| / max |ref| over the elements the reference has; NaN patterns must agree exactly."""
  got = np.asarray(got, np.float64)
  assert got.shape == ref.shape, (got.shape, ref.shape)
  gn, rn = np.isnan(got), np.isnan(ref)
  assert np.array_equal(gn, rn), 'written / unwritten elements differ: %d NaN where the reference has %d' % (gn.sum(), rn.sum())
  if rn.all():
    return 0.0
  return float(np.abs(got[~rn] - ref[~rn]).max() / np.abs(ref[~rn]).max())


WORST = {}   # (precision, site, tile, output) -> (worst error, its bar): printed when the module's fixture is torn down


def check(prec, site, p, got, tag, refs=None, second=False):
  """Every output of `got` against float64 under the bars of the module docstring; prints and records the figures."""
  ev = evaluate_second if second else evaluate
  refs = refs or ev(site, p)
  fmt, two = _fmt(prec), prec in TWO_PLANE
  emul = None
  for name, (ref, cls) in refs.items():
    err = _err(got[name], ref)
    bar2 = BARS[cls] * (2.0 if fmt == 'bf16' else 1.0)
    if two:
      bar, note = bar2, ''
    elif cls in ('gemm', 'qkv') or name == 'x':
      bar, note = ONE_PLANE_LINEAR[fmt], ''
    else:
      emul = emul or ev(site, p, fmt)
      e_emul = _err(np.where(np.isnan(ref), np.nan, emul[name][0]), ref)
      bar, note = 2.0 * e_emul + bar2, ' (emulation %.2e)' % e_emul
    print('GEMMSITE %s %s %s %s: %.2e bar %.2e%s' % (prec, site, tag, name, err, bar, note))
    key = (prec, site, tag.split()[0], name)
    if key not in WORST or err / bar > WORST[key][0] / WORST[key][1]:
      WORST[key] = (err, bar)
    assert err <= bar, (prec, site, tag, name, err, bar)


def _n_values(site, bn):
  kind = _kind(site)
  if kind == 'qkv':
    return [3 * bn, 6 * bn]          # 2 J % BN == 0 and 3 J % BN == 0 <=> J % BN == 0
  if bn == 48:
    return [96, 480]                 # partial sums per 32 columns: N % 32 == 0 as well
  return [bn, 5 * bn]


def _forms(site, bm):
  """(plainest form, the other forms) of a site's epilogue at M = 2 BM."""
  kind, m = _kind(site), 2 * bm
  if kind in ('qkv', 'store', 'mlp_in'):
    return {}, [dict(rowscale=True), dict(rowscale=True, bias=False)]
  if kind == 'residual':
    return {}, []
  if kind == 'in_proj':
    return {}, [dict(passes=2), dict(passes=2, with_y2=True), dict(with_y2=True)]
  if site.endswith('_dup'):
    return {}, []
  if site.endswith('_y2'):
    return dict(y2_rows=m), [dict(y2_rows=bm), dict(y2_rows=bm, split=0), dict(y2_rows=m, split=m, null_hi=True)]
  return dict(split=bm), [dict(split=0), dict(split=m), dict(split=bm, null_hi=True)]


# ---- (a) every instance, forced --------------------------------------------------------------------------------------
def test_site_list_is_the_librarys(env):
  """The sites this file names are all the library has: a new launch site fails here until it is added above."""
  _, native = env
  assert list(native.GEMM_SITES) == SINGLE_SITES + DUAL_SITES
  for prec in PRECISIONS:   # the binding's positions are the library's own names for them, in order
    names = native.gemm_site_names(prec)
    assert names == [s for s in SINGLE_SITES + DUAL_SITES if native.gemm_site_tiles(prec, s)], (prec, names)
    assert [native.GEMM_SITES[n] for n in names] == list(range(len(names)))
  for prec in PRECISIONS:
    assert native.gemm_site_tiles(prec, len(native.GEMM_SITES)) == []
    for site in SINGLE_SITES[:10]:
      assert native.gemm_site_tiles(prec, site), (prec, site)
    for site in SINGLE_SITES[10:] + DUAL_SITES:
      assert bool(native.gemm_site_tiles(prec, site)) == (prec in TWO_PLANE), (prec, site)


def _dual_case(env, prec, site, pair, m, n, k, m2, n2, k2, form, alone=False):
  """One dual launch on the tile pair: both problems against float64 (and, `alone`, problem 1 bit for bit against its
  single site on the same tile)."""
  bm, bn, ns, bm2, bn2, ns2 = pair
  p1 = make(site, m, n, k, seed=4, **form)
  p = _with_second(p1, m2, n2, k2, site != 'dual_qkv', seed=5)
  got, ran = launch(env, prec, site, p, force_bm=bm, force_bn=bn, force_bm2=bm2, force_bn2=bn2)
  assert ran['ran_dual'] == 1
  assert (ran['ran_bm'], ran['ran_bn'], ran['ran_ns'], ran['ran_bm2'], ran['ran_bn2'], ran['ran_ns2']) == pair
  tag = '%dx%d+%dx%d M%d N%d K%d / M%d N%d K%d %s' % (bm, bn, bm2, bn2, m, n, k, m2, n2, k2, form)
  check(prec, site, p, got, tag)
  check(prec, site, p, got, tag, second=True)
  if alone:
    single = {'dual_qkv': 'qkv', 'dual_out': 'resnorm_tall', 'dual_out_dup': 'resnorm_tall_dup'}[site]
    one, _ = launch(env, prec, single, p1, force_bm=bm, force_bn=bn)
    for name in one:
      np.testing.assert_array_equal(got[name], one[name], err_msg='%s %s %s %s' % (prec, site, tag, name))
  return p, got


def _every_pair_forced(env, prec, site):
  """Part (a) for a dual site: every tile pair; problem 1 on 2 x 3 tiles, problem 2 on 3 x 5 (never the same M, N or K);
  K / 64 = 1 .. 6 and 13 on each problem in turn while the other runs 7 K-tiles -- the 32 x 96 tile and EpiAddStoreH16 exist
  in dual launches only --; the other epilogue forms of problem 1 at K / 64 = 3 and 4."""
  _, native = env
  pairs = native.gemm_site_tiles(prec, site)
  assert bool(pairs) == (prec in TWO_PLANE)
  for pair in pairs:
    bm, bn, _, bm2, bn2, _ = pair
    if site == 'dual_qkv':
      plain, others = dict(rowscale=True), [dict(), dict(rowscale=True, bias=False)]
    elif site == 'dual_out':
      plain, others = dict(split=bm), [dict(split=bm, null_lo=True), dict(split=0), dict(split=2 * bm, null_hi=True)]
    else:
      plain, others = {}, []
    shape = (2 * bm, 3 * bn), (3 * bm2, 5 * bn2)
    cases = [(64 * nk, 448, plain) for nk in (1, 2, 3, 4, 5, 6, 13)] + [(448, 64 * nk, plain) for nk in (1, 2, 3, 4, 5, 6, 13)]
    cases += [(64 * nk, 448, f) for f in others for nk in (3, 4)]
    for k, k2, form in cases:
      _dual_case(env, prec, site, pair, shape[0][0], shape[0][1], k, shape[1][0], shape[1][1], k2, form)


@pytest.mark.parametrize('site', SINGLE_SITES + DUAL_SITES)
@pytest.mark.parametrize('prec', PRECISIONS)
def test_every_tile_forced(env, prec, site):
  """Each tile of the site's table, forced: one, an even and an odd number of row tiles (xcd_rows 1, 2, 1) times fewer
  column tiles than XCD column groups and a count that divides neither 4 nor 8; K / 64 = 1 .. 6 and 13 (nk < NS, == NS,
  NS + 1, NS + 2 and a long odd count for ring depths 2, 3 and 4) on the plainest epilogue form; the other forms at
  K / 64 = 3 and 4.  The entry must report the forced tile."""
  _, native = env
  if site in DUAL_SITES:   # (two problems per launch: _every_pair_forced)
    return _every_pair_forced(env, prec, site)
  tiles = native.gemm_site_tiles(prec, site)
  if not tiles:
    assert site == 'resnorm_tall_y2' and prec not in TWO_PLANE
    return
  for bm, bn, ns in tiles:
    tag = '%dx%d' % (bm, bn)
    plain, others = _forms(site, bm)
    ns_n = _n_values(site, bn)
    cases = [(mm * bm, nn, 192, plain) for mm in (1, 2, 3) for nn in ns_n]
    cases += [(2 * bm, ns_n[1], 64 * nk, plain) for nk in (1, 2, 4, 5, 6, 13)]
    cases += [(2 * bm, ns_n[1], 64 * nk, f) for f in others for nk in (3, 4)]
    for m, n, k, form in cases:
      form = dict(form)
      if _kind(site) == 'resnorm' and not site.endswith('_dup') and form.get('split', bm) > m:
        form['split'] = m
      if 'y2_rows' in form:
        form['y2_rows'] = min(form['y2_rows'], m)
      p = make(site, m, n, k, **form)
      got, ran = launch(env, prec, site, p, force_bm=bm, force_bn=bn)
      assert (ran['ran_bm'], ran['ran_bn'], ran['ran_ns']) == (bm, bn, ns), ran
      assert ran['ran_xcd_rows'] == (2 if (m // bm) % 2 == 0 else 1) and not ran['ran_dual']
      if _kind(site) == 'in_proj':
        assert ran['step_copy'] == STEP
      check(prec, site, p, got, '%s M%d N%d K%d %s' % (tag, m, n, k, form))


def test_forced_shape_outside_the_table_is_an_error(env):
  _, native = env
  p = make('store_f32', 64, 64, 64)
  with pytest.raises(ValueError):
    launch(env, 'f16x3', 'store_f32', p, force_bm=64, force_bn=64)    # a tile of other sites
  with pytest.raises(ValueError):
    launch(env, 'f16x3', 'qkv', make('qkv', 128, 288, 64), force_bm=128, force_bn=128)
  with pytest.raises(ValueError):
    launch(env, 'f16x3', 'qkv', make('qkv', 64, 288, 64), force_bm=128, force_bn=96)   # M no multiple of the tile
  with pytest.raises(NotImplementedError):   # a precision of the other build
    launch(env, 'bf16x3', 'store_f32', p, planes='f16')
  with pytest.raises(NotImplementedError):
    launch(env, 'f16', 'store_f32', p, planes='bf16')


@pytest.mark.parametrize('site', ['qkv', 'mlp_in', 'store_h16'])
@pytest.mark.parametrize('prec', TWO_PLANE)
def test_converting_epilogues_between_tiles(env, prec, site):
  """The epilogues that scale, add a bias or convert: the same problem on every tile of the site's table (256 rows; N
  divides by every tile), plain and with the row scale + bias.  Each result against float64; the largest difference
  between tiles is printed, not asserted (with a row scale the rows' statistics are summed in another order per BM).
  (EpiStoreF32 has one tile, 32 x 32: its bit-identity across tiles holds trivially and is not run.)"""
  _, native = env
  tiles = native.gemm_site_tiles(prec, site)
  n = {'qkv': 576, 'mlp_in': 256, 'store_h16': 480}[site]
  for form in ({}, dict(rowscale=True)):
    for k in (192, 256):
      p = make(site, 256, n, k, seed=1, **form)
      res = []
      for bm, bn, _ in tiles:
        got, _ = launch(env, prec, site, p, force_bm=bm, force_bn=bn, persistent=2)
        check(prec, site, p, got, '%dx%d between-tiles K%d %s' % (bm, bn, k, form))
        res.append(got['out'].astype(np.float64))
      for (bm, bn, _), r in zip(tiles[1:], res[1:]):
        print('GEMMSITE-TILES %s %s out %s: %dx%d against %dx%d, K %d: %.2e' %
              (prec, site, form, bm, bn, tiles[0][0], tiles[0][1], k, np.abs(r - res[0]).max() / np.abs(res[0]).max()))


@pytest.mark.parametrize('site', ['residual_square', 'residual_tall', 'resnorm_tall', 'resnorm_tall_dup', 'resnorm_square',
                                  'resnorm_tall_y2'])
@pytest.mark.parametrize('prec', PRECISIONS)
def test_add_and_store_outputs_have_the_same_bits_on_every_tile(env, prec, site):
  """gemm_tile promises one K order for every tile shape: x of the residual epilogues is bit-identical whichever tile of
  the site's table computes it (256 x 480 divides by every tile; K / 64 = 3 and 4).  y and the sums of squares differ by
  the grouping of the partial sums only: their largest difference between tiles is printed, not asserted."""
  _, native = env
  tiles = native.gemm_site_tiles(prec, site)
  for k in (192, 256):
    p = make(site, 256, 480, k, seed=1)
    res = [launch(env, prec, site, p, force_bm=bm, force_bn=bn)[0] for bm, bn, _ in tiles]
    for (bm, bn, _), r in zip(tiles[1:], res[1:]):
      np.testing.assert_array_equal(r['x'], res[0]['x'], err_msg='%s %s %dx%d K %d' % (prec, site, bm, bn, k))
      for name in r:
        if name != 'x':
          d = np.nanmax(np.abs(r[name].astype(np.float64) - res[0][name])) / np.nanmax(np.abs(res[0][name]))
          print('GEMMSITE-TILES %s %s %s: %dx%d against %dx%d, K %d: %.2e' % (prec, site, name, bm, bn, tiles[0][0], tiles[0][1], k, d))


# ---- (b) the dispatcher's own choice ---------------------------------------------------------------------------------
# (M, N, K) on both sides of each pick_tile rule, N and K as small as the rule allows.  What the rules ARE is not
# restated here: the results are held against float64 and the union of the tiles the entry reports against the table.
_PICK_SHAPES = {
    # J % 96 alignment present (576) or absent (192: N % 96 == 0 but 2 J % 96 != 0); the 64 x 96 / 64 x 64 tile cost; the
    # big-M threshold at 1984 / 2048 and 2112 (beyond it, no multiple of 128)
    'qkv': [(64, 576, 64), (1984, 576, 64), (2048, 576, 64), (2112, 576, 64), (2048, 192, 64), (64, 192, 64), (8256, 576, 64)],
    # N a multiple of 128 or not; the tile-cost tie of 64 x 128 against 64 x 64 at (2112, 1024): 2 x 192 == 3 x 128
    'mlp_in': [(64, 128, 64), (1088, 1024, 64), (2112, 1024, 64), (1984, 128, 64), (2048, 128, 64), (2048, 192, 64), (2112, 128, 64)],
    # N = D projections: 64 x 96 over 128 x 96 (2048 x 96: CUs without a tile) and 128 x 96 (2048 x 864); N % 96 != 0 (160);
    # tall against narrow by tile cost (1984 x 160 / 1984 x 96); the wide48 rule at K = 1472 / 1536
    'square': [(2048, 96, 64), (2048, 864, 64), (1984, 96, 64), (1984, 160, 64), (2112, 96, 64), (2112, 160, 64),
               (2048, 160, 64), (1024, 288, 1472), (1024, 288, 1536), (1984, 288, 64), (1024, 1248, 1536)],
    'narrow': [(64, 64, 64), (2048, 96, 64), (2112, 160, 64)],
}


# Shapes at which two tiles COST THE SAME (tile_cost: rounds of blocks over 256 CUs x (BM + BN)), and the tile the
# comparison's direction gives there -- `<=` takes the candidate, `<` keeps what it had.  A tie that flips shows here.
#   QKV (8256, 576): 774 blocks of 64 x 96 = 4 rounds x 160, 1161 of 64 x 64 = 5 x 128 (M is no multiple of 128: not big)
#   MLP-in (2112, 1024): 264 blocks of 64 x 128 = 2 x 192, 528 of 64 x 64 = 3 x 128
#   tall kinds (1984, 288): 279 blocks of 64 x 32 = 2 x 96, 558 of 32 x 32 = 3 x 64
#   wide48 (1024, 1248) at K = 1536: 832 blocks of 32 x 48 = 4 x 80, 1248 of 32 x 32 = 5 x 64: `<` keeps 32 x 32 on the
#     square kind (on the tall kind 64 x 32 is cheaper than both: 3 x 96)
# (64 x 96 against 128 x 96 for the N = D projections cannot tie: x and x / 2 blocks never make rounds in the ratio 7 : 5.)
_TIES = {
    ('qkv', (8256, 576, 64)): {2: (64, 96)},
    ('mlp_in', (2112, 1024, 64)): {2: (64, 128)},
    ('tall', (1984, 288, 64)): {1: (64, 32), 2: (64, 32)},
    ('resnorm_square', (1024, 1248, 1536)): {2: (32, 32)},
}


@pytest.mark.parametrize('site', SINGLE_SITES)
@pytest.mark.parametrize('prec', PRECISIONS)
def test_dispatchers_choice(env, prec, site):
  """No forced tile: pick_tile decides.  Every result against float64; the tiles chosen over these shapes are exactly the
  site's table (a tile pick_tile can no longer reach is found here; 32 x 96 exists only as a dual second problem)."""
  _, native = env
  tiles = native.gemm_site_tiles(prec, site)
  if not tiles:
    return
  kind = _kind(site)
  shapes = _PICK_SHAPES[kind if kind in ('qkv', 'mlp_in') else ('narrow' if site in ('store_f32', 'in_proj') else 'square')]
  chosen = set()
  for m, n, k in shapes:
    p = make(site, m, n, k, seed=2)
    got, ran = launch(env, prec, site, p)
    tile = (ran['ran_bm'], ran['ran_bn'], ran['ran_ns'])
    assert tile in tiles, (tile, tiles)
    chosen.add(tile)
    tie = _TIES.get(('tall' if '_tall' in site else (site if site == 'resnorm_square' else kind), (m, n, k)))
    if tie and (2 if prec in TWO_PLANE else 1) in tie:
      assert tile[:2] == tie[2 if prec in TWO_PLANE else 1], (site, (m, n, k), tile)
    check(prec, site, p, got, '%dx%d picked M%d N%d K%d' % (tile[0], tile[1], m, n, k))
  assert chosen == set(tiles), 'pick_tile reached %s of the table %s' % (sorted(chosen), tiles)


# ---- (c) the persistent MLP-in loop ----------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,blocks', [(384, 640, 8), (512, 640, 8), (512, 640, 16), (384, 640, 0)])
@pytest.mark.parametrize('prec', TWO_PLANE)
def test_persistent_mlp_in(env, prec, m, n, blocks):
  """gemm_h16_geglu_persist_kernel on the 128 x 128 tile, block b walking virtual blocks b, b + grid, ... of the plain
  launch's XCD-aware map (XCD = b % 8; column tiles fastest inside an XCD).
  (384, 640, 8 blocks): 3 x 5 tiles, xcd_rows 1: XCD x owns column tile x; blocks 0 - 4 walk the three row tiles of their
    column (statistics re-fetched for every tile), blocks 5 - 7 have no tile and exit at once.
  (512, 640, 8 blocks): 4 x 5 tiles, xcd_rows 2, XCD (xr, xc) with two column slots xc, 4 + xc: 20 tiles on 8 blocks.
    Blocks 0 and 4 (xc = 0) walk (xr, 0), (xr, 4), (2 + xr, 0), (2 + xr, 4): the row tile is kept, changed (statistics
    re-fetched mid-loop), kept.  Blocks 1 - 3 and 5 - 7 walk (xr, xc), a GAP (column 4 + xc does not exist),
    (2 + xr, xc), a gap: a gap in the middle of the walk with a row change across it.
  (512, 640, 16 blocks): blocks 0 - 7 take the first column slot of both row groups (row change every tile), blocks 8
    and 12 the second, the other six blocks have no tile.
  (384, 640, blocks of the product = one per CU): more blocks than the 15 tiles, one tile each.
  Against float64 with the GEGLU bar, and against the per-tile 128 x 128 launch on the same inputs: another contraction
  (fma of the scaled accumulator), so the difference is printed and its median held under 1e-5 of the range."""
  fmt_bar = BARS['geglu'] * (2.0 if _fmt(prec) == 'bf16' else 1.0)
  for k in (128, 192, 320, 64):
    p = make('mlp_in', m, n, k, seed=3, rowscale=True)
    got, ran = launch(env, prec, 'mlp_in', p, force_bm=128, force_bn=128, resident_blocks=blocks)
    assert (ran['ran_bm'], ran['ran_bn']) == (128, 128)
    assert ran['ran_persistent'] == (1 if k >= 128 else 0), (k, ran)   # K = 64: shorter than the ring, the per-tile launch
    check(prec, 'mlp_in', p, got, '128x128 persistent=%d blocks=%d M%d N%d K%d' % (ran['ran_persistent'], blocks, m, n, k))
    per_tile, ran2 = launch(env, prec, 'mlp_in', p, force_bm=128, force_bn=128, persistent=2)
    assert ran2['ran_persistent'] == 0
    ref = evaluate('mlp_in', p)['out'][0]
    assert _err(per_tile['out'], ref) <= fmt_bar
    d = np.abs(got['out'].astype(np.float64) - per_tile['out']) / np.abs(ref).max()
    print('GEMMSITE-PERSIST %s M%d N%d K%d blocks %d: against the per-tile launch max %.2e median %.2e' %
          (prec, m, n, k, blocks, d.max(), np.median(d)))
    assert np.median(d) < 1e-5
    if k < 128:
      np.testing.assert_array_equal(got['out'], per_tile['out'])


# ---- (d) dual launches -----------------------------------------------------------------------------------------------
def _with_second(p, m2, n2, k2, addend, seed):
  rng = np.random.default_rng([seed, m2, n2, k2])
  p = dict(p, m2=m2, n2=n2, k2=k2)
  p['a2'] = rng.standard_normal((m2, k2)).astype(np.float32)
  p['w2'] = (rng.standard_normal((k2, n2)) / np.sqrt(k2)).astype(np.float32)
  if addend:
    p['addend2'] = rng.standard_normal((m2, n2)).astype(np.float32)
  return p


@pytest.mark.parametrize('site', DUAL_SITES)
@pytest.mark.parametrize('prec', TWO_PLANE)
def test_dual_launches(env, prec, site):
  """Every tile pair of the dual site; the two problems differ in M, N and K, so a block that reads the other problem's
  parameters cannot pass; problem 1 has 8 and 24 blocks (one and three row tiles on three column tiles), problem 2 five
  column tiles.  Problem 1 must be bit-identical to the same problem run alone through its single site on the same tile
  -- also in the form the folded attention-out launch runs, without a gain for the rows below split_row; so must problem
  2 of the folded QKV launch (a float32 store: same bits on every tile, here against the 32 x 32 tile of the store site).
  Problem 2 of the attention-out launch (acc + addend to planes) has no single site: float64 only."""
  _, native = env
  pairs = native.gemm_site_tiles(prec, site)
  assert pairs
  for pair in pairs:
    bm, bn, _, bm2, bn2, _ = pair
    forms = {'dual_qkv': [dict(rowscale=True)], 'dual_out': [dict(split=bm), dict(split=bm, null_lo=True)], 'dual_out_dup': [{}]}[site]
    for row_tiles in (1, 3):
      for form in forms:
        p, got = _dual_case(env, prec, site, pair, row_tiles * bm, 3 * bn, 192, (3 if row_tiles == 1 else 5) * bm2, 5 * bn2, 320,
                            form, alone=True)
        if site == 'dual_qkv':
          p2 = dict(m=p['m2'], n=p['n2'], k=p['k2'], step=STEP, steps=STEPS, a=p['a2'], w=p['w2'])
          alone2, _ = launch(env, prec, 'store_f32', p2, force_bm=32, force_bn=32)
          np.testing.assert_array_equal(got['out2'], alone2['out'], err_msg='%s %s %s out2' % (prec, site, pair))


# ---- (e) the prefetch wave -------------------------------------------------------------------------------------------
def _grid(m, n, bm, bn, rx):
  """Blocks of a launch: 8 XCDs x column slots per XCD column group x row slots per XCD row group."""
  cx = 8 // rx
  return 8 * math.ceil(n // bn / cx) * math.ceil(m // bm / rx)


# the epilogues that never carry a weight target (gemm_h16.h epi_may_prefetch: the encoders' plain residual, the float32
# store): their sites have no PF = 1 twin and the entry reports that no prefetch wave ran
NEVER_PREFETCH = ('residual_square', 'residual_tall', 'store_f32')


@pytest.mark.parametrize('site', SINGLE_SITES + DUAL_SITES)
@pytest.mark.parametrize('prec', TWO_PLANE)
def test_prefetch_wave_changes_nothing(env, prec, site):
  """Every site, every tile, with a weight target: the entry's report (taken from the launchers' own predicate) says
  which sites ran the PF = 1 (320-thread) instance -- all but NEVER_PREFETCH, so a new site is run here without being
  listed --: same bits as without the
  target, the target untouched.  The target is a separate weight-shaped buffer, two planes of [rows][256] 16-bit
  elements (four lines a row: 16 rows per touch), a few rows more than one round of the launch's prefetch waves covers."""
  torch, native = env
  for tile in native.gemm_site_tiles(prec, site):
    bm, bn = tile[0], tile[1]
    n = {'qkv': 3 * bn, 'dual_qkv': 3 * bn}.get(site, 96 if bn == 48 else 2 * bn)
    p = make(site, 2 * bm, n, 192, seed=6, rowscale=_kind(site) in ('qkv', 'mlp_in', 'store'))
    force = dict(force_bm=bm, force_bn=bn)
    if site.startswith('dual'):
      p = _with_second(p, 2 * tile[3], 2 * tile[4], 128, site != 'dual_qkv', seed=7)
      force.update(force_bm2=tile[3], force_bn2=tile[4])
    base, ran0 = launch(env, prec, site, p, **force)
    assert ran0['ran_prefetch'] == 0
    blocks = _grid(p['m'], p['n'], bm, bn, ran0['ran_xcd_rows'])
    if site.startswith('dual'):
      blocks += _grid(p['m2'], p['n2'], tile[3], tile[4], ran0['ran_xcd_rows2'])
    rows = 16 * blocks + 5
    target = torch.randint(-30000, 30000, (2, rows, 256), dtype=torch.int16, device='cuda')
    before = target.clone()
    got, ran = launch(env, prec, site, p, prefetch=target, prefetch_rows=rows, prefetch_k=256, **force)
    assert ran['ran_prefetch'] == (0 if site in NEVER_PREFETCH else 1), ran   # (every other site has the twin: run it)
    for name in base:
      np.testing.assert_array_equal(got[name], base[name], err_msg='%s %s %dx%d %s' % (prec, site, bm, bn, name))
    assert torch.equal(target, before)


# ---- (f) the range flag through the product path ---------------------------------------------------------------------
def _range_problem(site, tile, a_val):
  """One output of the launch's LAST tile is a_val * 63.96875 (= 65504 for a_val = 1024) exactly: row m - 1 of a is
  a_val e_0 and element (0, n - 1) of the weight 63.96875 (GEGLU: wi_0 -> 1, wi_1 -> 65504 / 2^20, so that
  gelu(a_val) * a_val * 65504 / 2^20 is the product); residual, positions and addend are zero there and the gains one."""
  bm, bn = tile[0], tile[1]
  kind = _kind(site)
  n = 3 * bn if kind == 'qkv' else (96 if bn == 48 else 2 * bn)
  p = make(site, 2 * bm, n, 128, seed=8)
  if site.startswith('dual'):
    p = _with_second(p, 2 * tile[3], 2 * tile[4], 128, site != 'dual_qkv', seed=9)
  big = 65504.0 / 1024.0
  if site == 'dual_out':     # the converting epilogue under test is problem 2's (problem 1's is tested alone)
    p['a2'][-1, :] = 0.0; p['a2'][-1, 0] = a_val; p['w2'][0, -1] = big; p['addend2'][-1, -1] = 0.0
    return p
  p['a'][-1, :] = 0.0
  p['a'][-1, 0] = a_val
  if kind == 'mlp_in':   # (row 0 of both weights zero elsewhere: the row's other outputs are products of two such terms)
    p['w'][0, :] = 0.0
    p['w_gate'][0, :] = 0.0
    p['w'][0, -1] = 1.0
    p['w_gate'][0, -1] = 65504.0 / 2.0 ** 20
  else:
    p['w'][0, -1] = big
  if 'x' in p:
    p['x'][-1, -1] = 0.0
  if 'pos' in p:
    p['pos'][(2 * bm - 1) % T_POS, -1] = 0.0
  for g in ('g_lo', 'g_hi'):
    if g in p:
      p[g][:, -1] = 1.0
  return p


@pytest.mark.parametrize('site', ['qkv', 'mlp_in', 'store_h16', 'resnorm_tall', 'in_proj', 'dual_out'])
@pytest.mark.parametrize('prec', PRECISIONS)
def test_range_flag_through_the_product_path(env, prec, site):
  """One site per epilogue that converts to planes, first tile of its table: an output of exactly 65504 in the launch's
  last tile passes; one just beyond (1040 * 63.96875 = 66527.5) raises RangeError on the half-plane build and comes
  back right on the bfloat16 build."""
  _, native = env
  tiles = native.gemm_site_tiles(prec, site)
  if not tiles:
    return
  tile = tiles[0]
  force = dict(force_bm=tile[0], force_bn=tile[1])
  if len(tile) > 3:
    force.update(force_bm2=tile[3], force_bn2=tile[4])
  second = site == 'dual_out'
  p = _range_problem(site, tile, 1024.0)
  got, _ = launch(env, prec, site, p, **force)
  name = 'out2' if second else ('y' if 'y' in got else 'out')
  if prec != 'bf16':   # (one bfloat16 plane holds neither 63.96875 nor 65504)
    assert got[name][-1, -1] == 65504.0
  check(prec, site, p, got, '%dx%d range=65504' % tile[:2], second=second)
  p = _range_problem(site, tile, 1040.0)
  if _fmt(prec) == 'f16':
    with pytest.raises(native.RangeError):
      launch(env, prec, site, p, **force)
  else:
    got, _ = launch(env, prec, site, p, **force)
    check(prec, site, p, got, '%dx%d range>65504' % tile[:2], second=second)
