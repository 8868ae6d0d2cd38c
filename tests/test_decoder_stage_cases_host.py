"""No GPU: tests/decoder_stage_cases.py (the cases, the layouts and the reference of tests/test_gpu_decoder_stages.py) and
the oracle's trace (oracle/fast.py FastModel.decoder_pass(trace=...), set_film) checked on the CPU."""
import numpy as np
import pytest

from oracle import fast
from tests import decoder_stage_cases as dc

_cache = {}


def _songs(name):
  if name not in _cache:
    _cache[name] = dc.songs(name)
  return _cache[name]


def _oracle(name, depth, dtype, precision='f32', film=None, cls=None):
  key = (name, depth, dtype, precision, None if film is None else film.tobytes(), cls)
  if key not in _cache:
    fm = dc.make_oracle(name, depth, dtype, precision, film=film, cls=cls)
    dc.encode_songs(fm, _songs(name)[0], (0, 1))
    _cache[key] = fm
  return _cache[key]


def _film32(name, depth):
  """A float32 FiLM table in the device's layout [N, 2 Ld, 2 D]: the float32 oracle's own (what a device table is like)."""
  fm = _oracle(name, depth, 'float32')
  return np.stack([fm.film[l][k] for l in range(depth) for k in range(2)], 1).astype(np.float32)


# ---- 1. tracing changes nothing -------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_trace_returns_the_same_bits(dtype):
  fm = _oracle('N', 2, dtype)
  z = fm.xp.asarray(_songs('N')[1][:2])
  for cond in (True, False):
    trace = []
    a, b = fm.decoder_pass(z, 2, cond), fm.decoder_pass(z, 2, cond, trace=trace)
    assert a.dtype == b.dtype and np.array_equal(a, b)
    assert len(trace) == 2 and all(len(t[k]) == 2 for t in trace for k in fast.FastModel.TRACE_LAYER_KEYS)
    for j, t in enumerate(trace):
      assert t['eps'].dtype == np.dtype(dtype) and np.array_equal(t['eps'], a[j])
      assert (t['cross_in'][0] is not None) == cond and (len(t['cross'][0]) == 1) == cond
      if not cond:
        assert t['x2'][0] is t['x1'][0]
  # the f16x3 emulation too (the yardstick of the GPU test)
  fe = _oracle('N', 2, 'float32', 'f16x3')
  z = fe.xp.asarray(_songs('N')[1][:1])
  assert np.array_equal(fe.decoder_pass(z, 4, True), fe.decoder_pass(z, 4, True, trace=[]))


def test_set_film_takes_the_device_layout():
  fm = _oracle('N', 2, 'float64')
  table = _film32('N', 2)
  assert table.shape == (5, 4, 256)
  other = dc.make_oracle('N', 2, 'float64', film=table)
  for l in range(2):
    for k in range(2):
      assert other.film[l][k].dtype == np.float64 and np.array_equal(other.film[l][k], table[:, 2 * l + k].astype(np.float64))
  assert not np.array_equal(other.film[0][0], fm.film[0][0])


# ---- 2. truncation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,deep', [('N', 2), ('W', 3)])
def test_a_truncated_model_is_the_first_layers_of_the_deeper_one(name, deep):
  full = dc.build_params(name, deep)
  z = _songs(name)[1]
  if name == 'W':   # (cheap: the parameters and one unconditional pass of T 64)
    z = z[:, :64]
  traces = {}
  for depth in range(1, deep + 1):
    params = dc.build_params(name, depth)
    assert set(params) < set(full) or depth == deep
    assert all(params[k] is full[k] for k in params)
    fm = dc.make_oracle(name, depth, 'float64', film=None)
    fm.kv = [None]
    traces[depth] = dc.trace_song(fm, z[0], 2, False, 0)
  if name == 'N':   # ... and a conditional pass on the small spec
    for depth in (1, 2):
      traces[('c', depth)] = dc.trace_song(_oracle('N', depth, 'float64'), z[0], 2, True, 0)
    _same_prefix(traces[('c', 1)], traces[('c', 2)], 1)
  for depth in range(1, deep):
    _same_prefix(traces[depth], traces[deep], depth)


def _same_prefix(shallow, deeper, k):
  """NOTE: the FiLM tables of the two models come from the same time-embedding weights: layer l's rows are equal."""
  for key in fast.FastModel.TRACE_LAYER_KEYS:
    assert len(shallow[key]) == k
    for l in range(k):
      a, b = shallow[key][l], deeper[key][l]
      if key == 'cross':
        assert a.keys() == b.keys()
        for e in a:
          assert all(np.array_equal(u, v) for u, v in zip(a[e], b[e]))
      elif a is None:
        assert b is None
      else:
        assert np.array_equal(a, b), (key, l)


# ---- 3. why set_film exists ----------------------------------------------------------------------------------------
def test_a_shared_film_table_removes_the_table_from_the_comparison():
  """float32 oracle against float64 on eps: with its OWN float32 table 5e-5 (the float32 time signal), with the SAME
  table 5e-7 (the arithmetic) -- at least a factor 20."""
  z = _songs('N')[1][0]
  table = _film32('N', 2)
  ref_own = dc.trace_song(_oracle('N', 2, 'float64'), z, 2, True, 0)['eps']
  ref_shared = dc.trace_song(_oracle('N', 2, 'float64', film=table), z, 2, True, 0)['eps']
  f32 = dc.trace_song(_oracle('N', 2, 'float32'), z, 2, True, 0)['eps']
  own, shared = dc.stats(f32, ref_own), dc.stats(f32, ref_shared)
  print('eps of the float32 oracle against float64: own table rms %.2e max %.2e, shared table rms %.2e max %.2e' % (*own, *shared))
  assert own[0] >= 20 * shared[0] and own[1] >= 20 * shared[1]
  assert shared[0] < 5e-6


# ---- 4. separation --------------------------------------------------------------------------------------------------
class OnePlaneSite(fast.FastModel):
  """The f16x3 emulation with ONE named GEMM site's activation operand on one half plane (a dropped lo plane)."""
  site = None

  def mm(self, a, name):
    if name == self.site:
      w_parts, sc = self._w(name)
      hi = self._round16(a)
      return (self.xp.matmul(hi, w_parts[0]) + self.xp.matmul(hi, w_parts[1])) * (1.0 / sc)
    return super().mm(a, name)


@pytest.mark.parametrize('name,depth', [('N', 1), ('N', 2)])
def test_one_dropped_plane_at_any_site_is_ten_times_outside_the_bound(name, depth):
  """Every GEMM site of the last layer in turn: the buffer the site writes leaves 4 x the yardstick (the cap of the GPU
  test's factor) by at least a factor 10 in the rms statistic."""
  L = depth - 1
  z = _songs(name)[1][0]
  table = _film32(name, depth)
  ref = dc.expected(*_traced(name, depth, 'float64', 'f32', table, z), L)
  yard = dc.expected(*_traced(name, depth, 'float32', 'f16x3', table, z), L)
  bad = _oracle(name, depth, 'float32', 'f16x3', film=table, cls=OnePlaneSite)
  for site in dc.GEMM_SITES:
    bad.site = 'decoder/layers_%d/%s/kernel' % (L, site)
    try:
      got = dc.expected(bad, dc.trace_song(bad, z, 2, True, 0), L)
    finally:
      bad.site = None
    key = dc.SITE_BUFFER[site]
    s_bad, s_yard = dc.stats(got[key], ref[key]), dc.stats(yard[key], ref[key])
    print('%s depth %d site %-40s buffer %-4s rms %.2e against the yardstick %.2e: %.0f x' %
          (name, depth, site, key, s_bad[0], s_yard[0], s_bad[0] / s_yard[0]))
    assert s_bad[0] >= 10 * 4 * s_yard[0], (site, key, s_bad, s_yard)
    # ... and it stays visible in everything behind the site
    assert dc.stats(got['eps'], ref['eps'])[0] >= 4 * 4 * dc.stats(yard['eps'], ref['eps'])[0], site


def _traced(name, depth, dtype, precision, table, z):
  fm = _oracle(name, depth, dtype, precision, film=table)
  return fm, dc.trace_song(fm, z, 2, True, 0)


# ---- 5. the layout helpers on arrays filled with their own indices --------------------------------------------------
def test_row_ranges_per_pass_and_song():
  B, T = 3, 64
  rows = np.arange(2 * B * T)
  assert np.array_equal(rows[dc.pass_rows(1, B * T)], np.arange(B * T, 2 * B * T))
  seen = np.concatenate([rows[dc.song_rows(p, b, B, T)] for p in range(2) for b in range(B)])
  assert np.array_equal(seen, rows)
  assert rows[dc.song_rows(1, 2, B, T)][0] == (B + 2) * T
  flat = np.arange(2 * B * T * 5, dtype=np.float64)
  assert np.array_equal(dc.read_rows(flat, 5, dc.song_rows(1, 0, B, T))[:, 0], np.arange(B * T, (B + 1) * T) * 5)


def test_vt_permutation():
  J, T, segs = 128, 64, 3
  # the device writes key t of column j of segment s at [s][j][16 (t / 16) + perm16(t % 16)]: fill it that way
  vt = np.zeros((segs, J, T))
  s, j, t = np.meshgrid(np.arange(segs), np.arange(J), np.arange(T), indexing='ij')
  vt[s, j, dc.vt_key_pos(t)] = s * 1e6 + t * 1e3 + j
  for seg in range(segs):
    v = dc.read_v(vt.ravel(), J, T, seg)
    tt, jj = np.meshgrid(np.arange(T), np.arange(J), indexing='ij')
    assert np.array_equal(v, seg * 1e6 + tt * 1e3 + jj)
  assert sorted(dc.vt_key_pos(np.arange(16))) == list(range(16)) and dc.vt_key_pos(4) == 8   # (a real permutation, not the identity)


def test_stacked_cq_columns():
  B, T, J, nx, Bmax = 2, 64, 128, 2, 2
  flat = np.arange(nx * Bmax * T * J, dtype=np.float64)   # the allocation; the folded form uses its first BT nx J entries
  for b in range(B):
    for e in range(nx):
      got = dc.read_cq_folded(flat, B * T, nx, J, b, T, e)
      r, c = np.meshgrid(np.arange(b * T, (b + 1) * T), np.arange(e * J, (e + 1) * J), indexing='ij')
      assert np.array_equal(got, r * (nx * J) + c)


def test_ssq_slot_sum_reads_the_spare_slots():
  rng = np.random.default_rng(5)
  x = rng.standard_normal((4, 768))
  want = (x ** 2).sum(-1)
  s32 = dc.slot_sums32(x)
  assert s32.shape == (4, 24) and np.allclose(dc.ssq_row_sums(s32), want, rtol=1e-14)
  # a 48-column tiling: 16 partial sums in the first slots, the 8 spare slots zeroed (EpiResidualNorm::run48)
  s48 = np.zeros((4, 24))
  s48[:, :16] = (x.reshape(4, 16, 48) ** 2).sum(-1)
  assert np.allclose(dc.ssq_row_sums(s48), want, rtol=1e-14)
  stale = s48.copy()
  stale[:, 16:] = 3.0   # spare slots left as they were: the sum must show it
  assert np.all(np.abs(dc.ssq_row_sums(stale) - want) > 20)
  assert dc.has_32_wide_slots('N') and dc.has_32_wide_slots('M') and not dc.has_32_wide_slots('W')


# ---- the cases and the planner's restatement ------------------------------------------------------------------------
def test_the_matrix_reaches_what_it_says():
  fold = {c: dc.plans_fold(dc.cfg_call(*c), c[1] - 1) for c in dc.CFG_CASES}
  assert all(fold[(n, d, b, 'default')] for n in ('N', 'M') for d in (1, 2) for b in (1, 2))
  assert fold[('W', 2, 1, 'default')] and fold[('W', 2, 2, 'default')] and fold[('W', 2, 1, 'prefetch')] and fold[('W', 2, 1, 'no_dedup')]
  assert not fold[('W', 2, 3, 'default')] and not fold[('W', 2, 4, 'default')] and not fold[('W', 2, 1, 'no_fold')]
  for d in (1, 2):   # two modules un-folded: the only cases that read cq per module, cq2 among them
    call = dc.cfg_call('M', d, 2, 'no_fold')
    assert not fold[('M', d, 2, 'no_fold')] and {'cq', 'cq2', 'ao2'} <= set(dc.buffer_names(call)) and 'xg' not in dc.buffer_names(call)
  for name, depth, prec in dc.SINGLE_HANDLES:
    for call in dc.single_calls(name, depth, prec):
      assert dc.plans_fold(call, depth - 1) == (call.cond and prec != 'f16')
  assert len({c.tag for h in dc.SINGLE_HANDLES for c in dc.single_calls(*h)}) == 6 * len(dc.SINGLE_HANDLES)
  batch, z = dc.songs('W')
  counts = [(int((batch['encoder_input_tokens'][j] > 0).sum()), int(batch['encoder_continuous_mask'][j].sum())) for j in range(4)]
  assert counts[0] == (2047, 256) and counts[1] == (9, 0) and counts[2] == (0, 0) and counts[3][1] == 17 and counts[3][0] > 8
  assert z.shape == (4, 256, 128)


def test_stage_items_cut_device_and_reference_alike():
  """Buffers PACKED from the float64 expectation by the stated layout come back through stage_items as that expectation:
  a folded CFG step at layer 0 (dedup: no unconditional self rows) and an un-folded deeper one."""
  name, z = 'N', _songs('N')[1]
  sc = dc.SPECS[name]
  for depth, variant in ((1, 'default'), (2, 'no_fold')):
    call = dc.cfg_call(name, depth, 2, variant)
    fm = _oracle(name, depth, 'float64')
    L, B, T, J, D = depth - 1, 2, sc.T, sc.J, sc.emb
    exp = {(p, b): dc.expected(fm, dc.trace_song(fm, z[b], 0, p == 0, b), L) for p in range(2) for b in range(B)}
    M = 2 * B * T
    bufs = {'qk': np.full((M, 2 * J), np.nan), 'vt': np.full((2 * B, J, T), np.nan), 'ao': np.full((M, J), np.nan),
            'g': np.zeros((M, sc.mlp)), 'x': np.zeros((M, D)), 'ssq': np.zeros((M, D // 32)), 'y': np.zeros((M, D)),
            'eps': np.zeros((M, 128)), 'cq': np.full(B * T * J, np.nan), 'xg': np.zeros((B * T, D)), 'qp': np.zeros((B * T, J))}
    fold = dc.plans_fold(call, L)
    assert fold == (variant == 'default')
    for (p, b), e in exp.items():
      r = dc.song_rows(p, b, B, T)
      if not (L == 0 and p == 1):
        bufs['qk'][r] = np.concatenate([e['q'], e['k']], 1)
        bufs['vt'][p * B + b][:, dc.vt_key_pos(np.arange(T))] = e['v'].T
      if p == 0:
        bufs['ao'][r] = e['ao0']
        if fold:
          bufs['cq'].reshape(B * T, J)[b * T:(b + 1) * T] = e['cq_fold']
          bufs['xg'][b * T:(b + 1) * T], bufs['qp'][b * T:(b + 1) * T] = e['xg'], e['qp']
        else:
          bufs['cq'].reshape(B * T, J)[b * T:(b + 1) * T] = e['cq0']
      elif L > 0:
        bufs['ao'][r] = e['self_ao']
      bufs['g'][r], bufs['x'][r], bufs['ssq'][r], bufs['y'][r], bufs['eps'][r] = e['g'], e['x'], e['ssq32'], e['y'], e['eps']
    flat = {k: v.ravel() for k, v in bufs.items()}
    assert set(dc.buffer_names(call)) <= set(flat)
    for (p, b), e in exp.items():
      items = dc.stage_items(call, flat, p, b, e)
      labels = [i[0] for i in items]
      assert ('qk.q' in labels) == (not (L == 0 and p == 1)) and ('xg' in labels) == (fold and p == 0)
      assert ('ao(self)' in labels) == (p == 1 and L > 0) and ('ssq(slots)' in labels)
      for label, got, key in items:
        want = dc.pick(e, key)
        assert got.shape == want.shape and np.allclose(got, want, rtol=1e-13, atol=0), (depth, p, b, label)
