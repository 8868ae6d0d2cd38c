"""The case matrix and the layout helper of the attention launch forms (tests/attention_forms.py), without a GPU: what
tests/test_gpu_attention_forms.py runs is what the issue of the forms asks for, and the matrix cannot silently lose a path."""
import numpy as np
import pytest

from tests import attention_forms as af

MATRIX = af.MATRIX


def _mirror_query_blocks(blocks64, q_rows_per_seg, planes):
  """csrc/attention.h attention_query_blocks, line for line."""
  if blocks64 < 128: return 1
  if planes == 2 and blocks64 > 256 and q_rows_per_seg % 128 == 0: return 4
  return 2


def _mirror_launch_qb(case):
  """... and attention_launch_shape's argument to it (attention_blocks_seen): the launch's 64-row blocks, capped at one
  round of the chip unless the caller allows 128-row blocks and the queries are normalised."""
  ks = 1
  while 2 * ks <= case.ksplit: ks *= 2
  blocks64 = case.heads * (case.rows // 64) * ks * case.segs
  planes = 2 if case.prec in ('f16x3', 'bf16x3') else 1
  return _mirror_query_blocks(blocks64 if (case.allow_qb4 and not case.q_ssq) else min(blocks64, 256), case.rows, planes)


def test_ids_are_unique():
  ids = [c.id for c in MATRIX]
  assert len(set(ids)) == len(ids)
  assert len({c.seed for c in MATRIX}) == len(MATRIX)


@pytest.mark.parametrize('case', MATRIX, ids=lambda c: c.id)
def test_pack_then_unpack_is_the_identity(case):
  q_s, k_s, v_s, ssq_s, _ = af.make_inputs(case)
  arrays = af.pack(case, q_s, k_s, v_s, ssq_s)
  f = af.launch_fields(case)
  ka, r0, kr = case.window
  assert arrays['q'].shape == (case.segs * case.rows, f['ldq']) and arrays['k'].shape == (case.segs * ka, f['ldk'])
  assert arrays['v'].shape == (case.segs, ka, case.J) and arrays['n_keys'].dtype == np.int32
  assert (arrays['q'] is arrays['k']) == (case.layout == 'self')
  q_u, k_u, v_u = af.unpack(case, arrays)
  for s in range(case.segs):
    n = case.n_keys[s]
    assert np.array_equal(q_u[s], q_s[s])
    assert np.array_equal(k_u[s][:n], k_s[s][:n]) and np.array_equal(v_u[s][:n], v_s[s][:n])
    # behind the count: loud, finite, inside the half planes' range
    assert np.all(np.abs(k_u[s][n:]) == 100.0) and np.all(np.abs(v_u[s][n:]) == 1000.0)
    assert k_u[s].shape == (kr, case.J) and v_u[s].shape == (kr, case.J)
  # nothing but the windows (and the queries' columns) is data
  seen = np.zeros(case.segs * ka, bool)
  for a, b in af.k_windows(case):
    seen[a:b] = True
  assert np.isnan(arrays['v'].reshape(case.segs * ka, case.J)[~seen]).all() and np.isfinite(arrays['v'].reshape(case.segs * ka, case.J)[seen]).all()
  if case.layout == 'cross':
    assert np.isnan(arrays['k'][~seen]).all() and np.isfinite(arrays['k'][seen]).all()
    cols = np.zeros(f['ldq'], bool)
    cols[f['q_col']:f['q_col'] + case.J] = True
    assert np.isnan(arrays['q'][:, ~cols]).all() and np.isfinite(arrays['q'][:, cols]).all()
  else:
    assert np.isfinite(arrays['q']).all()
  if case.q_ssq:
    assert arrays['q_ssq'].shape == (case.segs * case.rows, af.SSQ_TILES)
    assert np.array_equal(arrays['q_ssq'][case.rows * (case.segs - 1):], ssq_s[-1])
  o = np.arange(case.segs * case.rows * case.J, dtype=np.float32).reshape(case.segs * case.rows, case.J)
  assert np.array_equal(np.concatenate(af.split_output(case, o), 0), o)


def test_windows_of_segments_and_regions_never_overlap():
  for regions in af.CACHES:
    ka = regions[0][0]
    assert all(w[0] == ka for w in regions)
    for segs in (1, 2, 4):
      spans = []
      for w in regions:
        c = af.Case(group='cross', prec='f16x3', heads=2, segs=segs, rows=256, layout='cross', window=w,
                    n_keys=(w[2],) * segs, seed=0)
        spans += af.k_windows(c)
      spans.sort()
      assert spans[0][0] >= 0 and spans[-1][1] <= segs * ka
      for (a0, b0), (a1, b1) in zip(spans, spans[1:]):
        assert a0 < b0 <= a1 < b1
  for c in MATRIX:   # every case's window lies inside its segment's allocation, on the alignment the op asks for
    ka, r0, kr = c.window
    assert 0 <= r0 and r0 + kr <= ka and kr % 32 == 0 and r0 % 32 == 0 and ka % 8 == 0
    assert len(c.n_keys) == c.segs and all(0 <= n <= kr for n in c.n_keys)


@pytest.mark.parametrize('case', MATRIX, ids=lambda c: c.id)
def test_expected_block_shape_is_the_launchers(case):
  ran = af.expected_ran(case)
  assert ran['ran_qb'] == _mirror_launch_qb(case)
  assert af.attention_query_blocks(200, 256, 2) == _mirror_query_blocks(200, 256, 2)
  if case.expect_qb is not None:
    assert ran['ran_qb'] == case.expect_qb
  if case.q_ssq:
    assert ran['ran_qb'] in (1, 2)
  if ran['ran_qb'] == 4:
    assert ran['ran_prefetch_wave'] == 0 and case.prec in af.TWO_PLANE
  assert ran['ran_touch_ahead'] <= ran['ran_prefetch_wave']


def test_the_matrix_reaches_every_path():
  ran = [af.expected_ran(c) for c in MATRIX]
  assert {r['ran_qb'] for r in ran} == {1, 2, 4}
  assert {r['ran_prefetch_wave'] for r in ran} == {0, 1} and {r['ran_touch_ahead'] for r in ran} == {0, 1}
  assert {c.merge_in_launch for c in MATRIX if c.ksplit > 1} == {False, True}
  assert any(c.segs > 1 and c.ksplit > 1 and c.merge_in_launch for c in MATRIX)
  assert any(c.segs > 1 and c.ksplit > 1 and not c.merge_in_launch for c in MATRIX)
  assert any(c.prefetch and r['ran_qb'] == 4 for c, r in zip(MATRIX, ran))   # a target given, no wave run
  by_group = {g: [c for c in MATRIX if c.group == g] for g in ('encoder_self', 'decoder_self', 'cross', 'touch_ahead', 'folded')}
  assert all(by_group.values())
  # 1. encoder self: every precision on every key count
  assert {(c.prec, c.rows, c.n_keys[0]) for c in by_group['encoder_self'] if c.qp == 0} == \
      {(p, r, n) for p in ('f16x3', 'f16', 'bf16x3', 'bf16') for r, n in ((128, 1), (128, 33), (128, 100), (128, 128), (192, 129))}
  assert {c.qp for c in by_group['encoder_self']} == {0, 1, 2, 3}
  # 2. decoder self: the three block shapes, with and without a weight target
  d = {(c.segs, c.prefetch): af.expected_ran(c) for c in by_group['decoder_self'] if c.prec == 'f16x3' and c.heads == 12}
  assert [d[(s, False)]['ran_qb'] for s in (2, 3, 8)] == [1, 2, 4] and [d[(s, True)]['ran_qb'] for s in (2, 3, 8)] == [1, 2, 4]
  assert [d[(s, True)]['ran_prefetch_wave'] for s in (2, 3, 8)] == [1, 1, 0]
  assert any(c.n_keys == (256, 77) and c.heads == 2 for c in by_group['decoder_self'])
  # 3. cross: every window with every segment count and split, both merges, both head counts; the counts of a launch differ
  x = by_group['cross']
  for w in af.WINDOWS:
    splits = {1, 2, 4, 8} if w == af.WIN_1024 else {1, 2, 4}
    for segs in (1, 2, 4):
      got = {(c.ksplit, c.merge_in_launch) for c in x if c.window == w and c.segs == segs}
      assert got == {(1, False)} | {(k, m) for k in splits - {1} for m in (False, True)}
    assert {c.heads for c in x if c.window == w} == {2, 12}
  for c in x:
    assert len(set(c.n_keys)) == c.segs and c.window[2] in c.n_keys and (c.segs == 1 or 0 in c.n_keys)
    assert c.repeats == (3 if c.merge_in_launch else 1)
  assert any(max(af.stages(n, c.ksplit)) > 0 and min(af.stages(n, c.ksplit)) == 0 for c in x for n in c.n_keys)   # parts without a stage
  assert {c.prec for c in x} == {'f16x3', 'f16', 'bf16x3', 'bf16'}
  # 4. touch-ahead: the wave's stage count 0, 1, 2, 3, below and above NS + ahead
  t = by_group['touch_ahead']
  assert all(r['ran_touch_ahead'] == 1 for c, r in zip(MATRIX, ran) if c.group == 'touch_ahead')
  assert {c.touch_ahead for c in t} == {1, 2, 16} and {c.pf_late for c in t} == {0, 1} and {c.ksplit for c in t} == {1, 4}
  assert {c.n_keys[0] for c in t if c.window == af.WIN_1024} == {0, 1, 129, 257, 1000, 1024}
  assert {af.stages(c.n_keys[0])[0] for c in t} >= {0, 1, 2, 3, 8}
  assert any(af.stages(c.n_keys[0])[0] > 2 + c.touch_ahead for c in t) and any(0 < af.stages(c.n_keys[0])[0] <= 2 + c.touch_ahead for c in t)
  assert {af.expected_ran(c)['ran_qb'] for c in t} == {1, 2}
  # 5. folded: both query columns, both precisions, both windows, one and two segments, with the wave at one segment
  f = by_group['folded']
  assert all(c.q_ssq and c.q_ld == 2 and c.prec in af.TWO_PLANE for c in f)
  assert {(c.q_col, c.segs) for c in f} >= {(0, 1), (1, 1), (0, 2), (1, 2)}
  assert {(c.window, c.ksplit, c.prec) for c in f} >= {(w, k, p) for w in (af.WIN_192, af.WIN_1024) for k in (1, 2) for p in af.TWO_PLANE}
  assert all(c.touch_ahead == 2 and c.prefetch for c in f if c.segs == 1 and c.qp == 0)
  assert any(c.heads * 4 * af.ran_ksplit(c.ksplit) * c.segs > 256 for c in f)   # would be 128-row blocks, were the queries normalised


def test_stage_counts():
  assert af.stages(0) == [0] and af.stages(1) == [1] and af.stages(129) == [2] and af.stages(1024) == [8]
  assert af.stages(129, 4) == [1, 1, 0, 0] and af.stages(1000, 4) == [2, 2, 2, 2] and af.stages(64, 3) == [1, 0]
