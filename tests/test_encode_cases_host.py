"""The encode-stage cases and their layout helper (tests/encode_cases.py), without a GPU: the helper is proven against
arrays built the other way round (scalar loops that follow the C++ index arithmetic of encode_impl and EpiQKV), the
gated interleave against EpiF32StoreGated's statement, and every case of the matrix runs through the oracle."""
import numpy as np
import pytest

from tests import encode_cases as ec


def _scalar_vt_perm16(o):
  """gemm_h16.h: return 8 * ((o >> 2) & 1) + (o & 3) + 4 * (o >> 3);"""
  return 8 * ((o >> 2) & 1) + (o & 3) + 4 * (o >> 3)


def test_the_matrix_is_what_the_issue_of_the_encode_stage_asks_for():
  assert ec.HANDLES == (('A', 'f16x3'), ('A', 'f16'), ('A_regular', 'f16x3'), ('B', 'f16x3'), ('C', 'f16x3'),
                        ('C', 'bf16x3'), ('D', 'f16x3'))
  assert {ec.NORM_VPL[s.emb] for s in ec.SPECS.values()} == {1, 2, 3}
  for name, sc in ec.SPECS.items():
    spec = ec.build_spec(name)
    t5 = spec.t5
    assert (t5.emb_dim, t5.num_heads, t5.mlp_dim, t5.num_encoder_layers, t5.num_decoder_layers) == \
        (sc.emb, sc.heads, sc.mlp, sc.enc_layers, sc.dec_layers)
    assert spec.task_feature_lengths['inputs'] == sc.inputs and spec.task_feature_lengths['targets'] == 64
    assert spec.task_feature_lengths.get('targets_context', 0) == sc.context and spec.has_context == bool(sc.context)
    assert sc.inputs % 64 == 0 and sc.context % 64 == 0
    assert spec.diffusion.sampler.schedule.num_steps == 3
    assert t5.decoder_cross_attend_style == sc.style and t5.context_positions == sc.positions
  assert ec.SPECS['B'].style == 'sum_cross_attends' and ec.SPECS['A_regular'].positions == 'regular'
  assert ec.SPECS['A'].positions == ec.SPECS['C'].positions == 'terminal_relative'
  # every case once in each row of a call; the rows of a call differ
  assert sorted(c[0] for c in ec.CALLS) == sorted(c[1] for c in ec.CALLS) == sorted(ec.COUNT_CASES)
  assert all(a != b for a, b in ec.CALLS)


@pytest.mark.parametrize('name', ['A', 'C', 'D'])
def test_valid_count_cases(name):
  sc = ec.SPECS[name]
  L, C = sc.inputs, sc.context
  want = {'1_C': (1, C), 'L_1': (L, min(1, C)), '63_0': (63, 0), '64_63': (64, min(63, C)), '65_64': (65, min(64, C)),
          '0_Cm1': (0, max(C - 1, 0)), 'holes': (40, 20 if C else 0)}
  for case in ec.COUNT_CASES:
    tok, ctx = ec.case_masks(case, L, C)
    assert (int(tok.sum()), int(ctx.sum())) == want[case]
    if case != 'holes':   # prefixes
      assert tok[:tok.sum()].all() and ctx[:ctx.sum()].all()
  tok, ctx = ec.case_masks('holes', L, C)
  assert tok[L - 1] and not tok[:tok.sum()].all()             # pos differs from arange, the last position is used
  assert np.nonzero(tok)[0].tolist() != list(range(40))
  if C:
    assert not ctx[0] and not ctx[1:1 + 20].all()
  for call in ec.CALLS:
    args = ec.make_call(name, call)
    assert args['tokens'].dtype == np.int32 and args['tokens'].shape == (2, L) and args['tokens'].max() < 256
    for b, case in enumerate(call):
      assert ec.valid_counts(args, b) == want[case]
      assert np.array_equal(args['tokens'][b] > 0, ec.case_masks(case, L, C)[0])
    assert ec.valid_counts(args, 0) != ec.valid_counts(args, 1)
    again = ec.make_call(name, call)
    assert np.array_equal(args['tokens'], again['tokens'])
    if C:
      assert args['ctx'].shape == (2, C, 128) and args['mask'].dtype == np.int32 and np.array_equal(args['ctx'], again['ctx'])
    else:
      assert args['ctx'] is None and args['mask'] is None


def test_vt_key_pos_is_the_kernels_permutation():
  perm = [_scalar_vt_perm16(o) for o in range(16)]
  assert sorted(perm) == list(range(16))
  assert perm == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
  keys = np.arange(200)
  assert np.array_equal(ec.vt_key_pos(keys), [(k & ~15) + perm[k & 15] for k in range(200)])


@pytest.mark.parametrize('name', ['A', 'B', 'C', 'D'])
@pytest.mark.parametrize('counts', [((1, 64), (128, 1)), ((63, 0), (37, 13)), ((65, 64), (0, 63)), ((40, 20), (17, 5))])
def test_layout_helper_against_arrays_built_the_other_way_round(name, counts):
  """The cache as encode_impl / EpiQKV write it, element by element with the C++ index arithmetic; read back through the
  helper.  Valid counts that are no multiples of 16 included."""
  lay = ec.Layout.of(name)
  sc = ec.SPECS[name]
  if not sc.context:
    counts = tuple((t, 0) for t, _ in counts)
  rng = np.random.default_rng(5)
  S_pad, J, Bmax, Ld = lay.S_pad, lay.J, lay.Bmax, lay.Ld
  assert S_pad == -(-sc.inputs // 64) * 64 + -(-sc.context // 64) * 64 and lay.key_off == (0, -(-sc.inputs // 64) * 64)
  assert lay.n_cross == (2 if (name == 'B') else 1)
  cross_k = np.full(Ld * Bmax * S_pad * J, np.nan, np.float32)
  cross_vt = np.full(Ld * Bmax * J * S_pad, np.nan, np.float32)
  truth = {}
  for l in range(Ld):
    for b, (n_tok, n_ctx) in enumerate(counts):
      reg_rows = (n_tok, n_ctx) if lay.n_cross == 2 else (n_tok + n_ctx,)
      koff = (l * Bmax + b) * S_pad * J                      # encode_impl: koff
      for e, n in enumerate(reg_rows):
        r0 = lay.key_off[e]
        k = rng.standard_normal((n, J)).astype(np.float32)
        v = rng.standard_normal((n, J)).astype(np.float32)
        truth[l, b, e] = (k, v)
        for i in range(n):
          # K: planes_at(kc, koff + r0 * J), row-major, ld_qk = J
          cross_k[koff + r0 * J + i * J: koff + r0 * J + (i + 1) * J] = k[i]
          # V^T: planes_at(vtc, koff + r0), [column j][vt_ld = S_pad], key permuted inside its 16
          pos = (i & ~15) + _scalar_vt_perm16(i & 15)
          cross_vt[koff + r0 + np.arange(J) * S_pad + pos] = v[i]   # off = (seg * vt_rows + j) * vt_ld + key position
  for (l, b, e), (k, v) in truth.items():
    n = k.shape[0]
    assert np.array_equal(lay.read_k(cross_k, l, b, e, n), k)
    assert np.array_equal(lay.read_v(cross_vt, l, b, e, n), v)
  # the helper's regions are what was written, and its masks name exactly the written entries
  for b, (n_tok, n_ctx) in enumerate(counts):
    regs = lay.regions(n_tok, n_ctx)
    assert [(e, n) for e, n, _ in regs] == [(e, truth[0, b, e][0].shape[0]) for e in range(lay.n_cross)]
    assert all(parts[0] + parts[1] == n for _, n, parts in regs)
  assert np.array_equal(lay.valid_mask_k(counts).ravel(), ~np.isnan(cross_k))
  assert np.array_equal(lay.valid_mask_vt(counts).ravel(), ~np.isnan(cross_vt))
  # regions tile the slab
  spans = [lay.region_rows(e) for e in range(lay.n_cross)]
  assert spans[0][0] == 0 and spans[-1][1] == S_pad and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
  # enc rows: the context behind the valid tokens (concat) or at its region (sum)
  for n_tok, n_ctx in counts:
    assert lay.enc_rows(n_tok, n_ctx) == (0, lay.key_off[1] if name == 'B' else n_tok)


@pytest.mark.parametrize('F', [256, 2048])
def test_gated_interleave_is_epif32storegated(F):
  """EpiF32StoreGated: out[m * ldc + (n / 16) * 32 + which * 16 + (n % 16)] = v -- written with scalar loops, read with
  the helper; the packed order is a permutation of the 2F columns in alternating blocks of 16."""
  row = np.full(2 * F, np.nan, np.float32)
  wi = [np.arange(F, dtype=np.float32), 10000 + np.arange(F, dtype=np.float32)]
  for which in range(2):
    for n in range(F):
      assert np.isnan(row[(n // 16) * 32 + which * 16 + (n % 16)])
      row[(n // 16) * 32 + which * 16 + (n % 16)] = wi[which][n]
  assert not np.isnan(row).any()
  a, b = ec.split_gated(row[None, None], F)
  assert a.shape == (1, 1, F) and np.array_equal(a[0, 0], wi[0]) and np.array_equal(b[0, 0], wi[1])
  assert np.array_equal(row[:16], wi[0][:16]) and np.array_equal(row[16:32], wi[1][:16]) and np.array_equal(row[32:48], wi[0][16:32])


def test_stats():
  ref = np.array([3.0, -4.0, 0.0, 5.0])
  got = ref + np.array([0.0, 0.5, 0.0, -0.1])
  scale = np.sqrt(50.0 / 4)
  r, m = ec.stats(got, ref)
  assert abs(r - np.sqrt(0.26 / 4) / scale) < 1e-15 and abs(m - 0.5 / scale) < 1e-15


@pytest.mark.parametrize('name', list(ec.SPECS))
def test_every_case_runs_through_the_oracle(name):
  """FastModel.encode takes every call of the matrix; what it records has the rows the layout expects."""
  spec = ec.build_spec(name)
  params = ec.build_params(name, spec)
  lay = ec.Layout.of(name)
  fm = ec.make_oracle(name, spec, params, 'float64')
  for call in ec.CALLS:
    args = ec.make_call(name, call)
    rows = ec.oracle_encode(fm, args)
    for b, row in enumerate(rows):
      n_tok, n_ctx = ec.valid_counts(args, b)
      tok, ctx = row['enc']
      assert (tok is None) == (n_tok == 0) and (ctx is None) == (n_ctx == 0)
      assert tok is None or tok.shape == (n_tok, lay.D)
      assert ctx is None or ctx.shape == (n_ctx, lay.D)
      for e, n, _ in lay.regions(n_tok, n_ctx):
        assert (e in row['kv']) == (n > 0)
        if n:
          assert len(row['kv'][e]) == lay.Ld
          for k, v in row['kv'][e]:
            assert k.shape == (n, lay.J) and v.shape == (n, lay.J) and np.isfinite(k).all() and np.isfinite(v).all()
