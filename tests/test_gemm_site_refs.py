"""CPU checks of the float64 restatements tests/test_gpu_gemm_sites.py compares the device against
(tests/gemm_site_refs.py): each one against an independent evaluation of the same function at one small shape, so that
a wrong restatement cannot pass for a right kernel."""
import numpy as np

from oracle import backend, ops
from tests import gemm_site_refs as R

XP = backend.NumpyBackend('float64')


def _inputs(m=6, k=64, n=96, steps=3, seed=0):
  rng = np.random.default_rng(seed)
  x = 3.0 * rng.standard_normal((m, n))
  x[:, ::7] *= 20.0
  return dict(x=x, a=rng.standard_normal((m, k)), w=rng.standard_normal((k, n)) / np.sqrt(k),
              gamma=1.0 + 0.3 * rng.standard_normal(n), scale=0.5 * rng.standard_normal((steps, n)),
              fbias=0.5 * rng.standard_normal((steps, n)), rng=rng)


def test_producer_and_folded_consumer_equal_norm_film_matmul():
  """residual_norm -> linear with its partial sums and bias . W  ==  (RMSNorm(x + a.w) (1 + s) + b) . W2."""
  d = _inputs()
  rng, n, step = d['rng'], 96, 1
  w2 = rng.standard_normal((n, 64)) / np.sqrt(n)
  g = d['gamma'][None, :] * (1.0 + d['scale'])           # [steps][n]
  bw = d['fbias'] @ w2                                     # [steps][64]
  x1, ssq_full, y, _ = R.residual_norm(d['x'], d['a'], d['w'], g, g, 3, step=step)
  got = R.linear(y, w2, ssq=R.partial_ssq(x1), bias=bw, step=step)
  h = ops.rms_layer_norm(XP, d['x'] + d['a'] @ d['w'], d['gamma']) * (1.0 + d['scale'][step]) + d['fbias'][step]
  np.testing.assert_allclose(got, h @ w2, rtol=1e-12, atol=1e-12)
  np.testing.assert_allclose(ssq_full, R.partial_ssq(x1).sum(axis=1), rtol=1e-13)
  # without the row scale the bias is not applied either (the epilogue's form 0)
  np.testing.assert_allclose(R.linear(y, w2), y @ w2, rtol=0, atol=0)


def test_residual_norm_forms_element_by_element():
  d = _inputs(m=4)
  g_lo, g_hi = d['gamma'][None, :] * (1.0 + d['scale']), d['gamma'][None, :] * (1.0 - d['scale'])
  upd = d['a'] @ d['w']
  x1, _, y, y2 = R.residual_norm(d['x'], d['a'], d['w'], g_lo, None, 1, step=2, g2=d['gamma'], y2_rows=2)
  for r in range(4):
    for c in range(0, 96, 5):
      xv = d['x'][r, c] + upd[r, c]
      assert x1[r, c] == xv
      assert (y[r, c] == xv * g_lo[2, c]) if r < 1 else np.isnan(y[r, c])
      assert (y2[r, c] == xv * d['gamma'][c]) if r < 2 else np.isnan(y2[r, c])
  # DUP: 4 rows computed, written again 4 rows further on with the other gain
  xd = np.concatenate([d['x'], np.full((4, 96), 7.0)])
  x2, ssq, yd, _ = R.residual_norm(xd, d['a'], d['w'], g_lo, g_hi, 0, step=0, dup_rows=4)
  np.testing.assert_array_equal(x2[4:], x2[:4])
  np.testing.assert_array_equal(x2[:4], d['x'] + upd)
  np.testing.assert_array_equal(yd[:4], x2[:4] * g_lo[0])
  np.testing.assert_array_equal(yd[4:], x2[:4] * g_hi[0])
  np.testing.assert_array_equal(ssq[4:], ssq[:4])
  np.testing.assert_array_equal(R.residual(d['x'], d['a'], d['w']), d['x'] + upd)


def test_mlp_in_equals_gated_gelu_of_the_normed_input():
  d = _inputs(n=64)
  rng, k, f, step = d['rng'], 64, 32, 2
  xr = 3.0 * rng.standard_normal((6, k))
  gamma = 1.0 + 0.3 * rng.standard_normal(k)
  sc, bi = 0.5 * rng.standard_normal((3, k)), 0.5 * rng.standard_normal((3, k))
  wi0, wi1 = 4.0 * rng.standard_normal((k, f)) / np.sqrt(k), rng.standard_normal((k, f)) / np.sqrt(k)
  a = xr * (gamma * (1.0 + sc[step]))
  bias = np.concatenate([bi @ wi0, bi @ wi1], axis=1)
  got = R.mlp_in(a, wi0, wi1, ssq=R.partial_ssq(xr), bias=bias, step=step)
  h = ops.rms_layer_norm(XP, xr, gamma) * (1.0 + sc[step]) + bi[step]
  ref = 0.5 * (h @ wi0) * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * ((h @ wi0) + 0.044715 * (h @ wi0) ** 3))) * (h @ wi1)
  np.testing.assert_allclose(got, ref, rtol=1e-11, atol=1e-12)
  np.testing.assert_allclose(R.mlp_in(a, wi0, wi1), ops.gelu_tanh(XP, a @ wi0) * (a @ wi1), rtol=1e-13)


def test_in_proj_and_add_store_element_by_element():
  d = _inputs(m=6, k=64, n=32)
  rng = d['rng']
  pos = rng.standard_normal((4, 32))
  g = d['gamma'][None, :] * (1.0 + d['scale'])
  x, ssq, y, y2 = R.in_proj(d['a'], d['w'], pos, g, step=1, passes=2, g2=d['gamma'])
  assert x.shape == (12, 32) and y2.shape == (6, 32)
  for p in range(2):
    for r in range(6):
      row = d['a'][r] @ d['w'] + pos[r % 4]
      np.testing.assert_allclose(x[p * 6 + r], row, rtol=1e-13)
      np.testing.assert_allclose(y[p * 6 + r], row * g[1], rtol=1e-13)
      np.testing.assert_allclose(ssq[p * 6 + r], np.dot(row, row), rtol=1e-13)
  np.testing.assert_allclose(y2, x[:6] * d['gamma'], rtol=1e-13)
  add = rng.standard_normal((6, 32))
  np.testing.assert_allclose(R.add_store(d['a'], d['w'], add), np.einsum('mk,kn->mn', d['a'], d['w']) + add, rtol=1e-13)


def test_plane_rounding_matches_the_number_formats():
  x = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.3], np.float32)
  h = R.round_plane(x, 'f16')
  assert h[0] == 1.0 and h[1] == 1.0 and h[2] == np.float32(1.0 + 2.0 ** -9) and h[3] == 65504.0   # ties to even
  b = R.round_plane(x, 'bf16')
  assert b[4] == 1.0 and b[5] == np.float32(1.0 + 2.0 ** -6) and abs(b[6] + 0.3) <= 0.3 * 2.0 ** -8
  # bfloat16 = the top 16 bits of a float32
  assert np.all(R.round_plane(x, 'bf16').view(np.uint32) & 0xFFFF == 0)
  w = np.array([0.03, 7e-6], np.float32)
  assert np.all(np.abs(R.round_weight(w, 'f16') - w) <= np.abs(w) * 2.0 ** -11)   # (7e-6 x 512 is a normal half)
