"""No GPU: helpers.planes_merged -- the exact reference of the device's operand planes (tests/test_gpu_sampler_planes.py and
the plane assertions of test_gpu_invert / _edit_strength / _resample) -- against a brute-force search for the nearest
representable value in float64, ties to the even code."""
import numpy as np
import pytest

from tests import helpers


def _table(kind):
  """Every finite value of the plane type, ascending, as float64, with its 16-bit code."""
  codes = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
  if kind == 'f16':
    vals = codes.view(np.float16).astype(np.float64)
  else:   # bfloat16 = the upper half of a float32
    with np.errstate(invalid='ignore'):   # (the NaN codes are dropped below)
      vals = (codes.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
  ok = np.isfinite(vals) & ~((vals == 0) & (codes >= 0x8000))   # (one zero)
  vals, codes = vals[ok], codes[ok]
  order = np.argsort(vals, kind='stable')
  return vals[order], codes[order]


def _nearest(x64, table):
  """The table value nearest to each x (float64, exact differences); of two equally near ones, the even code's."""
  vals, codes = table
  hi = np.clip(np.searchsorted(vals, x64), 1, len(vals) - 1)
  lo = hi - 1
  d_lo, d_hi = x64 - vals[lo], vals[hi] - x64
  take_hi = (d_hi < d_lo) | ((d_hi == d_lo) & (codes[hi] % 2 == 0))
  return np.where(take_hi, vals[hi], vals[lo]), d_hi == d_lo


def _values(kind):
  rng = np.random.default_rng(17)
  vals, _ = _table(kind)
  parts = [rng.standard_normal(1500), 1e-3 * rng.standard_normal(800), rng.uniform(-65504.0, 65504.0, 800),
           # the half subnormal range and below it (a lo plane lives there), both signs
           rng.uniform(-2.0 ** -14, 2.0 ** -14, 600), rng.uniform(-2.0 ** -23, 2.0 ** -23, 300)]
  x = np.concatenate(parts).astype(np.float32)
  # ties of the hi plane: the midpoint of two neighbours of the type (exact in float32), around random values, around 1,
  # in the subnormal range of half and at its lower end (2^-25: between 0 and the smallest subnormal)
  pick = rng.integers(1, len(vals) - 1, 600)
  mid = (vals[pick] + vals[pick + 1]) / 2
  mid = mid[np.abs(mid) > 1e-30].astype(np.float32)
  # ... and ties of the LO plane: a hi value plus the midpoint of two small neighbours
  small = np.flatnonzero((np.abs(vals) < 2.0 ** -10) & (np.abs(vals) > 2.0 ** -24))
  sp = rng.choice(small[:-1], 300)
  lo_mid = (1.0 + (vals[sp] + vals[sp + 1]) / 2)
  lo_mid = lo_mid[lo_mid.astype(np.float32).astype(np.float64) == lo_mid].astype(np.float32)
  edge = np.array([0.0, 65504.0, -65504.0, np.nextafter(np.float32(65504.0), np.float32(np.inf)),
                   -np.nextafter(np.float32(65504.0), np.float32(np.inf)), 65504.0 * (1 - 2.0 ** -12), 1.0, -1.0,
                   1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25, 2.0 ** -26,
                   2.0 ** -14, 2.0 ** -14 - 2.0 ** -25], np.float32)
  return np.concatenate([x, mid, lo_mid, edge])


@pytest.mark.parametrize('precision', ['f16x3', 'f16', 'bf16x3', 'bf16'])
def test_planes_merged_is_the_nearest_representable_split(precision):
  kind = 'bf16' if precision.startswith('bf16') else 'f16'
  table = _table(kind)
  z = _values(kind)
  assert len(z) > 3000 and (np.abs(z) == 65504.0).sum() == 2 and (z == 0).any()
  z64 = z.astype(np.float64)
  hi, hi_tie = _nearest(z64, table)
  assert (np.abs(hi) <= 65504.0).all() or kind == 'bf16'
  # the rounding alone, ties included
  np.testing.assert_array_equal(helpers.round_to_plane(z, precision).astype(np.float64), hi)
  r = z64 - hi
  assert (r.astype(np.float32).astype(np.float64) == r).all(), 'z - hi is exact in float32'
  lo, lo_tie = _nearest(r, table)
  assert hi_tie.sum() > 100 and lo_tie.sum() > 20, (hi_tie.sum(), lo_tie.sum())   # (ties in both planes)
  want = hi + lo if precision.endswith('x3') else hi
  assert (want.astype(np.float32).astype(np.float64) == want).all(), 'hi + lo is exact in float32'
  got = helpers.planes_merged(z, precision)
  assert got.dtype == np.float32
  np.testing.assert_array_equal(got.astype(np.float64), want)
  if kind == 'f16':   # subnormal lo values are there, and kept
    sub = (lo != 0) & (np.abs(lo) < 2.0 ** -14)
    assert sub.mean() > 0.05
    if precision == 'f16x3':
      assert (got.astype(np.float64)[sub] != hi[sub]).all()
  if precision.endswith('x3'):   # two planes say more than one, and less than float32
    assert (got != helpers.planes_merged(z, kind)).any() and (got != z).any()
    assert (np.abs(got.astype(np.float64) - z64) <= np.abs(hi - z64)).all()
