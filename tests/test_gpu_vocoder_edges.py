"""The device vocoder at the shapes, signals and corners tests/test_gpu_vocoder.py never visits.

Shapes (songs, frames) = vc.EDGE_SHAPES: (3, 63) puts every song boundary and every straddling row of the batched layout
on a 64-row GEMM tile edge with an odd number of songs, (2, 65) is one frame past a tile, (1, 129) has no straddling row
and more than two tiles, (1, 1) is a one-row launch whose overlap-add sees only the one-tap normalisation.  Song 1 of a
batch is silent (exact zeros).  Sample counts n = F * 320 - r, r in (0, 1, 319).  Everything is compared elementwise, on
every element, against the float64 specification in audio_codecs.py under forward error bounds built from float64
quantities (tools/vocoder_cases.py); the layout invariants the kernels' comments rely on (pad columns, straddling rows and
the zero extension of every padded signal are zero) are read back from the handle's work buffers
(msd_vocoder_debug_read), and the unit vector behind the phase update is fed the corners it documents through
msd_op_vocoder_phase and msd_op_vocoder_load_spec.  Measured ratios: profiles/vocoder_edges.log."""
import ctypes
import functools
import itertools
import os
import sys

import numpy as np
import pytest

import msd_amd
from msd_amd import audio_codecs as ac
from msd_amd import native

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import vocoder_cases as vc  # noqa: E402  (tools/vocoder_cases.py)
from tests.test_gpu_vocoder import _assert_mel  # noqa: E402  (the encoder's criterion, as it stands there)

pytestmark = pytest.mark.gpu

HOP, BINS, HALF, SPEC = vc.HOP, vc.BINS, 544, 1088
U = vc.U
LOG_FLOOR = np.float32(np.log(1e-5))
DIRTY = (2, 131)   # a call of more rows than any shape here: what the work buffers hold before a test's own call
shapes = pytest.mark.parametrize('shape', vc.EDGE_SHAPES, ids=lambda s: '%dx%d' % s)


@pytest.fixture(scope='module')
def voc():
  import torch
  assert torch.cuda.is_available()
  return msd_amd.vocoder.GriffinLimVocoder()


@functools.lru_cache(maxsize=None)
def _data(shape):
  """The inputs and float64 references of one shape, computed once and never written to."""
  b, f = shape
  x = vc.songs(b, f)
  logmel = vc.logmel_of(x)
  d = {'x': x, 'logmel': logmel, 'phase': vc.closed_form_phase(b, f).astype(np.float32),
       'mag': ac.mel_to_linear(logmel.astype(np.float64)), 'mag_bound': vc.mag_bound(logmel),
       'spec32': vc.pack_spec(ac.stft(x))}
  return d


def _silent(x64):
  """Per song: does the float64 specification see silence?  (All zeros -- or one sample under the window's zero.)"""
  return np.abs(ac.stft(x64)).max(axis=(1, 2)) == 0.0


def _dirty(voc):
  """Fill every work buffer, straddling rows and both halves of the Y pair included, with another call's numbers."""
  big = _data(DIRTY)
  voc.decode(big['logmel'], n_iters=2, seed=5)
  voc.encode(big['x'].astype(np.float32))   # (the encoder's |Y| in the magnitude rows: nonzero in the straddling rows)


def _istft_bound(a_abs, b, f):
  """The bound of test_gpu_vocoder.test_istft for spectrum rows of magnitudes a_abs [b, f, 2, 513]."""
  _, inv = vc.dft_bases()
  return (1026 + 2 + 4) * U * vc.overlap_add(a_abs.reshape(b, f, 2 * BINS) @ np.abs(inv).reshape(2 * BINS, 640))


def _ratio(err, bound):
  return float((err / np.maximum(bound, 1e-300)).max())


def _rows(a, b, f, width):
  """A read-back work buffer [b (f + 1), width] -> (the songs' rows [b, f, width], the straddling rows [b, width])."""
  a = a.reshape(b, f + 1, width)
  return a[:, :f], a[:, f]


def _bits_zero(a):
  return not np.ascontiguousarray(a, np.float32).view(np.uint32).any()


# ---- the STFT pair and the encoder ------------------------------------------------------------------------------------
@shapes
@pytest.mark.parametrize('trim', vc.EDGE_TRIMS)
def test_stft_and_encode(voc, shape, trim):
  b, f = shape
  x32 = np.ascontiguousarray(_data(shape)['x'][:, :f * HOP - trim], np.float32)
  x = x32.astype(np.float64)
  silent = _silent(x)
  _dirty(voc)
  got = voc.stft(x32)
  spec = ac.stft(x)
  want = np.stack([spec.real, spec.imag], axis=2)
  bound = vc.stft_bound(x)
  assert got.shape == (b, f, 2, BINS)
  err = np.abs(got - want)
  print('edges stft %dx%d n=%d: max err / bound %.4f' % (b, f, x.shape[1], _ratio(err, bound)))
  assert (err <= bound).all()
  assert _bits_zero(np.abs(got[silent]))   # silence comes out as exact zeros

  lin, mel_bound = vc.mel_bound(x)
  mel = voc.encode(x32)
  assert mel.shape == (b, f, 128)
  for i in range(b):
    if silent[i]:
      assert (mel[i] == LOG_FLOOR).all()
    else:
      _assert_mel(mel[i], lin[i], mel_bound[i], 'edges encode %dx%d n=%d song %d' % (b, f, x.shape[1], i))


@shapes
def test_istft(voc, shape):
  b, f = shape
  spec32 = _data(shape)['spec32']
  spec = spec32[:, :, 0].astype(np.float64) + 1j * spec32[:, :, 1].astype(np.float64)
  _dirty(voc)
  got = voc.istft(spec32)
  want = ac.istft(spec, f)
  bound = _istft_bound(np.abs(spec32.astype(np.float64)), b, f)
  assert got.shape == (b, f * HOP)
  err = np.abs(got - want)
  print('edges istft %dx%d: max err / bound %.4f' % (b, f, _ratio(err, bound)))
  assert (err <= bound).all()   # every sample: the first 320 (one tap, the floored window) and the last 320 included
  assert _bits_zero(np.abs(got[_silent(_data(shape)['x'])]))


# ---- decode: target magnitudes, the load, the work buffers -------------------------------------------------------------
@shapes
def test_target_magnitudes(voc, shape):
  """exp -> pinv GEMM -> max(., 0), element by element, on a handle whose magnitude rows hold an encoder's |Y|."""
  b, f = shape
  d = _data(shape)
  _dirty(voc)
  audio = voc.decode(d['logmel'], n_iters=0, init_phase=d['phase'])
  mag, straddle = _rows(voc.debug_read('mag'), b, f, HALF)
  err = np.abs(mag[:, :, :BINS].astype(np.float64) - d['mag'])
  yard = np.abs(vc.mag_float32(d['logmel']).astype(np.float64) - d['mag'])
  print('edges magnitudes %dx%d: max err / bound %.4f (float32 NumPy %.4f)'
        % (b, f, _ratio(err, d['mag_bound']), _ratio(yard, d['mag_bound'])))
  assert (err <= d['mag_bound']).all()
  assert _bits_zero(mag[:, :, BINS:]) and _bits_zero(straddle)

  # the same call's waveform: istft of mag . phase -- the istft bound on the float64 magnitudes (widened by their own
  # bound), the magnitude bound and the rounding of the product mag . phase pushed through |inverse basis|
  ph = np.abs(d['phase'].astype(np.float64))
  hi = d['mag'] + d['mag_bound']
  want = ac.istft(d['mag'] * (d['phase'][:, :, 0].astype(np.float64) + 1j * d['phase'][:, :, 1].astype(np.float64)), f)
  dx = (d['mag_bound'] + U * hi)[:, :, None, :] * ph
  _, inv = vc.dft_bases()
  bound = _istft_bound(hi[:, :, None, :] * ph, b, f) + vc.overlap_add(dx.reshape(b, f, 2 * BINS) @ np.abs(inv).reshape(2 * BINS, 640))
  err = np.abs(audio - want)
  print('edges decode(0) %dx%d: max err / bound %.4f' % (b, f, _ratio(err, bound)))
  assert audio.shape == (b, f * HOP) and (err <= bound).all()


@shapes
def test_work_buffers_after_one_iteration(voc, shape):
  import torch
  b, f = shape
  rows = b * (f + 1)
  d = _data(shape)
  _dirty(voc)
  voc.decode(d['logmel'], n_iters=1, momentum=0.99, init_phase=d['phase'])
  buf = {name: voc.debug_read(name) for name in ('audio', 'x', 'y0', 'y1', 'mag')}
  assert [buf[k].shape for k in ('audio', 'x', 'y0', 'y1', 'mag')] == [(rows, HOP), (rows, SPEC), (rows, SPEC), (rows, SPEC), (rows, HALF)]
  # the padded signals: samples [F * 320, (F + 1) * 320) of every song are the zero extension
  assert _bits_zero(buf['audio'].reshape(b, f + 1, HOP)[:, f])
  assert np.isfinite(buf['audio']).all() and np.abs(buf['audio']).max() > 0
  # target magnitudes as after decode(n_iters=0); Y_prev of the first iteration is zero whatever the buffer held
  mag, straddle = _rows(buf['mag'], b, f, HALF)
  assert (np.abs(mag[:, :, :BINS].astype(np.float64) - d['mag']) <= d['mag_bound']).all()
  assert _bits_zero(mag[:, :, BINS:]) and _bits_zero(straddle)
  assert _bits_zero(buf['y1'])
  # X: pad columns and straddling rows zero; the last row belongs to no launch but the load's, which writes +0
  x, straddle = _rows(buf['x'], b, f, SPEC)
  assert not x[:, :, BINS:HALF].any() and not x[:, :, HALF + BINS:].any() and not straddle.any()
  assert _bits_zero(buf['x'][rows - 1])
  assert np.isfinite(buf['x']).all()
  # ... and the launch inside decode is the stand-alone op's: same rows, same alpha, bit for bit
  alpha = float(np.float32(0.99) / (np.float32(1.0) + np.float32(0.99)))
  dev = {k: torch.from_numpy(buf[k][:rows - 1].copy()).cuda() for k in ('y0', 'y1', 'mag')}
  out = torch.full((rows - 1, SPEC), float('nan'), dtype=torch.float32, device='cuda')
  native.op_vocoder_phase(dev['y0'], dev['y1'], dev['mag'], out, alpha)
  assert np.array_equal(out.cpu().numpy().view(np.uint32), buf['x'][:rows - 1].view(np.uint32))
  # ... also in the second iteration, where Y_prev is the first one's spectrum and alpha enters: the pair has swapped
  voc.decode(d['logmel'], n_iters=2, momentum=0.99, init_phase=d['phase'])
  buf2 = {name: voc.debug_read(name) for name in ('x', 'y0', 'y1')}
  assert np.array_equal(buf2['y0'].view(np.uint32), buf['y0'].view(np.uint32)) and (b * f == 1 or buf2['y1'].any())
  dev2 = {k: torch.from_numpy(buf2[k][:rows - 1].copy()).cuda() for k in ('y0', 'y1')}
  out.fill_(float('nan'))
  native.op_vocoder_phase(dev2['y1'], dev2['y0'], dev['mag'], out, alpha)
  assert np.array_equal(out.cpu().numpy().view(np.uint32), buf2['x'][:rows - 1].view(np.uint32))
  assert _bits_zero(buf2['x'][rows - 1])


def _parity(d, got, n_iters, momentum, what):
  """test_gpu_vocoder._assert_parity's criterion at another momentum."""
  ph = d['phase'].astype(np.float64)
  want = ac.griffin_lim(d['mag'], n_iters, momentum, init_phase=(ph[:, :, 0], ph[:, :, 1]))
  yard = vc.rel_l2(vc.griffin_lim_matrix(d['logmel'], n_iters, momentum, d['phase'], np.float32), want)
  dev = vc.rel_l2(got, want)
  print('edges %s, %d iterations, momentum %g: device %.3e, float32 NumPy %.3e from float64 (ratio %.2f)'
        % (what, n_iters, momentum, dev, yard, dev / yard))
  assert dev <= 16.0 * yard and dev <= 1e-4, (dev, yard)


@pytest.mark.parametrize('shape', [(3, 63), (2, 65)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('momentum', [0.0, 0.99])
def test_decode_waveform_parity(voc, shape, momentum):
  b, f = shape
  d = _data(shape)
  _dirty(voc)
  got = voc.decode(d['logmel'], n_iters=1, momentum=momentum, init_phase=d['phase'])
  assert got.shape == (b, f * HOP) and np.isfinite(got).all()
  _parity(d, got, 1, momentum, 'decode %dx%d' % shape)
  if momentum == 0.0:   # plain Griffin-Lim never reads Y_prev: two iterations on the used handle and on a fresh one
    used = voc.decode(d['logmel'], n_iters=2, momentum=0.0, init_phase=d['phase'])
    fresh = msd_amd.vocoder.GriffinLimVocoder().decode(d['logmel'], n_iters=2, momentum=0.0, init_phase=d['phase'])
    assert np.array_equal(used.view(np.uint32), fresh.view(np.uint32))
    _parity(d, used, 2, 0.0, 'decode %dx%d' % shape)   # alpha = 0 with a non-zero Y_prev, against the specification


# ---- the unit vector and the phase update on their own -----------------------------------------------------------------
CORNER_BINS = (0, 512, 257)   # the first bin, the last real one (alone in its float4 group with three pad columns), mid-row


def _spectrum_rows(pairs):
  """float32 [R, 2, 513] -> spectrum rows [R, 1088] (real parts at 0, imaginary parts at 544, zeros between)."""
  rows = np.zeros((pairs.shape[0], SPEC), np.float32)
  rows[:, :BINS], rows[:, HALF:HALF + BINS] = pairs[:, 0], pairs[:, 1]
  return rows


def _mag_rows(n):
  """float32 [n, 544]: positive seven-bit magnitudes in [1/4, 5/4), zeros in the pad columns."""
  r, k = np.arange(n)[:, None], np.arange(BINS)[None, :]
  mag = np.zeros((n, HALF), np.float32)
  mag[:, :BINS] = 0.25 + ((31 * r + 7 * k) % 64) / 64.0
  return mag


def _corner_pairs():
  """[18, 2, 513]: corner pair r at the three CORNER_BINS of row r, the zero vector everywhere else."""
  c = vc.unit_corners()
  pairs = np.zeros((len(c), 2, BINS), np.float32)
  for k in CORNER_BINS:
    pairs[:, :, k] = c
  return pairs


def _phase_op(y, prev, mag, alpha):
  """msd_op_vocoder_phase into an all-NaN output -> NumPy [R, 1088]"""
  import torch
  out = torch.full(y.shape, float('nan'), dtype=torch.float32, device='cuda')
  native.op_vocoder_phase(torch.from_numpy(y).cuda(), torch.from_numpy(prev).cuda(), torch.from_numpy(mag).cuda(), out, alpha)
  return out.cpu().numpy()


def _load_op(src, mag, normalise):
  """msd_op_vocoder_load_spec into an all-NaN output -> NumPy [B (F + 1), 1088]"""
  import torch
  b, f = src.shape[:2]
  out = torch.full((b * (f + 1), SPEC), float('nan'), dtype=torch.float32, device='cuda')
  native.op_vocoder_load_spec(torch.from_numpy(src).cuda(), None if mag is None else torch.from_numpy(mag).cuda(), out, normalise)
  return out.cpu().numpy()


def _unit_error(x, u_re, u_im, mag):
  """Largest |x - mag . direction(u)| / mag over the rows' real bins, in units of 2^-24; pad columns must be exactly 0
  and nothing unwritten.  x [R, 1088] float32, u_* [R, 513] float32, mag [R, 513]."""
  assert not np.isnan(x).any()
  assert not x[:, BINS:HALF].any() and not x[:, HALF + BINS:].any()
  c, s = vc.unit_reference(u_re, u_im)
  m = mag.astype(np.float64)
  err = np.maximum(np.abs(x[:, :BINS] - m * c), np.abs(x[:, HALF:HALF + BINS] - m * s)) / m
  return err / U


def _assert_corner_results(x, mag, what):
  """The exact results of the corner table in spectrum rows x [18, 1088] = mag . direction."""
  c = vc.unit_corners()
  is_corner = np.zeros(BINS, bool)
  is_corner[list(CORNER_BINS)] = True
  re, im = x[:, :BINS], x[:, HALF:HALF + BINS]
  assert np.array_equal(re[:, ~is_corner], mag[:, ~is_corner]) and not im[:, ~is_corner].any(), what   # zero vector -> (mag, 0)
  for r, (want_c, want_s) in ((0, (1, 0)), (1, (1, 0)), (2, (1, 0)), (6, (0, -1)), (7, (-1, 0))):
    for k in CORNER_BINS:
      assert (re[r, k], im[r, k]) == (want_c * mag[r, k], want_s * mag[r, k]), (what, c[r], k, re[r, k], im[r, k])


def test_unit_vector_corners_through_the_phase_update():
  pairs = _corner_pairs()
  mag = _mag_rows(len(pairs))
  x = _phase_op(_spectrum_rows(pairs), np.zeros((len(pairs), SPEC), np.float32), mag, 0.5)
  err = _unit_error(x, pairs[:, 0], pairs[:, 1], mag[:, :BINS])
  print('edges unit vector, corner table through the phase update: max %.2f x 2^-24 of mag' % err.max())
  for r in np.argsort(err.max(axis=1))[-3:]:
    print('  pair', vc.unit_corners()[r], '%.2f' % err[r].max())
  assert (err <= 7.0).all()
  _assert_corner_results(x, mag[:, :BINS], 'phase update')


def test_unit_vector_corners_through_the_load():
  pairs = _corner_pairs()
  x = _load_op(pairs[None], None, True)   # one song of 18 frames, no magnitudes: the directions themselves
  assert not x[len(pairs)].any()          # (its row k = F)
  ones = np.ones((len(pairs), BINS), np.float32)
  err = _unit_error(x[:len(pairs)], pairs[:, 0], pairs[:, 1], ones)
  print('edges unit vector, corner table through the load: max %.2f x 2^-24' % err.max())
  assert (err <= 6.0).all()
  _assert_corner_results(x[:len(pairs)], ones, 'load')


def test_unit_vector_random_pairs():
  """64 rows of pairs over every exponent, through both kernels; the first is the measured maximum on record."""
  pairs = np.ascontiguousarray(np.moveaxis(vc.unit_random(np.random.default_rng(20260101), (64, BINS)), -1, 1))
  mag = _mag_rows(64)
  x = _phase_op(_spectrum_rows(pairs), np.zeros((64, SPEC), np.float32), mag, 0.5)
  err = _unit_error(x, pairs[:, 0], pairs[:, 1], mag[:, :BINS])
  ones = np.ones((64, BINS), np.float32)
  direct = _unit_error(_load_op(pairs[None], None, True)[:64], pairs[:, 0], pairs[:, 1], ones)
  print('edges unit vector, 64 x 513 random pairs: max %.2f x 2^-24 (direction alone), %.2f x 2^-24 of mag (phase update)'
        % (direct.max(), err.max()))
  assert (direct <= 6.0).all() and (err <= 7.0).all()


def test_unit_vector_on_an_axis_is_exact():
  """A pair with one component zero has the direction (+-1, 0) or (0, +-1) exactly, at every magnitude: the reciprocal
  square root alone gave -3 -> -(1 - 2^-24).  The DC and Nyquist bins of every frame are such pairs."""
  pairs = np.ascontiguousarray(np.moveaxis(vc.unit_random(np.random.default_rng(20260105), (64, BINS)), -1, 1))
  keep = np.argmax(np.abs(pairs), axis=1)   # the larger component stays, the other becomes a zero of either sign
  zero = np.where((np.arange(64)[:, None] + np.arange(BINS)[None, :]) % 2 == 0, np.float32(0.0), np.float32(-0.0))
  pairs[:, 0], pairs[:, 1] = np.where(keep == 0, pairs[:, 0], zero), np.where(keep == 1, pairs[:, 1], zero)
  want = np.sign(pairs)
  mag = _mag_rows(64)
  x = _phase_op(_spectrum_rows(pairs), np.zeros((64, SPEC), np.float32), mag, 0.5)
  assert np.array_equal(x[:, :BINS], mag[:, :BINS] * want[:, 0]) and np.array_equal(x[:, HALF:HALF + BINS], mag[:, :BINS] * want[:, 1])
  x = _load_op(pairs[None], None, True)[:64]
  assert np.array_equal(x[:, :BINS], want[:, 0]) and np.array_equal(x[:, HALF:HALF + BINS], want[:, 1])


def test_phase_update_subtraction_exact_operands():
  """alpha = 1/2 and operands of at most 12 significand bits with exponents within 2^10 of each other: U = Y - alpha Y_prev
  is exact, contracted into one FMA or not; rows 0 .. 7 have Y = alpha Y_prev exactly (U = 0, mag > 0 -> (mag, 0))."""
  rng = np.random.default_rng(20260102)

  def twelve_bits(shape):
    return (rng.integers(-2048, 2049, size=shape) * 2.0 ** rng.integers(-5, 6, size=shape)).astype(np.float32)

  y, prev = twelve_bits((32, 2, BINS)), twelve_bits((32, 2, BINS))
  prev[:8] = 2.0 * y[:8]
  mag = _mag_rows(32)
  u = y.astype(np.float64) - 0.5 * prev.astype(np.float64)
  assert np.array_equal(u, u.astype(np.float32)) and not u[:8].any() and np.abs(u[8:]).max() > 0
  x = _phase_op(_spectrum_rows(y), _spectrum_rows(prev), mag, 0.5)
  err = _unit_error(x, u[:, 0].astype(np.float32), u[:, 1].astype(np.float32), mag[:, :BINS])
  print('edges phase update, exact U: max %.2f x 2^-24 of mag' % err.max())
  assert (err <= 7.0).all()
  assert np.array_equal(x[:8, :BINS], mag[:8, :BINS]) and not x[:8, HALF:].any()


def test_phase_update_subtraction_either_rounding():
  """alpha = 0.99 / 1.99 in float32: U is the separately rounded multiply and subtract, or one FMA -- both computed here
  (exactly: 24-bit operands within 2^2 of each other keep alpha Y_prev and the difference inside float64), a quarter of the
  components with Y = fl(alpha Y_prev), where the two differ in everything but the bound."""
  rng = np.random.default_rng(20260103)
  alpha = np.float32(0.99) / (np.float32(1.0) + np.float32(0.99))

  def draws(shape):
    return (np.ldexp(1.0 + rng.random(shape), rng.integers(-1, 2, size=shape)) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)

  y, prev = draws((64, 2, BINS)), draws((64, 2, BINS))
  y = np.where(rng.random(y.shape) < 0.25, alpha * prev, y).astype(np.float32)
  mag = _mag_rows(64)
  exact = y.astype(np.float64) - np.float64(alpha) * prev.astype(np.float64)
  u_fma = exact.astype(np.float32)
  u_sep = y - alpha * prev
  assert u_sep.dtype == np.float32 and (u_fma != u_sep).mean() > 0.2
  x = _phase_op(_spectrum_rows(y), _spectrum_rows(prev), mag, float(alpha))
  ok = np.zeros((64, BINS), bool)
  best = np.full((64, BINS), np.inf)
  for re, im in itertools.product((u_sep, u_fma), repeat=2):
    err = _unit_error(x, re[:, 0], im[:, 1], mag[:, :BINS])
    ok |= err <= 7.0
    best = np.minimum(best, err)
  print('edges phase update, alpha = 0.99 / 1.99: max %.2f x 2^-24 of mag from the nearer rounding of U' % best.max())
  assert ok.all()


@pytest.mark.parametrize('shape', [(3, 63), (1, 1)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('normalise', [False, True])
@pytest.mark.parametrize('with_mag', [False, True])
def test_load_spec_layout(shape, normalise, with_mag):
  """Every sounding element is the product the kernel's comment promises; straddling rows and pad columns are exactly 0
  (whatever the magnitude rows hold there: NaN here); the imaginary half starts at column 544."""
  b, f = shape
  rng = np.random.default_rng(20260104)
  src = rng.standard_normal((b, f, 2, BINS)).astype(np.float32)
  mag = None
  if with_mag:
    mag = np.full((b, f + 1, HALF), np.nan, np.float32)
    mag[:, :f, :BINS] = 0.25 + rng.random((b, f, BINS))
    mag = mag.reshape(b * (f + 1), HALF)
  x, straddle = _rows(_load_op(src, mag, normalise), b, f, SPEC)
  assert _bits_zero(straddle) and _bits_zero(x[:, :, BINS:HALF]) and _bits_zero(x[:, :, HALF + BINS:])
  m = mag.reshape(b, f + 1, HALF)[:, :f, :BINS] if with_mag else np.ones((b, f, BINS), np.float32)
  got = np.stack([x[:, :, :BINS], x[:, :, HALF:HALF + BINS]], axis=2)
  if not normalise:
    assert np.array_equal(got.view(np.uint32), (m[:, :, None, :] * src).view(np.uint32))   # one float32 product
  else:
    c, s = vc.unit_reference(src[:, :, 0], src[:, :, 1])
    err = np.abs(got - m[:, :, None, :].astype(np.float64) * np.stack([c, s], axis=2)) / m[:, :, None, :] / U
    assert (err <= (7.0 if with_mag else 6.0)).all(), err.max()


# ---- one handle, every entry point, shapes going down and up -----------------------------------------------------------
def test_handle_reuse_across_entry_points():
  """decode at (2, 65), then stft, istft, encode and decode at (3, 63) and at (1, 1), then grown to (1, 129): every result
  is, bit for bit, a fresh handle's."""
  used = msd_amd.vocoder.GriffinLimVocoder()

  def calls(shape):
    d = _data(shape)
    x32 = np.ascontiguousarray(d['x'][:, :shape[1] * HOP - 1], np.float32)
    return (('stft', lambda v: v.stft(x32)), ('istft', lambda v: v.istft(d['spec32'])), ('encode', lambda v: v.encode(x32)),
            ('decode', lambda v: v.decode(d['logmel'], n_iters=2, momentum=0.99, init_phase=d['phase'])),
            ('decode(seed)', lambda v: v.decode(d['logmel'], n_iters=1, seed=9)))

  first = _data((2, 65))
  used.decode(first['logmel'], n_iters=2, seed=4)
  for shape in ((3, 63), (1, 1), (1, 129)):
    for name, call in calls(shape):
      fresh = msd_amd.vocoder.GriffinLimVocoder()   # has served nothing else at all
      got, want = call(used), call(fresh)
      fresh.close()
      assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (shape, name)


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(voc):
  import torch
  d = _data((1, 1))
  before = voc.decode(d['logmel'], n_iters=1, init_phase=d['phase'])
  lib, h = voc.lib, voc.handle
  small = torch.zeros(4096, dtype=torch.float32, device='cuda')
  p = small.data_ptr()
  bad = native.MSD_ERR_INVALID_ARGUMENT
  rows = ctypes.c_int64(-1)
  host = np.zeros(8, np.float32)
  # 2^20 + 1 rows: refused by the shape check, in front of the allocation (the handle's row count does not move)
  assert lib.msd_vocoder_decode(h, 1, 2 ** 20, p, 1, 0.99, 0, None, p, None) == bad
  assert b'msd_vocoder_decode' in lib.msd_vocoder_last_error(h)
  assert lib.msd_vocoder_istft(h, 1, 2 ** 20, p, p, None) == bad
  assert lib.msd_vocoder_stft(h, 1, 2 ** 20 * HOP, p, p, None) == bad
  assert lib.msd_vocoder_encode(h, 1, 2 ** 20 * HOP, p, p, None) == bad
  assert lib.msd_vocoder_debug_read(h, b'mag', host.ctypes.data, 8, ctypes.byref(rows)) == 0 and rows.value == 2
  for momentum in (-0.5, float('nan'), float('inf')):
    with pytest.raises(ValueError):
      voc.decode(d['logmel'], n_iters=1, momentum=momentum, init_phase=d['phase'])
  # the three new entry points' own
  assert lib.msd_op_vocoder_phase(None, p, p, p, 1, 0.5, None) == bad
  assert lib.msd_op_vocoder_phase(p, None, p, p, 1, 0.5, None) == bad
  assert lib.msd_op_vocoder_phase(p, p, None, p, 1, 0.5, None) == bad
  assert lib.msd_op_vocoder_phase(p, p, p, None, 1, 0.5, None) == bad
  assert lib.msd_op_vocoder_phase(p, p, p, p, 0, 0.5, None) == bad
  assert lib.msd_op_vocoder_phase(p, p, p, p, 2 ** 20 + 1, 0.5, None) == bad
  assert lib.msd_op_vocoder_load_spec(None, None, p, 1, 1, 0, None) == bad
  assert lib.msd_op_vocoder_load_spec(p, None, None, 1, 1, 0, None) == bad
  assert lib.msd_op_vocoder_load_spec(p, None, p, 0, 1, 0, None) == bad
  assert lib.msd_op_vocoder_load_spec(p, None, p, 1, 0, 0, None) == bad
  assert lib.msd_op_vocoder_load_spec(p, None, p, 1, 2 ** 20, 0, None) == bad
  assert lib.msd_vocoder_debug_read(None, b'mag', host.ctypes.data, 8, None) == bad
  assert lib.msd_vocoder_debug_read(h, None, host.ctypes.data, 8, None) == bad
  assert lib.msd_vocoder_debug_read(h, b'mag', None, 8, None) == bad
  assert lib.msd_vocoder_debug_read(h, b'mag', host.ctypes.data, 0, None) == bad
  assert lib.msd_vocoder_debug_read(h, b'lin', host.ctypes.data, 8, None) == bad
  with pytest.raises(ValueError):
    voc.debug_read('draws')
  new = msd_amd.vocoder.GriffinLimVocoder()
  with pytest.raises(RuntimeError):   # MSD_ERR_BAD_STATE: nothing has run on it
    new.debug_read('x')
  # ... and the handle goes on as before
  assert np.array_equal(before, voc.decode(d['logmel'], n_iters=1, init_phase=d['phase']))
