"""Shared inputs, float64 references and rounding bounds of the vocoder tests (tests/test_vocoder_host.py,
tests/test_gpu_vocoder.py, tests/test_gpu_vocoder_edges.py) and of tools/vocoder_report.py (tools/ may not import tests/, so the module lives here).  Everything here is closed form: no RNG of its own (unit_random takes the caller's seeded generator), no file."""
import functools

import numpy as np

from msd_amd import audio_codecs as ac

HOP, FRAME, FFT, BINS, MELS = 320, 640, 1024, 513, 128
U = 2.0 ** -24   # unit roundoff of float32


def signal(n_frames: int) -> np.ndarray:
  """Twelve decaying five-harmonic notes a minor third apart, overlapping; float64 [n_frames * 320], peak 0.5."""
  n = n_frames * HOP
  t = np.arange(n) / 16000.0
  dur = n / 16000.0
  x = np.zeros(n)
  for j in range(12):
    f0 = 110.0 * 2.0 ** (3.0 * j / 12.0)
    st, ln = dur * j / 15.0, 0.25 * dur
    env = ((t >= st) & (t < st + ln)) * np.exp(-3.0 * (t - st) / ln)
    for h in range(1, 6):
      x += env * np.sin(2.0 * np.pi * f0 * h * t) / h
  return 0.5 * x / np.abs(x).max()


def two_songs(n_frames: int) -> np.ndarray:
  """[2, n]: the signal and its time reversal (a leak from one song into the other shows)."""
  x = signal(n_frames)
  return np.stack([x, x[::-1]])


@functools.lru_cache(maxsize=None)
def mel_basis() -> np.ndarray:
  return ac.linear_to_mel_weight_matrix(MELS, BINS, 16000, 0.0, 8000.0).astype(np.float64)


@functools.lru_cache(maxsize=None)
def dft_bases():
  """float64 (forward [640, 2, 513], inverse [2, 513, 640]): frame . forward = (re, im) of rfft(frame * hann, 1024);
  (re, im) . inverse = irfft(., 1024)[:640] * hann."""
  w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FRAME) / FRAME)
  cos_t, sin_t = np.cos(2.0 * np.pi * np.arange(FFT) / FFT), np.sin(2.0 * np.pi * np.arange(FFT) / FFT)
  sin_t[[0, FFT // 2]] = 0.0           # exact zeros of the table (sin(pi) rounds to 1.2e-16): the imaginary parts of
  cos_t[[FFT // 4, 3 * FFT // 4]] = 0.0   # the DC and Nyquist bins are exactly zero, as an FFT returns them
  j = (np.arange(FRAME)[:, None] * np.arange(BINS)[None, :]) % FFT
  fwd = np.stack([w[:, None] * cos_t[j], -w[:, None] * sin_t[j]], axis=1)
  ck = np.full(BINS, 2.0)
  ck[0] = ck[-1] = 1.0
  inv = np.stack([(ck[None, :] / FFT * cos_t[j] * w[:, None]).T, (-ck[None, :] / FFT * sin_t[j] * w[:, None]).T])
  return fwd, inv


def frames_of(x: np.ndarray) -> np.ndarray:
  """[B, n] -> [B, F, 640] frames of the zero-extended signal."""
  b, n = x.shape
  f = -(-n // HOP)
  padded = np.zeros((b, (f - 1) * HOP + FRAME), x.dtype)
  padded[:, :n] = x
  return padded[:, np.arange(FRAME)[None, :] + HOP * np.arange(f)[:, None]]


def ola_norm(n_frames: int, floor: float = 1e-3) -> np.ndarray:
  w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FRAME) / FRAME)
  norm = np.zeros((n_frames - 1) * HOP + FRAME)
  for k in range(n_frames):
    norm[k * HOP:k * HOP + FRAME] += w * w
  return np.maximum(norm, floor)


def overlap_add(frames: np.ndarray) -> np.ndarray:
  """[B, F, 640] -> [B, F * 320], divided by the window normalisation."""
  b, f = frames.shape[:2]
  out = np.zeros((b, (f - 1) * HOP + FRAME), frames.dtype)
  for k in range(f):
    out[:, k * HOP:k * HOP + FRAME] += frames[:, k]
  return (out / ola_norm(f).astype(frames.dtype))[:, :f * HOP]


def pack_spec(spec: np.ndarray) -> np.ndarray:
  """complex [B, F, 513] -> the ABI's float32 [B, F, 2, 513]."""
  return np.ascontiguousarray(np.stack([spec.real, spec.imag], axis=2), np.float32)


def dot_bound(a_abs: np.ndarray, b_abs: np.ndarray, k: int) -> np.ndarray:
  """Forward error bound of a float32 dot product of length k whose second operand was rounded to float32 first:
  |fl(a . b) - a . b| <= (k + 2) u (|a| . |b|)  (Higham, Accuracy and Stability, 3.5: gamma_k <= (k + 1) u here,
  plus u for the rounding of b)."""
  return (k + 2) * U * (a_abs @ b_abs)


def stft_bound(x: np.ndarray) -> np.ndarray:
  """Elementwise bound [B, F, 2, 513] for the device STFT of float32-exact samples x (K = 640)."""
  fwd, _ = dft_bases()
  return dot_bound(np.abs(frames_of(x)), np.abs(fwd).reshape(FRAME, 2 * BINS), FRAME).reshape(x.shape[0], -1, 2, BINS)


def mel_bound(x: np.ndarray):
  """(float64 linear mel [B, F, 128] clipped to [1e-5, 1e8], its bound): the STFT bound pushed through |.| -- the
  magnitude moves by at most the length of the error vector, <= e_re + e_im, and sqrt / squares add 3 u relative --
  and through the mel product (K = 513), plus 8 u relative for the logarithm (half an ulp at |log| < 16 is 2^-21)."""
  spec = ac.stft(x)
  e = stft_bound(x)
  mag = np.abs(spec)
  mag_err = e[:, :, 0] + e[:, :, 1] + 3 * U * mag
  lin = mag @ mel_basis()
  bound = mag_err @ mel_basis() + dot_bound(mag + mag_err, mel_basis(), BINS)
  lin = np.clip(lin, 1e-5, 1e8)
  return lin, bound + 8 * U * lin


# ---- Griffin-Lim with explicit bases in one dtype: the float32 yardstick of the device's float32 run ----------------
def griffin_lim_matrix(logmel: np.ndarray, n_iters: int, momentum: float, phase: np.ndarray, dtype) -> np.ndarray:
  """audio_codecs.griffin_lim(mel_to_linear(logmel)) restated with matrix products, every array and basis in `dtype`.
  phase [B, F, 2, 513]."""
  fwd, inv = dft_bases()
  fwd = fwd.reshape(FRAME, 2 * BINS).astype(dtype)
  inv = inv.reshape(2 * BINS, FRAME).astype(dtype)
  pinv = ac.mel_pseudo_inverse(mel_basis()).astype(dtype)
  mag = np.maximum(np.exp(logmel.astype(dtype)) @ pinv, dtype(0))
  b, f = mag.shape[:2]
  alpha = dtype(momentum / (1.0 + momentum))

  def inverse(xs):
    return overlap_add((xs.reshape(b, f, 2 * BINS) @ inv).astype(dtype))

  xs = (mag[:, :, None, :] * phase.astype(dtype)).astype(dtype)
  prev = np.zeros_like(xs)
  for _ in range(n_iters):
    y = (frames_of(inverse(xs)) @ fwd).reshape(b, f, 2, BINS).astype(dtype)
    u = y - alpha * prev
    prev = y
    a = np.sqrt(u[:, :, 0] ** 2 + u[:, :, 1] ** 2)
    safe = np.where(a > 0, a, dtype(1))
    c = np.where(a > 0, u[:, :, 0] / safe, dtype(1))
    s = np.where(a > 0, u[:, :, 1] / safe, dtype(0))
    xs = (mag[:, :, None, :] * np.stack([c, s], axis=2)).astype(dtype)
  return inverse(xs)


def closed_form_phase(b: int, f: int) -> np.ndarray:
  """A fixed, rough phase field [b, f, 2, 513] (cos, sin): angles from a quadratic in (song, frame, bin)."""
  i = np.arange(b)[:, None, None]
  j = np.arange(f)[None, :, None]
  k = np.arange(BINS)[None, None, :]
  ang = 2.0 * np.pi * np.mod(0.61803398875 * (k * k + 7 * j * k + 3 * j * j) + 0.37 * i + 0.5 * j, 1.0)
  return np.stack([np.cos(ang), np.sin(ang)], axis=2)


def rel_l2(a, b) -> float:
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- the edge cases of tests/test_gpu_vocoder_edges.py (and their host checks in tests/test_vocoder_host.py) ----------
# (songs, frames): 63 + 1 = 64 puts every song boundary and every straddling row on a GEMM tile edge, with an odd number
# of songs; 65 is one past a tile; (1, 129) has no straddling row and more than two tiles; (1, 1) is a one-row launch.
EDGE_SHAPES = ((1, 1), (3, 63), (2, 65), (1, 129))
EDGE_TRIMS = (0, 1, 319)   # n = F * 320 - r samples: the exact multiple, one short, one sample in the last frame


def songs(b: int, n_frames: int) -> np.ndarray:
  """float32-exact float64 [b, n_frames * 320], b <= 3: song 0 is the signal with DC and Nyquist content (0.01 + 0.01
  (-1)^i), song 1 is SILENT (all zeros, between sounding ones when b = 3), song 2 is song 0 reversed in time."""
  x = signal(n_frames) + 0.01 + 0.01 * (-1.0) ** np.arange(n_frames * HOP)
  return np.stack([x, np.zeros_like(x), x[::-1]][:b]).astype(np.float32).astype(np.float64)


def logmel_of(x: np.ndarray) -> np.ndarray:
  """float32 log-mel [B, F, 128] of float64 signals (the float64 codec); a silent song is log(1e-5) in every bin."""
  return np.log(np.clip(np.abs(ac.stft(x)) @ mel_basis(), 1e-5, 1e8)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pinv32() -> np.ndarray:
  """pinv(mel basis) [128, 513] as the vocoder uploads it: taken in float64, stored as float32."""
  return ac.mel_pseudo_inverse(mel_basis()).astype(np.float32)


def mag_bound(logmel32: np.ndarray) -> np.ndarray:
  """Elementwise bound [B, F, 513] of the device's target magnitudes against mel_to_linear(logmel32 as float64): the
  K = 128 dot-product bound (dot_bound: the pseudo-inverse was rounded to float32 first) plus 4 u for expf; max(., 0)
  moves nothing further apart."""
  return (MELS + 2 + 4) * U * (np.exp(logmel32.astype(np.float64)) @ np.abs(pinv32().astype(np.float64)))


def mag_float32(logmel32: np.ndarray) -> np.ndarray:
  """The float32 NumPy restatement of the target magnitudes."""
  return np.maximum(np.exp(logmel32.astype(np.float32)) @ pinv32(), np.float32(0))


# -- the unit vector behind the phase update and the drawn initial phases (csrc/vocoder.h voc_unit) --
# Per component, absolute.  The power-of-two scaling is exact; a^2 + b^2 carries at most two roundings (2 u relative on
# the squared length, so u on its inverse root); the reciprocal square root instruction is within one ulp (2 u relative);
# the product adds half an ulp (u): 4 u on a component of size <= 1, and 6 leaves room for the second-order terms.  The
# emulation below with its reciprocal square root moved +-1 ulp reaches 4.3 u over 10^6 pairs of every exponent.
UNIT_BOUND = 6 * U
FLT_MAX = float(np.finfo(np.float32).max)


def unit_corners() -> np.ndarray:
  """float32 [18, 2]: the pairs (a, b) voc_unit documents and no audio-sized run reaches."""
  d = 2.0 ** -149
  return np.array([
      (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0),                          # the zero vector -> exactly (1, 0)
      (d, 0.0), (-d, d), (1e-40, -2e-40),                             # denormals are not the zero vector
      (0.0, -5.0), (-3.0, 0.0),                                       # on an axis -> exactly (0, -1), (-1, 0)
      (3.0, 4.0), (-5.0, 12.0), (-8.0, -15.0), (7.0, -24.0),         # one pair per quadrant
      (1e30, 1e-30),
      (2.0 ** 125, 2.0 ** 125), (2.0 ** 126, -2.0 ** 126), (2.0 ** 127, 2.0 ** 127), (FLT_MAX, -FLT_MAX), (3e38, 1.0),
  ], np.float32)   # ... exponent fields 252, 253, 254: where the max(253 - e, 1) clamp acts


def unit_random(rng: np.random.Generator, shape) -> np.ndarray:
  """float32 shape + (2,): pairs whose larger component has an exponent anywhere in -149 .. 127 and whose smaller one is
  up to 2^30 below it, either component first, every sign."""
  hi = rng.integers(-149, 128, size=shape)
  lo = np.maximum(hi - rng.integers(0, 31, size=shape), -149)
  m_hi = np.ldexp(1.0 + rng.random(shape), hi) * rng.choice([-1.0, 1.0], size=shape)
  m_lo = np.ldexp(1.0 + rng.random(shape), lo) * rng.choice([-1.0, 1.0], size=shape)
  swap = rng.random(shape) < 0.5
  pair = np.stack([np.where(swap, m_lo, m_hi), np.where(swap, m_hi, m_lo)], axis=-1)
  return np.clip(pair, -FLT_MAX, FLT_MAX).astype(np.float32)


def unit_reference(a, b):
  """(cos, sin) of the direction of float32 (a, b) in float64; (1, 0) for the zero vector."""
  a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
  h = np.hypot(a, b)
  safe = np.where(h > 0, h, 1.0)
  return np.where(h > 0, a / safe, 1.0), np.where(h > 0, b / safe, 0.0)


def unit_emulated(a, b, rsq_ulps: int = 0):
  """voc_unit step by step in float32 NumPy: the power-of-two scale from the exponent field of max(|a|, |b|), the two
  squares summed, the reciprocal square root rounded to float32 and moved by `rsq_ulps` ulps (the instruction is within
  one), one product per component -- or, on an axis, the exact +-1."""
  a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
  m = np.maximum(np.abs(a), np.abs(b))
  e = ((m.view(np.uint32) >> 23) & 0xFF).astype(np.int64)
  sc = (np.maximum(253 - e, 1).astype(np.uint32) << np.uint32(23)).view(np.float32)
  a, b = a * sc, b * sc
  n2 = a * a + b * b
  with np.errstate(divide='ignore'):
    r = (1.0 / np.sqrt(n2.astype(np.float64))).astype(np.float32)
  for _ in range(abs(rsq_ulps)):
    r = np.nextafter(r, np.float32(np.inf if rsq_ulps > 0 else 0))
  pos = n2 > 0
  with np.errstate(invalid='ignore'):
    c = np.where(b == 0, np.copysign(np.float32(1), a), a * r)   # on an axis: the exact direction, not 1 -+ an ulp
    s = np.where(a == 0, np.copysign(np.float32(1), b), b * r)
  return np.where(pos, c, np.float32(1)), np.where(pos, s, np.float32(0))
