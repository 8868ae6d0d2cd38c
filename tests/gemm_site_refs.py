"""Float64 restatements of what each GEMM launch site of the decoder computes (include/msd_amd.h, msd_op_gemm_site).

Plain NumPy, from the formulas of the epilogues' documentation; nothing here touches the package's native layer.
tests/test_gemm_site_refs.py checks each of them on the CPU against an independent evaluation (oracle/ops.py and
element-by-element loops); tests/test_gpu_gemm_sites.py compares the device against them.

Conventions: float32 inputs are widened by `f64`; `ssq` are partial sums of squares per 32 columns, [rows][K / 32]; a
step-indexed table (bias, gains) is [steps][n] and read at row `step`; a row the epilogue does not write is NaN.
"""
import numpy as np

from oracle import backend, ops

_XP = backend.NumpyBackend('float64')


def f64(a):
  return None if a is None else np.asarray(a, np.float64)


def rstd_of(ssq, k):
  """1 / sqrt(mean of squares + 1e-6) of rows whose partial sums of squares are ssq [rows][tiles], k columns."""
  return 1.0 / np.sqrt(f64(ssq).sum(axis=1) / k + 1e-6)


def partial_ssq(x, group=32):
  x = f64(x)
  return (x.reshape(x.shape[0], x.shape[1] // group, group) ** 2).sum(axis=2)


def linear(a, w, ssq=None, bias=None, step=0):
  """[rstd .] (a . w) [+ bias[step]]: the store sites and QKV (q | k | v are its columns)."""
  h = f64(a) @ f64(w)
  if ssq is not None:
    h = h * rstd_of(ssq, a.shape[1])[:, None]
    if bias is not None:
      h = h + f64(bias)[step][None, :]
  return h


def mlp_in(a, wi0, wi1, ssq=None, bias=None, step=0):
  """gelu_tanh(h0) . h1, h = [rstd .] (a . (wi_0 | wi_1)) [+ (b0 | b1)[step]]."""
  f = wi0.shape[1]
  h = linear(a, np.concatenate([f64(wi0), f64(wi1)], axis=1), ssq, bias, step)
  return ops.gelu_tanh(_XP, h[:, :f]) * h[:, f:]


def residual(x, a, w):
  return f64(x) + f64(a) @ f64(w)


def residual_norm(x, a, w, g_lo, g_hi, split_row, step=0, dup_rows=None, g2=None, y2_rows=0):
  """x += a . w; the rows' sums of squares; y = x (.) g (g_lo[step] below split_row, g_hi[step] from there; rows of a
  missing gain stay NaN).  dup_rows: x has dup_rows + m rows, rows [0, m) are updated and copied to [dup_rows,
  dup_rows + m), y = x (.) g_lo for the first copy and x (.) g_hi for the second.  g2: y2 = x (.) g2 for rows < y2_rows.
  Returns x, ssq (full row sums), y, y2."""
  x = f64(x).copy()
  m = a.shape[0]
  x[:m] += f64(a) @ f64(w)
  y = np.full_like(x, np.nan)
  if dup_rows is not None:
    x[dup_rows:dup_rows + m] = x[:m]
    y[:m] = x[:m] * f64(g_lo)[step]
    y[dup_rows:dup_rows + m] = x[:m] * f64(g_hi)[step]
  else:
    if g_lo is not None:
      y[:split_row] = x[:split_row] * f64(g_lo)[step]
    if g_hi is not None:
      y[split_row:] = x[split_row:] * f64(g_hi)[step]
  y2 = None
  if g2 is not None:
    y2 = np.full((m, x.shape[1]), np.nan)
    y2[:y2_rows] = x[:y2_rows] * f64(g2)
  return x, (x ** 2).sum(axis=1), y, y2


def in_proj(z, w, pos, g, step=0, passes=1, g2=None):
  """x[p][m] = z[m] . w + pos[m % T]; y = x (.) g[step]; the rows' sums of squares; y2 = x (.) g2 of the first pass."""
  m = z.shape[0]
  x1 = f64(z) @ f64(w) + f64(pos)[np.arange(m) % pos.shape[0]]
  x = np.concatenate([x1] * passes, axis=0)
  y2 = None if g2 is None else x1 * f64(g2)
  return x, (x ** 2).sum(axis=1), x * f64(g)[step], y2


def add_store(a, w, addend):
  return f64(a) @ f64(w) + f64(addend)


# ---- one-plane emulation: the operands as the library rounds them (csrc/common.h, elementwise.h pack_wt_kernel) ----
def round_plane(x, fmt):
  """float32 -> one 16-bit plane (round to nearest even) -> float32.  fmt: 'f16' (IEEE half) or 'bf16'."""
  x = np.ascontiguousarray(x, np.float32)
  if fmt == 'f16':
    return x.astype(np.float16).astype(np.float32)
  u = x.view(np.uint32).astype(np.uint64)
  r = ((u >> 16) & 1) + 0x7FFF
  return ((u + r) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def round_weight(w, fmt):
  """The half-plane build packs w times 2^9 and scales the accumulators back (exact); the bfloat16 build packs w."""
  w = np.ascontiguousarray(w, np.float32)
  if fmt == 'f16':
    return round_plane(w * np.float32(512.0), fmt) / np.float32(512.0)
  return round_plane(w, fmt)
