"""ctypes binding of the C ABI in include/msd_amd.h (libmsd_amd.so).

This is the ONLY compute path of the package: there is no CPU or PyTorch
fallback.  ``load()`` raises ``NativeLibraryError`` when the HIP library has not
been built (run ``python music-spectrogram-diffusion_amd/build_native.py`` or
``__graft_entry__.build()``), and every wrapper converts a non-zero msd_status
into the Python exception the reference raises for the same condition
(ValueError for unknown sampler/schedule/..., see msd_amd.h).

PyTorch is plumbing here: device memory (``tensor.data_ptr()``), streams and
``torch.distributed``; no torch op is on the hot path.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libmsd_amd.so')
LIB_PATHS = {'f16': LIB_PATH, 'bf16': os.path.join(_HERE, 'csrc', 'libmsd_amd_bf16.so')}

MSD_PREC_F16 = 0      # one IEEE-half plane per operand
MSD_PREC_F16X3 = 1    # hi + lo half planes, three MFMAs per product (the parity mode, the default)
MSD_PREC_BF16 = 2     # one bfloat16 plane                       } libmsd_amd_bf16.so; msd_create of the other
MSD_PREC_BF16X3 = 3   # hi + lo bfloat16 planes                  } build answers MSD_ERR_UNSUPPORTED
ABI_VERSION = 7        # MSD_AMD_ABI_VERSION of include/msd_amd.h (tests/test_abi.py)
MSD_SAMPLER_DDPM = 0
MSD_SAMPLER_DDIM = 1
MSD_SAMPLER_DPMPP_2M = 2   # (appended to ABI 7) DPM-Solver++(2M): deterministic, second order (msd_sample_steps)
SAMPLERS = {'ddpm': MSD_SAMPLER_DDPM, 'ddim': MSD_SAMPLER_DDIM, 'dpmpp_2m': MSD_SAMPLER_DPMPP_2M}
MSD_RNG_PHILOX = 0    # the library's own generator (msd_fill_normal)
MSD_RNG_THREEFRY = 1  # the reference's: jax.random's Threefry draws for PRNGKey(seed), made on the device (ABI 7)
RNGS = {'philox': MSD_RNG_PHILOX, 'threefry': MSD_RNG_THREEFRY}
MAX_KERNEL_CLASSES = 16

# precision name -> (msd_precision value, plane format).  The plane format is a property of the LIBRARY build
# (csrc/common.h): libmsd_amd.so holds operand planes in IEEE half -- 'f16x3' (hi + lo planes, 22 significand bits,
# three MFMAs per product: the parity mode and the default) and 'f16' (one plane) --, libmsd_amd_bf16.so in
# bfloat16 -- 'bf16x3' / 'bf16': 16 / 8 significand bits but float32's exponent range, for weights or activations
# beyond the half range (|w| >= 128, |x| >= 131008).
PRECISIONS = {'f16': MSD_PREC_F16, 'f16x3': MSD_PREC_F16X3, 'bf16': MSD_PREC_BF16, 'bf16x3': MSD_PREC_BF16X3}
_PLANES_OF = {MSD_PREC_F16: 'f16', MSD_PREC_F16X3: 'f16', MSD_PREC_BF16: 'bf16', MSD_PREC_BF16X3: 'bf16'}


def plane_format(precision: str) -> str:
  if precision not in PRECISIONS:
    raise ValueError('precision must be one of %s' % sorted(PRECISIONS))
  return 'bf16' if precision.startswith('bf16') else 'f16'


# every symbol include/msd_amd.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = (
    'msd_version', 'msd_device_count', 'msd_create', 'msd_destroy', 'msd_last_error',
    'msd_num_weights', 'msd_weight_info', 'msd_set_weight', 'msd_finalize_weights',
    'msd_encode', 'msd_sample', 'msd_reset_graph', 'msd_decoder_pass', 'msd_fill_normal', 'msd_get_schedule',
    'msd_debug_read', 'msd_profile_steps', 'msd_op_gemm_h16', 'msd_op_gemm_bf16', 'msd_op_gemm_f32',
    'msd_op_attention', 'msd_op_attention_qp', 'msd_op_attention_split', 'msd_op_attention_ex', 'msd_op_sampler_step', 'msd_op_residual_norm_gemm', 'msd_op_geglu',
    'msd_op_qkv', 'msd_op_final_proj', 'msd_sample_rng', 'msd_fill_normal_threefry', 'msd_op_threefry',
    # (appended to ABI 7) the device vocoder
    'msd_vocoder_create', 'msd_vocoder_destroy', 'msd_vocoder_last_error', 'msd_vocoder_stft', 'msd_vocoder_istft',
    'msd_vocoder_encode', 'msd_vocoder_decode',
    # (appended to ABI 7) one generator key per row of a batched call
    'msd_sample_rows',
    # (appended to ABI 7) known frames in the sampler
    'msd_sample_keep', 'msd_op_sampler_step_keep',
    # (appended to ABI 7) one GEMM launch site at a time
    'msd_op_gemm_site', 'msd_op_gemm_site_tiles', 'msd_op_gemm_site_name',
    # (appended to ABI 7) edit strength: per-frame release words and a part-way start of the sampler
    'msd_sample_edit', 'msd_op_sampler_step_release', 'msd_op_diffuse_to_step',
    # (appended to ABI 7) a step count and a sampler per call; the second-order multistep sampler
    'msd_sample_steps', 'msd_op_sampler_step_multistep',
    # (appended to ABI 7) one attention launch the way the decoder fills it
    'msd_op_attention_launch',
    # (appended to ABI 7) a launch with a weight target in either carrier form; how a target is dealt over the waves
    'msd_op_gemm_site_carrier', 'msd_op_attention_launch_carrier', 'msd_op_touch_deal', 'msd_set_touch_carrier',
    # (appended to ABI 7) known-frame edits with resampling jumps (RePaint) in the sampler scan
    'msd_sample_resample', 'msd_op_renoise',
    # (appended to ABI 7) a guidance weight per call or per row, applied in an interval of the scan
    'msd_sample_guided', 'msd_op_sampler_step_guided', 'msd_op_sampler_step_multistep_guided',
    # (appended to ABI 7) the denoising loss of a mel under the encoded tokens
    'msd_loss', 'msd_op_diffusion_loss',
    # (appended to ABI 7) deterministic DDIM inversion: the noise that renders a mel under the encoded tokens
    'msd_invert', 'msd_op_invert_step',
    # (appended to ABI 7) a sampler update of any form with its operand planes, range flag and published scan index
    'msd_op_sampler_step_planes',
    # (appended to ABI 7) the vocoder's phase update, its row layout and its work buffers, for the tests
    'msd_op_vocoder_phase', 'msd_op_vocoder_load_spec', 'msd_vocoder_debug_read')


LOSS_CONDITIONINGS = {'cond': 0, 'uncond': 1, 'both': 2}   # MSD_LOSS_COND, _UNCOND, _BOTH
LOSS_TYPES = {'x0': 0, 'eps': 1, 'max_x0_eps': 2, 'x0_and_eps': 3}   # MSD_LOSS_X0 ... (diffusion_utils.calculate_loss's names)
LOSS_NORMS = {'l1': 0, 'l2': 1}


def plan_loss_times(num_steps: int, times):
  """The time indices of a loss call on a handle of N = num_steps steps (index i = row i of the step tables, time
  (i + 1) / N).  An integer K with 1 <= K <= N gives the stratified grid i_j = ((2 j + 1) N) // (2 K), j = 0 .. K - 1: the
  middle of each of K equal strata, strictly increasing, every index for K == N.  A sequence gives its own entries, each an
  integer in [0, N), in the given order, repeats allowed.  Anything else is a ValueError.  No device needed."""
  n = _check_num_steps(num_steps)
  if isinstance(times, (bool, np.bool_)):
    raise ValueError('times must be an integer in [1, %d] or a sequence of time indices, not a bool' % n)
  if isinstance(times, (int, np.integer)):
    k = int(times)
    if not 1 <= k <= n:
      raise ValueError('times = %d is outside [1, %d] (the model\'s steps)' % (k, n))
    return [((2 * j + 1) * n) // (2 * k) for j in range(k)]
  try:
    idx = list(times)
  except TypeError:
    raise ValueError('times must be an integer in [1, %d] or a sequence of time indices: %r' % (n, times))
  if not idx:
    raise ValueError('times is empty: a loss call needs at least one time index')
  for i in idx:
    if not _is_int(i, 0) or i >= n:
      raise ValueError('time index %r is not an integer in [0, %d)' % (i, n))
  return [int(i) for i in idx]


class LossArgs(ctypes.Structure):
  """msd_loss_args of include/msd_amd.h, field for field."""
  _fields_ = [(n, ctypes.c_int32) for n in ('struct_size', 'batch', 'rng', 'per_row')] + [
      ('seeds', ctypes.POINTER(ctypes.c_uint64)), ('stream_ids', ctypes.POINTER(ctypes.c_uint64)),
      ('target_dev', ctypes.c_void_p), ('mask_dev', ctypes.c_void_p), ('eps_dev', ctypes.c_void_p),
      ('times_host', ctypes.POINTER(ctypes.c_int32))] + [
          (n, ctypes.c_int32) for n in ('n_times', 'conditioning', 'loss_type', 'loss_norm')] + [('out_dev', ctypes.c_void_p)]


class InvertArgs(ctypes.Structure):
  """msd_invert_args of include/msd_amd.h, field for field."""
  _fields_ = [('struct_size', ctypes.c_int32), ('batch', ctypes.c_int32), ('mel_dev', ctypes.c_void_p),
              ('num_steps', ctypes.c_int32), ('n_weights', ctypes.c_int32), ('weights_host', ctypes.POINTER(ctypes.c_float)),
              ('out_dev', ctypes.c_void_p)]


def invert_rows(logsnr_t, logsnr_s) -> np.ndarray:
  """The Python twin of build_invert_rows (csrc/msd_api.hip): the inversion's side table [K, 4] = {a, b, 0, 0} from the
  float32 log-SNRs of a K-step call's coefficient rows (row i: logsnr_t at time (i + 1) / K, logsnr_s at i / K; words 0 and 1
  of NativeModel.schedule()'s rows for K = N).  alpha = sqrt(sigmoid(logsnr)), sigma = sqrt(sigmoid(-logsnr)); a =
  alpha_t / alpha_s and b = sigma_t - a sigma_s, row 0 (alpha_t, sigma_t); in double, rounded once.  No device needed."""
  lt = np.asarray(logsnr_t, np.float32).astype(np.float64).reshape(-1)
  ls = np.asarray(logsnr_s, np.float32).astype(np.float64).reshape(-1)
  if lt.shape != ls.shape or lt.size < 1:
    raise ValueError('logsnr_t and logsnr_s must be two arrays of K >= 1 values: got %r and %r' % (lt.shape, ls.shape))
  alpha_t, sigma_t = np.sqrt(1.0 / (1.0 + np.exp(-lt))), np.sqrt(1.0 / (1.0 + np.exp(lt)))
  alpha_s, sigma_s = np.sqrt(1.0 / (1.0 + np.exp(-ls))), np.sqrt(1.0 / (1.0 + np.exp(ls)))
  a = alpha_t / alpha_s
  a[0] = alpha_t[0]
  b = sigma_t - a * sigma_s
  b[0] = sigma_t[0]
  out = np.zeros((lt.size, 4), np.float32)
  out[:, 0], out[:, 1] = a, b
  return out


def check_guidance(guidance, batch: int):
  """guidance of a call over `batch` rows -> its weights as a list of 1 or `batch` Python floats (the values float32
  holds); a ValueError for anything that is not a finite number or `batch` of them."""
  if isinstance(guidance, bool):
    raise ValueError('guidance must be a number or %d numbers, not a bool' % batch)
  try:
    w = np.asarray(guidance, dtype=np.float64)
  except (TypeError, ValueError):
    raise ValueError('guidance must be a number or %d numbers: %r' % (batch, guidance))
  if w.ndim > 1 or (w.ndim == 1 and w.size != batch):
    raise ValueError('guidance must be a number or one per row (%d): got shape %s' % (batch, tuple(w.shape)))
  with np.errstate(over='ignore'):   # (a weight beyond float32 becomes inf and is refused below)
    w32 = w.astype(np.float32).reshape(-1)
  if not np.all(np.isfinite(w32)):
    raise ValueError('guidance must be finite (in float32): %r' % (guidance,))
  return [float(x) for x in w32]


def check_guide_range(guide_range, num_steps: int):
  """(g_lo, g_hi), scan indices of a call of num_steps steps -> two ints with 0 <= g_lo < g_hi <= num_steps."""
  try:
    g_lo, g_hi = guide_range
  except (TypeError, ValueError):
    raise ValueError('guide_range must be (g_lo, g_hi): %r' % (guide_range,))
  _check_ints(('g_lo', g_lo, 0), ('g_hi', g_hi, 1))
  if not g_lo < g_hi <= num_steps:
    raise ValueError('guide_range needs 0 <= g_lo < g_hi <= %d: got (%d, %d)' % (num_steps, g_lo, g_hi))
  return int(g_lo), int(g_hi)


def divisors(n: int):
  return [k for k in range(1, n + 1) if n % k == 0]


def _is_int(v, lo: int) -> bool:
  """v is an integer (no bool) >= lo."""
  return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer)) and v >= lo


def _check_ints(*named):
  """(name, value, lowest) triples: a ValueError unless every value is an integer (no bool) >= its lowest."""
  for name, v, lo in named:
    if not _is_int(v, lo):
      raise ValueError('%s must be an integer >= %d: %r' % (name, lo, v))


def _check_num_steps(num_steps) -> int:
  """The step count of a handle, as plan_steps and plan_loss_times take it."""
  if not _is_int(num_steps, 1):
    raise ValueError('num_steps must be a positive integer: %r' % (num_steps,))
  return int(num_steps)


def plan_resample(start_step: int, jump: int, times: int):
  """The schedule of a call with resampling jumps (RePaint; msd_sample_resample) as a list of operations, in order:
  ('steps', top, bottom) -- the steps with scan indices top - 1 .. bottom -- and ('jump', bottom, top, p) -- the state
  diffused from level `bottom` back to level `top`, the call's p-th jump (p = 1, 2, ...; everything behind it is pass p).
  A level is the number of steps still to run; the call starts at level S = start_step + 1.  Block k has top S - k jump and
  bottom max(top - jump, 0); every block is descended `times` times with a jump after each descent but the last.
  times * S steps, (times - 1) ceil(S / jump) jumps; times == 1 is the plain descent whatever jump.  No device needed.
  jump and times must be integers >= 1 and start_step an integer >= -1: anything else is a ValueError."""
  _check_ints(('start_step', start_step, -1), ('jump', jump, 1), ('times', times, 1))
  level, jump, times = int(start_step) + 1, int(jump), int(times)
  ops, p = [], 0
  while level > 0:
    bottom = max(level - jump, 0)
    for r in range(times):
      ops.append(('steps', level, bottom))
      if r < times - 1:
        p += 1
        ops.append(('jump', bottom, level, p))
    level = bottom
  return ops


def check_resample(resample):
  """resample=(jump, times) of sample / predict -> (int jump, int times); a ValueError unless it is a pair of integers >= 1."""
  try:
    jump, times = resample
  except (TypeError, ValueError):
    raise ValueError('resample must be a (jump, times) pair: %r' % (resample,))
  _check_ints(('jump', jump, 1), ('times', times, 1))
  if jump > 0x7FFFFFFF or times > 0x7FFFFFFF:   # (the entry point takes C ints; a jump beyond the call's steps is one block)
    raise ValueError('jump and times must fit a 32-bit int: %r' % (resample,))
  return int(jump), int(times)


def plan_steps(num_steps: int, steps: int):
  """A K-step call on a handle of N = num_steps steps as a view of the handle's step-indexed tables: (row_offset, stride)
  = (N / K - 1, N / K) -- step j of the call has the time of table row (j + 1) N / K - 1, because (j + 1) / K and
  (r + 1) / N are the same rational, correctly rounded.  K must be a positive integer that divides N: anything else
  (0, negatives, bools, non-integers, non-divisors) is a ValueError that names the divisors of N.  No device needed."""
  n = _check_num_steps(num_steps)
  if not _is_int(steps, 1) or n % int(steps):
    raise ValueError('steps must divide the model\'s %d steps: got %r; the divisors are %s'
                     % (n, steps, ', '.join(str(k) for k in divisors(n))))
  return n // int(steps) - 1, n // int(steps)


class NativeLibraryError(RuntimeError):
  pass


class RangeError(ArithmeticError):
  """MSD_ERR_RANGE: an activation left the range of the IEEE-half operand planes (|x| > 65504) during the call;
  its result is invalid.  The bfloat16-plane precisions ('bf16x3') have float32's exponent range."""


MSD_SCHEDULE_COSINE, MSD_SCHEDULE_LINEAR = 0, 1
MSD_OUTPUT_EPS, MSD_OUTPUT_X0, MSD_OUTPUT_V = 0, 1, 2
MSD_LOGVAR_LARGE, MSD_LOGVAR_SMALL, MSD_LOGVAR_MEDIUM = 0, 1, 2
SCHEDULES = {'cosine': MSD_SCHEDULE_COSINE, 'linear': MSD_SCHEDULE_LINEAR}
MODEL_OUTPUTS = {'eps': MSD_OUTPUT_EPS, 'x0': MSD_OUTPUT_X0, 'v': MSD_OUTPUT_V}


class MsdConfig(ctypes.Structure):
  """msd_config of include/msd_amd.h (ABI 6 and 7), field for field."""
  _fields_ = [(n, ctypes.c_int32) for n in (
      'struct_size', 'has_context', 'vocab_size', 'emb_dim', 'num_heads', 'head_dim',
      'mlp_dim', 'num_encoder_layers', 'num_decoder_layers', 'inputs_length',
      'targets_length', 'context_length', 'n_dims', 'num_steps', 'sampler', 'clip_x0',
      'context_terminal_relative', 'precision', 'max_batch')] + [
          (n, ctypes.c_float) for n in (
              'max_decoder_noise_time', 'cfg_weight', 'feature_min', 'feature_max')] + [
      ('model_output', ctypes.c_int32), ('logvar_type', ctypes.c_int32), ('logvar_frac', ctypes.c_float),
      ('sampler_schedule', ctypes.c_int32), ('sampler_schedule_start', ctypes.c_float),
      ('sampler_schedule_stop', ctypes.c_float), ('train_schedule', ctypes.c_int32),
      ('train_schedule_start', ctypes.c_float), ('train_schedule_stop', ctypes.c_float),
      ('train_schedule_num_steps', ctypes.c_int32), ('cross_attend_sum', ctypes.c_int32),
      ('attn_q_planes', ctypes.c_int32), ('attn_p_planes', ctypes.c_int32), ('graph_steps', ctypes.c_int32),
      ('weight_prefetch', ctypes.c_int32),
      ('dedup_layer0', ctypes.c_int32), ('cross_key_split', ctypes.c_int32), ('keep_raw_weights', ctypes.c_int32),
      ('kv_touch_ahead', ctypes.c_int32),
      ('cross_merge_in_launch', ctypes.c_int32), ('cross_q_fold', ctypes.c_int32),
      ('mlp_in_persistent', ctypes.c_int32),
      ('touch_carrier', ctypes.c_int32)]   # (appended to ABI 7)


class GemmSiteArgs(ctypes.Structure):
  """msd_gemm_site_args of include/msd_amd.h, field for field."""
  _INTS = ('struct_size', 'precision', 'site', 'm', 'n', 'k', 'step', 'steps', 'force_bm', 'force_bn', 'persistent',
           'resident_blocks', 'seg_len', 'split_row', 'dup_rows', 'y2_rows', 'passes', 'm2', 'n2', 'k2', 'force_bm2',
           'force_bn2', 'prefetch_rows', 'prefetch_k',
           'ran_bm', 'ran_bn', 'ran_ns', 'ran_xcd_rows', 'ran_persistent', 'ran_dual', 'ran_prefetch',
           'ran_bm2', 'ran_bn2', 'ran_ns2', 'ran_xcd_rows2', 'step_copy')
  _PTRS = ('a', 'w', 'w_gate', 'ssq', 'bias', 'g_lo', 'g_hi', 'g2', 'pos', 'a2', 'w2', 'addend2', 'prefetch',
           'x', 'out', 'y', 'y2', 'ssq_out', 'out2')
  _fields_ = [(n, ctypes.c_int32) for n in _INTS] + [(n, ctypes.c_void_p) for n in _PTRS]


class CarrierArgs(ctypes.Structure):
  """msd_carrier_args of include/msd_amd.h, field for field."""
  _INTS = ('struct_size', 'form', 'n_touch', 'delay', 'target_rows', 'target_k', 'ran_form', 'ran_touch_blocks',
           'ran_range_flag')
  _fields_ = [(n, ctypes.c_int32) for n in _INTS]


CARRIER_FORMS = {'none': 0, 'wave': 1, 'blocks': 2}   # msd_carrier_args.form


class SamplerPlanesArgs(ctypes.Structure):
  """msd_sampler_planes_args of include/msd_amd.h, field for field."""
  _INTS = ('struct_size', 'step_index', 'n_dims', 'keep_is_flags', 'first', 'rows', 'ran_range_flag', 'ran_next_step')
  _PTRS = ('z', 'out_cond', 'out_uncond', 'noise', 'known_scaled', 'keep', 'x0_prev')
  _fields_ = [(n, ctypes.c_int32) for n in _INTS] + [('n', ctypes.c_int64), ('cfg', ctypes.POINTER(MsdConfig))] + [
      (n, ctypes.c_void_p) for n in _PTRS] + [('weights', ctypes.POINTER(ctypes.c_float)), ('z_out', ctypes.c_void_p),
                                              ('z_planes_out', ctypes.c_void_p)]


class AttentionLaunchArgs(ctypes.Structure):
  """msd_attention_launch_args of include/msd_amd.h, field for field."""
  _INTS = ('struct_size', 'precision', 'qp', 'heads', 'segs', 'q_rows_per_seg', 'repeats', 'ksplit', 'merge_in_launch',
           'allow_qb4', 'ldq', 'q_col', 'ldk', 'k_col', 'k_alloc_rows', 'k_row0', 'k_rows', 'prefetch_rows', 'prefetch_k',
           'touch_ahead', 'pf_late', 'q_tiles', 'ran_qb', 'ran_prefetch_wave', 'ran_touch_ahead', 'ran_ksplit')
  _PTRS = ('q', 'k', 'v', 'n_keys', 'q_ssq', 'o')
  _fields_ = [(n, ctypes.c_int32) for n in _INTS] + [(n, ctypes.c_void_p) for n in _PTRS]


# launch sites of msd_op_gemm_site: positions in GemmSites / DualSites of csrc/msd_api.hip (include/msd_amd.h).  The
# library names its sites from their types (gemm_site_names); tests/test_gpu_gemm_sites.py holds this table against it.
GEMM_SITES = {'qkv': 0, 'mlp_in': 1, 'residual_square': 2, 'residual_tall': 3, 'resnorm_tall': 4, 'resnorm_tall_dup': 5,
              'resnorm_square': 6, 'store_h16': 7, 'store_f32': 8, 'in_proj': 9, 'resnorm_tall_y2': 10,
              'dual_qkv': 11, 'dual_out': 12, 'dual_out_dup': 13}


# msd_config only ever grows at its end, so an OLDER library can be driven by passing it the struct size it knows
# (same-box A/B of a previous round's binary through MSD_AMD_LIB: tools/ab/); the newer fields are then simply not seen.
ABI_STRUCT_SIZES = {4: MsdConfig.weight_prefetch.offset + 4, 5: MsdConfig.kv_touch_ahead.offset + 4,
                    6: MsdConfig.mlp_in_persistent.offset + 4,
                    7: MsdConfig.mlp_in_persistent.offset + 4}   # ABI 7 appends entry points only ...


def config_struct_size(lib) -> int:
  """The msd_config size to hand to `lib`: this package's own library -- and any build that exports msd_op_touch_deal --
  knows the field appended to ABI 7 since (touch_carrier); an older build under MSD_AMD_LIB gets the size of its ABI."""
  if hasattr(lib, 'msd_op_touch_deal'):
    return ctypes.sizeof(MsdConfig)
  return ABI_STRUCT_SIZES[getattr(lib, '_msd_abi', None) or ABI_VERSION]

_libs = {}


def load(planes: str = 'f16') -> ctypes.CDLL:
  """dlopen libmsd_amd.so (planes 'f16') or libmsd_amd_bf16.so ('bf16') and declare prototypes.  Fails loudly
  if missing."""
  if planes in _libs:
    return _libs[planes]
  LIB_PATH = LIB_PATHS[planes]
  # same-box A/B of two builds (tools/ab_bench.sh, the experiments build of tools/ubench/exp): MSD_AMD_LIB=<path>
  # replaces the half-plane library.  This is the ONLY environment variable the package reads; the library itself
  # reads none.  An older build may lack the newest entry points: they stay unbound (calling one raises
  # AttributeError) and a warning names them.
  override = os.environ.get('MSD_AMD_LIB') if planes == 'f16' else None
  if override:
    LIB_PATH = override
  if not os.path.exists(LIB_PATH):
    raise NativeLibraryError(
        'HIP library not built: %s is missing. Build it with '
        '`python music-spectrogram-diffusion_amd/build_native.py` (needs hipcc); '
        'there is no CPU fallback for this path.' % LIB_PATH)
  try:
    lib = ctypes.CDLL(LIB_PATH)
  except OSError as e:  # missing ROCm runtime etc.
    raise NativeLibraryError('cannot load %s: %s' % (LIB_PATH, e)) from e
  present = [sym for sym in EXPORTED_SYMBOLS if hasattr(lib, sym)]
  if len(present) != len(EXPORTED_SYMBOLS):
    missing = sorted(set(EXPORTED_SYMBOLS) - set(present))
    if not override:
      raise NativeLibraryError('%s does not export %s' % (LIB_PATH, missing))
    import warnings
    warnings.warn('MSD_AMD_LIB=%s does not export %s: those entry points are unbound' % (LIB_PATH, missing), RuntimeWarning)
  if override:
    if 'msd_version' not in present:   # (the warning above is no help for the one symbol this check needs)
      raise NativeLibraryError('MSD_AMD_LIB=%s does not export msd_version: cannot verify its ABI (this package binds ABI %d)'
                               % (LIB_PATH, ABI_VERSION))
    lib.msd_version.restype = ctypes.c_char_p
    ver = lib.msd_version() or b''
    lib._msd_abi = next((a for a in ABI_STRUCT_SIZES if ('abi %d' % a).encode() in ver), None)
    if lib._msd_abi is None:
      raise NativeLibraryError('MSD_AMD_LIB=%s is %r: this package binds ABI %d (and drives ABI %s through their msd_config size)'
                               % (LIB_PATH, ver, ABI_VERSION, sorted(set(ABI_STRUCT_SIZES) - {ABI_VERSION})))
  c = ctypes
  vp, i32, i64, u64, u32 = c.c_void_p, c.c_int, c.c_int64, c.c_uint64, c.c_uint32
  lib.msd_version.restype = c.c_char_p
  lib.msd_device_count.restype = i32
  lib.msd_create.argtypes = [c.POINTER(MsdConfig), c.POINTER(vp)]
  lib.msd_destroy.argtypes = [vp]
  lib.msd_destroy.restype = None
  lib.msd_last_error.argtypes = [vp]
  lib.msd_last_error.restype = c.c_char_p
  lib.msd_num_weights.argtypes = [vp]
  lib.msd_weight_info.argtypes = [vp, i32, c.POINTER(c.c_char_p), c.POINTER(i64), c.POINTER(i32)]
  lib.msd_set_weight.argtypes = [vp, c.c_char_p, vp, c.POINTER(i64), i32]
  lib.msd_finalize_weights.argtypes = [vp, vp]
  lib.msd_encode.argtypes = [vp, i32, vp, vp, vp, vp]
  lib.msd_sample.argtypes = [vp, i32, u64, u64, vp, vp, vp, vp]
  lib.msd_decoder_pass.argtypes = [vp, i32, i32, vp, i32, vp, vp]
  lib.msd_reset_graph.argtypes = [vp]
  lib.msd_fill_normal.argtypes = [u64, u64, u32, vp, i64, vp]
  if 'msd_sample_rng' in present:
    lib.msd_sample_rng.argtypes = [vp, i32, i32, u64, u64, vp, vp, vp, vp]
  if 'msd_sample_rows' in present:   # (appended to ABI 7)
    lib.msd_sample_rows.argtypes = [vp, i32, i32, c.POINTER(u64), c.POINTER(u64), vp, vp, vp, vp]
  if 'msd_sample_keep' in present:   # (appended to ABI 7)
    lib.msd_sample_keep.argtypes = [vp, i32, i32, i32, c.POINTER(u64), c.POINTER(u64), vp, vp, vp, vp, vp, vp]
    lib.msd_op_sampler_step_keep.argtypes = [c.POINTER(MsdConfig), i32, vp, vp, vp, vp, vp, vp, i32, vp, i64, vp]
  if 'msd_sample_edit' in present:   # (appended to ABI 7)
    lib.msd_sample_edit.argtypes = [vp, i32, i32, i32, c.POINTER(u64), c.POINTER(u64), vp, vp, vp, vp, i32, vp, vp]
    lib.msd_op_sampler_step_release.argtypes = [c.POINTER(MsdConfig), i32, vp, vp, vp, vp, vp, vp, i32, vp, i64, vp]
    lib.msd_op_diffuse_to_step.argtypes = [c.POINTER(MsdConfig), i32, vp, vp, vp, vp, vp, i64, vp]
  if 'msd_sample_steps' in present:   # (appended to ABI 7)
    lib.msd_sample_steps.argtypes = [vp, i32, i32, i32, c.POINTER(u64), c.POINTER(u64), vp, vp, i32, i32, vp, vp]
    lib.msd_op_sampler_step_multistep.argtypes = [c.POINTER(MsdConfig), i32, vp, vp, vp, vp, i32, vp, i64, vp]
  if 'msd_sample_resample' in present:   # (appended to ABI 7)
    lib.msd_sample_resample.argtypes = [vp, i32, i32, i32, c.POINTER(u64), c.POINTER(u64), vp, vp, vp, i32, i32, i32, vp, vp]
    lib.msd_op_renoise.argtypes = [c.POINTER(MsdConfig), i32, i32, vp, vp, vp, vp, i64, vp]
  if 'msd_sample_guided' in present:   # (appended to ABI 7)
    fp = c.POINTER(c.c_float)
    lib.msd_sample_guided.argtypes = [vp, i32, i32, i32, c.POINTER(u64), c.POINTER(u64), vp, vp, i32, i32, fp, i32, i32, i32, vp, vp]
    lib.msd_op_sampler_step_guided.argtypes = [c.POINTER(MsdConfig), i32, vp, vp, vp, vp, fp, i32, vp, i64, vp]
    lib.msd_op_sampler_step_multistep_guided.argtypes = [c.POINTER(MsdConfig), i32, vp, vp, vp, vp, i32, fp, i32, vp, i64, vp]
  if 'msd_loss' in present:   # (appended to ABI 7)
    lib.msd_loss.argtypes = [vp, c.POINTER(LossArgs), vp]
    lib.msd_op_diffusion_loss.argtypes = [c.POINTER(MsdConfig), i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, i64, vp]
  if 'msd_invert' in present:   # (appended to ABI 7)
    lib.msd_invert.argtypes = [vp, c.POINTER(InvertArgs), vp]
    lib.msd_op_invert_step.argtypes = [c.POINTER(MsdConfig), i32, vp, vp, vp, c.POINTER(c.c_float), i32, vp, vp, i64, vp]
  if 'msd_op_sampler_step_planes' in present:   # (appended to ABI 7)
    lib.msd_op_sampler_step_planes.argtypes = [c.POINTER(SamplerPlanesArgs), vp]
  if 'msd_fill_normal_threefry' in present:
    lib.msd_fill_normal_threefry.argtypes = [u64, i64, vp, i64, vp]
  if 'msd_op_threefry' in present:
    lib.msd_op_threefry.argtypes = [i32, u64, i64, vp, vp, i64, vp]
  lib.msd_get_schedule.argtypes = [vp, vp]
  lib.msd_debug_read.argtypes = [vp, c.c_char_p, vp, i64, c.POINTER(i64)]
  lib.msd_profile_steps.argtypes = [vp, i32, i32, c.POINTER(c.POINTER(c.c_char_p)),
                                    c.POINTER(c.c_double), c.POINTER(i64), vp]
  if 'msd_op_gemm_h16' in present:
    lib.msd_op_gemm_h16.argtypes = [i32, vp, vp, vp, i32, i32, i32, vp]
  lib.msd_op_gemm_bf16.argtypes = [i32, vp, vp, vp, i32, i32, i32, vp]
  lib.msd_op_gemm_f32.argtypes = [vp, vp, vp, i32, i32, i32, vp]
  lib.msd_op_attention.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, vp]
  if 'msd_op_attention_qp' in present:
    lib.msd_op_attention_qp.argtypes = [i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp]
  if 'msd_op_attention_split' in present:
    lib.msd_op_attention_split.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp]
  if 'msd_op_attention_ex' in present:
    lib.msd_op_attention_ex.argtypes = [i32, i32, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp]
  lib.msd_op_sampler_step.argtypes = [c.POINTER(MsdConfig), i32, vp, vp, vp, vp, vp, i64, vp]
  lib.msd_op_residual_norm_gemm.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
  lib.msd_op_geglu.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
  lib.msd_op_qkv.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
  lib.msd_op_final_proj.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
  if 'msd_vocoder_create' in present:   # (appended to ABI 7: an older library under MSD_AMD_LIB has none of them)
    lib.msd_vocoder_create.argtypes = [vp, vp, c.POINTER(vp)]
    lib.msd_vocoder_destroy.argtypes = [vp]
    lib.msd_vocoder_destroy.restype = None
    lib.msd_vocoder_last_error.argtypes = [vp]
    lib.msd_vocoder_last_error.restype = c.c_char_p
    lib.msd_vocoder_stft.argtypes = [vp, i32, i64, vp, vp, vp]
    lib.msd_vocoder_istft.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.msd_vocoder_encode.argtypes = [vp, i32, i64, vp, vp, vp]
    lib.msd_vocoder_decode.argtypes = [vp, i32, i32, vp, i32, c.c_float, u64, vp, vp, vp]
  if 'msd_vocoder_debug_read' in present:   # (appended to ABI 7)
    lib.msd_op_vocoder_phase.argtypes = [vp, vp, vp, vp, i32, c.c_float, vp]
    lib.msd_op_vocoder_load_spec.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    lib.msd_vocoder_debug_read.argtypes = [vp, c.c_char_p, vp, i64, c.POINTER(i64)]
  if 'msd_op_gemm_site' in present:   # (appended to ABI 7)
    lib.msd_op_gemm_site.argtypes = [c.POINTER(GemmSiteArgs), vp]
    lib.msd_op_gemm_site_tiles.argtypes = [i32, i32, i32, c.POINTER(c.c_int32), c.POINTER(c.c_int32), c.POINTER(c.c_int32)]
    lib.msd_op_gemm_site_name.argtypes = [i32, i32]
    lib.msd_op_gemm_site_name.restype = c.c_char_p
  if 'msd_op_attention_launch' in present:   # (appended to ABI 7)
    lib.msd_op_attention_launch.argtypes = [c.POINTER(AttentionLaunchArgs), vp]
  if 'msd_op_touch_deal' in present:   # (appended to ABI 7)
    lib.msd_op_gemm_site_carrier.argtypes = [c.POINTER(GemmSiteArgs), c.POINTER(CarrierArgs), vp]
    lib.msd_op_attention_launch_carrier.argtypes = [c.POINTER(AttentionLaunchArgs), c.POINTER(CarrierArgs), vp]
    lib.msd_op_touch_deal.argtypes = [i64, i32, i32, i32, c.POINTER(c.c_int32), i32]
    lib.msd_set_touch_carrier.argtypes = [vp, i32]
  for name in present:
    fn = getattr(lib, name)
    if name not in ('msd_version', 'msd_last_error', 'msd_destroy', 'msd_vocoder_last_error', 'msd_vocoder_destroy',
                    'msd_op_gemm_site_name'):
      fn.restype = i32
  _libs[planes] = lib
  return lib


MSD_ERR_INVALID_ARGUMENT = 1   # msd_status of include/msd_amd.h
_EXC = {1: ValueError, 2: KeyError, 3: ValueError, 4: RuntimeError, 5: RuntimeError,
        6: NotImplementedError, 7: RangeError}


def _check(lib, handle, rc, what):
  if rc == 0:
    return
  msg = lib.msd_last_error(handle).decode('utf-8', 'replace') if handle else ''
  raise _EXC.get(rc, RuntimeError)('%s failed (msd_status %d): %s' % (what, rc, msg))


def _ptr(t) -> Optional[int]:
  """Device/host pointer of a torch tensor or numpy array (None -> NULL)."""
  if t is None:
    return None
  if isinstance(t, np.ndarray):
    return t.ctypes.data
  return t.data_ptr()


class NativeModel:
  """Owns one ``msd_model*`` on the current HIP device."""

  def __init__(self, cfg: MsdConfig, planes: Optional[str] = None):
    """`planes` (which library build) follows from cfg.precision; passing the other build's name is an error the
    library itself reports (msd_create -> MSD_ERR_UNSUPPORTED -> NotImplementedError)."""
    if planes is None:
      if cfg.precision not in _PLANES_OF:
        raise ValueError('unknown msd_precision %r' % (cfg.precision,))
      planes = _PLANES_OF[cfg.precision]
    self.lib = load(planes)
    self.planes = planes
    self.cfg = cfg
    self.handle = ctypes.c_void_p()
    cfg.struct_size = config_struct_size(self.lib)
    rc = self.lib.msd_create(ctypes.byref(cfg), ctypes.byref(self.handle))
    if rc != 0:
      msg = self.lib.msd_last_error(self.handle).decode() if self.handle else 'invalid config'
      if self.handle:
        self.lib.msd_destroy(self.handle)
        self.handle = ctypes.c_void_p()
      raise _EXC.get(rc, RuntimeError)('msd_create failed (msd_status %d): %s' % (rc, msg))

  def close(self):
    if getattr(self, 'handle', None):
      self.lib.msd_destroy(self.handle)
      self.handle = ctypes.c_void_p()

  def __del__(self):
    try:
      self.close()
    except Exception:  # interpreter shutdown
      pass

  # -- weights ---------------------------------------------------------------
  def weight_specs(self) -> List[Tuple[str, Tuple[int, ...]]]:
    out = []
    for i in range(self.lib.msd_num_weights(self.handle)):
      name = ctypes.c_char_p()
      shape = (ctypes.c_int64 * 2)()
      ndim = ctypes.c_int()
      _check(self.lib, self.handle,
             self.lib.msd_weight_info(self.handle, i, ctypes.byref(name), shape, ctypes.byref(ndim)),
             'msd_weight_info')
      out.append((name.value.decode(), tuple(int(shape[k]) for k in range(ndim.value))))
    return out

  def set_weight(self, name: str, array):
    """array: float32 numpy array or torch tensor (host or device), C-contiguous."""
    if isinstance(array, np.ndarray):
      array = np.ascontiguousarray(array, dtype=np.float32)
      shape = array.shape
    else:
      array = array.contiguous().float()
      shape = tuple(array.shape)
    cshape = (ctypes.c_int64 * max(len(shape), 1))(*shape)
    _check(self.lib, self.handle,
           self.lib.msd_set_weight(self.handle, name.encode(), _ptr(array), cshape, len(shape)),
           'msd_set_weight(%s)' % name)

  def load_weights(self, params: Dict[str, np.ndarray], stream: int = 0):
    specs = dict(self.weight_specs())
    missing = [k for k in specs if k not in params]
    if missing:
      raise KeyError('parameter dict is missing %d weights, e.g. %s' % (len(missing), missing[:3]))
    for name in specs:
      self.set_weight(name, params[name])
    _check(self.lib, self.handle, self.lib.msd_finalize_weights(self.handle, stream),
           'msd_finalize_weights')

  # -- hot path ----------------------------------------------------------------
  def encode(self, batch: int, tokens, ctx=None, ctx_mask=None, stream: int = 0):
    _check(self.lib, self.handle,
           self.lib.msd_encode(self.handle, batch, _ptr(tokens), _ptr(ctx), _ptr(ctx_mask), stream),
           'msd_encode')

  def sample(self, batch: int, out, seed: int = 0, stream_id: int = 0, init_z=None,
             noise=None, stream: int = 0, rng: str = 'philox', keep=None, keep_mask=None, release=None,
             start_step: Optional[int] = None, steps: Optional[int] = None, sampler: Optional[str] = None,
             resample=None, guidance=None, guide_range=None):
    """rng: the generator of the draws that are not given -- 'philox' (the library's own, keyed by seed and stream_id)
    or 'threefry' (the reference's jax.random draws for PRNGKey(seed), made on the device; stream_id is ignored).

    seed / stream_id may be sequences of `batch` integers (a scalar beside a sequence is broadcast): every row then
    has a key of its own and draws what the one-row call (seed[b], stream_id[b]) draws (msd_sample_rows).  Scalars
    key ONE draw over the whole [batch, T, n] array, as before.

    keep (float32 device tensor [batch, T, n], mel units) / keep_mask (int32 [batch, T], NumPy or device; non-zero = the
    frame is known): the kept frames come back as given and the others are sampled around them (msd_sample_keep); both
    or neither.  The keys and the draws are those of the call without them.

    keep with release (int32 NumPy [batch, T], the frames' release words) and start_step instead of keep_mask: the edit
    form (msd_sample_edit) -- a frame with word v >= 1 is known at scan indices >= v - 1 and free below, 0 = free
    throughout; the scan starts at start_step from the known mel diffused to that step (None = num_steps - 1: from
    init_z, as ever).

    steps (K, a divisor of the handle's num_steps; None = all of them) / sampler ('ddpm', 'ddim', 'dpmpp_2m'; None = the
    handle's): a step count and a sampler for THIS call (msd_sample_steps); noise is then [K, batch, T, n].  Not with
    keep / release.

    resample (jump, times), with keep: resampling jumps (RePaint; msd_sample_resample, plan_resample) -- every block of
    `jump` steps is descended `times` times, the state diffused back up in between under a key of the pass's own.  The
    extra draws are made on the device: not with noise, nor with steps / sampler.  keep_mask is taken as release words
    (1 = known throughout).  times == 1 makes no jump: msd_sample_resample then returns the bits of the call without
    resample, like None.

    guidance (a finite float, or `batch` of them: row b takes guidance[b]) / guide_range ((g_lo, g_hi), scan indices of
    the call's K steps with 0 <= g_lo < g_hi <= K; None = all of them): the classifier-free guidance weight of THIS call
    in the handle's cfg_weight's place, applied at scan indices in [g_lo, g_hi) only; every other step -- and a row whose
    weight is exactly 1 -- runs the reference's weight-1 branch, one decoder pass (msd_sample_guided).  guide_range alone
    takes the handle's weight.  With steps / sampler, every rng and key form, init_z / noise; not with keep / release /
    resample, nor on a handle created with cfg_weight 1."""
    if guidance is not None or guide_range is not None:
      if keep is not None or keep_mask is not None or release is not None or start_step is not None or resample is not None:
        raise ValueError('guidance / guide_range cannot be combined with keep / keep_mask / release / start_step / resample')
      weights = check_guidance(self.cfg.cfg_weight if guidance is None else guidance, batch)
      k_call = self.cfg.num_steps if steps is None else steps
      g_lo, g_hi = (0, 0) if guide_range is None else check_guide_range(guide_range, k_call)
    few, edit = steps is not None or sampler is not None, release is not None
    if resample is not None:
      jump, times = check_resample(resample)
      if keep is None:
        raise ValueError('resample needs keep: resampling jumps harmonise free frames with known ones')
      if few:
        raise ValueError('resample cannot be combined with steps / sampler')
      if noise is not None:
        raise ValueError('resample cannot be combined with noise: the jumps\' and the later passes\' draws are made on the device')
      if not edit:   # msd_sample_keep's flags as release words (host): any non-zero flag = known throughout = 1
        if keep_mask is None:
          raise ValueError('keep and keep_mask go together')
        flags = keep_mask.detach().cpu().numpy() if hasattr(keep_mask, 'detach') else np.asarray(keep_mask)
        release, keep_mask, edit = np.ascontiguousarray(flags != 0, dtype=np.int32), None, True
    # (1) what the call may not combine or name
    _check_rng(rng)
    if few and (keep is not None or keep_mask is not None or edit or start_step is not None):
      raise ValueError('steps / sampler cannot be combined with keep / keep_mask / release / start_step')
    if sampler is not None and sampler not in SAMPLERS:
      raise ValueError('sampler must be one of %s: %r' % (sorted(SAMPLERS), sampler))
    if steps is not None:
      plan_steps(self.cfg.num_steps, steps)   # (its checks: a ValueError that names the divisors)
    if edit and (keep is None or keep_mask is not None):
      raise ValueError('release goes with keep and without keep_mask')
    if edit:
      release = np.ascontiguousarray(release, dtype=np.int32)
      if release.size != batch * self.cfg.targets_length:
        raise ValueError('release must hold one word per frame: [%d, %d]' % (batch, self.cfg.targets_length))
    elif start_step is not None:
      raise ValueError('start_step goes with release')
    elif (keep is None) != (keep_mask is None):
      raise ValueError('keep and keep_mask go together')
    # (2) the keys: one for the whole array, or one per row
    per_row, *keys = _key_arrays(batch, seed, stream_id)
    # (3) the entry point
    lib, h, kind, draws, tail = self.lib, self.handle, RNGS[rng], (_ptr(init_z), _ptr(noise)), (_ptr(out), stream)
    if guidance is not None or guide_range is not None:
      w = (ctypes.c_float * len(weights))(*weights)
      name, rc = 'msd_sample_guided', lib.msd_sample_guided(h, batch, kind, int(per_row), *keys, *draws, int(steps or 0),
                                                            -1 if sampler is None else SAMPLERS[sampler], w, len(weights),
                                                            g_lo, g_hi, *tail)
    elif few:
      name, rc = 'msd_sample_steps', lib.msd_sample_steps(h, batch, kind, int(per_row), *keys, *draws, int(steps or 0),
                                                          -1 if sampler is None else SAMPLERS[sampler], *tail)
    elif edit and resample is not None:
      start = self.cfg.num_steps - 1 if start_step is None else int(start_step)
      name, rc = 'msd_sample_resample', lib.msd_sample_resample(h, batch, kind, int(per_row), *keys, _ptr(init_z), _ptr(keep),
                                                                _ptr(release), start, jump, times, *tail)
    elif edit:
      start = self.cfg.num_steps - 1 if start_step is None else int(start_step)
      name, rc = 'msd_sample_edit', lib.msd_sample_edit(h, batch, kind, int(per_row), *keys, *draws, _ptr(keep), _ptr(release), start, *tail)
    elif keep is not None:
      name, rc = 'msd_sample_keep', lib.msd_sample_keep(h, batch, kind, int(per_row), *keys, *draws, _ptr(keep), _ptr(keep_mask), *tail)
    elif per_row:
      name, rc = 'msd_sample', lib.msd_sample_rows(h, batch, kind, *keys, *draws, *tail)
    elif rng == 'philox':   # (the entry point every ABI has: an older library under MSD_AMD_LIB still runs)
      name, rc = 'msd_sample', lib.msd_sample(h, batch, seed, stream_id, *draws, *tail)
    else:
      name, rc = 'msd_sample', lib.msd_sample_rng(h, batch, kind, seed, stream_id, *draws, *tail)
    _check(lib, h, rc, name)

  def loss(self, batch: int, target, out, times, seed=0, stream_id=0, rng: str = 'philox', conditioning: str = 'cond',
           loss_type: str = 'eps', loss_norm: str = 'l1', mask=None, eps=None, stream: int = 0):
    """The denoising loss of `target` (float32 device tensor [batch, T, n], mel units) under the encoded tokens
    (msd_loss), per frame: out (float32 device tensor [len(times), passes, batch, T]; passes = 2 for conditioning 'both' --
    0 = conditional --, else 1).  times: time indices in [0, num_steps) (plan_loss_times).  mask: float32 device
    [batch, T] or None = ones; eps: float32 device [len(times), batch, T, n] or None = drawn under (seed, stream_id) with
    `rng`, scalars or one per row as in sample().  A time index that appears twice draws the same eps twice.  loss_type /
    loss_norm: diffusion_utils.calculate_loss's names.  Argument errors are raised before the library is called."""
    _check_rng(rng)
    if conditioning not in LOSS_CONDITIONINGS:
      raise ValueError('conditioning must be one of %s: %r' % (sorted(LOSS_CONDITIONINGS), conditioning))
    if loss_type not in LOSS_TYPES:
      raise ValueError('Unknown diffusion loss_type: %r (one of %s)' % (loss_type, sorted(LOSS_TYPES)))
    if loss_norm not in LOSS_NORMS:
      raise ValueError('Unknown diffusion loss norm: %r (one of %s)' % (loss_norm, sorted(LOSS_NORMS)))
    idx = plan_loss_times(self.cfg.num_steps, times)
    per_row, seeds, stream_ids = _key_arrays(batch, seed, stream_id)
    passes = 2 if conditioning == 'both' else 1
    frames = batch * self.cfg.targets_length
    _check_holds('target', target, frames * self.cfg.n_dims)
    _check_holds('out', out, len(idx) * passes * frames)
    if mask is not None:
      _check_holds('mask', mask, frames)
    if eps is not None:
      _check_holds('eps', eps, len(idx) * frames * self.cfg.n_dims)
    a = LossArgs()
    a.struct_size, a.batch, a.rng, a.per_row = ctypes.sizeof(LossArgs), batch, RNGS[rng], int(per_row)
    a.seeds, a.stream_ids = seeds, stream_ids
    a.target_dev, a.mask_dev, a.eps_dev, a.out_dev = _ptr(target), _ptr(mask), _ptr(eps), _ptr(out)
    a.times_host, a.n_times = (ctypes.c_int32 * len(idx))(*idx), len(idx)
    a.conditioning, a.loss_type, a.loss_norm = LOSS_CONDITIONINGS[conditioning], LOSS_TYPES[loss_type], LOSS_NORMS[loss_norm]
    _check(self.lib, self.handle, self.lib.msd_loss(self.handle, ctypes.byref(a), stream), 'msd_loss')

  def invert(self, batch: int, out, mel, steps: Optional[int] = None, guidance=None, stream: int = 0):
    """Deterministic DDIM inversion under the encoded tokens (msd_invert): mel (float32 device tensor [batch, T, n], mel
    units) -> out (float32 device tensor [batch, T, n]): z at the top level of a K-step scan, in MODEL units -- the init_z
    with which sample(steps=K, sampler='ddim', guidance=...) renders the mel again, up to the inversion's own error.
    steps: K, a divisor of the handle's num_steps (plan_steps); None = all of them.  guidance: a finite float or `batch` of
    them; None = 1.0 (NOT the handle's weight: one decoder pass per step, and inversion under a large weight is
    unstable).  The sampler's clip is ignored (it cannot be inverted).  Argument errors are raised before the library is
    called."""
    if steps is not None:
      plan_steps(self.cfg.num_steps, steps)   # (its checks: a ValueError that names the divisors)
    weights = check_guidance(1.0 if guidance is None else guidance, batch)
    want = batch * self.cfg.targets_length * self.cfg.n_dims
    _check_holds('mel', mel, want)
    _check_holds('out', out, want)
    a = InvertArgs()
    a.struct_size, a.batch, a.num_steps = ctypes.sizeof(InvertArgs), batch, int(steps or 0)
    a.mel_dev, a.out_dev = _ptr(mel), _ptr(out)
    a.weights_host, a.n_weights = (ctypes.c_float * len(weights))(*weights), len(weights)
    _check(self.lib, self.handle, self.lib.msd_invert(self.handle, ctypes.byref(a), stream), 'msd_invert')

  def set_touch_carrier(self, touch_carrier: Optional[int]):
    """msd_config.touch_carrier of this handle from the next sampling call on (None = the library's choice, 1, 2)."""
    _check(self.lib, self.handle, self.lib.msd_set_touch_carrier(self.handle, int(touch_carrier or 0)), 'msd_set_touch_carrier')

  def reset_graph(self):
    _check(self.lib, self.handle, self.lib.msd_reset_graph(self.handle), 'msd_reset_graph')

  def decoder_pass(self, batch: int, step_index: int, z, include_conditioning: bool, eps_out,
                   stream: int = 0):
    _check(self.lib, self.handle,
           self.lib.msd_decoder_pass(self.handle, batch, step_index, _ptr(z),
                                     int(bool(include_conditioning)), _ptr(eps_out), stream),
           'msd_decoder_pass')

  def schedule(self) -> np.ndarray:
    out = np.zeros((self.cfg.num_steps, 8), np.float32)
    _check(self.lib, self.handle, self.lib.msd_get_schedule(self.handle, out.ctypes.data),
           'msd_get_schedule')
    return out

  def debug_read(self, buffer: str, max_elems: Optional[int] = None) -> np.ndarray:
    """An internal buffer as flat float32 (msd_debug_read; 16-bit planes merged).  The encode stage: 'enc' [S_pad, D]
    (the last encoded row), 'cross_k' [Ld, Bmax, S_pad, J], 'cross_vt' [Ld, Bmax, J, S_pad] (keys permuted per 16).  The
    load-time tables: 'film' [N, 2 Ld, 2 D], 'g_table' [N, 2 Ld, D], 'bw_self' [N, Ld, 3 J], 'bw_mlp' [N, Ld, 2 F] (the
    gated projection's packed column order).

    The decoder's per-step buffers hold what the LAST decoder evaluation left, and of its layers the last one's (they
    are overwritten layer by layer).  B songs of T frames, BT = B T, pass p in rows [p BT, (p + 1) BT) -- the conditional
    pass first in a CFG step --, J = heads 64, F = the MLP width, nq = n_cross J (tests/decoder_stage_cases.py reads them
    this way, tests/test_gpu_decoder_stages.py holds each to float64):
      'qk'  [M, 2 J]       q | k of the self-attention; layer 0 of a CFG step under dedup_layer0: the first BT rows only
      'vt'  [M / T, J, T]  v transposed per (pass, song), keys permuted per 16
      'ao'  [M, J]         conditional rows: the FIRST cross-attention module's output (it overwrites the self-attention
                           output); unconditional rows: the self-attention output (layer 0 under dedup: not written)
      'ao2' [Bmax T, J]    the second module's output (sum_cross_attends with a context encoder; else an unknown buffer)
      'cq'  folded query projection: [BT, nq], the modules' UN-normalised queries (x1 (.) gamma_cross) Wq_e side by side
            (the attention applies 1 / rms from 'ssq'); un-folded: [Bmax T, J] per module, the normalised queries --
            'cq2' [Bmax T, J] is the second module's part (un-folded only; an unknown buffer without a second module)
      'qp'  [BT, nq] float32, 'xg' [BT, D]: (x0 (.) gamma_cross) Wq_e and x0 (.) gamma_cross, x0 = the stream entering
            the layer (handles with the folded projection only; written on the passes that fold)
      'g'   [M, F]         the gated product          'x'  [M, D]  the residual stream after the MLP
      'ssq' [M, D / 32]    partial sums of x^2 per row: the slots ADD UP to sum x^2; which columns a slot covers depends
                           on the producing tile's width (32 columns each where D has no 48-column tiling; spare slots 0)
      'y'   [M, D]         x (.) gamma_decoder_norm, un-normalised (the consumer applies 1 / rms)
      'eps' [M, 128]       the model output of every pass."""
    n = ctypes.c_int64()
    probe = np.zeros(1, np.float32)
    _check(self.lib, self.handle,
           self.lib.msd_debug_read(self.handle, buffer.encode(), probe.ctypes.data, 0, ctypes.byref(n)),
           'msd_debug_read')
    count = n.value if max_elems is None else min(n.value, max_elems)
    out = np.zeros(count, np.float32)
    _check(self.lib, self.handle,
           self.lib.msd_debug_read(self.handle, buffer.encode(), out.ctypes.data, count, ctypes.byref(n)),
           'msd_debug_read')
    return out

  def profile_steps(self, batch: int, n_steps: int, stream: int = 0) -> Dict[str, Tuple[float, int]]:
    names = ctypes.POINTER(ctypes.c_char_p)()
    ms = (ctypes.c_double * MAX_KERNEL_CLASSES)()
    launches = (ctypes.c_int64 * MAX_KERNEL_CLASSES)()
    _check(self.lib, self.handle,
           self.lib.msd_profile_steps(self.handle, batch, n_steps, ctypes.byref(names), ms,
                                      launches, stream), 'msd_profile_steps')
    out = {}
    i = 0
    while i < MAX_KERNEL_CLASSES and names[i]:
      out[names[i].decode()] = (float(ms[i]), int(launches[i]))
      i += 1
    return out


def row_keys(batch: int, seed, stream_id) -> Tuple[List[int], List[int]]:
  """(seeds, stream_ids) of a call with per-row keys: each argument a sequence of `batch` integers, or a scalar that
  is broadcast to every row."""
  def rows(v, what):
    v = [int(v)] * batch if np.isscalar(v) else [int(x) for x in v]
    if len(v) != batch:
      raise ValueError('%s has %d entries for a batch of %d' % (what, len(v), batch))
    return v
  return rows(seed, 'seed'), rows(stream_id, 'stream_id')


def _key_arrays(batch: int, seed, stream_id):
  """(per_row, seeds, stream_ids) as the entry points take a call's keys: two uint64 arrays, `batch` long for per-row keys
  (either argument a sequence; a scalar beside it is broadcast), else of the one key."""
  per_row = not (np.isscalar(seed) and np.isscalar(stream_id))
  seeds, stream_ids = row_keys(batch if per_row else 1, seed, stream_id)
  return per_row, (ctypes.c_uint64 * len(seeds))(*seeds), (ctypes.c_uint64 * len(seeds))(*stream_ids)


def _check_holds(name: str, t, want: int):
  """Tensor `name` (torch or NumPy) must hold `want` float32 values."""
  if t is None or int(np.prod(tuple(t.shape))) != want:
    raise ValueError('%s must hold %d float32 values: got %s' % (name, want, None if t is None else tuple(t.shape)))


def _check_rng(rng):
  if rng not in RNGS:
    raise ValueError('rng must be one of %s: %r' % (sorted(RNGS), rng))


def fill_normal(out, seed: int, stream_id: int, subseq: int, stream: int = 0):
  lib = load()
  rc = lib.msd_fill_normal(seed, stream_id, subseq, _ptr(out), out.numel(), stream)
  if rc:
    raise RuntimeError('msd_fill_normal failed (%d)' % rc)


def fill_normal_threefry(out, seed: int, fold: int = -1, stream: int = 0):
  """jax.random.normal(key, [out.numel()]) into the float32 device tensor `out`; key = PRNGKey(seed), or
  fold_in(PRNGKey(seed), fold) when fold >= 0."""
  lib = load()
  _op_check(lib.msd_fill_normal_threefry(seed, fold, _ptr(out), out.numel(), stream), 'msd_fill_normal_threefry')


def op_threefry(stage: int, out, seed: int = 0, fold: int = -1, bits_in=None, stream: int = 0):
  """The stages of that draw into `out` (4-byte elements): 0 = raw bits, 1 = uniform, 2 = normal, 3 = the normal stage's
  -log1p(-u*u); bits_in (int32 /
  uint32 device words, same count): stages 1 / 2 of the caller's words instead."""
  lib = load()
  if bits_in is not None and bits_in.numel() != out.numel():
    raise ValueError('bits_in and out must have the same element count')
  _op_check(lib.msd_op_threefry(stage, seed, fold, _ptr(bits_in), _ptr(out), out.numel(), stream), 'msd_op_threefry')


def op_gemm_h16(precision: str, a, w, c, stream: int = 0):
  """C = A.W with 16-bit operand planes in the format `precision` names."""
  lib = load(plane_format(precision))
  m, k = a.shape
  n = w.shape[1]
  rc = lib.msd_op_gemm_h16(PRECISIONS[precision], _ptr(a), _ptr(w), _ptr(c), m, n, k, stream)
  if rc:
    raise _EXC.get(rc, RuntimeError)('msd_op_gemm_h16 failed (%d)' % rc)


op_gemm_bf16 = op_gemm_h16   # ABI <= 2 name


def op_gemm_f32(a, w, c, stream: int = 0):
  lib = load()
  m, k = a.shape
  n = w.shape[1]
  rc = lib.msd_op_gemm_f32(_ptr(a), _ptr(w), _ptr(c), m, n, k, stream)
  if rc:
    raise _EXC.get(rc, RuntimeError)('msd_op_gemm_f32 failed (%d)' % rc)


def op_attention(precision: str, q, k, v, o, heads: int, n_keys_valid: Optional[int] = None,
                 stream: int = 0, qp: int = 0):
  """qp: query-side single-plane switches (bit 0: Q, bit 1: P); the decoder runs 'f16x3' with qp = 3."""
  lib = load(plane_format(precision))
  n_q, n_keys = q.shape[0], k.shape[0]
  nv = n_keys if n_keys_valid is None else n_keys_valid
  rc = lib.msd_op_attention_qp(PRECISIONS[precision], qp, _ptr(q), _ptr(k), _ptr(v), _ptr(o), n_q,
                               n_keys, nv, heads, stream)
  if rc:
    raise _EXC.get(rc, RuntimeError)('msd_op_attention failed (%d)' % rc)


def op_attention_split(precision: str, q, k, v, o, heads: int, ksplit: int, merge_in_launch: bool, repeats: int = 1,
                       n_keys_valid: Optional[int] = None, stream: int = 0, qp: int = 0):
  """op_attention with the key axis split over `ksplit` blocks per (head, query tile); the partials are merged by the
  separate merge launch or -- merge_in_launch -- inside the attention launch by the last block to arrive; `repeats`
  launches back to back (the in-launch merge's arrival counters must be zero again after each)."""
  lib = load(plane_format(precision))
  n_q, n_keys = q.shape[0], k.shape[0]
  nv = n_keys if n_keys_valid is None else n_keys_valid
  rc = lib.msd_op_attention_split(PRECISIONS[precision], qp, ksplit, int(bool(merge_in_launch)), repeats, _ptr(q), _ptr(k),
                                  _ptr(v), _ptr(o), n_q, n_keys, nv, heads, stream)
  if rc:
    raise _EXC.get(rc, RuntimeError)('msd_op_attention_split failed (%d)' % rc)


def op_attention_ex(precision: str, q, k, v, o, heads: int, ksplit: int = 1, merge_in_launch: bool = False, repeats: int = 1,
                    allow_qb4: bool = False, q_ssq=None, n_keys_valid: Optional[int] = None, stream: int = 0, qp: int = 0):
  """op_attention_split with the decoder's two other launch forms: allow_qb4 lets a launch of more than 256 64-row blocks
  (n_q % 128 == 0) run on 128-row blocks; q_ssq (float32 [n_q, q_tiles] on the device) makes the queries UN-normalised,
  row r's logits scaled by 1 / sqrt(sum(q_ssq[r]) / (32 q_tiles) + 1e-6)."""
  lib = load(plane_format(precision))
  n_q, n_keys = q.shape[0], k.shape[0]
  nv = n_keys if n_keys_valid is None else n_keys_valid
  q_tiles = 0 if q_ssq is None else q_ssq.shape[1]
  if q_ssq is not None and tuple(q_ssq.shape) != (n_q, q_tiles):
    raise ValueError('q_ssq must be [n_q, q_tiles]')
  rc = lib.msd_op_attention_ex(PRECISIONS[precision], qp, ksplit, int(bool(merge_in_launch)), repeats, int(bool(allow_qb4)),
                               None if q_ssq is None else _ptr(q_ssq), q_tiles, _ptr(q), _ptr(k), _ptr(v), _ptr(o), n_q,
                               n_keys, nv, heads, stream)
  if rc:
    raise _EXC.get(rc, RuntimeError)('msd_op_attention_ex failed (%d)' % rc)


def op_attention_launch(precision: str, stream: int = 0, planes: Optional[str] = None, **fields) -> Dict[str, int]:
  """One attention launch the way the decoder fills it (msd_op_attention_launch).  `fields`: the members of
  msd_attention_launch_args by name -- integers, and device tensors for the pointers (float32; n_keys int32), kept alive
  by the caller.  Defaults: one launch, no split, qp 0.  Returns the ran_* out-fields."""
  lib = load(planes or plane_format(precision))
  args = _attention_launch_args(precision, fields)
  rc = lib.msd_op_attention_launch(ctypes.byref(args), stream)
  if rc:
    raise _EXC.get(rc, RuntimeError)('msd_op_attention_launch failed (msd_status %d)' % rc)
  return {n: getattr(args, n) for n in AttentionLaunchArgs._INTS if n.startswith('ran_')}


def _attention_launch_args(precision, fields) -> AttentionLaunchArgs:
  args = AttentionLaunchArgs()
  args.struct_size = ctypes.sizeof(AttentionLaunchArgs)
  args.precision = PRECISIONS[precision]
  args.repeats = args.ksplit = 1
  for name, value in fields.items():
    if name in AttentionLaunchArgs._PTRS:
      setattr(args, name, _ptr(value))
    elif name in AttentionLaunchArgs._INTS and not name.startswith('ran_') and name != 'precision':
      setattr(args, name, int(value))
    else:
      raise TypeError('msd_attention_launch_args has no input field %r' % name)
  return args


def _carrier_args(form, n_touch, delay, target_rows, target_k) -> CarrierArgs:
  ca = CarrierArgs()
  ca.struct_size = ctypes.sizeof(CarrierArgs)
  ca.form = CARRIER_FORMS.get(form, form)
  ca.n_touch, ca.delay, ca.target_rows, ca.target_k = int(n_touch), int(delay), int(target_rows), int(target_k)
  return ca


def op_attention_launch_carrier(precision: str, form, n_touch: int = 0, delay: int = 0, target_rows: int = 0,
                                target_k: int = 0, stream: int = 0, **fields) -> Dict[str, int]:
  """op_attention_launch with a weight target the op makes itself -- two planes [target_rows][target_k] in one allocation
  of exactly their size -- carried in `form`: 'none' (no target), 'wave' (the in-block prefetch wave) or 'blocks'
  (`n_touch` touch blocks behind the compute grid, `delay` sleep rounds in front of their touches).  The status is
  RETURNED (key 'status', 0 = MSD_OK) next to the ran_* out-fields of both structs."""
  lib = load(plane_format(precision))
  args = _attention_launch_args(precision, fields)
  ca = _carrier_args(form, n_touch, delay, target_rows, target_k)
  rc = lib.msd_op_attention_launch_carrier(ctypes.byref(args), ctypes.byref(ca), stream)
  out = {n: getattr(args, n) for n in AttentionLaunchArgs._INTS if n.startswith('ran_')}
  out.update({n: getattr(ca, n) for n in CarrierArgs._INTS if n.startswith('ran_')}, status=rc)
  return out


def op_touch_deal(target_bytes: int, row_bytes: int, row_pitch: int, waves: int) -> np.ndarray:
  """How a target is dealt over `waves` touching waves (msd_op_touch_deal; host only, no GPU): int32
  [waves, touches per wave, 3] of (first row, rows, 128-byte lines per row); rows 0 = that touch covers nothing."""
  lib = load()
  per_wave = 12
  while True:
    buf = np.zeros(waves * per_wave * 3, np.int32)
    rc = lib.msd_op_touch_deal(target_bytes, row_bytes, row_pitch, waves, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), buf.size)
    if rc == -MSD_ERR_INVALID_ARGUMENT and per_wave < 64:   # (a library that deals more touches per wave: a larger buffer)
      per_wave *= 2
      continue
    if rc <= 0:
      raise _EXC.get(-rc, RuntimeError)('msd_op_touch_deal failed (msd_status %d)' % -rc)
    return buf[:waves * rc * 3].reshape(waves, rc, 3)


def _op_check(rc, what):
  if rc:
    raise _EXC.get(rc, RuntimeError)('%s failed (msd_status %d)' % (what, rc))


def op_sampler_step(cfg: MsdConfig, step_index: int, z, out_cond, out_uncond, noise, z_out, stream: int = 0):
  """One sampler update (msd_op_sampler_step).  Tensors: float32 device tensors of equal numel."""
  lib = load()
  cfg.struct_size = config_struct_size(lib)
  _op_check(lib.msd_op_sampler_step(ctypes.byref(cfg), step_index, _ptr(z), _ptr(out_cond), _ptr(out_uncond),
                                    _ptr(noise), _ptr(z_out), z.numel(), stream), 'msd_op_sampler_step')


def op_sampler_step_keep(cfg: MsdConfig, step_index: int, z, out_cond, out_uncond, noise, known_scaled, keep_mask,
                         z_out, stream: int = 0):
  """op_sampler_step with known frames (msd_op_sampler_step_keep): known_scaled float32 [..., frames, n_dims] in model
  units, keep_mask int32 device tensor with one flag per frame."""
  lib = load()
  cfg.struct_size = config_struct_size(lib)
  n_dims = int(known_scaled.shape[-1])
  if known_scaled.numel() != z.numel() or keep_mask.numel() * n_dims != z.numel():
    raise ValueError('known_scaled must have z\'s element count and keep_mask one flag per frame of %d' % n_dims)
  _op_check(lib.msd_op_sampler_step_keep(ctypes.byref(cfg), step_index, _ptr(z), _ptr(out_cond), _ptr(out_uncond),
                                         _ptr(noise), _ptr(known_scaled), _ptr(keep_mask), n_dims, _ptr(z_out), z.numel(),
                                         stream), 'msd_op_sampler_step_keep')


def op_sampler_step_release(cfg: MsdConfig, step_index: int, z, out_cond, out_uncond, noise, known_scaled, release,
                            z_out, stream: int = 0):
  """op_sampler_step_keep with release words (msd_op_sampler_step_release): release int32 device tensor, one word per
  frame -- 0 = free, v >= 1 = known at scan indices >= v - 1."""
  lib = load()
  cfg.struct_size = config_struct_size(lib)
  n_dims = int(known_scaled.shape[-1])
  if known_scaled.numel() != z.numel() or release.numel() * n_dims != z.numel():
    raise ValueError('known_scaled must have z\'s element count and release one word per frame of %d' % n_dims)
  _op_check(lib.msd_op_sampler_step_release(ctypes.byref(cfg), step_index, _ptr(z), _ptr(out_cond), _ptr(out_uncond),
                                            _ptr(noise), _ptr(known_scaled), _ptr(release), n_dims, _ptr(z_out), z.numel(),
                                            stream), 'msd_op_sampler_step_release')


def op_sampler_step_guided(cfg: MsdConfig, step_index: int, z, out_cond, out_uncond, noise, weights, z_out, stream: int = 0):
  """op_sampler_step in the guided form (msd_op_sampler_step_guided): z is [rows, ...] and row b combines with weights[b]
  (host floats) in cfg.cfg_weight's place; a row's element count must be a multiple of 1024."""
  lib = load()
  cfg.struct_size = config_struct_size(lib)
  w = (ctypes.c_float * len(weights))(*[float(x) for x in weights])
  _op_check(lib.msd_op_sampler_step_guided(ctypes.byref(cfg), step_index, _ptr(z), _ptr(out_cond), _ptr(out_uncond),
                                           _ptr(noise), w, len(weights), _ptr(z_out), z.numel(), stream),
            'msd_op_sampler_step_guided')
  return z_out


def op_sampler_step_multistep_guided(cfg: MsdConfig, step_index: int, z, out_cond, out_uncond, x0_prev, first: bool, weights,
                                     z_out, stream: int = 0):
  """op_sampler_step_multistep in the guided form (msd_op_sampler_step_multistep_guided); weights as op_sampler_step_guided."""
  lib = load()
  cfg.struct_size = config_struct_size(lib)
  w = (ctypes.c_float * len(weights))(*[float(x) for x in weights])
  _op_check(lib.msd_op_sampler_step_multistep_guided(ctypes.byref(cfg), step_index, _ptr(z), _ptr(out_cond), _ptr(out_uncond),
                                                     _ptr(x0_prev), int(bool(first)), w, len(weights), _ptr(z_out), z.numel(),
                                                     stream), 'msd_op_sampler_step_multistep_guided')
  return z_out


def op_sampler_step_multistep(cfg: MsdConfig, step_index: int, z, out_cond, out_uncond, x0_prev, first: bool, z_out,
                              stream: int = 0):
  """One update of the 'dpmpp_2m' sampler (msd_op_sampler_step_multistep): x0_prev float32 device tensor of z's element
  count, the previous step's pred_x0 on entry (not read when `first`) and this step's on return."""
  lib = load()
  cfg.struct_size = config_struct_size(lib)
  if x0_prev.numel() != z.numel() or z_out.numel() != z.numel():
    raise ValueError('x0_prev and z_out must have z\'s element count')
  _op_check(lib.msd_op_sampler_step_multistep(ctypes.byref(cfg), step_index, _ptr(z), _ptr(out_cond), _ptr(out_uncond),
                                              _ptr(x0_prev), int(bool(first)), _ptr(z_out), z.numel(), stream),
            'msd_op_sampler_step_multistep')


def op_sampler_step_planes(cfg: MsdConfig, step_index: int, z, out_cond, out_uncond, z_out, z_planes_out, noise=None,
                           known_scaled=None, keep_mask=None, release=None, x0_prev=None, first: bool = False, weights=None,
                           stream: int = 0):
  """One sampler update in any form of the op_sampler_step* functions above, with z_out's operand planes of cfg.precision
  merged back to float32 in z_planes_out (msd_op_sampler_step_planes; the library of cfg.precision's plane format runs it).
  The form follows from the arguments: known_scaled with keep_mask (flags) or release (words) = known frames; x0_prev
  (and first) = the multistep update; weights (host floats, one per row) = guided.  Returns (range flag word, the scan
  index the launch published); RangeError when the flag was set."""
  lib = load(_PLANES_OF[cfg.precision])
  cfg.struct_size = config_struct_size(lib)
  if not (z.numel() == out_cond.numel() == z_out.numel() == z_planes_out.numel()):
    raise ValueError('z, out_cond and the two outputs must have the same element count')
  if (keep_mask is not None) and (release is not None):
    raise ValueError('keep_mask (flags) or release (words), not both')
  a = SamplerPlanesArgs()
  a.struct_size = ctypes.sizeof(SamplerPlanesArgs)
  a.step_index, a.n, a.cfg = step_index, z.numel(), ctypes.pointer(cfg)
  a.z, a.out_cond, a.out_uncond, a.noise = _ptr(z), _ptr(out_cond), _ptr(out_uncond), _ptr(noise)
  if known_scaled is not None:
    a.known_scaled, a.n_dims = _ptr(known_scaled), int(known_scaled.shape[-1])
    a.keep, a.keep_is_flags = _ptr(keep_mask if keep_mask is not None else release), int(keep_mask is not None)
  if x0_prev is not None:
    a.x0_prev, a.first = _ptr(x0_prev), int(bool(first))
  if weights is not None:
    a.weights, a.rows = (ctypes.c_float * len(weights))(*[float(x) for x in weights]), len(weights)
  a.z_out, a.z_planes_out = _ptr(z_out), _ptr(z_planes_out)
  _op_check(lib.msd_op_sampler_step_planes(ctypes.byref(a), stream), 'msd_op_sampler_step_planes')
  return a.ran_range_flag, a.ran_next_step


def op_vocoder_phase(y, y_prev, mag, x_out, alpha: float, stream: int = 0):
  """The vocoder's phase update on the caller's rows (msd_op_vocoder_phase): y, y_prev, x_out float32 device tensors
  [rows, 1088], mag [rows, 544]; x_out = mag . U / |U| with U = y - alpha y_prev."""
  rows = int(y.shape[0])
  if tuple(y.shape) != (rows, 1088) or y_prev.shape != y.shape or x_out.shape != y.shape or tuple(mag.shape) != (rows, 544):
    raise ValueError('y, y_prev and x_out must be [rows, 1088] and mag [rows, 544]')
  _op_check(load().msd_op_vocoder_phase(_ptr(y), _ptr(y_prev), _ptr(mag), _ptr(x_out), rows, float(alpha), stream),
            'msd_op_vocoder_phase')
  return x_out


def op_vocoder_load_spec(src, mag, x_out, normalise: bool, stream: int = 0):
  """The vocoder's spectrum loader on the caller's arrays (msd_op_vocoder_load_spec): src float32 device tensor
  [B, F, 2, 513], mag [B (F + 1), 544] or None, x_out [B (F + 1), 1088]."""
  b, f = int(src.shape[0]), int(src.shape[1])
  if tuple(src.shape) != (b, f, 2, 513) or tuple(x_out.shape) != (b * (f + 1), 1088) or \
      (mag is not None and tuple(mag.shape) != (b * (f + 1), 544)):
    raise ValueError('src must be [B, F, 2, 513], x_out [B (F + 1), 1088] and mag [B (F + 1), 544] or None')
  _op_check(load().msd_op_vocoder_load_spec(_ptr(src), _ptr(mag), _ptr(x_out), b, f, int(bool(normalise)), stream),
            'msd_op_vocoder_load_spec')
  return x_out


def op_invert_step(cfg: MsdConfig, step_index: int, z, out_cond, out_uncond, weights, z_out, z_planes_out, stream: int = 0):
  """One inversion update (msd_op_invert_step): z is [rows, ...] and row b combines with weights[b] (host floats); z_out =
  fmaf(b, eps, a * z) at step_index of cfg's tables and z_planes_out its operand planes of cfg.precision merged back to
  float32.  out_uncond: None if and only if every weight is 1.  A row's element count must be a multiple of 1024."""
  lib = load(_PLANES_OF[cfg.precision])
  cfg.struct_size = config_struct_size(lib)
  if not (z.numel() == out_cond.numel() == z_out.numel() == z_planes_out.numel()):
    raise ValueError('z, out_cond and the two outputs must have the same element count')
  w = (ctypes.c_float * len(weights))(*[float(x) for x in weights])
  _op_check(lib.msd_op_invert_step(ctypes.byref(cfg), step_index, _ptr(z), _ptr(out_cond), _ptr(out_uncond), w, len(weights),
                                   _ptr(z_out), _ptr(z_planes_out), z.numel(), stream), 'msd_op_invert_step')


def op_diffuse_to_step(cfg: MsdConfig, step_index: int, mel, eps, z_out, z_planes_out, xk_out, stream: int = 0):
  """The part-way start of msd_sample_edit on its own (msd_op_diffuse_to_step): mel (mel units) and eps in; z = alpha xk +
  sigma eps at step_index's noise level, z's operand planes of cfg.precision merged back to float32, and xk =
  scale_features(clip=True) of mel out.  float32 device tensors of equal numel (% 4 == 0)."""
  lib = load(_PLANES_OF[cfg.precision])
  cfg.struct_size = config_struct_size(lib)
  if not (mel.numel() == eps.numel() == z_out.numel() == z_planes_out.numel() == xk_out.numel()):
    raise ValueError('mel, eps and the three outputs must have the same element count')
  _op_check(lib.msd_op_diffuse_to_step(ctypes.byref(cfg), step_index, _ptr(mel), _ptr(eps), _ptr(z_out), _ptr(z_planes_out),
                                       _ptr(xk_out), mel.numel(), stream), 'msd_op_diffuse_to_step')


def op_diffusion_loss(cfg: MsdConfig, step_index: int, loss_type: str, loss_norm: str, o, z, x0, eps, mask, out, n_dims: int,
                      stream: int = 0):
  """diffusion_loss_kernel alone (msd_op_diffusion_loss): out [n / n_dims] = the per-frame loss of one pass's model output o
  at step_index of cfg's tables over the caller's z, x0 (model units), eps and mask (float [n / n_dims] or None); float32
  device tensors."""
  lib = load(_PLANES_OF.get(cfg.precision, 'f16'))
  cfg.struct_size = config_struct_size(lib)
  _op_check(lib.msd_op_diffusion_loss(ctypes.byref(cfg), step_index, LOSS_TYPES[loss_type], LOSS_NORMS[loss_norm], _ptr(o),
                                      _ptr(z), _ptr(x0), _ptr(eps), _ptr(mask), n_dims, _ptr(out), z.numel(), stream),
            'msd_op_diffusion_loss')


def op_renoise(cfg: MsdConfig, from_level: int, to_level: int, z, eps, z_out, z_planes_out, stream: int = 0):
  """The resampling jump of msd_sample_resample on its own (msd_op_renoise): z_out = fmaf(b, eps, a * z) from level
  from_level up to level to_level (a = alpha_to / alpha_from, b = sqrt(1 - a^2)) and z_out's operand planes of
  cfg.precision merged back to float32.  float32 device tensors of equal numel (% 4 == 0)."""
  lib = load(_PLANES_OF[cfg.precision])
  cfg.struct_size = config_struct_size(lib)
  if not (z.numel() == eps.numel() == z_out.numel() == z_planes_out.numel()):
    raise ValueError('z, eps and the two outputs must have the same element count')
  _op_check(lib.msd_op_renoise(ctypes.byref(cfg), from_level, to_level, _ptr(z), _ptr(eps), _ptr(z_out), _ptr(z_planes_out),
                               z.numel(), stream), 'msd_op_renoise')


def op_residual_norm_gemm(folded: bool, x_in, a, w1, gamma, film_scale, film_bias, w2, x_out, h_out,
                          stream: int = 0):
  lib = load()
  m, k = a.shape
  d, n = w2.shape
  _op_check(lib.msd_op_residual_norm_gemm(int(folded), _ptr(x_in), _ptr(a), _ptr(w1), _ptr(gamma),
                                          _ptr(film_scale), _ptr(film_bias), _ptr(w2), _ptr(x_out), _ptr(h_out),
                                          m, k, d, n, stream), 'msd_op_residual_norm_gemm')


def op_geglu(a, wi0, wi1, out, stream: int = 0):
  lib = load()
  m, k = a.shape
  _op_check(lib.msd_op_geglu(_ptr(a), _ptr(wi0), _ptr(wi1), _ptr(out), m, k, wi0.shape[1], stream), 'msd_op_geglu')


def op_qkv(a, wq, wk, wv, q, k_out, v, seg_len: int, stream: int = 0):
  lib = load()
  m, k = a.shape
  _op_check(lib.msd_op_qkv(_ptr(a), _ptr(wq), _ptr(wk), _ptr(wv), _ptr(q), _ptr(k_out), _ptr(v), m, k,
                           wq.shape[1], seg_len, stream), 'msd_op_qkv')


def op_final_proj(x, gamma, w, out, stream: int = 0):
  lib = load()
  m, d = x.shape
  _op_check(lib.msd_op_final_proj(_ptr(x), _ptr(gamma), _ptr(w), _ptr(out), m, d, w.shape[1], stream),
            'msd_op_final_proj')


def gemm_site_tiles(precision: str, site) -> List[Tuple[int, ...]]:
  """The tiles of a launch site, from the library's tile table (msd_op_gemm_site_tiles): (bm, bn, ns) per tile; for a
  dual site (bm, bn, ns, bm2, bn2, ns2) per tile pair.  A site the precision does not have gives an empty list."""
  lib = load(plane_format(precision))
  site = GEMM_SITES.get(site, site)
  out = []
  bm, bn, ns = (ctypes.c_int32 * 2)(), (ctypes.c_int32 * 2)(), (ctypes.c_int32 * 2)()
  while True:
    rc = lib.msd_op_gemm_site_tiles(PRECISIONS[precision], site, len(out), bm, bn, ns)
    if rc == MSD_ERR_INVALID_ARGUMENT:   # past the last tile (or the last site)
      return out
    _op_check(rc, 'msd_op_gemm_site_tiles')
    out.append((bm[0], bn[0], ns[0]) + ((bm[1], bn[1], ns[1]) if bm[1] else ()))


def gemm_site_names(precision: str) -> List[str]:
  """The launch sites of `precision` in the library's order, named by the library from their types."""
  lib = load(plane_format(precision))
  out = []
  while True:
    name = lib.msd_op_gemm_site_name(PRECISIONS[precision], len(out))
    if not name:
      return out
    out.append(name.decode())


def op_gemm_site(precision: str, site, stream: int = 0, planes: Optional[str] = None, **fields) -> Dict[str, int]:
  """One launch site of the decoder through the product's dispatcher (msd_op_gemm_site).  `fields`: the members of
  msd_gemm_site_args by name -- integers, and float32 device tensors for the pointers (kept alive by the caller).
  Returns the ran_* out-fields and step_copy.  `planes` names the library build to call when it is not the one
  `precision` belongs to (which that build answers with MSD_ERR_UNSUPPORTED)."""
  lib = load(planes or plane_format(precision))
  args = _gemm_site_args(precision, site, fields)
  _op_check(lib.msd_op_gemm_site(ctypes.byref(args), stream), 'msd_op_gemm_site')
  return {n: getattr(args, n) for n in GemmSiteArgs._INTS if n.startswith('ran_') or n == 'step_copy'}


def _gemm_site_args(precision, site, fields) -> GemmSiteArgs:
  args = GemmSiteArgs()
  args.struct_size = ctypes.sizeof(GemmSiteArgs)
  args.precision = PRECISIONS[precision]
  args.site = GEMM_SITES.get(site, site)
  args.steps = 1
  for name, value in fields.items():
    if name in GemmSiteArgs._PTRS:
      setattr(args, name, _ptr(value))
    elif name in GemmSiteArgs._INTS and not name.startswith('ran_'):
      setattr(args, name, int(value))
    else:
      raise TypeError('msd_gemm_site_args has no input field %r' % name)
  return args


def op_gemm_site_carrier(precision: str, site, form, n_touch: int = 0, delay: int = 0, target_rows: int = 0,
                         target_k: int = 0, stream: int = 0, **fields) -> Dict[str, int]:
  """op_gemm_site with a weight target the op makes itself, carried in `form` (op_attention_launch_carrier).  The status
  is RETURNED (key 'status') next to the ran_* out-fields of both structs."""
  lib = load(plane_format(precision))
  args = _gemm_site_args(precision, site, fields)
  ca = _carrier_args(form, n_touch, delay, target_rows, target_k)
  rc = lib.msd_op_gemm_site_carrier(ctypes.byref(args), ctypes.byref(ca), stream)
  out = {n: getattr(args, n) for n in GemmSiteArgs._INTS if n.startswith('ran_') or n == 'step_copy'}
  out.update({n: getattr(ca, n) for n in CarrierArgs._INTS if n.startswith('ran_')}, status=rc)
  return out
