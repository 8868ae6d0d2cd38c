"""The specification of EDIT STRENGTH (msd_sample_edit, predict(keep=, strength=)): an SDEdit-style restart of the sampler
with a per-frame release schedule on top of tests/keep_spec.py's x0-replacement, written from oracle.sampler's functions.

Every frame of every row carries the number f of FINAL scan steps during which it is free, 0 <= f <= N:

    keep(i) := (i >= f)      evaluated per step: known (x0-replacement, keep_spec.eval_step_keep) while the noise is high,
                             released to the sampler for scan indices f - 1 .. 0

and the scan runs over reversed(range(start_step + 1)) only, start_step = max f - 1: above it every frame is known.
Below N - 1 the start state is a direct sample of q(z_t | x0 = xk) at the start index (the reference's diffusion_forward,
models/diffusion/diffusion_utils.py:109-117), with the call's own initial draw as eps:

    z = sigma * eps + (alpha * xk),   alpha = sqrt(sigmoid(logsnr_t)), sigma = sqrt(sigmoid(-logsnr_t))

(the device: the product alpha * xk rounded, then one fused multiply-add).  f == 0 frames are the caller's mel in the
result; all others are what the scan made of them.  TEST INFRASTRUCTURE: shared by tests/test_edit_strength_host.py and
tests/test_gpu_edit_strength.py."""
import numpy as np

from oracle import sampler as du
from tests import keep_spec


def free_steps(words, num_steps):
  """Release words (0 = free throughout, v >= 1 = known at scan indices >= v - 1) -> f, int64 of the same shape."""
  words = np.asarray(words, np.int64)
  return np.where(words == 0, num_steps, words - 1)


def start_coefs(xp, diffusion_config, batch_size, start_step):
  """(alpha, sigma) [B] of the start index in the backend's type: sqrt(sigmoid(+-logsnr_t)) of the SAMPLER schedule."""
  schedule = diffusion_config.sampler.schedule
  t = (xp.full((batch_size,), 0.0) + (float(start_step) + 1.0)) / float(schedule.num_steps)
  logsnr_t = du.get_logsnr_t(xp, t, schedule)
  return xp.sqrt(xp.sigmoid(logsnr_t)), xp.sqrt(xp.sigmoid(-logsnr_t))


def start_state(xp, diffusion_config, xk, eps, start_step):
  """z at scan index start_step: eps itself for the full scan, else the known mel diffused to that step."""
  if start_step == diffusion_config.sampler.schedule.num_steps - 1:
    return eps
  alpha, sigma = start_coefs(xp, diffusion_config, xk.shape[0], start_step)
  alpha = du.broadcast_to_shape_from_left(xp, alpha, xk.shape)
  sigma = du.broadcast_to_shape_from_left(xp, sigma, xk.shape)
  return sigma * eps + alpha * xk


def eval_scan_edit(xp, z, noise, pred_fn, diffusion_config, xk, f, start_step):
  """eval_scan of oracle/sampler.py from start_step down, over eval_step_keep with keep := (i >= f) per step.
  f: integer NumPy array [B, T]."""
  f = np.asarray(f)
  for i in reversed(range(start_step + 1)):
    keep = keep_spec.frame_mask(xp, (i >= f).astype(np.int32))
    z = keep_spec.eval_step_keep(xp, noise, diffusion_config, z.shape[0], pred_fn, xk, keep)(z, i)
  return z


def predict_edit(fm, batch, init_z, noise, known, words, start_step):
  """What InferenceModel.predict(batch, init_z=, noise=, keep=known, strength=) specifies for the release words and start
  index plan_strength gives, on an oracle.fast.FastModel: (decodes [B,T,n] in mel units as float64 NumPy, x0 of the scan,
  xk).  Frames with word 1 (f == 0) hold the caller's own values."""
  xp = fm.xp
  keep_spec.encode(fm, batch)
  known = np.asarray(known)
  words = np.asarray(words)
  xk = fm.codec.scale_features(xp, xp.asarray(known), (-1., 1.), clip=True)
  if start_step < 0:
    return known.astype(np.float64), xp.to_numpy(xk), xp.to_numpy(xk)
  f = free_steps(words, fm.dc.sampler.schedule.num_steps)
  z = start_state(xp, fm.dc, xk, xp.asarray(init_z), start_step)
  x0 = eval_scan_edit(xp, z, None if noise is None else xp.asarray(noise), keep_spec.fast_pred_fn(fm), fm.dc, xk, f, start_step)
  dec = np.asarray(xp.to_numpy(fm.codec.scale_to_features(xp, x0, input_range=(-1., 1.))), np.float64)
  dec = np.where((words == 1)[..., None], known.astype(np.float64), dec)
  return dec, xp.to_numpy(x0), xp.to_numpy(xk)
