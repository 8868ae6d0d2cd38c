"""The specification of RESAMPLING JUMPS in the known-frame scan (msd_sample_resample, predict(keep=, resample=(jump, times))):
tests/edit_spec.py's scan with RePaint's schedule (Lugmayr et al. 2022) on top, written from oracle.sampler's functions.

A LEVEL L is the number of steps still to run: the step with scan index i takes level i + 1 to level i; a call starts at
level S = start_step + 1.  Block k = 0, 1, ... has top S - k jump and bottom max(top - jump, 0); every block is descended
`times` times, and after each descent but the last the state is diffused from the bottom level s back to the top level t,
one sample of q(z_t | z_s), known and free frames alike:

    z' = b * eps + (a * z),   a = alpha_t / alpha_s,  b = sqrt(1 - a^2),  alpha = sqrt(sigmoid(logsnr(L / N)))

(the device: a, b in double from the float32 table value and rounded once; the product a * z rounded, then one fused
multiply-add).  Whether a frame is known in a step is a function of the scan index alone (i >= f), in every descent.

PASS p is everything behind the call's p-th jump (pass 0: the call as it is keyed without resampling).  Every pass has a
generator key of its own; its jump draws what that key's initial draw would be, its steps what that key's steps would
draw (draw_keys).  TEST INFRASTRUCTURE: shared by tests/test_resample_host.py and tests/test_gpu_resample.py; the product
never imports it."""
import numpy as np

from oracle import sampler as du
from tests import edit_spec, keep_spec


def plan(start_step, jump, times):
  """The schedule, written out independently of the product's plan_resample: [('steps', top, bottom) | ('jump', bottom,
  top, p)], p = 1, 2, ... counting the call's jumps."""
  ops, p, top = [], 0, start_step + 1
  while top > 0:
    bottom = max(top - jump, 0)
    for r in range(times):
      ops.append(('steps', top, bottom))
      if r != times - 1:
        p += 1
        ops.append(('jump', bottom, top, p))
    top = bottom
  return ops


def level_alpha(xp, schedule, batch_size, level):
  """alpha [B] of a level: sqrt(sigmoid(logsnr)) of the SAMPLER schedule at time level / N (level L > 0: scan index
  L - 1's logsnr_t; level 0: scan index 0's logsnr_s)."""
  t = (xp.full((batch_size,), 0.0) + float(level)) / float(schedule.num_steps)
  return xp.sqrt(xp.sigmoid(du.get_logsnr_t(xp, t, schedule)))


def jump_coefs(xp, schedule, batch_size, from_level, to_level):
  """(a, b) [B] of the jump from_level -> to_level in the backend's type."""
  a = level_alpha(xp, schedule, batch_size, to_level) / level_alpha(xp, schedule, batch_size, from_level)
  return a, xp.sqrt(1.0 - a * a)


def jump_state(xp, diffusion_config, z, eps, from_level, to_level):
  """One sample of q(z_t | z_s): the state z at from_level diffused to to_level with the draw eps."""
  a, b = jump_coefs(xp, diffusion_config.sampler.schedule, z.shape[0], from_level, to_level)
  a = du.broadcast_to_shape_from_left(xp, a, z.shape)
  b = du.broadcast_to_shape_from_left(xp, b, z.shape)
  return b * eps + a * z


def eval_scan_resample(xp, z, pass_noise, pass_eps, pred_fn, diffusion_config, xk, f, start_step, jump, times):
  """edit_spec.eval_scan_edit with the schedule above.  pass_noise[p]: the step draws [N, B, T, n] of pass p, indexed by
  scan index (None: a sampler that draws nothing); pass_eps[p]: the draw of the p-th jump (pass_eps[0] is not read)."""
  f = np.asarray(f)
  p = 0
  for op in plan(start_step, jump, times):
    if op[0] == 'jump':
      p = op[3]
      z = jump_state(xp, diffusion_config, z, xp.asarray(pass_eps[p]), op[1], op[2])
      continue
    noise = None if pass_noise[p] is None else xp.asarray(pass_noise[p])
    for i in reversed(range(op[2], op[1])):
      keep = keep_spec.frame_mask(xp, (i >= f).astype(np.int32))
      z = keep_spec.eval_step_keep(xp, noise, diffusion_config, z.shape[0], pred_fn, xk, keep)(z, i)
  return z


def predict_resample(fm, batch, init_z, pass_noise, pass_eps, known, words, start_step, jump, times):
  """What predict(batch, keep=known, keep_mask= | strength=, resample=(jump, times)) specifies for the release words and
  start index of the call, on an oracle.fast.FastModel, with every pass's draws given: (decodes [B,T,n] in mel units as
  float64 NumPy, x0 of the scan, xk).  Frames with word 1 hold the caller's own values.  times == 1 reads pass 0 only
  and is edit_spec.predict_edit."""
  xp = fm.xp
  keep_spec.encode(fm, batch)
  known = np.asarray(known)
  words = np.asarray(words)
  xk = fm.codec.scale_features(xp, xp.asarray(known), (-1., 1.), clip=True)
  if start_step < 0:
    return known.astype(np.float64), xp.to_numpy(xk), xp.to_numpy(xk)
  f = edit_spec.free_steps(words, fm.dc.sampler.schedule.num_steps)
  z = edit_spec.start_state(xp, fm.dc, xk, xp.asarray(init_z), start_step)
  x0 = eval_scan_resample(xp, z, pass_noise, pass_eps, keep_spec.fast_pred_fn(fm), fm.dc, xk, f, start_step, jump, times)
  dec = np.asarray(xp.to_numpy(fm.codec.scale_to_features(xp, x0, input_range=(-1., 1.))), np.float64)
  dec = np.where((words == 1)[..., None], known.astype(np.float64), dec)
  return dec, xp.to_numpy(x0), xp.to_numpy(xk)


def n_passes(start_step, jump, times):
  """Passes of a call, pass 0 included: 1 + (times - 1) ceil(S / jump)."""
  s = start_step + 1
  return 1 + (times - 1) * (-(-s // jump)) if s > 0 else 1


def pass_key(rng, seed, stream_id, num_steps, p):
  """The generator key of pass p.  'philox': (seed, stream_id + (p << 32)) (stream_id < 2^32 for p > 0); 'threefry': the
  key words -- PRNGKey(seed) for pass 0, fold_in(PRNGKey(seed), N + p - 1) behind, the first fold indices the plain call
  (which folds 0 .. N - 1) leaves unused."""
  if rng == 'philox':
    if p > 0 and stream_id >> 32:
      raise ValueError('a call with resampling needs stream_id < 2^32')
    return (int(seed), int(stream_id) + (p << 32))
  from msd_amd import jax_random
  key = jax_random.prng_key(seed)
  return key if p == 0 else jax_random.fold_in(key, num_steps + p - 1)


def draw_keys(rng, seed, stream_id, num_steps, start_step, jump, times, draws_noise=True, init_given=False):
  """Every draw of a call, in order: [(p, kind, key, sub)] -- kind 'init' (pass 0's initial draw), 'jump' (the p-th jump's
  eps) or 'step' (one step's noise; none at scan index 0, which returns x0, and none for a sampler that draws nothing).
  'philox': sub is the sub-sequence under key = (seed, stream_id) -- 0 for 'init' / 'jump', 1 + i for step i.  'threefry':
  sub is None for 'init' / 'jump' (normal(key, shape)) and i for step i (normal(fold_in(key, i), shape))."""
  out = []
  if not init_given:
    out.append((0, 'init', pass_key(rng, seed, stream_id, num_steps, 0), 0 if rng == 'philox' else None))
  p = 0
  for op in plan(start_step, jump, times):
    if op[0] == 'jump':
      p = op[3]
      out.append((p, 'jump', pass_key(rng, seed, stream_id, num_steps, p), 0 if rng == 'philox' else None))
    elif draws_noise:
      key = pass_key(rng, seed, stream_id, num_steps, p)
      out.extend((p, 'step', key, 1 + i if rng == 'philox' else i) for i in reversed(range(max(op[2], 1), op[1])))
  return out
