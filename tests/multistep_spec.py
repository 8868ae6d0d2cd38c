"""The specification of FEW-STEP rendering (msd_sample_steps, predict(steps=, sampler=)), written from oracle.sampler's
functions.  TEST INFRASTRUCTURE: shared by tests/test_few_steps_host.py and tests/test_gpu_few_steps.py.

1. A call of K steps on a model of N (K | N) is the reference's eval_scan with sampler.schedule.num_steps = K: times
   t = (j + 1) / K, s = j / K.  (j + 1) / K is the time of row r = (j + 1) N / K - 1 of the N-step tables: strided_rows.

2. sampler 'dpmpp_2m' is DPM-Solver++(2M) in data-prediction form (Lu et al. 2022, Algorithm 2).  With the half-log-SNR
   lambda = logsnr / 2, alpha = sqrt(sigmoid(logsnr)), sigma = sqrt(sigmoid(-logsnr)), h = lambda_s - lambda_t and
   r = h_prev / h (h_prev: h of the step before):

       D   = x0_t                                     on the first step of a call
       D   = (1 + 1/(2r)) x0_t - (1/(2r)) x0_prev     afterwards
       z_s = (sigma_s / sigma_t) z_t - alpha_s expm1(-h) D          scan index 0 returns x0_t, as ddim_step does

   x0_t is eval_step.body's pred_x0: after the model-output conversion, the CFG combine and the clip.  With D = x0_t the
   last line is ddim_step, rearranged (test_few_steps_host.py (a)).  No noise is drawn after init_z."""
import dataclasses

import numpy as np

from oracle import sampler as du


def strided_rows(num_steps, steps):
  """Rows of the N-step tables a K-step call reads, for j = 0 .. K - 1: (j + 1) N / K - 1."""
  assert num_steps % steps == 0
  return np.arange(1, steps + 1) * (num_steps // steps) - 1


def with_steps(diffusion_config, steps, name=None):
  """The oracle's DiffusionConfig with sampler.schedule.num_steps = steps.  A linear sampler schedule keeps its grid: the
  call evaluates the model's own schedule function (see msd_sample_steps), so only `cosine` may be re-configured here."""
  s = diffusion_config.sampler
  assert s.schedule.name == 'cosine' or steps == s.schedule.num_steps
  return dataclasses.replace(diffusion_config, sampler=dataclasses.replace(
      s, name=name or s.name, schedule=dataclasses.replace(s.schedule, num_steps=steps)))


def logsnrs(xp, diffusion_config, batch_size, i):
  """(logsnr_t, logsnr_s) [B] of scan index i, as eval_step.body computes them."""
  schedule = diffusion_config.sampler.schedule
  n = schedule.num_steps
  t = (xp.full((batch_size,), 0.0) + (float(i) + 1.0)) / float(n)
  s = (xp.full((batch_size,), 0.0) + float(i)) / float(n)
  return du.get_logsnr_t(xp, t, schedule), du.get_logsnr_t(xp, s, schedule)


def coefficients(xp, diffusion_config, batch_size, i):
  """The 2M coefficients of scan index i: (sigma_s / sigma_t, -alpha_s expm1(-h), 1 / (2r)) [B]; the last is 0 on the
  top row (no step before it)."""
  n = diffusion_config.sampler.schedule.num_steps
  lt, ls = logsnrs(xp, diffusion_config, batch_size, i)
  h = 0.5 * (ls - lt)
  c_z = xp.sqrt(xp.sigmoid(-ls)) / xp.sqrt(xp.sigmoid(-lt))
  c_d = -xp.sqrt(xp.sigmoid(ls)) * xp.expm1(-h)
  if i + 1 < n:
    lt_p, ls_p = logsnrs(xp, diffusion_config, batch_size, i + 1)
    hist = h / (2.0 * (0.5 * (ls_p - lt_p)))
  else:
    hist = 0.0 * h
  return c_z, c_d, hist


def pred_x0(xp, diffusion_config, z_t, i, pred_fn):
  """eval_step.body's pred_x0 (oracle/sampler.py): conversion at the train schedule, CFG combine, clip."""
  n = diffusion_config.sampler.schedule.num_steps
  b = z_t.shape[0]
  time = (xp.full((b,), 0.0) + (float(i) + 1.0)) / float(n)
  logsnr_t, _ = logsnrs(xp, diffusion_config, b, i)
  out = du.get_x0_and_eps_from_model_output(xp, z_t, time, pred_fn(z=z_t, time=time, include_conditioning=True),
                                            diffusion_config)
  eps, x0 = out['eps'], out['x0']
  w = diffusion_config.classifier_free_guidance.eval_condition_weight
  if w != 1:
    un = du.get_x0_and_eps_from_model_output(xp, z_t, time, pred_fn(z=z_t, time=time, include_conditioning=False),
                                             diffusion_config)
    eps = w * eps + (1. - w) * un['eps']
    x0 = du.predict_x0_from_eps(xp, z=z_t, eps=eps, logsnr=logsnr_t)
  if diffusion_config.sampler.clip_x0:
    x0 = xp.clip(x0, -1.0, 1.0)
  return x0


def step(xp, diffusion_config, z_t, i, pred_fn, x0_prev, first, history_weight=None):
  """One update at scan index i -> (z_s, x0_t).  first: no history (D = x0_t).  history_weight overrides 1 / (2r)
  (0.0 makes every step first-order)."""
  x0 = pred_x0(xp, diffusion_config, z_t, i, pred_fn)
  c_z, c_d, hist = coefficients(xp, diffusion_config, z_t.shape[0], i)
  if history_weight is not None:
    hist = 0.0 * hist + history_weight
  c_z, c_d, hist = (du.broadcast_to_shape_from_left(xp, c, z_t.shape) for c in (c_z, c_d, hist))
  d = x0 if first else (1.0 + hist) * x0 - hist * x0_prev
  z_s = c_z * z_t + c_d * d
  return (x0 if i == 0 else z_s), x0


def scan(xp, init_z, pred_fn, diffusion_config, history_weight=None):
  """The K-step scan from init_z (K = the config's num_steps) -> x0."""
  z, prev = init_z, None
  n = diffusion_config.sampler.schedule.num_steps
  for i in reversed(range(n)):
    z, prev = step(xp, diffusion_config, z, i, pred_fn, prev, first=(i == n - 1), history_weight=history_weight)
  return z


def predict(fm, batch, init_z):
  """What predict(batch, init_z=, sampler='dpmpp_2m') specifies on an oracle.fast.FastModel whose config holds the call's
  step count: decodes [B,T,n] in mel units, float64 NumPy."""
  from tests import keep_spec
  xp = fm.xp
  keep_spec.encode(fm, batch)
  x0 = scan(xp, xp.asarray(init_z), keep_spec.fast_pred_fn(fm), fm.dc)
  return np.asarray(xp.to_numpy(fm.codec.scale_to_features(xp, x0, input_range=(-1., 1.))), np.float64)


# ---- the closed-form case: per-element Gaussian data, ideal denoiser ------------------------------------------------
DATA_VAR = 0.09   # c^2


def ideal_x0(alpha, sigma, z, var=DATA_VAR):
  """E[x0 | z_t] for x0 ~ N(0, var): alpha var z / (alpha^2 var + sigma^2)."""
  return alpha * var * z / (alpha * alpha * var + sigma * sigma)


def ideal_pred_fn(xp, diffusion_config, model_output='eps'):
  """The ideal denoiser as eval_step's pred_fn for model_output 'eps' (cosine schedule: train == sampler log-SNR)."""
  assert model_output == 'eps'
  schedule = diffusion_config.sampler.schedule

  def pred_fn(z, time, include_conditioning):
    logsnr = du.broadcast_to_shape_from_left(xp, du.get_logsnr_t(xp, time, schedule), z.shape)
    alpha, sigma = xp.sqrt(xp.sigmoid(logsnr)), xp.sqrt(xp.sigmoid(-logsnr))
    return (z - alpha * ideal_x0(alpha, sigma, z)) / sigma
  return pred_fn


def exact_end_point(z1, var=DATA_VAR):
  """The probability-flow ODE's solution at t = 0 from z1 at t = 1: z1 sqrt(var) / sqrt(alpha_1^2 var + sigma_1^2), float64
  (alpha_0 = 1 and sigma_0 ~ 0: logsnr 20)."""
  l1 = np.float64(-20.0)
  a1, s1 = 1.0 / (1.0 + np.exp(-l1)), 1.0 / (1.0 + np.exp(l1))   # alpha_1^2, sigma_1^2
  return np.asarray(z1, np.float64) * np.sqrt(var) / np.sqrt(a1 * var + s1)
