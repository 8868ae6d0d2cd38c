"""The specification of deterministic DDIM INVERSION (msd_invert, msd_op_invert_step, InferenceModel.invert / rerender),
written from oracle.sampler's functions.  TEST INFRASTRUCTURE: shared by tests/test_invert_host.py and
tests/test_gpu_invert.py.

A call of K steps (K = the config's sampler.schedule.num_steps; tests/multistep_spec.py with_steps) has levels 0 .. K.  Level
l has time l / K, logsnr_l of the SAMPLER schedule, alpha_l = sqrt(sigmoid(logsnr_l)), sigma_l = sqrt(sigmoid(-logsnr_l)).

The forward DDIM step at scan index i takes level i + 1 to level i: z_i = alpha_i x0 + sigma_i eps with (x0, eps) of
eval_step.body at time (i + 1) / K; index 0 returns x0.

The inverse step at index i = 0 .. K - 1 is one evaluation OF THE STATE IT HAS (level i) at the UPPER level's time, no draw:

    u     = z at level i           (level 0: scale_features(clip=True) of the caller's mel)
    eps   = body's pred_eps(u, time (i + 1) / K): model output -> eps at the TRAIN schedule, w eps_c + (1 - w) eps_u when
            w != 1.  NO clip: it is not invertible where it binds; sampler.clip_x0 is ignored.
    z_up  = a_i u + b_i eps
    a_i = alpha_{i+1} / alpha_i,  b_i = sigma_{i+1} - a_i sigma_i     (i >= 1)
    a_0 = alpha_1,                b_0 = sigma_1                       (the mirror of "index 0 returns x0")

With eps FROZEN (the eps the forward step used) this is the forward step's exact inverse: z_{i+1} = alpha_{i+1} x0 +
sigma_{i+1} eps and x0 = (z_i - sigma_i eps) / alpha_i -- where train and sampler schedule agree at t, which is where the
forward step's eps and x0 are tied by the sampler's alpha, sigma.  The result is z at level K, model units."""
import numpy as np

from oracle import sampler as du
from tests import guidance_spec as gs, multistep_spec as ms


def coefficients(xp, diffusion_config, batch_size, i):
  """(a_i, b_i) [B] of scan index i."""
  lt, ls = ms.logsnrs(xp, diffusion_config, batch_size, i)
  alpha_t, sigma_t = xp.sqrt(xp.sigmoid(lt)), xp.sqrt(xp.sigmoid(-lt))
  if i == 0:
    return alpha_t, sigma_t
  alpha_s, sigma_s = xp.sqrt(xp.sigmoid(ls)), xp.sqrt(xp.sigmoid(-ls))
  a = alpha_t / alpha_s
  return a, sigma_t - a * sigma_s


def pred_eps(xp, diffusion_config, u, i, pred_fn):
  """eval_step.body's pred_eps of the state u at time (i + 1) / K (oracle/sampler.py): conversion at the train schedule, CFG
  combine; no clip."""
  n = diffusion_config.sampler.schedule.num_steps
  b = u.shape[0]
  time = (xp.full((b,), 0.0) + (float(i) + 1.0)) / float(n)
  eps = du.get_x0_and_eps_from_model_output(xp, u, time, pred_fn(z=u, time=time, include_conditioning=True),
                                            diffusion_config)['eps']
  w = diffusion_config.classifier_free_guidance.eval_condition_weight
  if w != 1:
    un = du.get_x0_and_eps_from_model_output(xp, u, time, pred_fn(z=u, time=time, include_conditioning=False),
                                             diffusion_config)
    eps = w * eps + (1. - w) * un['eps']
  return eps


def step(xp, diffusion_config, u, i, pred_fn, eps=None):
  """One step up, level i -> i + 1.  eps: a frozen eps instead of the model's (the exact-inverse identity)."""
  if eps is None:
    eps = pred_eps(xp, diffusion_config, u, i, pred_fn)
  a, b = (du.broadcast_to_shape_from_left(xp, c, u.shape) for c in coefficients(xp, diffusion_config, u.shape[0], i))
  return a * u + b * eps


def scan(xp, x0, pred_fn, diffusion_config, weights=None):
  """The K-step inversion chain from x0 [B,T,n] (model units) -> z at level K.  weights: one per row, or None = the
  config's own for every row."""
  z = x0
  for i in range(diffusion_config.sampler.schedule.num_steps):
    if weights is None:
      z = step(xp, diffusion_config, z, i, pred_fn)
    else:
      ws = [float(w) for w in weights]
      z = gs._rows(xp, ws, {w: step(xp, gs.with_weight(diffusion_config, w), z, i, pred_fn) for w in set(ws)})
  return z


def forward_scan(xp, init_z, pred_fn, diffusion_config, weights=None):
  """The K-step DDIM scan from init_z -> x0, the config's sampler taken as 'ddim' (the render of a round trip)."""
  import dataclasses
  dc = dataclasses.replace(diffusion_config, sampler=dataclasses.replace(diffusion_config.sampler, name='ddim'))
  k = dc.sampler.schedule.num_steps
  ws = [dc.classifier_free_guidance.eval_condition_weight] * init_z.shape[0] if weights is None else list(weights)
  return gs.scan(xp, init_z, None, pred_fn, dc, ws, 0, k)


def invert(fm, batch, mel, weights):
  """What InferenceModel.invert(batch + decoder_target_tokens = mel, steps = K, guidance = weights) specifies on an
  oracle.fast.FastModel whose config holds the call's step count: the noise [B,T,n] in model units, float64 NumPy."""
  from tests import keep_spec
  xp = fm.xp
  keep_spec.encode(fm, batch)
  x0 = fm.codec.scale_features(xp, xp.asarray(np.asarray(mel)), (-1., 1.), clip=True)
  z = scan(xp, x0, keep_spec.fast_pred_fn(fm), fm.dc, list(weights))
  return np.asarray(xp.to_numpy(z), np.float64)


def round_trip(fm, batch, mel, weights):
  """invert, then the K-step DDIM render from that noise under the same weights: (noise, decodes in mel units), float64."""
  from tests import keep_spec
  xp = fm.xp
  keep_spec.encode(fm, batch)
  pred_fn = keep_spec.fast_pred_fn(fm)
  x0 = fm.codec.scale_features(xp, xp.asarray(np.asarray(mel)), (-1., 1.), clip=True)
  z = scan(xp, x0, pred_fn, fm.dc, list(weights))
  back = forward_scan(xp, z, pred_fn, fm.dc, list(weights))
  dec = fm.codec.scale_to_features(xp, back, input_range=(-1., 1.))
  return np.asarray(xp.to_numpy(z), np.float64), np.asarray(xp.to_numpy(dec), np.float64)


# ---- the closed-form case: per-element Gaussian data, ideal denoiser (multistep_spec.ideal_pred_fn) -----------------
def exact_top_point(x, var=ms.DATA_VAR):
  """The probability-flow ODE's solution at t = 1 from x at t = 0: x sqrt(alpha_1^2 var + sigma_1^2) / sqrt(var), float64
  (the inverse of multistep_spec.exact_end_point)."""
  l1 = np.float64(-20.0)
  a1, s1 = 1.0 / (1.0 + np.exp(-l1)), 1.0 / (1.0 + np.exp(l1))   # alpha_1^2, sigma_1^2
  return np.asarray(x, np.float64) * np.sqrt(a1 * var + s1) / np.sqrt(var)
