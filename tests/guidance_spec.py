"""The specification of PER-CALL GUIDANCE (msd_sample_guided, predict(guidance=, guidance_interval=)), written from
oracle.sampler's functions.  TEST INFRASTRUCTURE: shared by tests/test_guidance_host.py and tests/test_gpu_guidance.py.

A call has per-row weights w[b] and an interval [g_lo, g_hi) in scan indices of its K steps:

  row b at scan index i = eval_step.body with eval_condition_weight = w[b]   if g_lo <= i < g_hi
                        = eval_step.body with eval_condition_weight = 1      otherwise

eval_step.body's own `cond_wt != 1` decides the branch, so a row whose weight is exactly 1 follows the == 1 branch inside
the interval too (no combine, pred_x0 NOT recomputed from eps at the sampler schedule), and "row b is its one-row call"
holds for every mix of weights.  'dpmpp_2m' is multistep_spec.step under the same per-step weight; x0_prev runs through the
interval's edges unchanged.

Nothing here but eval_step bodies (multistep_spec steps) of a dataclasses.replace'd config, evaluated on the whole batch
once per distinct weight of the step, and a row selection."""
import dataclasses

import numpy as np

from oracle import sampler as du
from tests import multistep_spec as ms


def with_weight(diffusion_config, w):
  """The oracle's DiffusionConfig with eval_condition_weight = w."""
  return dataclasses.replace(diffusion_config, classifier_free_guidance=dataclasses.replace(
      diffusion_config.classifier_free_guidance, eval_condition_weight=float(w)))


def step_weights(weights, g_lo, g_hi, i):
  """The weight every row runs scan index i with."""
  return [float(w) if g_lo <= i < g_hi else 1.0 for w in weights]


def _rows(xp, ws, by_weight):
  """Row b of the result is row b of by_weight[ws[b]]."""
  out = by_weight[ws[0]]
  for w in sorted(set(ws) - {ws[0]}):
    pick = xp.asarray(np.asarray([x == w for x in ws]).reshape((-1,) + (1,) * (out.ndim - 1))) != 0
    out = xp.where(pick, by_weight[w], out)
  return out


def scan(xp, init_z, noise, pred_fn, diffusion_config, weights, g_lo, g_hi, sampler=None):
  """The K-step scan (K = the config's num_steps) from init_z [B,T,n] with weights [B] in [g_lo, g_hi) -> x0.  sampler:
  None = the config's ('ddpm' / 'ddim'); 'dpmpp_2m' = the multistep form."""
  b = init_z.shape[0]
  k = diffusion_config.sampler.schedule.num_steps
  assert len(weights) == b and 0 <= g_lo <= g_hi <= k
  z, prev = init_z, None
  for i in reversed(range(k)):
    ws = step_weights(weights, g_lo, g_hi, i)
    zs, x0s = {}, {}
    for w in set(ws):
      cfg = with_weight(diffusion_config, w)
      if sampler == 'dpmpp_2m':
        zs[w], x0s[w] = ms.step(xp, cfg, z, i, pred_fn, prev, first=(i == k - 1))
      else:
        zs[w] = du.eval_step(xp, noise, cfg, b, pred_fn)(z, i)
    z = _rows(xp, ws, zs)
    if sampler == 'dpmpp_2m':
      prev = _rows(xp, ws, x0s)
  return z


def predict(fm, batch, init_z, noise, weights, g_lo, g_hi, sampler=None):
  """What predict(batch, init_z=, noise=, guidance=weights, <interval = [g_lo, g_hi)>, sampler=) specifies on an
  oracle.fast.FastModel whose config holds the call's step count: decodes [B,T,n] in mel units, float64 NumPy."""
  from tests import keep_spec
  xp = fm.xp
  keep_spec.encode(fm, batch)
  x0 = scan(xp, xp.asarray(init_z), None if noise is None else xp.asarray(noise), keep_spec.fast_pred_fn(fm), fm.dc,
            list(weights), g_lo, g_hi, sampler)
  return np.asarray(xp.to_numpy(fm.codec.scale_to_features(xp, x0, input_range=(-1., 1.))), np.float64)
