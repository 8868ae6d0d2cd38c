"""The specification of sampling with KNOWN frames (msd_sample_keep): the reference's eval_step.body
(models/diffusion/diffusion_utils.py:398-453, restated in oracle/sampler.py) with the two lines its
`# TODO(williamchan): Modify the sampler according to the mask.` (:438) leaves open, written from oracle.sampler's own
functions.  x0-replacement: after the CFG combine and after the clip_x0 branch, on the kept elements

    pred_x0  := xk
    pred_eps := predict_eps_from_x0(z_t, xk, logsnr_t)

and the ordinary ddpm_step / ddim_step.  TEST INFRASTRUCTURE: shared by tests/test_keep_frames_host.py and
tests/test_gpu_keep_frames.py."""
import numpy as np

from oracle import sampler as du


def eval_step_keep(xp, noise, diffusion_config, batch_size, pred_fn, xk, keep):
  """eval_step of oracle/sampler.py with the replacement; xk [B,T,n] the known mel in MODEL units, keep a boolean
  array that broadcasts against it (True = known)."""
  schedule = diffusion_config.sampler.schedule
  num_steps = schedule.num_steps

  def body(z_t, i):
    t = xp.full((batch_size,), 0.0) + (float(i) + 1.0)
    t = t / float(num_steps)
    s = (xp.full((batch_size,), 0.0) + float(i)) / float(num_steps)
    logsnr_t = du.get_logsnr_t(xp, t, schedule)
    logsnr_s = du.get_logsnr_t(xp, s, schedule)
    time = t

    model_output = pred_fn(z=z_t, time=time, include_conditioning=True)
    outputs = du.get_x0_and_eps_from_model_output(xp, z_t, time, model_output, diffusion_config)
    pred_eps, pred_x0 = outputs['eps'], outputs['x0']

    cond_wt = diffusion_config.classifier_free_guidance.eval_condition_weight
    if cond_wt != 1:
      uncond_wt = 1. - cond_wt
      uncond_model_output = pred_fn(z=z_t, time=time, include_conditioning=False)
      uncond_outputs = du.get_x0_and_eps_from_model_output(xp, z_t, time, uncond_model_output, diffusion_config)
      pred_eps = cond_wt * pred_eps + uncond_wt * uncond_outputs['eps']
      pred_x0 = du.predict_x0_from_eps(xp, z=z_t, eps=pred_eps, logsnr=logsnr_t)

    if diffusion_config.sampler.clip_x0:
      pred_x0 = xp.clip(pred_x0, -1.0, 1.0)
      pred_eps = du.predict_eps_from_x0(xp, z=z_t, x0=pred_x0, logsnr=logsnr_t)

    # the two lines of the TODO
    pred_x0 = xp.where(keep, xk, pred_x0)
    pred_eps = xp.where(keep, du.predict_eps_from_x0(xp, z=z_t, x0=xk, logsnr=logsnr_t), pred_eps)

    if diffusion_config.sampler.name == 'ddim':
      return du.ddim_step(xp, i, logsnr_s, logsnr_t, pred_x0, pred_eps)
    elif diffusion_config.sampler.name == 'ddpm':
      eps = None if noise is None else noise[i]
      return du.ddpm_step(xp, i, eps, logsnr_s, logsnr_t, pred_x0, z_t, diffusion_config.sampler.logvar_type)
    raise ValueError('Unknown sampler type: %s' % diffusion_config.sampler.name)

  return body


def eval_scan_keep(xp, init_z, noise, pred_fn, diffusion_config, xk, keep):
  """eval_scan of oracle/sampler.py over eval_step_keep."""
  step_fn = eval_step_keep(xp, noise, diffusion_config, init_z.shape[0], pred_fn, xk, keep)
  z = init_z
  for i in reversed(range(diffusion_config.sampler.schedule.num_steps)):
    z = step_fn(z, i)
  return z


def frame_mask(xp, keep_mask):
  """[B,T] flags -> boolean [B,T,1] in the backend's array type."""
  return xp.asarray(np.asarray(keep_mask)[..., None] != 0) != 0


def fast_pred_fn(fm):
  """oracle.fast.FastModel.decoder_pass as eval_step's pred_fn (time = (i + 1) / N names the scan index)."""
  n = fm.dc.sampler.schedule.num_steps

  def pred_fn(z, time, include_conditioning):
    i = int(round(float(time[0]) * n)) - 1
    return fm.decoder_pass(z, i, include_conditioning)
  return pred_fn


def encode(fm, batch):
  if fm.context:
    fm.encode(batch['encoder_input_tokens'], batch['encoder_continuous_inputs'], batch['encoder_continuous_mask'])
  else:
    fm.encode(batch['encoder_input_tokens'])


def predict_keep(fm, batch, init_z, noise, keep, keep_mask):
  """What InferenceModel.predict(batch, init_z=, noise=, keep=, keep_mask=) specifies, on an oracle.fast.FastModel:
  (decodes [B,T,n] in mel units as float64 NumPy, x0 [B,T,n] of the scan, xk).  The known mel enters as the context
  does (scale_features(clip=True)); the kept frames of the result are the caller's own values."""
  xp = fm.xp
  encode(fm, batch)
  keep = np.asarray(keep)
  xk = fm.codec.scale_features(xp, xp.asarray(keep), (-1., 1.), clip=True)
  kb = frame_mask(xp, keep_mask)
  x0 = eval_scan_keep(xp, xp.asarray(init_z), None if noise is None else xp.asarray(noise), fast_pred_fn(fm), fm.dc, xk, kb)
  dec = np.asarray(xp.to_numpy(fm.codec.scale_to_features(xp, x0, input_range=(-1., 1.))), np.float64)
  dec = np.where(np.asarray(keep_mask)[..., None] != 0, keep.astype(np.float64), dec)
  return dec, xp.to_numpy(x0), xp.to_numpy(xk)


# the masks of the parity cases: row 0 keeps [0, 24) and [50, 64), row 1 keeps [10, 33)
def parity_masks(batch, t=64):
  m = np.zeros((2, t), np.int32)
  m[0, :24] = 1
  m[0, 50:] = 1
  m[1, 10:33] = 1
  return m[:batch]
