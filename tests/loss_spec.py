"""The denoising loss (InferenceModel.loss, msd_loss) restated over oracle/: the reference's evaluation loss --
models.py loss_fn over diffusion_utils.get_diffusion_training_input and calculate_loss -- at a time index of the model's
step grid, with dropout off and the time and the noise given instead of drawn:

    x0    = scale_features(target, clip=True)
    z_t   = alpha x0 + sigma eps,  (alpha, sigma) = sqrt(sigmoid(+-logsnr)) of the TRAIN schedule at t = (i + 1) / N
    o     = one decoder pass on z_t at that time, conditional or unconditional
    (eps_hat, x0_hat) = get_x0_and_eps_from_model_output(z_t, t, o)
    loss  = |d| or d^2 of x0_hat - x0, eps_hat - eps, their maximum or their sum, times mask[b, t], summed over the frame

Every function takes a backend of oracle/backend.py, so the same text runs in float64 (the reference the fixtures of
tests/golden/ref_loss_*.npz pin it to) and in float32 (the yardstick of the device tests)."""
import numpy as np

from oracle import predict as opredict
from oracle import sampler as du

LOSS_TYPES = ('x0', 'eps', 'max_x0_eps', 'x0_and_eps')
LOSS_NORMS = ('l1', 'l2')
CONDITIONINGS = ('cond', 'uncond')


def time_of(xp, i, num_steps, batch):
  """t = (i + 1) / N as the sampler's body computes it (float32 scalars in the reference)."""
  return (xp.full((batch,), 0.0) + (float(i) + 1.0)) / float(num_steps)


def diffuse(xp, dc, x0, eps, i, num_steps):
  """diffusion_forward (diffusion_utils.py:109-117) at the train schedule's log-SNR: z_t = mean + std * eps."""
  logsnr = du.broadcast_to_shape_from_left(xp, du.get_logsnr_t(xp, time_of(xp, i, num_steps, x0.shape[0]), dc.train_schedule),
                                           x0.shape)
  return xp.sqrt(xp.sigmoid(logsnr)) * x0 + xp.sqrt(xp.sigmoid(-logsnr)) * eps


def element_losses(xp, dc, z, o, x0, eps, i, num_steps, loss_type, loss_norm):
  """calculate_loss (diffusion_utils.py:325-366) for one (loss_type, loss_norm): per element, unmasked."""
  out = du.get_x0_and_eps_from_model_output(xp, z, time_of(xp, i, num_steps, z.shape[0]), o, dc)

  def norm(a, b):
    if loss_norm == 'l1':
      return abs(a - b)
    if loss_norm == 'l2':
      return (a - b) * (a - b)
    raise ValueError('Unknown diffusion loss norm: %s' % loss_norm)
  x0_loss, eps_loss = norm(out['x0'], x0), norm(out['eps'], eps)
  if loss_type == 'x0':
    return x0_loss
  if loss_type == 'eps':
    return eps_loss
  if loss_type == 'max_x0_eps':
    return xp.maximum(x0_loss, eps_loss)
  if loss_type == 'x0_and_eps':
    return eps_loss + x0_loss
  raise ValueError('Unknown diffusion loss_type: %s' % loss_type)


def frame_losses(xp, dc, z, o, x0, eps, mask, i, num_steps, loss_type, loss_norm):
  """loss * mask[..., None] summed over the frame's elements: [B, T] as NumPy."""
  l = element_losses(xp, dc, z, o, x0, eps, i, num_steps, loss_type, loss_norm)
  return xp.to_numpy(xp.sum(l * xp.expand_dims(mask, -1), -1))


def op_frame_losses(dtype, dc, z, o, x0, eps, mask, i, num_steps, loss_type, loss_norm):
  """frame_losses over NumPy inputs in `dtype` ('float64' / 'float32'): what msd_op_diffusion_loss computes."""
  from oracle import backend
  xp = backend.TorchBackend(dtype, threads=1)
  a = [xp.asarray(np.asarray(v, dtype)) for v in (z, o, x0, eps, mask)]
  return frame_losses(xp, dc, a[0], a[1], a[2], a[3], a[4], i, num_steps, loss_type, loss_norm)


def encode(fm, batch):
  if fm.context:
    fm.encode(batch['encoder_input_tokens'], batch['encoder_continuous_inputs'], batch['encoder_continuous_mask'])
  else:
    fm.encode(batch['encoder_input_tokens'])


def evaluate(xp, fm, dc, target, mask, eps, i, combos=None):
  """One evaluation at index i on an ENCODED oracle model (oracle/fast.py FastModel; encode() above): per-frame masked
  losses {(conditioning, loss_type, loss_norm): [B, T]} for both conditioning forms, plus z_t under the key 'z'."""
  num_steps = dc.sampler.schedule.num_steps
  x0 = opredict.MelGANCodec().scale_features(xp, xp.asarray(target), (-1., 1.), clip=True)
  e, m = xp.asarray(eps), xp.asarray(mask)
  z = diffuse(xp, dc, x0, e, i, num_steps)
  out = {'z': xp.to_numpy(z)}
  for cond in CONDITIONINGS:
    o = fm.decoder_pass(z, i, cond == 'cond')
    for lt, ln in (combos or [(a, b) for a in LOSS_TYPES for b in LOSS_NORMS]):
      out[(cond, lt, ln)] = frame_losses(xp, dc, z, o, x0, e, m, i, num_steps, lt, ln)
  return out


# ---- the cases of tests/golden/ref_loss_<case>.npz (make_ref_loss_golden.py) and of the device tests ---------------------
CASES = ('tiny_ddpm', 'tiny_context_ddpm', 'tiny_context_v_small', 'tiny_context_x0_medium_noclip', 'tiny_context_linear')


def case_indices(num_steps):
  return (0, num_steps // 2, num_steps - 1)


def case_inputs(name):
  """(spec, params, batch, target, mask, eps [3, B, T, n]) of a fixture case: ref_cases' model and batch, helpers.known_mel
  as the target, the mask of row 1 zero on its last 19 frames, eps = the case's step noise at the three indices."""
  from tests import helpers, ref_cases
  spec, params, batch, init_z, noise = ref_cases.inputs(name)
  target = helpers.known_mel(init_z.shape)
  mask = np.ones(init_z.shape[:2], np.float32)
  mask[1, -19:] = 0.0
  idx = case_indices(spec.diffusion.sampler.schedule.num_steps)
  return spec, params, batch, target, mask, np.stack([noise[i] for i in idx], 0), idx


def fixture_key(cond, loss_type, loss_norm):
  return '%s__%s__%s' % (cond, loss_type, loss_norm)
