"""Fixtures of the denoising loss produced by the REFERENCE's own code: tests/golden/ref_loss_<case>.npz.

Runs only in the build container (needs /root/reference), over the NumPy stand-in of jax + flax in ref_shim.py, float64,
with make_ref_golden.reference_model's objects.  For every case of tests/loss_spec.py CASES, at the time indices
(0, N // 2, N - 1) and for both conditioning forms, the statements of models.py loss_fn with dropout off and the time and the
noise given instead of drawn:

    targets = model.audio_codec.scale_features(target, output_range=[-1., 1.], clip=True)
    z_dist  = diffusion_utils.diffusion_forward(x0=targets, logsnr=get_logsnr_t(time, train_schedule) broadcast)
    z_t     = z_dist['mean'] + z_dist['std'] * eps
    output  = model.module.apply({'params': params}, encoder_input_tokens=tokens * include_conditioning, ...,
                                 decoder_input_tokens=z_t, decoder_noise_time=time, enable_dropout=False)
    loss    = diffusion_utils.calculate_loss(x0=targets, eps=eps, z=z_t, time=time, model_output=output, diffusion_config=dc)
    loss    = (loss * mask[..., None]).sum(-1)                       # per frame: loss_fn sums over everything

for all 4 loss types x 2 norms.  Stored per case: '<cond>__<type>__<norm>' float64 [3, B, T], the indices and a digest of the
inputs (tests/loss_spec.py case_inputs rebuilds them from seeds).

    python tests/golden/make_ref_loss_golden.py [case ...]      # default: all cases
"""
import dataclasses
import hashlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import ref_shim  # noqa: E402
import make_ref_golden  # noqa: E402
from tests import loss_spec  # noqa: E402


def digest(params, batch, target, mask, eps):
  h = hashlib.sha256()
  for k in sorted(params):
    h.update(k.encode())
    h.update(np.ascontiguousarray(params[k]).tobytes())
  for k in sorted(batch):
    h.update(k.encode())
    h.update(np.ascontiguousarray(batch[k]).tobytes())
  for a in (target, mask, eps):
    h.update(np.ascontiguousarray(a).tobytes())
  return h.hexdigest()[:16]


def run_case(ref, name):
  spec, params, batch, target, mask, eps, idx = loss_spec.case_inputs(name)
  ref_shim.WIDE = True
  model = make_ref_golden.reference_model(ref, spec)
  du = ref.diffusion_utils
  tree = make_ref_golden.nest(params)
  f64 = lambda a: np.asarray(a, np.float64)
  n_steps = spec.diffusion.sampler.schedule.num_steps
  t0 = time.time()
  targets = model.audio_codec.scale_features(f64(target), output_range=[-1., 1.], clip=True)
  out = {}
  for j, i in enumerate(idx):
    tm = np.full((target.shape[0],), (i + 1.0) / n_steps)
    logsnr = du.get_logsnr_t(tm, model.diffusion_config.train_schedule)
    z_dist = du.diffusion_forward(x0=targets, logsnr=du.broadcast_to_shape_from_left(logsnr, targets.shape))
    z_t = z_dist['mean'] + z_dist['std'] * f64(eps[j])
    for cond in loss_spec.CONDITIONINGS:
      flag = int(cond == 'cond')
      kw = dict(encoder_input_tokens=batch['encoder_input_tokens'] * flag)
      if spec.has_context:
        kw.update(encoder_continuous_inputs=model.audio_codec.scale_features(
            f64(batch['encoder_continuous_inputs']), output_range=[-1., 1.], clip=True),
                  encoder_continuous_mask=batch['encoder_continuous_mask'] * flag)
      output = model.module.apply({'params': tree}, decoder_input_tokens=z_t, decoder_noise_time=tm, enable_dropout=False, **kw)
      for lt in loss_spec.LOSS_TYPES:
        for ln in loss_spec.LOSS_NORMS:
          dc = dataclasses.replace(model.diffusion_config, loss_type=lt, loss_norm=ln)
          loss = du.calculate_loss(x0=targets, eps=f64(eps[j]), z=z_t, time=tm, model_output=output, diffusion_config=dc)
          frames = np.asarray(np.sum(np.asarray(loss) * f64(mask)[..., np.newaxis], axis=-1), np.float64)
          out.setdefault(loss_spec.fixture_key(cond, lt, ln), []).append(frames)
  out = {k: np.stack(v, 0) for k, v in out.items()}
  out['indices'] = np.asarray(idx, np.int32)
  out['digest'] = digest(params, batch, target, mask, eps)
  np.savez_compressed(os.path.join(HERE, 'ref_loss_%s.npz' % name), **out)
  print('%-32s %6.1fs  eps/l1 cond total %.6f  digest %s' % (
      name, time.time() - t0, float(out[loss_spec.fixture_key('cond', 'eps', 'l1')].sum()), out['digest']), flush=True)


def main():
  ref = ref_shim.load_models()
  for n in [a for a in sys.argv[1:] if not a.startswith('--')] or list(loss_spec.CASES):
    run_case(ref, n)


if __name__ == '__main__':
  main()
