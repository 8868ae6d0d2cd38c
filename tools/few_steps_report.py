"""Measure few-step rendering on the GPU and write profiles/few_steps.json (run by hand; not a test):

  python tools/few_steps_report.py [--out profiles/few_steps.json] [--preset base_with_context] [--steps 1000]

One process, ONE model of `--steps` steps, one segment.  For K in {1000, 250, 100, 50, 20} (those that divide --steps)
and the samplers 'ddim' and 'dpmpp_2m', from the same init_z: the time of predict(steps=K, sampler=) from call to returned
device tensor (after one warm-up call of the same form: tables and step graphs are then in place), with the encode part
beside it, and the rms distance of the mel to the K = --steps DDIM mel of the same init_z.  Both samplers are solvers of the
same ODE, so that distance is the SOLVER's error on this network -- meaningful on synthetic weights, and no statement
about how anything sounds.  Expected time from the code: the encode part plus K / steps of the full call's sampling part."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

STEP_COUNTS = (1000, 250, 100, 50, 20)
SAMPLERS = ('ddim', 'dpmpp_2m')


def main(argv=None) -> int:
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'few_steps.json'))
  ap.add_argument('--preset', default='base_with_context')
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--repeats', type=int, default=3, help='timed calls of each form')
  args = ap.parse_args(argv)

  import numpy as np
  import torch
  import msd_amd
  assert torch.cuda.is_available(), 'needs a GPU'
  spec = msd_amd.config.preset(args.preset, num_steps=args.steps)
  t, n = spec.task_feature_lengths['targets'], 128
  model = msd_amd.InferenceModel('synthetic:0', spec)
  rng = np.random.default_rng(0)
  batch = {'encoder_input_tokens': msd_amd.synthetic.segment_tokens(spec, 1)}
  if spec.has_context:
    c = spec.task_feature_lengths['targets_context']
    batch['encoder_continuous_inputs'] = rng.uniform(-11.0, 4.0, (1, c, n)).astype(np.float32)
    batch['encoder_continuous_mask'] = np.ones((1, c), np.int32)
  init_z = torch.as_tensor(rng.standard_normal((1, t, n)).astype(np.float32)).to(model.device)
  counts = [k for k in STEP_COUNTS if k <= args.steps and args.steps % k == 0]
  if args.steps not in counts:
    counts.insert(0, args.steps)

  def timed(k, sampler):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, _ = model.predict(batch, init_z=init_z, steps=k, sampler=sampler, return_torch=True)
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0), 1e3 * model.last_timing['encode_s'], 1e3 * model.last_timing['sample_s']

  rows, mels = {}, {}
  for k in counts:
    for sampler in SAMPLERS:
      timed(k, sampler)   # warm-up: this form's tables and graphs
      runs = [timed(k, sampler) for _ in range(args.repeats)]
      mels[(k, sampler)] = runs[-1][0].double().cpu().numpy()
      total, enc, smp = ([r[j] for r in runs] for j in (1, 2, 3))
      rows['%s_%d' % (sampler, k)] = {
          'sampler': sampler, 'steps': k, 'ms_per_segment': total, 'mean_ms': float(np.mean(total)),
          'spread_ms': float(max(total) - min(total)), 'encode_mean_ms': float(np.mean(enc)),
          'sample_mean_ms': float(np.mean(smp))}
  ref = mels[(args.steps, 'ddim')]
  full = rows['ddim_%d' % args.steps]
  for (k, sampler), mel in mels.items():
    r = rows['%s_%d' % (sampler, k)]
    r['rms_mel_vs_full_ddim'] = float(np.sqrt(np.mean((mel - ref) ** 2)))
    r['expected_ms'] = full['encode_mean_ms'] + full['sample_mean_ms'] * k / float(args.steps)
    r['measured_minus_expected_ms'] = r['mean_ms'] - r['expected_ms']
  report = {'device': torch.cuda.get_device_name(0), 'library': msd_amd.native.load().msd_version().decode(),
            'preset': args.preset, 'steps': args.steps, 'frames': t, 'repeats': args.repeats, 'weights': 'synthetic:0',
            'forms': rows, 'reference': 'ddim, %d steps, same init_z' % args.steps,
            'expectation': 'full ddim call: encode part + sampling part x K / steps',
            'note': 'rms_mel_vs_full_ddim is the solver error on synthetic weights (mel units); no perceptual claim'}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fh:
    json.dump(report, fh, indent=1, sort_keys=True)
    fh.write('\n')
  for name, r in rows.items():
    print('%-14s %8.2f ms (spread %.2f; encode %.2f), expected %8.2f, %+6.2f ms; rms mel vs %d-step ddim %.3e'
          % (name, r['mean_ms'], r['spread_ms'], r['encode_mean_ms'], r['expected_ms'], r['measured_minus_expected_ms'],
             args.steps, r['rms_mel_vs_full_ddim']))
  print('wrote %s' % args.out)
  return 0


if __name__ == '__main__':
  sys.exit(main())
