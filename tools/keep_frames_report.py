"""Measure what known frames cost a sampling call on the GPU and write profiles/keep_frames.json (run by hand; not a test):

  python tools/keep_frames_report.py [--out profiles/keep_frames.json] [--preset base_with_context] [--steps 1000]

One process, one model: after a warm-up call of each form (weights, tables and both sets of step graphs are then in
place), `--segments` predict calls without a mask and as many with the second half of the frames known, alternating, each
timed from call to returned device tensor.  The sampler launch is latency-bound, so the two are expected to agree within
the spread of the repeats."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)


def main(argv=None) -> int:
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'keep_frames.json'))
  ap.add_argument('--preset', default='base_with_context')
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--segments', type=int, default=3, help='timed calls of each form')
  args = ap.parse_args(argv)

  import numpy as np
  import torch
  import msd_amd
  assert torch.cuda.is_available(), 'needs a GPU'
  spec = msd_amd.config.preset(args.preset, num_steps=args.steps)
  t, n = spec.task_feature_lengths['targets'], 128
  model = msd_amd.InferenceModel('synthetic:0', spec)
  known = torch.as_tensor(np.random.default_rng(0).uniform(-11.0, 4.0, (1, t, n)).astype(np.float32)).to(model.device)
  mask = np.zeros((1, t), np.int32)
  mask[:, t // 2:] = 1
  keep = dict(keep=known, keep_mask=mask)

  def batch(k):
    b = {'encoder_input_tokens': msd_amd.synthetic.segment_tokens(spec, k)}
    if spec.has_context:
      c = spec.task_feature_lengths['targets_context']
      b['encoder_continuous_inputs'] = known[:, :c]
      b['encoder_continuous_mask'] = np.ones((1, c), np.int32)
    return b

  def timed(k, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.predict(batch(k), seed=0, segment=k, return_torch=True, **kw)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)

  timed(0)
  timed(0, **keep)
  ms = {'plain': [], 'half_mask': []}
  for k in range(1, args.segments + 1):
    ms['plain'].append(timed(k))
    ms['half_mask'].append(timed(k, **keep))
  rows = {name: {'ms_per_segment': v, 'mean_ms': float(np.mean(v)), 'spread_ms': float(max(v) - min(v))}
          for name, v in ms.items()}
  diff = rows['half_mask']['mean_ms'] - rows['plain']['mean_ms']
  report = {'device': torch.cuda.get_device_name(0), 'library': msd_amd.native.load().msd_version().decode(),
            'preset': args.preset, 'steps': args.steps, 'kept_frames': int(mask.sum()), 'frames': t, 'forms': rows,
            'half_mask_minus_plain_ms': diff, 'half_mask_minus_plain_percent': 100.0 * diff / rows['plain']['mean_ms'],
            'within_spread': bool(abs(diff) <= max(rows['plain']['spread_ms'], rows['half_mask']['spread_ms']))}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fh:
    json.dump(report, fh, indent=1, sort_keys=True)
    fh.write('\n')
  print(json.dumps(report['forms']))
  print('half mask - plain: %+.2f ms (%+.3f %%), within the repeats\' spread: %s; wrote %s'
        % (diff, report['half_mask_minus_plain_percent'], report['within_spread'], args.out))
  return 0


if __name__ == '__main__':
  sys.exit(main())
