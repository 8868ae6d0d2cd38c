"""Measure what edit strength costs a sampling call on the GPU and write profiles/edit_strength.json (run by hand; not a test):

  python tools/edit_strength_report.py [--out profiles/edit_strength.json] [--preset base_with_context] [--steps 1000]

One process, one model: after a warm-up call of each form (weights, tables and every step graph are then in place),
`--segments` predict calls of each form, interleaved, each timed from call to returned device tensor: the plain call; a
variation of a known segment at strength 0.25, 0.5 and 1.0 (predict(keep=, strength=), what InferenceModel.vary runs per
segment); and a half-ramp regenerate -- the last quarter of the frames sampled again, the quarter before it released
along a linear ramp, the first half known (what regenerate(blend_frames=) runs on a segment it touches).  From the code
the expectation is the plain call's encode time plus strength x its sampling time: a part-way call runs start_step + 1
of the same steps behind one extra elementwise launch; the ramp form starts at the top and runs them all."""
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
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'edit_strength.json'))
  ap.add_argument('--preset', default='base_with_context')
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--segments', type=int, default=3, help='timed calls of each form')
  args = ap.parse_args(argv)

  import numpy as np
  import torch
  import msd_amd
  from msd_amd import inference
  assert torch.cuda.is_available(), 'needs a GPU'
  spec = msd_amd.config.preset(args.preset, num_steps=args.steps)
  t, n = spec.task_feature_lengths['targets'], 128
  model = msd_amd.InferenceModel('synthetic:0', spec)
  known = torch.as_tensor(np.random.default_rng(0).uniform(-11.0, 4.0, (1, t, n)).astype(np.float32)).to(model.device)
  ramp = np.zeros((1, t))
  ramp[0, t // 2:3 * t // 4] = np.arange(1, t // 4 + 1) / float(t // 4 + 1)
  ramp[0, 3 * t // 4:] = 1.0
  forms = {'plain': {}, 'vary_0.25': dict(keep=known, strength=0.25), 'vary_0.5': dict(keep=known, strength=0.5),
           'vary_1.0': dict(keep=known, strength=1.0), 'half_ramp': dict(keep=known, strength=ramp)}
  run_steps = {name: (args.steps if 'strength' not in kw else
                      inference.plan_strength(np.broadcast_to(np.asarray(kw['strength'], np.float64), (1, t)), args.steps)[1] + 1)
               for name, kw in forms.items()}

  def batch(k):
    b = {'encoder_input_tokens': msd_amd.synthetic.segment_tokens(spec, k)}
    if spec.has_context:
      c = spec.task_feature_lengths['targets_context']
      b['encoder_continuous_inputs'] = known[:, :c]
      b['encoder_continuous_mask'] = np.ones((1, c), np.int32)
    return b

  def timed(k, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.predict(batch(k), seed=0, segment=k, return_torch=True, **kw)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), 1e3 * model.last_timing['encode_s'], 1e3 * model.last_timing['sample_s']

  for kw in forms.values():
    timed(0, kw)
  ms = {name: [] for name in forms}
  for k in range(1, args.segments + 1):
    for name, kw in forms.items():
      ms[name].append(timed(k, kw))
  rows = {}
  for name, v in ms.items():
    total, enc, smp = ([x[j] for x in v] for j in range(3))
    rows[name] = {'ms_per_segment': total, 'mean_ms': float(np.mean(total)), 'spread_ms': float(max(total) - min(total)),
                  'encode_mean_ms': float(np.mean(enc)), 'sample_mean_ms': float(np.mean(smp)), 'steps_run': int(run_steps[name])}
  plain = rows['plain']
  for name, r in rows.items():
    r['expected_ms'] = plain['mean_ms'] - plain['sample_mean_ms'] * (1.0 - r['steps_run'] / float(args.steps))
    r['measured_minus_expected_ms'] = r['mean_ms'] - r['expected_ms']
    r['percent_of_plain'] = 100.0 * r['mean_ms'] / plain['mean_ms']
  report = {'device': torch.cuda.get_device_name(0), 'library': msd_amd.native.load().msd_version().decode(),
            'preset': args.preset, 'steps': args.steps, 'frames': t, 'segments_timed': args.segments, 'forms': rows,
            'expectation': 'plain total - plain sampling time x (1 - steps_run / steps)'}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fh:
    json.dump(report, fh, indent=1, sort_keys=True)
    fh.write('\n')
  for name, r in rows.items():
    print('%-10s %4d steps: %8.2f ms (spread %.2f), expected %8.2f, %+6.2f ms; %5.1f %% of the plain call'
          % (name, r['steps_run'], r['mean_ms'], r['spread_ms'], r['expected_ms'], r['measured_minus_expected_ms'],
             r['percent_of_plain']))
  print('wrote %s' % args.out)
  return 0


if __name__ == '__main__':
  sys.exit(main())
