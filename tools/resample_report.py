"""Measure what resampling jumps cost a known-frame sampling call on the GPU and write profiles/resample.json (run by hand;
not a test):

  python tools/resample_report.py [--out profiles/resample.json] [--preset base_with_context] [--steps 1000]

One process, one model: after a warm-up call of each form (weights, tables and both keep-form step graphs are then in
place), `--segments` predict calls of each form, interleaved, each timed from call to returned device tensor with a device
synchronisation on either side: a regenerate-style call with the first half of the frames known (predict(keep=,
keep_mask=), what InferenceModel.regenerate runs on a segment it touches) at resample = None, (8, 2), (8, 4) and
(10, 10).  The figure to compare against is the same handle's own resample=None call.  From the code the expectation is
that call's encode time plus `times` x its sampling time plus the jump launches: a call with resampling replays the same
step graphs times x steps times, with one elementwise launch per jump between them and one more key upload in front."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

FORMS = (None, (8, 2), (8, 4), (10, 10))


def main(argv=None) -> int:
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resample.json'))
  ap.add_argument('--preset', default='base_with_context')
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--segments', type=int, default=2, help='timed calls of each form')
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
  mask = np.zeros((1, t), np.int32)
  mask[0, :t // 2] = 1
  name_of = lambda r: 'none' if r is None else '%d:%d' % r
  plans = {name_of(r): inference.plan_resample(args.steps - 1, *(r or (1, 1))) for r in FORMS}
  counts = {k: (sum(o[1] - o[2] for o in ops if o[0] == 'steps'), sum(o[0] == 'jump' for o in ops)) for k, ops in plans.items()}

  def batch(k):
    b = {'encoder_input_tokens': msd_amd.synthetic.segment_tokens(spec, k)}
    if spec.has_context:
      c = spec.task_feature_lengths['targets_context']
      b['encoder_continuous_inputs'] = known[:, :c]
      b['encoder_continuous_mask'] = np.ones((1, c), np.int32)
    return b

  def timed(k, r):
    kw = {} if r is None else dict(resample=r)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.predict(batch(k), seed=0, segment=k, return_torch=True, keep=known, keep_mask=mask, **kw)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), 1e3 * model.last_timing['encode_s'], 1e3 * model.last_timing['sample_s']

  for r in FORMS:
    timed(0, r)
  ms = {name_of(r): [] for r in FORMS}
  for k in range(1, args.segments + 1):
    for r in FORMS:
      ms[name_of(r)].append(timed(k, r))
  rows = {}
  for name, v in ms.items():
    total, enc, smp = ([x[j] for x in v] for j in range(3))
    rows[name] = {'ms_per_segment': total, 'mean_ms': float(np.mean(total)), 'spread_ms': float(max(total) - min(total)),
                  'encode_mean_ms': float(np.mean(enc)), 'sample_mean_ms': float(np.mean(smp)),
                  'steps_run': int(counts[name][0]), 'jumps': int(counts[name][1])}
  plain = rows['none']
  for name, r in rows.items():
    times = r['steps_run'] / float(args.steps)
    r['expected_without_jump_launches_ms'] = plain['mean_ms'] - plain['sample_mean_ms'] + times * plain['sample_mean_ms']
    r['measured_minus_expected_ms'] = r['mean_ms'] - r['expected_without_jump_launches_ms']
    r['residual_us_per_jump'] = 1e3 * r['measured_minus_expected_ms'] / r['jumps'] if r['jumps'] else None
    r['times_the_plain_call'] = r['mean_ms'] / plain['mean_ms']
  report = {'device': torch.cuda.get_device_name(0), 'library': msd_amd.native.load().msd_version().decode(),
            'preset': args.preset, 'steps': args.steps, 'frames': t, 'frames_known': int(mask.sum()),
            'segments_timed': args.segments, 'forms': rows,
            'expectation': "the resample=None call's encode time + times x its sampling time (+ the jump launches: the residual)"}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fh:
    json.dump(report, fh, indent=1, sort_keys=True)
    fh.write('\n')
  for name, r in rows.items():
    print('%-6s %5d steps %4d jumps: %9.2f ms (spread %.2f), expected %9.2f, %+7.2f ms; x%.3f the plain call'
          % (name, r['steps_run'], r['jumps'], r['mean_ms'], r['spread_ms'], r['expected_without_jump_launches_ms'],
             r['measured_minus_expected_ms'], r['times_the_plain_call']))
  print('wrote %s' % args.out)
  return 0


if __name__ == '__main__':
  sys.exit(main())
