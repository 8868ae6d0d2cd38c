"""Measure the denoising loss on the GPU and write profiles/denoising_loss.json (run by hand; not a test, nothing asserted):

  python tools/denoising_loss_report.py [--out profiles/denoising_loss.json] [--preset base_with_context] [--steps 1000]
      [--tests-log LOG]

One process, one model.

cost       ms per evaluation of msd_loss for conditioning cond / uncond / both at K = 64 time indices: after a warm-up call
           of each form (its graph is then captured), `--calls` timed calls of each, interleaved, NativeModel.loss alone with
           a device synchronisation on either side (the encode stage is the warm-up call's).  Beside them the same handle's
           one-pass and two-pass step times from guided calls in the same process (predict(steps=100, guidance=1.0) runs 100
           one-pass steps, the model's own weight 100 two-pass steps; sample time / 100).  From the code the expectation is one
           step of the matching plan -- the same decoder launches -- with the two loss launches in the sampler launch's place.
regenerate the loss (cond, K = 16, mean over times, summed over frames) of predict_sequence's own output under its tokens, of
           a regenerate() of its middle without resample= and of the same regenerate with resample=(8, 4): per segment and
           over the regenerated frames alone.  Synthetic weights: the figures are recorded, no claim about sound follows.
ratios     with --tests-log: the device / float32 error ratios that tests/test_gpu_loss.py printed (run with -s), copied in."""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)


def ratios_from_log(path):
  """The ratios of test_op_against_float64 / test_call_against_the_reference / test_full_size_against_float64."""
  text = open(path).read()
  op = [float(x) for x in re.findall(r'op loss \S+ \S+ \S+ i=\d+: .*?\(ratio ([0-9.]+)\)', text)]
  call = re.findall(r'(tiny\w*) (\w+)/(\w+) (\w+) (\w+): per-frame relative error, largest .*?\(ratio ([0-9.]+)\); median .*?\(ratio ([0-9.]+)\)', text)
  out = {}
  if op:
    out['op_level'] = {'cases': len(op), 'largest_ratio': max(op), 'median_ratio': sorted(op)[len(op) // 2], 'bound': 4.0}
  for form in ('cond', 'uncond', 'both'):
    rows = [(float(a), float(b)) for name, f, _, _, _, a, b in call if f == form and name != 'base_with_context']
    if rows:
      out['call_level_' + form] = {'cases': len(rows), 'largest_ratio_of_largest_errors': max(r[0] for r in rows),
                                   'largest_ratio_of_median_errors': max(r[1] for r in rows), 'bound': 2.0}
  full = re.findall(r'base_with_context (\w+): per-frame relative error, largest .*?\(ratio ([0-9.]+)\); median .*?\(ratio ([0-9.]+)\)', text)
  if full:
    out['full_size'] = {c: {'ratio_of_largest_errors': float(a), 'ratio_of_median_errors': float(b)} for c, a, b in full}
  return out


def main(argv=None) -> int:
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'denoising_loss.json'))
  ap.add_argument('--preset', default='base_with_context')
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--times', type=int, default=64)
  ap.add_argument('--calls', type=int, default=3, help='timed calls of each form')
  ap.add_argument('--tests-log', default=None, help='output of `pytest tests/test_gpu_loss.py -m gpu -s` to copy the ratios from')
  args = ap.parse_args(argv)

  import numpy as np
  import torch
  import msd_amd
  from msd_amd import native
  assert torch.cuda.is_available(), 'needs a GPU'
  spec = msd_amd.config.preset(args.preset, num_steps=args.steps)
  t, n = spec.task_feature_lengths['targets'], 128
  model = msd_amd.InferenceModel('synthetic:0', spec)
  mel = torch.as_tensor(np.random.default_rng(0).uniform(-11.0, 4.0, (1, t, n)).astype(np.float32)).to(model.device)

  def batch(k):
    b = {'encoder_input_tokens': msd_amd.synthetic.segment_tokens(spec, k), 'decoder_target_tokens': mel}
    if spec.has_context:
      c = spec.task_feature_lengths['targets_context']
      b['encoder_continuous_inputs'] = mel[:, :c]
      b['encoder_continuous_mask'] = np.ones((1, c), np.int32)
    return b

  # ---- cost ----
  idx = native.plan_loss_times(args.steps, args.times)
  forms = ('cond', 'uncond', 'both')
  for f in forms:
    model.loss(batch(0), times=idx, conditioning=f)   # warm-up: encode, buffers, the form's graph
  nm = model._get_native()
  outs = {f: torch.empty((len(idx), 2 if f == 'both' else 1, 1, t), dtype=torch.float32, device=model.device) for f in forms}
  ms = {f: [] for f in forms}
  for _ in range(args.calls):
    for f in forms:
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      nm.loss(1, mel, outs[f], idx, conditioning=f, stream=model._stream.cuda_stream)
      torch.cuda.synchronize()
      ms[f].append(1e3 * (time.perf_counter() - t0) / len(idx))
  k_steps = 100 if args.steps % 100 == 0 else args.steps
  step_ms = {}
  for name, kw in (('one_pass', dict(guidance=1.0)), ('two_pass', dict())):
    v = []
    for r in range(args.calls + 1):
      model.predict(batch(0), seed=0, return_torch=True, steps=k_steps, **kw)
      if r:
        v.append(1e3 * model.last_timing['sample_s'] / k_steps)
    step_ms[name] = v
  cost = {f: {'ms_per_evaluation': ms[f], 'mean_ms': float(np.mean(ms[f])), 'spread_ms': float(max(ms[f]) - min(ms[f]))} for f in forms}
  for name, v in step_ms.items():
    cost[name + '_step'] = {'ms_per_step': v, 'mean_ms': float(np.mean(v)), 'spread_ms': float(max(v) - min(v)), 'steps_per_call': k_steps}
  for f, plan in (('cond', 'one_pass'), ('uncond', 'one_pass'), ('both', 'two_pass')):
    cost[f]['times_the_matching_step'] = cost[f]['mean_ms'] / cost[plan + '_step']['mean_ms']

  # ---- regenerate with and without resampling ----
  segs = [msd_amd.synthetic.segment_tokens(spec, k)[0] for k in range(3)]
  song = model.predict_sequence(segs, seed=0, return_torch=True)
  lo, hi = t + t // 4, t + 3 * t // 4   # the middle half of segment 1
  songs = {'predict_sequence': song, 'regenerate': model.regenerate(song, segs, lo, hi, seed=1, return_torch=True),
           'regenerate_resample_8_4': model.regenerate(song, segs, lo, hi, seed=1, return_torch=True, resample=(8, 4))}
  regen = {}
  for name, s in songs.items():
    r = model.score_sequence(s, segs, times=16, seed=0)
    regen[name] = {'per_segment': [float(v) for v in r['per_segment'][0]], 'loss': float(r['loss'][0]),
                   'regenerated_frames': float(r['per_frame'][0, lo:hi].sum()), 'per_frame_mean': float(r['per_frame'][0].mean())}
  report = {'device': torch.cuda.get_device_name(0), 'library': native.load().msd_version().decode(), 'preset': args.preset,
            'steps': args.steps, 'times': len(idx), 'calls_timed': args.calls, 'cost': cost,
            'cost_expectation': 'one step of the matching plan, with the two loss launches in the sampler launch\'s place',
            'regenerate': dict(regen, frames=[lo, hi], note='synthetic weights: recorded, nothing about sound follows')}
  if args.tests_log:
    report['error_ratios_device_over_float32'] = ratios_from_log(args.tests_log)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fh:
    json.dump(report, fh, indent=1, sort_keys=True)
    fh.write('\n')
  for f in forms:
    print('%-6s %.4f ms per evaluation (spread %.4f), x%.3f the matching step' % (f, cost[f]['mean_ms'], cost[f]['spread_ms'],
                                                                                cost[f]['times_the_matching_step']))
  print('one-pass step %.4f ms, two-pass step %.4f ms' % (cost['one_pass_step']['mean_ms'], cost['two_pass_step']['mean_ms']))
  for name, r in regen.items():
    print('%-26s loss %.1f, regenerated frames %.1f, per segment %s' % (name, r['loss'], r['regenerated_frames'], r['per_segment']))
  print('wrote %s' % args.out)
  return 0


if __name__ == '__main__':
  sys.exit(main())
