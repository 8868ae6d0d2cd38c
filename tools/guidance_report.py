"""Measure per-call guidance on the GPU and write profiles/guidance.json (run by hand; not a test):

  python tools/guidance_report.py [--out profiles/guidance.json] [--preset base_with_context] [--steps 1000] [--rows 8]

One process, ONE one-row model of `--steps` steps and weight 5, one segment, every form from the same keys; each form is
timed `--repeats` times after one warm-up call of the same form (graphs in place) and reported as the median with its
spread (max - min):

  plain            the call as it always was
  guidance_4       guidance=4.0: every step through the guided kernels.  Expected: the plain call's time -- the difference
                   is one table load in the sampler launch; read it against the plain call's own spread
  guidance_1       guidance=1.0: every step one-pass.  Gives the one-pass step time t1 beside the two-pass t2
  interval_a_b     guidance_interval=(a, b) with the model's weight.  Expected: encode + inside-share x t2-part +
                   outside-share x t1-part; `excess_ms` is what the call takes beyond that

and, on a second model of `--rows` rows: `--rows` weights in ONE call with equal tokens and keys (a guidance sweep) against
the same weights as `--rows` one-row calls on that model.  Nothing here says anything about sound: the weights are
synthetic."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

INTERVALS = ((0.2, 0.8), (0.0, 0.5))


def main(argv=None) -> int:
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'guidance.json'))
  ap.add_argument('--preset', default='base_with_context')
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--rows', type=int, default=8)
  ap.add_argument('--repeats', type=int, default=3, help='timed calls of each form')
  args = ap.parse_args(argv)

  import numpy as np
  import torch
  import msd_amd
  assert torch.cuda.is_available(), 'needs a GPU'
  spec = msd_amd.config.preset(args.preset, num_steps=args.steps)
  n = 128

  def make_batch(rows):
    batch = {'encoder_input_tokens': np.repeat(msd_amd.synthetic.segment_tokens(spec, 1), rows, axis=0)}
    if spec.has_context:
      c = spec.task_feature_lengths['targets_context']
      ctx = np.random.default_rng(1).uniform(-11.0, 4.0, (1, c, n)).astype(np.float32)
      batch['encoder_continuous_inputs'] = np.repeat(ctx, rows, axis=0)
      batch['encoder_continuous_mask'] = np.ones((rows, c), np.int32)
    return batch

  def timed(model, batch, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, _ = model.predict(batch, return_torch=True, **kw)
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0), 1e3 * model.last_timing['encode_s'], 1e3 * model.last_timing['sample_s']

  def measure(model, batch, calls):
    """calls: the keyword sets one measurement consists of (run back to back); -> (row, last outputs)"""
    for kw in calls:
      timed(model, batch, **kw)   # warm-up: this form's graphs
    totals, encs, smps, outs = [], [], [], None
    for _ in range(args.repeats):
      runs = [timed(model, batch, **kw) for kw in calls]
      totals.append(sum(r[1] for r in runs)); encs.append(sum(r[2] for r in runs)); smps.append(sum(r[3] for r in runs))
      outs = [r[0] for r in runs]
    return {'ms': totals, 'median_ms': float(np.median(totals)), 'spread_ms': float(max(totals) - min(totals)),
            'encode_median_ms': float(np.median(encs)), 'sample_median_ms': float(np.median(smps))}, outs

  model = msd_amd.InferenceModel('synthetic:0', spec)
  one = make_batch(1)
  keys = dict(seed=3, segment=1)
  forms = {}
  forms['plain'], plain_out = measure(model, one, [dict(keys)])
  forms['guidance_4'], _ = measure(model, one, [dict(keys, guidance=4.0)])
  forms['guidance_1'], _ = measure(model, one, [dict(keys, guidance=1.0)])
  # the model's own weight through the guided kernels: the plain call's bits
  forms['guidance_4']['model_weight_through_guided_kernels_is_plain_bitwise'] = bool(torch.equal(
      timed(model, one, guidance=[spec.diffusion.classifier_free_guidance.eval_condition_weight], **keys)[0], plain_out[0]))
  t2, t1 = forms['plain']['sample_median_ms'], forms['guidance_1']['sample_median_ms']
  forms['guidance_4']['minus_plain_ms'] = forms['guidance_4']['median_ms'] - forms['plain']['median_ms']
  for lo, hi in INTERVALS:
    row, _ = measure(model, one, [dict(keys, guidance_interval=(lo, hi))])
    g_lo, g_hi = (int(np.floor(x * args.steps + 0.5)) for x in (lo, hi))
    inside = (g_hi - g_lo) / float(args.steps)
    row['scan_indices'] = [g_lo, g_hi]
    row['expected_ms'] = forms['plain']['encode_median_ms'] + inside * t2 + (1.0 - inside) * t1
    row['excess_ms'] = row['median_ms'] - row['expected_ms']
    forms['interval_%g_%g' % (lo, hi)] = row
  del model
  torch.cuda.empty_cache()

  rows = args.rows
  wide = msd_amd.InferenceModel('synthetic:0', spec, batch_size=rows)
  weights = [float(w) for w in np.linspace(1.5, 7.5, rows)]
  sweep, outs = measure(wide, make_batch(rows), [dict(seed=[3] * rows, segment=[1] * rows, guidance=weights)])
  singles, outs1 = measure(wide, one, [dict(keys, guidance=w) for w in weights])
  # (at base size a batched call runs other GEMM tiles than a one-row call: its rows agree with the one-row calls to the
  # rounding of a batched launch, as predict_sequence(batch_segments=) says; on `tiny` they are the same bits, tests/)
  sweep['rows_bitwise_equal_to_one_row_calls'] = bool(all(torch.equal(outs[0][b:b + 1], outs1[b]) for b in range(rows)))
  sweep['rows_rms_to_one_row_calls'] = [float((outs[0][b:b + 1].double() - outs1[b].double()).pow(2).mean().sqrt()) for b in range(rows)]
  sweep['rows_rms_to_next_weight'] = [float((outs1[b + 1].double() - outs1[b].double()).pow(2).mean().sqrt()) for b in range(rows - 1)]
  sweep['speedup_over_one_row_calls'] = singles['median_ms'] / sweep['median_ms']
  forms['sweep_%d_rows_one_call' % rows] = sweep
  forms['sweep_%d_one_row_calls' % rows] = singles

  report = {'device': torch.cuda.get_device_name(0), 'library': msd_amd.native.load().msd_version().decode(),
            'preset': args.preset, 'steps': args.steps, 'repeats': args.repeats, 'weights': 'synthetic:0', 'model_weight': 5.0,
            'two_pass_sample_ms': t2, 'one_pass_sample_ms': t1, 'one_pass_over_two_pass': t1 / t2, 'sweep_weights': weights,
            'forms': forms,
            'expectation': 'interval call: plain encode part + inside share x two-pass sampling part + outside share x one-pass sampling part',
            'note': 'times in ms from call to returned device tensor; synthetic weights, no perceptual claim'}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fh:
    json.dump(report, fh, indent=1, sort_keys=True)
    fh.write('\n')
  for name, r in forms.items():
    print('%-28s %9.2f ms (spread %.2f; encode %.2f)%s' % (name, r['median_ms'], r['spread_ms'], r['encode_median_ms'],
                                                            '  expected %.2f, excess %+.2f' % (r['expected_ms'], r['excess_ms']) if 'expected_ms' in r else ''))
  print('one-pass / two-pass sampling part: %.3f' % (t1 / t2))
  print('wrote %s' % args.out)
  return 0


if __name__ == '__main__':
  sys.exit(main())
