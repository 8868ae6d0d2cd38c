"""Measure DDIM inversion on the GPU and write profiles/invert.json (run by hand; not a test):

  python tools/invert_report.py [--out profiles/invert.json] [--preset base_with_context] [--steps 1000] [--test-log LOG]

One process, ONE one-row model of `--steps` steps and weight 5, one segment.  For K in --levels (1000 / 250 / 50):

  invert_K      InferenceModel.invert(steps=K) at weight 1, timed `--repeats` times after one warm-up call (graphs in place):
                the median with its spread (max - min).  Expected: that handle's encode time + K x its own measured one-pass
                step time, taken from a weight-1 predict of all `--steps` steps (predict(guidance=1.0)); `excess_ms` is what
                the call takes beyond that
  round_trip_K  invert(steps=K), then predict(init_z=noise, sampler='ddim', steps=K, guidance=1.0): the rms distance of the
                rendering to the mel that was inverted, in mel units.  RECORDED, not asserted: on synthetic weights the
                network's eps moves freely between two levels and nothing here says anything about sound

--test-log: the output of `pytest -s tests/test_gpu_invert.py`; the figures the tests print (the chains' median errors
against the float64 specification, the closed-form chain's ratio to the float32 restatement) are copied into the report."""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)


def test_figures(path):
  """The figures tests/test_gpu_invert.py prints, from a `pytest -s` log."""
  text = open(path).read()
  chains = [{'case': m.group(1), 'median_abs_err': float(m.group(2)), 'noise_rms': float(m.group(3))}
            for m in re.finditer(r"inversion (\{.*?\}): median \|err\| (\S+), rms of the noise (\S+)", text)]
  out = {'chains_vs_float64_spec': chains}
  m = re.search(r'ideal-denoiser inversion, K = 50: rms distance to the float64 chain device (\S+) / float32 NumPy (\S+) \(ratio (\S+)\)', text)
  if m:
    out['closed_form_k50'] = {'device_rms': float(m.group(1)), 'float32_numpy_rms': float(m.group(2)), 'ratio': float(m.group(3)), 'bound': 4.0}
  m = re.search(r'round trip, 24 steps, weight 1: rms mel error of the spec ([0-9.eE+-]+), of the device ([0-9.eE+-]+) \(mel rms ([0-9.eE+-]+)\)', text)
  if m:
    out['tiny_round_trip_24'] = {'spec_rms': float(m.group(1)), 'device_rms': float(m.group(2)), 'mel_rms': float(m.group(3))}
  return out


def main(argv=None) -> int:
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'invert.json'))
  ap.add_argument('--preset', default='base_with_context')
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--levels', type=int, nargs='*', default=[1000, 250, 50])
  ap.add_argument('--repeats', type=int, default=3, help='timed calls of each form')
  ap.add_argument('--test-log', default=None)
  args = ap.parse_args(argv)

  import numpy as np
  import torch
  import msd_amd
  assert torch.cuda.is_available(), 'needs a GPU'
  spec = msd_amd.config.preset(args.preset, num_steps=args.steps)
  n, t = 128, spec.task_feature_lengths['targets']
  batch = {'encoder_input_tokens': msd_amd.synthetic.segment_tokens(spec, 1)}
  if spec.has_context:
    c = spec.task_feature_lengths['targets_context']
    batch['encoder_continuous_inputs'] = np.random.default_rng(1).uniform(-11.0, 4.0, (1, c, n)).astype(np.float32)
    batch['encoder_continuous_mask'] = np.ones((1, c), np.int32)
  mel = np.random.default_rng(2).uniform(-10.0, 3.0, (1, t, n)).astype(np.float32)
  batch['decoder_target_tokens'] = mel
  model = msd_amd.InferenceModel('synthetic:0', spec)

  def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0), 1e3 * model.last_timing['encode_s'], 1e3 * model.last_timing['sample_s']

  def measure(fn):
    timed(fn)   # warm-up: this form's graphs
    runs = [timed(fn) for _ in range(args.repeats)]
    totals = [r[1] for r in runs]
    return {'ms': totals, 'median_ms': float(np.median(totals)), 'spread_ms': float(max(totals) - min(totals)),
            'encode_median_ms': float(np.median([r[2] for r in runs])), 'sample_median_ms': float(np.median([r[3] for r in runs]))}, runs[-1][0]

  forms = {}
  forms['predict_weight_1'], _ = measure(lambda: model.predict(batch, seed=3, segment=1, guidance=1.0, return_torch=True)[0])
  step_ms = forms['predict_weight_1']['sample_median_ms'] / args.steps
  encode_ms = forms['predict_weight_1']['encode_median_ms']
  for k in args.levels:
    row, noise = measure(lambda: model.invert(batch, steps=k, return_torch=True))
    row['expected_ms'] = encode_ms + k * step_ms
    row['excess_ms'] = row['median_ms'] - row['expected_ms']
    forms['invert_%d' % k] = row
    back, _ = model.predict(batch, init_z=noise, sampler='ddim', steps=k, guidance=1.0)
    nz = noise.double()
    forms['round_trip_%d' % k] = {'rms_mel': float(np.sqrt(np.mean((back.astype(np.float64) - mel) ** 2))),
                                  'mel_rms': float(np.sqrt(np.mean(mel.astype(np.float64) ** 2))),
                                  'noise_rms': float(nz.pow(2).mean().sqrt()), 'noise_finite': bool(torch.isfinite(noise).all()),
                                  'asserted': False}
  report = {'device': torch.cuda.get_device_name(0), 'library': msd_amd.native.load().msd_version().decode(),
            'preset': args.preset, 'steps': args.steps, 'repeats': args.repeats, 'weights': 'synthetic:0', 'model_weight': 5.0,
            'one_pass_step_ms': step_ms, 'encode_ms': encode_ms, 'forms': forms,
            'expectation': 'invert_K: the weight-1 predict\'s encode part + K x its sampling part / steps',
            'note': 'times in ms from call to returned device tensor; the round-trip error is recorded, not asserted; '
                    'synthetic weights, no perceptual claim'}
  if args.test_log:
    report['test_figures'] = test_figures(args.test_log)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fh:
    json.dump(report, fh, indent=1, sort_keys=True)
    fh.write('\n')
  for name, r in forms.items():
    if 'median_ms' in r:
      print('%-20s %9.2f ms (spread %.2f; encode %.2f)%s' % (name, r['median_ms'], r['spread_ms'], r['encode_median_ms'],
                                                            '  expected %.2f, excess %+.2f' % (r['expected_ms'], r['excess_ms']) if 'expected_ms' in r else ''))
    else:
      print('%-20s rms mel error %.4g (mel rms %.3f; noise rms %.3f)' % (name, r['rms_mel'], r['mel_rms'], r['noise_rms']))
  print('wrote %s' % args.out)
  return 0


if __name__ == '__main__':
  sys.exit(main())
