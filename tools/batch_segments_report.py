"""Measure predict_sequence(batch_segments=) on the GPU and write profiles/batch_segments.json (run by hand; not a test):

  python tools/batch_segments_report.py [--out profiles/batch_segments.json] [--steps 1000] [--skip-base]

  * `small` (no context), 12 synthetic segments (synthetic.segment_tokens(spec, k)), 1000 steps, in ONE process:
    batch_segments 1 (the sequential loop: the path without this option), 4 and 12, each after a warm-up group of its
    own size (weights, tables and the step graphs of that batch size are then in place);
  * base_with_context under always_mask_context, 16 segments (two full groups of 8), batch_segments 1 and 8.
Every figure is the wall time of the whole predict_sequence call (encode + sample of every group), as mel-frames/s and
ms per segment, and its ratio to the batch_segments=1 run of the same process."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)


def update_report(path, section, value):
  """Merge `value` under `section` of the JSON report at `path` (created when missing)."""
  report = {}
  if os.path.exists(path):
    with open(path) as fh:
      report = json.load(fh)
  report[section] = value
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, 'w') as fh:
    json.dump(report, fh, indent=1, sort_keys=True)
    fh.write('\n')


def measure(preset, n_segments, sizes, steps, always_mask_context=False):
  import torch
  import msd_amd
  spec = msd_amd.config.preset(preset, num_steps=steps)
  t = spec.task_feature_lengths['targets']
  segs = [msd_amd.synthetic.segment_tokens(spec, k) for k in range(n_segments)]
  model = msd_amd.InferenceModel('synthetic:0', spec, batch_size=max(sizes))
  kw = dict(seed=0, always_mask_context=always_mask_context, return_torch=True)
  rows = {}
  for bs in sizes:
    model.predict_sequence(segs[:bs], batch_segments=bs, **kw)   # warm-up group of this size
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.predict_sequence(segs, batch_segments=bs, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rows[str(bs)] = {'seconds': dt, 'ms_per_segment': 1e3 * dt / n_segments, 'mel_frames_per_s': n_segments * t / dt}
  base = rows[str(sizes[0])]['mel_frames_per_s']
  for bs in sizes:
    rows[str(bs)]['rate_over_batch_segments_1'] = rows[str(bs)]['mel_frames_per_s'] / base
    print('%s, %d segments, %d steps, batch_segments=%d: %.1f mel-frames/s, %.1f ms per segment (x%.2f)'
          % (preset, n_segments, steps, bs, rows[str(bs)]['mel_frames_per_s'], rows[str(bs)]['ms_per_segment'],
             rows[str(bs)]['rate_over_batch_segments_1']))
  return {'segments': n_segments, 'steps': steps, 'always_mask_context': bool(always_mask_context), 'batch_segments': rows}


def main(argv=None) -> int:
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'batch_segments.json'))
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--skip-base', action='store_true', help='skip the base_with_context leg')
  args = ap.parse_args(argv)

  import torch
  import msd_amd
  assert torch.cuda.is_available(), 'needs a GPU'
  update_report(args.out, 'device', torch.cuda.get_device_name(0))
  update_report(args.out, 'library', msd_amd.native.load().msd_version().decode())
  update_report(args.out, 'small', measure('small', 12, (1, 4, 12), args.steps))
  if not args.skip_base:
    update_report(args.out, 'base_with_context', measure('base_with_context', 16, (1, 8), args.steps, always_mask_context=True))
  print('wrote', args.out)
  return 0


if __name__ == '__main__':
  sys.exit(main())
