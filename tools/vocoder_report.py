"""Measure the device vocoder on the GPU and write profiles/vocoder_parity.json (run by hand; not a test):

  python tools/vocoder_report.py [--out profiles/vocoder_parity.json] [--no-sampling]

  * waveform parity of decode at 1 and 4 Griffin-Lim iterations (F = 70, B = 2, explicit phases): relative L2 distance
    of the device and of the float32 NumPy restatement to the float64 specification -- the two numbers
    tests/test_gpu_vocoder.py compares (device <= 16 x restatement);
  * spectral convergence after 32 iterations, device and float64;
  * wall time of decode for 12 segments (3072 frames, 32 iterations, one call), beside the sampling time of ONE
    256-frame segment of base_with_context (1000 steps, synthetic weights) in the same process."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tools')):
  if _p not in sys.path:
    sys.path.insert(0, _p)


def main(argv=None) -> int:
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vocoder_parity.json'))
  ap.add_argument('--no-sampling', action='store_true', help='skip the base_with_context sampling time')
  args = ap.parse_args(argv)

  import torch
  import msd_amd
  from msd_amd import audio_codecs as ac
  import vocoder_cases as vc   # next to this file
  assert torch.cuda.is_available(), 'needs a GPU'
  voc = msd_amd.vocoder.GriffinLimVocoder()
  f, b = 70, 2
  logmel = np.log(np.clip(np.abs(ac.stft(vc.two_songs(f))) @ vc.mel_basis(), 1e-5, 1e8)).astype(np.float32)
  phase = vc.closed_form_phase(b, f).astype(np.float32)
  mag = ac.mel_to_linear(logmel.astype(np.float64))
  ph64 = phase.astype(np.float64)

  def ref(n):
    return ac.griffin_lim(mag, n, 0.99, init_phase=(ph64[:, :, 0], ph64[:, :, 1]))

  report = {'device': torch.cuda.get_device_name(0), 'library': msd_amd.native.load().msd_version().decode(),
            'frames': f, 'batch': b, 'parity': {}}
  for n in (1, 4):
    want = ref(n)
    dev = vc.rel_l2(voc.decode(logmel, n_iters=n, init_phase=phase), want)
    yard = vc.rel_l2(vc.griffin_lim_matrix(logmel, n, 0.99, phase, np.float32), want)
    report['parity'][str(n)] = {'device_rel_l2': dev, 'float32_numpy_rel_l2': yard, 'ratio': dev / yard}
    print('%d iterations: device %.3e, float32 NumPy %.3e (x%.2f)' % (n, dev, yard, dev / yard))
  sc_dev = ac.spectral_convergence(voc.decode(logmel, n_iters=32, init_phase=phase), mag)
  sc_ref, sc_0 = ac.spectral_convergence(ref(32), mag), ac.spectral_convergence(ref(0), mag)
  report['spectral_convergence'] = {'iterations_0_float64': sc_0, 'iterations_32_float64': sc_ref, 'iterations_32_device': sc_dev}
  print('spectral convergence: %.4f at 0 iterations; after 32: device %.4f, float64 %.4f' % (sc_0, sc_dev, sc_ref))

  # timing: 12 segments in one call
  frames = 12 * 256
  song = torch.as_tensor(vc.signal(frames)[None].astype(np.float32)).cuda()
  mel = voc.encode(song, return_torch=True)
  times = {'encode': [], 'decode': []}
  for rep in range(4):   # the first pass allocates the work buffers
    for what, fn in (('encode', lambda: voc.encode(song, return_torch=True)),
                     ('decode', lambda: voc.decode(mel, n_iters=32, seed=0, return_torch=True))):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn()
      torch.cuda.synchronize()
      if rep:
        times[what].append(time.perf_counter() - t0)
  long_sc = ac.spectral_convergence(voc.decode(mel, n_iters=32, seed=0), ac.mel_to_linear(mel.cpu().numpy().astype(np.float64)))
  report['timing'] = {'frames': frames, 'spectral_convergence_of_the_timed_decode': long_sc, 'iterations': 32, 'decode_seconds': float(np.median(times['decode'])),
                      'encode_seconds': float(np.median(times['encode'])), 'audio_seconds': frames * 320 / 16000.0}
  print('decode of %d frames (%.1f s of audio), 32 iterations: %.4f s; encode %.5f s'
        % (frames, frames * 0.02, report['timing']['decode_seconds'], report['timing']['encode_seconds']))
  if not args.no_sampling:
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'diag'))
    import _inputs as helpers
    spec = msd_amd.config.preset('base_with_context')
    model = msd_amd.InferenceModel('synthetic:0', spec)
    batch = helpers.make_batch(spec)
    model.predict(batch, seed=0, return_torch=True)            # loads the weights, captures the step graphs
    model.predict(batch, seed=1, return_torch=True)
    report['timing']['sampling_seconds_per_segment'] = float(model.last_timing['total_s'])
    report['timing']['sampling'] = 'base_with_context, %d steps, synthetic weights, one 256-frame segment' % spec.diffusion.sampler.schedule.num_steps
    print('sampling one segment: %.3f s' % model.last_timing['total_s'])
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fh:
    json.dump(report, fh, indent=1, sort_keys=True)
    fh.write('\n')
  print('wrote', args.out)
  return 0


if __name__ == '__main__':
  sys.exit(main())
