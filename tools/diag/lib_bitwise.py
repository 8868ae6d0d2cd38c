"""Do two builds of the library compute the same bits and launch the same kernels?  (GPU box.)  Runs short samples, two
single decoder passes and one profiled step per configuration on the library named by MSD_AMD_LIB (or the in-tree one)
and prints the sha256 of every output and the launch count of every kernel class.  One library per process: run it once
per build and compare the two outputs (every line but the first must be equal).

The configurations reach the launch paths of the decoder step (msd_api.hip plan_step): one song (the fold, key split 4),
`small`, 8 songs (128-row tiles, persistent MLP-in), 2 songs (the fold with CFG rows at its M <= 1024 limit), 3 songs
(no fold, self-attention on 128-row blocks from layer 1), two cross modules (sum_cross_attends), and one song with
dedup_layer0, cross_q_fold or the key split turned off.

usage: [MSD_AMD_LIB=<other build>] python tools/diag/lib_bitwise.py"""
import dataclasses
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import msd_amd
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _inputs as helpers   # (not tests.helpers: that imports oracle/)


def digest(a):
  return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def spec_of(preset, steps, sum_cross=False):
  spec = msd_amd.config.preset(preset, num_steps=steps)
  if sum_cross:
    spec = dataclasses.replace(spec, t5=dataclasses.replace(spec.t5, decoder_cross_attend_style='sum_cross_attends'))
  return spec


# (name, preset, songs, steps, sum_cross_attends, InferenceModel knobs)
CONFIGS = [
    ('base_with_context x1', 'base_with_context', 1, 8, False, {}),
    ('small x1', 'small', 1, 8, False, {}),
    ('base_with_context x8', 'base_with_context', 8, 8, False, {}),
    ('base_with_context x2', 'base_with_context', 2, 4, False, {}),
    ('base_with_context x3', 'base_with_context', 3, 4, False, {}),
    ('base_with_context sum_cross x1', 'base_with_context', 1, 4, True, {}),
    ('base_with_context x1 dedup_layer0=False', 'base_with_context', 1, 4, False, {'dedup_layer0': False}),
    ('base_with_context x1 cross_q_fold=False', 'base_with_context', 1, 4, False, {'cross_q_fold': False}),
    ('base_with_context x1 cross_key_split=1', 'base_with_context', 1, 4, False, {'cross_key_split': 1}),
]

print('lib=%s' % os.path.basename(os.environ.get('MSD_AMD_LIB', 'in-tree')))
for i, (name, preset, nb, steps, sum_cross, knobs) in enumerate(CONFIGS):
  spec = spec_of(preset, steps, sum_cross)
  model = msd_amd.InferenceModel('synthetic:0', spec, batch_size=nb, **knobs)
  batch = helpers.make_batch(spec, batch=nb)
  init_z, noise = helpers.make_noise(spec, batch=nb)
  got, _ = model.predict(batch, init_z=init_z, noise=noise)
  torch.cuda.synchronize()
  line = '%s | sample %s' % (name, digest(got))
  nm = model._get_native()   # (predict has encoded the batch)
  if i == 0:   # single decoder passes, with and without conditioning
    z = torch.as_tensor(init_z).cuda()
    for cond in (True, False):
      eps = torch.zeros_like(z)
      nm.decoder_pass(nb, 2, z, cond, eps)
      torch.cuda.synchronize()
      line += ' | decoder_pass cond=%d %s' % (cond, digest(eps.cpu().numpy()))
  prof = nm.profile_steps(nb, 1)
  torch.cuda.synchronize()
  print(line + ' | launches ' + ' '.join('%s=%d' % (k, v[1]) for k, v in prof.items()), flush=True)
  nm.close()
  del model, nm
