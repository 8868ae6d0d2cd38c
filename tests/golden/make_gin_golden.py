"""tests/golden/shipped_gin_specs.json: the typed ModelSpec (as plain JSON fields) that ``parse_training_gin_file`` +
``gin_lite.model_spec_from_bindings`` resolve from the reference's shipped training gin files (model gin + task gin +
the MelGAN codec gin, includes followed), one record per case of tests/test_config_gin.py.  Only the resolved settings
are stored, so the test runs without the reference tree.

    python tests/golden/make_gin_golden.py <reference checkout>/music_spectrogram_diffusion/gin
"""
import dataclasses
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import msd_amd  # noqa: E402
from msd_amd import gin_lite  # noqa: E402

CASES = [
    ('models/diffusion/context/t5_base.gin', 'tasks/mt3/context_mega.gin'),
    ('models/diffusion/basic/t5_small.gin', 'tasks/mt3/base.gin'),
    ('models/diffusion/context/t5_small.gin', 'tasks/mt3/context_mega.gin'),
]


def main(gin_dir):
  out = {}
  for model_gin, task_gin in CASES:
    cfg = msd_amd.parse_training_gin_file(
        os.path.join(gin_dir, model_gin),
        ["include '%s'" % os.path.join(gin_dir, task_gin),
         "include '%s'" % os.path.join(gin_dir, 'audio_codecs/melgan.gin')])
    spec = gin_lite.model_spec_from_bindings(gin_lite.parse(cfg))
    out['%s + %s' % (model_gin, task_gin)] = dataclasses.asdict(spec)
  path = os.path.join(HERE, 'shipped_gin_specs.json')
  with open(path, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
  print(path)


if __name__ == '__main__':
  main(sys.argv[1])
