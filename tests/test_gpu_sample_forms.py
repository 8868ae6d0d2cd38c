"""-m gpu: every form of sampling call on ONE handle gives the bits a fresh handle gives, in either order.

The suites of the single features check the forms in pairs; this one runs all of them through one handle's graph cache
and step views: a wrong graph key or a view that leaks from one call into the next shows as a changed bit.

Preset tiny_context, 24 steps, two rows, ragged context mask, 8 steps per graph (the default): a 24-step call is three
graphs, the 11 steps of strength 0.45 one graph and three single steps from a part-way start, 12 steps one graph and four
single steps on strided tables, 6 steps of dpmpp_2m single steps only with the side table and the history buffer."""
import numpy as np
import pytest

import msd_amd
from tests import helpers
from tests.helpers import gpu_torch  # noqa: F401  (the `torch` fixture)

pytestmark = pytest.mark.gpu

N, B = 24, 2


def _forms(spec):
  """name -> predict's keywords, in the order a .. g"""
  rng = np.random.default_rng(21)
  known = rng.uniform(-11.0, 4.0, (B, 64, 128)).astype(np.float32)
  mask = np.zeros((B, 64), np.int32)
  mask[0, :32] = 1
  mask[1, ::2] = 1
  init_z, noise = helpers.make_noise(spec, batch=B)
  return [
      ('a: scalar key, philox', dict(seed=4, segment=2, rng='philox')),
      ('b: per-row keys, threefry', dict(seed=[4, 9], segment=[2, 5], rng='threefry')),
      ('c: keep, half of the frames', dict(seed=4, segment=2, keep=known, keep_mask=mask)),
      ('d: keep, strength 0.45', dict(seed=4, segment=2, keep=known, strength=0.45)),
      ('e: 12 steps, ddim', dict(seed=4, segment=2, steps=12, sampler='ddim')),
      ('f: 6 steps, dpmpp_2m', dict(seed=4, segment=2, steps=6, sampler='dpmpp_2m')),
      ('g: supplied init_z and noise', dict(init_z=init_z, noise=noise)),
  ]


def test_every_form_on_one_handle_is_the_fresh_handles_call(torch):
  spec = msd_amd.config.preset('tiny_context', num_steps=N)
  params = msd_amd.synthetic.init_params(spec, 3, norm_scale_jitter=0.1)
  make = lambda: msd_amd.InferenceModel(params, spec, batch_size=B, **helpers.ALL_PLANES)
  batch = helpers.make_batch(spec, batch=B, ctx_mask='ragged')
  forms = _forms(spec)
  fresh = {}
  for name, kw in forms:   # each form as the FIRST call of a handle of its own
    model = make()
    fresh[name] = model.predict(batch, **kw)[0]
    assert np.isfinite(fresh[name]).all(), name
    model._get_native().close()
  assert len({helpers.bits(v).tobytes() for v in fresh.values()}) == len(forms)   # (seven different calls)
  model = make()
  first = {name: model.predict(batch, **kw)[0] for name, kw in forms}
  model._get_native().reset_graph()
  second = {name: model.predict(batch, **kw)[0] for name, kw in reversed(forms)}
  for name, _ in forms:
    np.testing.assert_array_equal(helpers.bits(first[name]), helpers.bits(fresh[name]), err_msg='a .. g, ' + name)
    np.testing.assert_array_equal(helpers.bits(second[name]), helpers.bits(fresh[name]), err_msg='g .. a, ' + name)
    np.testing.assert_array_equal(helpers.bits(first[name]), helpers.bits(second[name]), err_msg='both passes, ' + name)
