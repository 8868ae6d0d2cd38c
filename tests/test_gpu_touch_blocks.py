"""-m gpu: the touch-block carrier form of the weight prefetch (csrc/gemm_h16.h "Touch blocks"), one launch at a time
through msd_op_gemm_site_carrier / msd_op_attention_launch_carrier, and once through a whole model.

A touch has no reader.  So every case asserts the existing invariant, three ways: the output BITS of a launch that carries
its target on touch blocks equal those of the same launch with no target and those of the in-block wave form; the
half-plane range flag is untouched; the op returns MSD_OK.  The op makes the target itself -- two planes of 128 rows x 128
elements = 64 KiB, one allocation of exactly that size -- so the last line a touch may read ends where the allocation
ends: a touch dealt past the target is an out-of-range read for the allocator to fault, not a silent one."""
import numpy as np
import pytest

from tests import helpers
from tests.test_gpu_gemm_sites import make as make_site

pytestmark = pytest.mark.gpu

TARGET = dict(target_rows=128, target_k=128)   # 2 planes x 128 x 128 x 2 bytes = 64 KiB


@pytest.fixture(scope='module')
def env():
  import torch
  import msd_amd
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  msd_amd.native.load()
  return torch, msd_amd.native


def _dev(torch, a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


def _forms(n_touch):
  return (('none', {}), ('wave', TARGET), ('blocks', dict(TARGET, n_touch=n_touch)))


# ---- GEMM: the cross-attention output projection's site on its narrow tile ------------------------------------------
def _gemm(env, k, form, opts):
  torch, native = env
  m = n = 64
  p = make_site('resnorm_square', m, n, k)
  fields = {f: p[f] for f in ('m', 'n', 'k', 'step', 'steps', 'split_row')}
  fields.update({f: _dev(torch, p[f]) for f in ('a', 'w', 'g_lo', 'g_hi')})
  nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
  outs = dict(x=_dev(torch, p['x']), y=nan(m, n), ssq_out=nan(m, n // 32))
  ran = native.op_gemm_site_carrier('f16x3', 'resnorm_square', form, force_bm=32, force_bn=32, **opts, **fields, **outs)
  torch.cuda.synchronize()
  return {name: t.cpu().numpy().view(np.uint32) for name, t in outs.items()}, ran


@pytest.mark.parametrize('n_touch', [1, 8])
@pytest.mark.parametrize('k', [64, 128, 320])   # shorter than the 4-deep ring (nk < NS) twice; ring depth + 1
def test_gemm_narrow_tile(env, k, n_touch):
  got = {}
  for form, opts in _forms(n_touch):
    got[form], ran = _gemm(env, k, form, opts)
    assert ran['status'] == 0 and ran['ran_range_flag'] == 0, (form, ran)
    assert (ran['ran_bm'], ran['ran_bn'], ran['ran_ns']) == (32, 32, 4), ran
    assert ran['ran_form'] == {'none': 0, 'wave': 1, 'blocks': 2}[form], (form, ran)
    assert ran['ran_touch_blocks'] == (n_touch if form == 'blocks' else 0), (form, ran)
    assert ran['ran_prefetch'] == (form != 'none'), (form, ran)
  for form in ('wave', 'blocks'):
    for name in got['none']:
      assert np.array_equal(got[form][name], got['none'][name]), (form, name)
  assert not np.isnan(got['blocks']['y'].view(np.float32)).any()


# ---- attention: 2 heads x 64 query rows --------------------------------------------------------------------------
ATTN_CASES = {
    '256 keys, two stages, no split': dict(keys=256),
    '384 keys, split 2, merged in the launch': dict(keys=384, ksplit=2, merge_in_launch=1, segs=2, repeats=2),
    'no keys: all masked': dict(keys=256, n_valid=0),
    'un-normalised queries': dict(keys=256, qs=True),
    'K / V touch-ahead: wave and touch blocks': dict(keys=384, touch_ahead=1, pf_late=1),
}


def _attention(env, case, form, opts):
  torch, native = env
  heads, rows, j = 2, 64, 128
  keys, segs = case['keys'], case.get('segs', 1)
  rng = np.random.default_rng(11)
  t = lambda *shape: _dev(torch, (rng.standard_normal(shape) * 0.35).astype(np.float32))
  fields = dict(heads=heads, segs=segs, q_rows_per_seg=rows, ldq=j, q_col=0, ldk=j, k_col=0, k_alloc_rows=keys, k_row0=0,
                k_rows=keys, q=t(segs * rows, j), k=t(segs * keys, j), v=t(segs, keys, j),
                n_keys=_dev(torch, [case.get('n_valid', keys)] * segs, np.int32))
  for f in ('ksplit', 'merge_in_launch', 'repeats', 'touch_ahead', 'pf_late'):
    if f in case:
      fields[f] = case[f]
  if case.get('qs'):
    fields.update(q_ssq=_dev(torch, rng.uniform(0.5, 2.0, (segs * rows, 24))), q_tiles=24)
  o = torch.full((segs * rows, j), float('nan'), dtype=torch.float32, device='cuda')
  ran = native.op_attention_launch_carrier('f16x3', form, o=o, **opts, **fields)
  torch.cuda.synchronize()
  return o.cpu().numpy().view(np.uint32), ran


@pytest.mark.parametrize('name', sorted(ATTN_CASES))
def test_attention(env, name):
  case = ATTN_CASES[name]
  per_row = 2 * case.get('segs', 1)   # touch blocks come in rows of heads x segments
  got = {}
  for form, opts in _forms(2 * per_row):
    got[form], ran = _attention(env, case, form, opts)
    assert ran['status'] == 0 and ran['ran_range_flag'] == 0, (form, ran)
    assert ran['ran_qb'] == 1 and ran['ran_ksplit'] == case.get('ksplit', 1), ran
    assert ran['ran_form'] == {'none': 0, 'wave': 1, 'blocks': 2}[form], (form, ran)
    assert ran['ran_touch_blocks'] == (2 * per_row if form == 'blocks' else 0), (form, ran)
    # the touch-ahead rides on a prefetch wave: with touch blocks the wave stays for it alone, without it there is none
    touch_ahead = form != 'none' and case.get('touch_ahead', 0) > 0
    assert ran['ran_touch_ahead'] == touch_ahead, (form, ran)
    assert ran['ran_prefetch_wave'] == (form == 'wave' or touch_ahead), (form, ran)
  for form in ('wave', 'blocks'):
    assert np.array_equal(got[form], got['none']), form
  out = got['blocks'].view(np.float32)
  assert not np.isnan(out).any()
  if case.get('n_valid') == 0:
    np.testing.assert_array_equal(out, 0.0)


# ---- the whole model ---------------------------------------------------------------------------------------------
def test_model_is_bit_identical_in_both_forms_and_across_a_switch(env):
  """tiny preset, 8 steps, CFG, the weight prefetch on (the library turns it off for models this small).  The two carrier
  forms give the same bits; a handle switched 2 -> reset_graph -> 1 gives a fresh handle's bits."""
  torch, native = env
  import msd_amd
  spec = msd_amd.config.preset('tiny_context', num_steps=8)
  batch = helpers.make_batch(spec)
  init_z, noise = helpers.make_noise(spec)

  def fresh(carrier):
    return msd_amd.InferenceModel('synthetic:0', spec, weight_prefetch=True, touch_carrier=carrier)

  def run(model):
    mel, scores = model.predict(batch, init_z=init_z, noise=noise)
    assert np.isfinite(mel).all() and (scores == 0).all()
    return np.asarray(mel, np.float32).view(np.uint32)

  def ran(model):   # touch blocks of the last self- / cross-attention launch the handle enqueued
    return model._get_native().debug_read('touch_blocks').tolist()

  waves = fresh(1)
  want = run(waves)
  assert ran(waves) == [0.0, 0.0]
  model = fresh(2)
  assert np.array_equal(run(model), want)
  assert min(ran(model)) > 0, 'the plan asked for touch blocks and the launcher ran none: %s' % ran(model)
  nm = model._get_native()
  nm.reset_graph()
  nm.set_touch_carrier(1)
  assert np.array_equal(run(model), want) and ran(model) == [0.0, 0.0]
  nm.set_touch_carrier(2)          # and back, next to the cached graph of form 1
  assert np.array_equal(run(model), want) and min(ran(model)) > 0
