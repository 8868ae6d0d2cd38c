"""-m gpu: the tail every sampler-update kernel ends with -- z as fp32, z's 16-bit operand planes, the half-plane range
flag, the published scan index -- one kernel at a time through msd_op_sampler_step_planes: sampler_step_kernel in its
plain, keep / release and guided instances, sampler_multistep_kernel in its plain and guided ones, each for the three
model outputs and the four precisions (both library builds).

z against the forms' float64 specifications (oracle.sampler.eval_step, tests/keep_spec.py, multistep_spec.py,
guidance_spec.py) with the stand-alone ops' criterion, and bit for bit the existing entry point's; the merged planes bit for
bit helpers.planes_merged(z_out) (tests/test_planes_merged_host.py); sizes of one thread, one full block, and three
blocks with a partial last one (the block that publishes the index); 65504 exactly and one float32 above it in every
element of the launch's last float4."""
import numpy as np
import pytest

import msd_amd
from tests import guidance_spec as gs, helpers, keep_spec, multistep_spec as ms
from tests.helpers import gpu_torch  # noqa: F401  (the `torch` fixture)

pytestmark = pytest.mark.gpu

PRECISIONS = ['f16x3', 'f16', 'bf16x3', 'bf16']
MODES = ['eps', 'x0', 'v']
# (form, sampler): DDPM and DDIM where the form has both; the multistep update draws nothing and reads no sampler
FORMS = [('plain', 'ddpm'), ('plain', 'ddim'), ('keep', 'ddpm'), ('keep', 'ddim'), ('release', 'ddpm'), ('release', 'ddim'),
         ('multistep', 'ddpm'), ('guided', 'ddpm'), ('guided', 'ddim'), ('multistep_guided', 'ddpm')]
# one thread; one full block; three blocks of 1024 elements, the last one partial (37 threads): the publishing block.
# Frames of 4 / 128 / 12 elements for the keep forms.
SHAPES = [(1, 1, 4), (1, 8, 128), (1, (2 * 1024 + 4 * 37) // 12, 12)]
# guided: a row is a whole number of blocks; 1.0 = the one-pass branch, first and last
GUIDED = [((3, 8, 128), [1.0, 5.0, 0.0]), ((2, 16, 128), [2.5, 1.0])]
# the range cases: element 0 and the launch's last float4 lie in rows of weight 1, a guided row between them
RANGE_GUIDED = ((3, 8, 128), [1.0, 5.0, 1.0])
BIG = np.float32(65504.0)
ABOVE = np.nextafter(BIG, np.float32(np.inf))


def _id(v):
  return '-'.join(v) if isinstance(v, tuple) else str(v)


def _guided(form):
  return form.endswith('guided')


def _multistep(form):
  return form.startswith('multistep')


def _geometries(form):
  return GUIDED if _guided(form) else [(s, None) for s in SHAPES]


def _cfg(spec, precision):
  from msd_amd import inference
  return inference._to_native_config(spec, msd_amd.audio_codecs.MelGAN(), 1, precision)


def _frames(form, shape, i):
  """The keep forms' per-frame words (flags for 'keep', release words for 'release') and which frames are known at index i."""
  f = np.arange(shape[1])
  if form == 'keep':
    words = np.where(f % 3 == 0, 7, 0).astype(np.int32)[None]   # (any non-zero flag)
    return words, words != 0
  kinds = np.array([1, 0, i, i + 1, i + 2], np.int32)
  words = kinds[f % 5][None]
  return words, (words >= 1) & (i >= words - 1)


def _run(torch, form, cfg, i, a, planes):
  """One launch of `form` on the inputs a: through msd_op_sampler_step_planes (planes) or the form's existing entry point.
  -> dict(z, planes, flag, next, x0_prev)"""
  from msd_amd import native
  d = lambda x, t=np.float32: None if x is None else helpers.dev(torch, x, t)
  shape = a['z'].shape
  z_out = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
  zp = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
  prev = None
  if _multistep(form):
    prev = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda') if a['first'] else d(a['prev'])
  z, oc, ou, nz = d(a['z']), d(a['oc']), d(a['ou']), d(a['nz'])
  r = dict(planes=None, flag=None, next=None)
  if planes:
    kw = {}
    if form == 'keep':
      kw = dict(known_scaled=d(a['xk']), keep_mask=d(a['words'], np.int32))
    elif form == 'release':
      kw = dict(known_scaled=d(a['xk']), release=d(a['words'], np.int32))
    if _multistep(form):
      kw.update(x0_prev=prev, first=a['first'])
    if _guided(form):
      kw.update(weights=a['weights'])
    r['flag'], r['next'] = native.op_sampler_step_planes(cfg, i, z, oc, ou, z_out, zp, noise=nz, **kw)
    r['planes'] = zp.cpu().numpy()
  elif form == 'plain':
    native.op_sampler_step(cfg, i, z, oc, ou, nz, z_out)
  elif form == 'keep':
    native.op_sampler_step_keep(cfg, i, z, oc, ou, nz, d(a['xk']), d(a['words'], np.int32), z_out)
  elif form == 'release':
    native.op_sampler_step_release(cfg, i, z, oc, ou, nz, d(a['xk']), d(a['words'], np.int32), z_out)
  elif form == 'multistep':
    native.op_sampler_step_multistep(cfg, i, z, oc, ou, prev, a['first'], z_out)
  elif form == 'guided':
    native.op_sampler_step_guided(cfg, i, z, oc, ou, nz, a['weights'], z_out)
  else:
    native.op_sampler_step_multistep_guided(cfg, i, z, oc, ou, prev, a['first'], a['weights'], z_out)
  r['z'] = z_out.cpu().numpy()
  r['x0_prev'] = None if prev is None else prev.cpu().numpy()
  return r


def _reference(form, dc, i, a):
  """The form's specification on the inputs a, in float64 and float32."""
  from oracle import backend, sampler
  steps = dc.sampler.schedule.num_steps
  shape = a['z'].shape
  out = {}
  for name, xp in (('f32', backend.NumpyBackend('float32')), ('f64', backend.NumpyBackend('float64'))):
    rows = []
    for b in range(shape[0] if _guided(form) else 1):
      row = slice(b, b + 1) if _guided(form) else slice(None)
      cfg_b = gs.with_weight(dc, a['weights'][b]) if _guided(form) else dc
      batch = 1 if _guided(form) else shape[0]
      pred = lambda z, time, include_conditioning, _xp=xp, _r=row: _xp.asarray((a['oc'] if include_conditioning else a['ou_all'])[_r])
      noise = [None] * steps
      noise[i] = xp.asarray(a['nz'][row])
      zr = xp.asarray(a['z'][row])
      if _multistep(form):
        got = ms.step(xp, cfg_b, zr, i, pred, xp.asarray(a['prev'][row]), a['first'])[0]
      elif form in ('keep', 'release'):
        got = keep_spec.eval_step_keep(xp, noise, cfg_b, batch, pred, xp.asarray(a['xk']), keep_spec.frame_mask(xp, a['known']))(zr, i)
      else:
        got = sampler.eval_step(xp, noise, cfg_b, batch, pred)(zr, i)
      rows.append(np.asarray(got, np.float64))
    out[name] = np.concatenate(rows, 0)
  return out


# (form, sampler, mode) -> per (geometry, scan index): the inputs, the two evaluations of the specification and the existing
# entry point's result -- computed once, shared by the four precisions (none of them depends on the precision)
_shared = {}


def _cases(torch, form, smp, mode):
  key = (form, smp, mode)
  if key in _shared:
    return _shared[key]
  spec = helpers.sampler_spec(sampler=smp, model_output=mode)
  _, dc = helpers.oracle_configs(spec)
  steps = dc.sampler.schedule.num_steps
  cfg = _cfg(spec, 'f16x3')
  rng = np.random.default_rng(5)
  cases = []
  for shape, weights in _geometries(form):
    for i in (steps - 1, steps // 2, 1, 0):
      z, oc, ou, nz = (rng.standard_normal(shape).astype(np.float32) for _ in range(4))
      if i > steps // 2 and mode == 'eps':   # at logsnr ~ -20 only eps ~ z leaves x0 inside [-1, 1]
        oc, ou = z + 1e-5 * oc, z + 1e-5 * ou
      a = dict(z=z, oc=oc, ou=ou, ou_all=ou, nz=nz, weights=weights, first=i == steps - 1,
               xk=rng.uniform(-1.0, 1.0, shape).astype(np.float32), prev=rng.uniform(-1.0, 1.0, shape).astype(np.float32))
      if form in ('keep', 'release'):
        a['words'], a['known'] = _frames(form, shape, i)
      cases.append(dict(i=i, a=a, ref=_reference(form, dc, i, a), old=_run(torch, form, cfg, i, a, planes=False)))
  _shared[key] = (spec, cases)
  return _shared[key]


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('form', FORMS, ids=_id)
def test_planes_flag_and_index_of_every_form(torch, form, mode, precision):
  """(a) z_out with planes requested: the existing entry point's bits, and the float64 criterion of the stand-alone sampler
  ops (e_dev <= 1e-6 + 4 e_f32, scaled).  (b) the merged planes: helpers.planes_merged(z_out) bit for bit, every element;
  with two planes neither a copy of z nor the hi plane alone.  (c) the published index: i - 1, -1 at i == 0, from a full
  and from a partial last block."""
  form, smp = form
  spec, cases = _cases(torch, form, smp, mode)
  cfg = _cfg(spec, precision)
  two = precision.endswith('x3')
  one_plane = precision[:-2] if two else precision
  not_z = not_hi = False
  for c in cases:
    i, a, ref, old = c['i'], c['a'], c['ref'], c['old']
    got = _run(torch, form, cfg, i, a, planes=True)
    what = '%s %s %s %s n=%d i=%d' % (form, smp, mode, precision, a['z'].size, i)
    # (a)
    np.testing.assert_array_equal(helpers.bits(got['z']), helpers.bits(old['z']), err_msg=what)
    if _multistep(form):
      np.testing.assert_array_equal(helpers.bits(got['x0_prev']), helpers.bits(old['x0_prev']), err_msg=what)
    scale = max(1.0, float(np.abs(ref['f64']).max()))
    e_dev = np.abs(got['z'].astype(np.float64) - ref['f64']).max() / scale
    e_f32 = np.abs(ref['f32'] - ref['f64']).max() / scale
    print('%s: scaled error device %.3e / float32 %.3e' % (what, e_dev, e_f32))
    assert e_dev <= 1e-6 + 4 * e_f32, (what, e_dev, e_f32)
    # (b)
    want = helpers.planes_merged(got['z'], precision)
    np.testing.assert_array_equal(helpers.bits(got['planes']), helpers.bits(want), err_msg=what)
    not_z = not_z or bool((got['planes'] != got['z']).any())
    not_hi = not_hi or bool((got['planes'] != helpers.planes_merged(got['z'], one_plane)).any())
    # (c)
    assert got['next'] == i - 1, (what, got['next'])
    assert got['flag'] == 0, (what, got['flag'])
  assert not_z, 'the planes are a copy of z'
  assert not_hi == two, 'the lo plane is missing' if two else 'one plane holds more than its hi values'


# --------------------------------------------------------------------------------------------------
# the range flag
# --------------------------------------------------------------------------------------------------
def _x0_setup(form, smp, shape, weights):
  """The setup in which the update returns an input's bits: model output x0, clip off, scan index 0, weight 1 (not guided:
  cfg_weight 1, one pass; guided: the first and the last row's weight is 1) -- sampler_update returns x0 = o_cond at i == 0, the multistep
  form too; a kept frame returns xk.  Everything a unit normal."""
  spec = helpers.sampler_spec(sampler=smp, model_output='x0', clip=False, cfg_weight=5.0 if _guided(form) else 1.0)
  rng = np.random.default_rng(23)
  z, oc, ou, nz, xk, prev = (rng.standard_normal(shape).astype(np.float32) for _ in range(6))
  a = dict(z=z, oc=oc, ou=ou if _guided(form) else None, nz=nz, xk=xk, prev=prev, first=False, weights=weights)
  assert weights is None or weights[0] == weights[-1] == 1.0
  return spec, a


def _placements(form, shape):
  """(element, through) of the single large value: each element of the launch's last float4 -- the last thread of the last,
  partial, block; guided: the last four of the last row -- and element 0; the keep forms once through xk in a kept frame and
  once through o in a free one."""
  n = int(np.prod(shape))
  spots = [n - 4, n - 3, n - 2, n - 1, 0]
  if form in ('keep', 'release'):
    return [(e, t) for e in spots for t in ('xk', 'o')]
  return [(e, 'o') for e in spots]


def _place(form, a, e, through, value):
  """a with `value` at flat element e, and the keep forms' frame of e kept (through xk) or free (through o)."""
  b = dict(a)
  src = 'xk' if through == 'xk' else 'oc'
  arr = a[src].copy()
  arr.reshape(-1)[e] = value
  b[src] = arr
  if form in ('keep', 'release'):
    n_dims = a['z'].shape[-1]
    f = np.arange(a['z'].shape[1])
    kept = (f % 2 == 0) if through == 'o' else (f % 2 == 1)
    kept[e // n_dims] = through == 'xk'
    # flags: any non-zero; words at i == 0: 1 = known, 0 and >= 2 = free
    b['words'] = (np.where(kept, 7, 0) if form == 'keep' else np.where(kept, 1, np.where(f % 3 == 0, 2, 0))).astype(np.int32)[None]
  return b


def _inputs_bits(form, b):
  """What z_out holds in the setup above, and where: o_cond, xk on the kept frames; guided, on the rows of weight 1."""
  shape = b['z'].shape
  want = b['oc'].copy()
  if form in ('keep', 'release'):
    kept = np.broadcast_to((b['words'] == (1 if form == 'release' else 7))[..., None], shape)
    want[kept] = b['xk'][kept]
  sel = np.ones(shape, bool)
  if _guided(form):
    sel[np.asarray(b['weights']) != 1.0] = False
  return want, sel


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('form', FORMS, ids=_id)
def test_range_flag_at_the_half_plane_limit(torch, form, precision):
  """65504 exactly passes -- z_out and the merged planes hold it, the flag word is 0 --, one float32 above it raises
  RangeError on the half-plane build, with either sign, in every element of the launch's last float4 (a partial block's) and
  in element 0; the bfloat16-plane build takes all three."""
  from msd_amd import native
  form, smp = form
  half = not precision.startswith('bf16')
  shape, weights = RANGE_GUIDED if _guided(form) else (SHAPES[2], None)
  n = int(np.prod(shape))
  assert _guided(form) or n % 1024 != 0
  spec, a = _x0_setup(form, smp, shape, weights)
  cfg = _cfg(spec, precision)
  for e, through in _placements(form, shape):
    for value in (BIG, ABOVE, -ABOVE):
      what = '%s %s %s element %d of %d through %s, %r' % (form, smp, precision, e, n, through, float(value))
      b = _place(form, a, e, through, value)
      if half and abs(value) > BIG:
        with pytest.raises(native.RangeError):
          _run(torch, form, cfg, 0, b, planes=True)
          pytest.fail('no RangeError: ' + what)
        continue
      got = _run(torch, form, cfg, 0, b, planes=True)
      assert got['flag'] == 0 and got['next'] == -1, (what, got['flag'], got['next'])
      assert got['z'].reshape(-1)[e] == value, (what, got['z'].reshape(-1)[e])
      np.testing.assert_array_equal(helpers.bits(got['planes']), helpers.bits(helpers.planes_merged(got['z'], precision)), err_msg=what)
      if value == BIG and precision != 'bf16':   # (65504 = 65536 - 32 takes two bfloat16 planes; one holds 65536)
        assert got['planes'].reshape(-1)[e] == BIG, (what, got['planes'].reshape(-1)[e])
      # every other element is untouched by the large one: the inputs' bits
      want, sel = _inputs_bits(form, b)
      np.testing.assert_array_equal(helpers.bits(got['z'][sel]), helpers.bits(want[sel]), err_msg=what)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('form', FORMS, ids=_id)
def test_a_nan_stays_visible(torch, form, precision):
  """One NaN in o_cond, in the setup above: NaN at that element of z_out and of the merged planes, every other element the
  inputs' bits.  The range flag sees Inf but not NaN (RangeCheck, common.h): the NaN call passes with flag 0, an Inf in its
  place raises on the half-plane build."""
  from msd_amd import native
  form, smp = form
  shape, weights = RANGE_GUIDED if _guided(form) else (SHAPES[2], None)
  n = int(np.prod(shape))
  spec, a = _x0_setup(form, smp, shape, weights)
  cfg = _cfg(spec, precision)
  e = n - 3
  b = _place(form, a, e, 'o', np.float32(np.nan))
  got = _run(torch, form, cfg, 0, b, planes=True)
  assert got['flag'] == 0 and got['next'] == -1
  nan = np.zeros(n, bool)
  nan[e] = True
  nan = nan.reshape(shape)
  for what in ('z', 'planes'):
    np.testing.assert_array_equal(np.isnan(got[what]), nan, err_msg=what)
  want, sel = _inputs_bits(form, b)
  sel = sel & ~nan
  np.testing.assert_array_equal(helpers.bits(got['z'][sel]), helpers.bits(want[sel]))
  np.testing.assert_array_equal(helpers.bits(got['planes'][sel]), helpers.bits(helpers.planes_merged(want, precision)[sel]))
  b = _place(form, a, e, 'o', np.float32(np.inf))
  if precision.startswith('bf16'):
    assert _run(torch, form, cfg, 0, b, planes=True)['z'].reshape(-1)[e] == np.inf
  else:
    with pytest.raises(native.RangeError):
      _run(torch, form, cfg, 0, b, planes=True)


def test_the_op_refuses_what_its_entry_points_refuse(torch):
  """A precision of the other library build, forms that do not combine, missing outputs."""
  from msd_amd import native
  spec = helpers.sampler_spec(cfg_weight=1.0)
  t = lambda: torch.zeros((1, 8, 128), dtype=torch.float32, device='cuda')
  words = torch.zeros((1, 8), dtype=torch.int32, device='cuda')
  cfg = _cfg(spec, 'f16x3')
  assert native.op_sampler_step_planes(cfg, 3, t(), t(), None, t(), t()) == (0, 2)
  with pytest.raises(ValueError):   # known frames with the multistep update
    native.op_sampler_step_planes(cfg, 3, t(), t(), None, t(), t(), known_scaled=t(), keep_mask=words, x0_prev=t())
  with pytest.raises(ValueError):   # ... and with row weights
    native.op_sampler_step_planes(cfg, 3, t(), t(), t(), t(), t(), known_scaled=t(), keep_mask=words, weights=[1.0])
  with pytest.raises(ValueError):   # a scan index beyond the table
    native.op_sampler_step_planes(cfg, 50, t(), t(), None, t(), t())
  # the half-plane library asked for bfloat16 planes: MSD_ERR_UNSUPPORTED
  a = native.SamplerPlanesArgs()
  a.struct_size = native.ctypes.sizeof(native.SamplerPlanesArgs)
  bf = _cfg(spec, 'bf16x3')
  bf.struct_size = native.config_struct_size(native.load())
  z = [t() for _ in range(4)]
  a.step_index, a.n, a.cfg = 3, z[0].numel(), native.ctypes.pointer(bf)
  a.z, a.out_cond, a.z_out, a.z_planes_out = (x.data_ptr() for x in z)
  assert native.load().msd_op_sampler_step_planes(native.ctypes.byref(a), 0) == 6
