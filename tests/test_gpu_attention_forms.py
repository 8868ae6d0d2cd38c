"""-m gpu: attention_kernel in every form the decoder launches it (csrc/msd_api.hip attention<NP>() and its callers),
one launch at a time through msd_op_attention_launch -- interleaved q | k, several segments, windows of a K / V^T cache,
the key split with both merges, the prefetch wave with and without its K / V^T touch-ahead, un-normalised queries at a
column of a wider buffer.  The cases are tests/attention_forms.py's matrix (checked without a GPU by
tests/test_attention_forms_host.py).  Every launch is held against three things:
  a. the plain op (msd_op_attention_ex) on each segment's contiguous q, k, v: the SAME BITS, whatever block shape,
     prefetch wave or touch-ahead the launch ran on -- the kernel contracts nothing by itself (fp contract(off)), a touch
     has no reader, and both merges are one function.  Any wrong stride, window, segment or ticket group shows here;
  b. the float64 oracle per segment, under the bounds tests/test_gpu_ops.py holds for the same input scales;
  c. bookkeeping: a segment without keys is exact zeros, no element is NaN, and the launcher ran what the mirror of its
     rule expects.
The op's planes are NaN outside each segment's window.  What that can show: a V^T column read outside the window reaches
the output as NaN (a zero weight times NaN), and so does an output row nobody stored.  What it cannot: K rows read outside
the window are always masked (their keys lie behind n_keys), so their values never reach the output -- the K clamp
(attention.h: last_row = k_rows - 1 in MSD_A_ISSUE and kv_touch_ahead) is checked by reading the code, not by a value."""
import ctypes
import dataclasses

import numpy as np
import pytest

from tests import attention_forms as af
from tests.helpers import attention_ref

pytestmark = pytest.mark.gpu

TOL = {'f16x3': 2e-5, 'bf16x3': 3e-5, 'f16': 5e-3, 'bf16': 3e-2}   # relative to max(1, |ref|max): test_gpu_ops.py test_attention
QP_TOL = {1: 6e-4, 2: 3e-4, 3: 8e-4}                                # 'f16x3' with query-side single planes


@pytest.fixture(scope='module')
def env():
  import torch
  import msd_amd
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  msd_amd.native.load()
  return torch, msd_amd.native


def _dev(torch, a):
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _upload(torch, arrays):
  d = {'q': _dev(torch, arrays['q'])}
  d['k'] = d['q'] if arrays['k'] is arrays['q'] else _dev(torch, arrays['k'])   # self-attention: ONE buffer
  d['v'] = _dev(torch, arrays['v'])
  d['n_keys'] = _dev(torch, arrays['n_keys'])
  if 'q_ssq' in arrays:
    d['q_ssq'] = _dev(torch, arrays['q_ssq'])
  return d


def _launch(env, case, d):
  torch, native = env
  o = torch.full((case.segs * case.rows, case.J), float('nan'), dtype=torch.float32, device='cuda')
  ran = native.op_attention_launch(case.prec, o=o, **d, **af.launch_fields(case))
  return o.cpu().numpy(), ran


def _tolerance(case):
  if case.qp:
    assert case.prec == 'f16x3'
    return QP_TOL[case.qp]
  return TOL[case.prec]


@pytest.mark.parametrize('case', af.MATRIX, ids=lambda c: c.id)
def test_launch_form(env, case):
  torch, native = env
  q_s, k_s, v_s, ssq_s, rstd_s = af.make_inputs(case)
  d = _upload(torch, af.pack(case, q_s, k_s, v_s, ssq_s))
  got, ran = _launch(env, case, d)
  # c. bookkeeping
  assert ran == af.expected_ran(case)
  assert not np.isnan(got).any(), 'NaN: a V^T read outside the window, or a row nobody wrote'
  for s, got_s in enumerate(af.split_output(case, got)):
    n = case.n_keys[s]
    # a. the plain op on this segment alone (its keys behind n carry the random values, not the loud ones)
    o = torch.full((case.rows, case.J), float('nan'), dtype=torch.float32, device='cuda')
    native.op_attention_ex(case.prec, _dev(torch, q_s[s]), _dev(torch, k_s[s]), _dev(torch, v_s[s]), o, case.heads,
                           ksplit=case.ksplit, merge_in_launch=case.merge_in_launch, allow_qb4=case.allow_qb4,
                           q_ssq=None if ssq_s is None else _dev(torch, ssq_s[s]), n_keys_valid=n, qp=case.qp)
    plain = o.cpu().numpy()
    assert np.array_equal(got_s, plain), (s, n, np.abs(got_s - plain).max())
    if n == 0:
      np.testing.assert_array_equal(got_s, 0.0)
      continue
    # b. float64
    ref = attention_ref(q_s[s], k_s[s], v_s[s], case.heads, n, None if rstd_s is None else rstd_s[s])
    err = np.abs(got_s - ref).max() / max(1.0, np.abs(ref).max())
    print('%s segment %d, %d keys: max err %.2e' % (case.id, s, n, err))
    assert err < _tolerance(case), (s, n, err)
  if case.touch_ahead:   # the same launch without the touch-ahead, and without the prefetch wave: the same bits
    for twin in (dataclasses.replace(case, touch_ahead=0), dataclasses.replace(case, touch_ahead=0, prefetch=False)):
      got2, ran2 = _launch(env, twin, d)
      assert ran2 == af.expected_ran(twin) and ran2['ran_touch_ahead'] == 0
      assert np.array_equal(got, got2), (twin.id, np.abs(got - got2).max())


def _small(torch, heads=1, rows=64, ka=64, ldq=None, ldk=None):
  j = 64 * heads
  rng = np.random.default_rng(3)
  t = lambda *shape: _dev(torch, (rng.standard_normal(shape) * 0.35).astype(np.float32))
  return dict(heads=heads, segs=1, q_rows_per_seg=rows, ldq=ldq or j, q_col=0, ldk=ldk or j, k_col=0, k_alloc_rows=ka, k_row0=0,
              k_rows=ka, q=t(rows, ldq or j), k=t(ka, ldk or j), v=t(1, ka, j), n_keys=_dev(torch, np.asarray([ka], np.int32)),
              o=torch.zeros((rows, j), dtype=torch.float32, device='cuda'))


def test_argument_checks(env):
  """Bad sizes, a window outside its allocation or off the 32-key grid, head columns that do not fit a row, touch_ahead
  outside 0 .. 16, a count beyond the window: MSD_ERR_INVALID_ARGUMENT; un-normalised queries on a one-plane precision
  and a precision of the other build: MSD_ERR_UNSUPPORTED -- the codes of msd_op_attention_ex."""
  torch, native = env
  ok = _small(torch)
  assert native.op_attention_launch('f16x3', **ok) == {'ran_qb': 1, 'ran_prefetch_wave': 0, 'ran_touch_ahead': 0, 'ran_ksplit': 1}
  wide = dict(_small(torch, ka=128), n_keys=_dev(torch, np.asarray([64], np.int32)))
  native.op_attention_launch('f16x3', **dict(wide, k_row0=64, k_rows=64))   # a window at the end of the allocation: fine
  bad = [dict(ok, heads=0), dict(ok, segs=0), dict(ok, q_rows_per_seg=96), dict(ok, q_rows_per_seg=0), dict(ok, qp=4),
         dict(ok, ksplit=0), dict(ok, ksplit=9), dict(ok, repeats=0), dict(ok, q=None), dict(ok, n_keys=None), dict(ok, o=None),
         dict(wide, k_row0=64, k_rows=128),              # k_row0 + k_rows > k_alloc_rows
         dict(wide, k_row0=96, k_rows=64),
         dict(wide, k_rows=48), dict(wide, k_rows=0),    # k_rows % 32
         dict(wide, k_row0=16, k_rows=64),               # ... and the window's start
         dict(ok, k_alloc_rows=-64),
         dict(ok, q_col=8), dict(ok, ldq=56),            # the heads' columns do not fit ldq
         dict(ok, k_col=64), dict(ok, ldk=32), dict(ok, q_col=-8),
         dict(ok, touch_ahead=-1), dict(ok, touch_ahead=17), dict(ok, pf_late=2),
         dict(ok, prefetch_rows=64), dict(ok, prefetch_rows=64, prefetch_k=96), dict(ok, prefetch_rows=64, prefetch_k=8192),
         dict(ok, n_keys=_dev(torch, np.asarray([65], np.int32))), dict(ok, n_keys=_dev(torch, np.asarray([-1], np.int32))),
         dict(ok, q_ssq=torch.ones((64, 6), dtype=torch.float32, device='cuda'), q_tiles=6),
         dict(ok, q_ssq=torch.ones((64, 36), dtype=torch.float32, device='cuda'), q_tiles=36),
         dict(ok, k=ok['q'], ldk=64, k_alloc_rows=128, k_rows=128)]   # shared q | k: the key allocation is the segment
  for fields in bad:
    with pytest.raises(ValueError):
      native.op_attention_launch('f16x3', **fields)
  with pytest.raises(NotImplementedError):
    native.op_attention_launch('f16', **dict(ok, q_ssq=torch.ones((64, 24), dtype=torch.float32, device='cuda'), q_tiles=24))
  with pytest.raises(NotImplementedError):
    native.op_attention_launch('bf16x3', planes='f16', **ok)
  with pytest.raises(TypeError):
    native.op_attention_launch('f16x3', **dict(ok, ran_qb=1))
  # struct_size comes first and must be this ABI's: a larger (unknown trailing bytes) or smaller struct is rejected
  lib = native.load()
  for delta in (8, -8):
    args = native.AttentionLaunchArgs()
    args.struct_size = ctypes.sizeof(native.AttentionLaunchArgs) + delta
    assert lib.msd_op_attention_launch(ctypes.byref(args), None) == native.MSD_ERR_INVALID_ARGUMENT
  assert native.AttentionLaunchArgs.struct_size.offset == 0
