"""What predict, invert and loss share, without a device: the one range fallback (InferenceModel._with_range_fallback), the
one encode stage (InferenceModel._encode_batch) with its refusals, and the key arrays NativeModel.sample / .loss hand to
the library."""
import contextlib
import ctypes
import types
import warnings

import numpy as np
import pytest
import torch

from msd_amd import native
from tests.test_host_logic import _bare_model

WARNING = (r"an activation left the half-plane range \(\|x\| > 65504\): switching this model from precision '%s' to '%s' "
           r"\(bfloat16 planes\) and repeating the call")


def _batch(rows=1, **over):
  batch = {'encoder_input_tokens': np.zeros((rows, 128), np.int32),
           'encoder_continuous_inputs': np.zeros((rows, 64, 128), np.float32),
           'encoder_continuous_mask': np.ones((rows, 64), np.int32),
           'decoder_target_tokens': np.zeros((rows, 64, 128), np.float32)}
  batch.update(over)
  return batch


# the three entry points: (name, the _once method behind it, the call)
ENTRIES = [('predict', '_predict_once', lambda m, batch: m.predict(batch)),
           ('invert', '_invert_once', lambda m, batch: m.invert(batch)),
           ('loss', '_loss_once', lambda m, batch: m.loss(batch, times=2))]
IDS = [e[0] for e in ENTRIES]


class _Handle:
  def __init__(self):
    self.closed = 0

  def close(self):
    self.closed += 1


def _overflowing(m, once, precision, range_fallback=True):
  """m's `once` method raises RangeError on its first call and returns a marker on the second; returns (calls, handle)."""
  m.rng, m.range_fallback, m.precision = 'philox', range_fallback, precision
  m._native = handle = _Handle()
  calls = []

  def fn(*args):
    calls.append((m.precision, m._native, args))
    if len(calls) == 1:
      raise native.RangeError('msd_sample failed (msd_status 7): out of range')
    return 'second'
  setattr(m, once, fn)
  return calls, handle


# ---- 1. the fallback ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('old, new', [('f16x3', 'bf16x3'), ('f16', 'bf16')])
@pytest.mark.parametrize('name, once, call', ENTRIES, ids=IDS)
def test_a_range_error_switches_the_planes_and_repeats_the_call_once(name, once, call, old, new):
  m = _bare_model('tiny_context')
  calls, handle = _overflowing(m, once, old)
  with pytest.warns(RuntimeWarning, match=WARNING % (old, new)) as caught:
    assert call(m, _batch()) == 'second'
  assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == 1
  assert len(calls) == 2 and m.precision == new                    # exactly one repeat
  assert calls[0][0] == old and calls[0][1] is handle              # the first call ran on the half planes' handle,
  assert calls[1][0] == new and calls[1][1] is None                # the second after the switch, on a handle yet to be built
  assert handle.closed == 1 and m._native is None
  assert len(calls[0][2]) == len(calls[1][2]) and all(a is b for a, b in zip(calls[0][2], calls[1][2]))   # the same arguments


@pytest.mark.parametrize('precision, range_fallback', [('f16x3', False), ('f16', False), ('bf16x3', True), ('bf16', True)])
@pytest.mark.parametrize('name, once, call', ENTRIES, ids=IDS)
def test_without_a_fallback_the_range_error_comes_out(name, once, call, precision, range_fallback):
  m = _bare_model('tiny_context')
  calls, handle = _overflowing(m, once, precision, range_fallback)
  with warnings.catch_warnings():
    warnings.simplefilter('error')
    with pytest.raises(native.RangeError, match='out of range'):
      call(m, _batch())
  assert len(calls) == 1 and m.precision == precision and handle.closed == 0 and m._native is handle


def test_a_second_range_error_is_not_repeated_again():
  m = _bare_model('tiny_context')
  calls, _ = _overflowing(m, '_predict_once', 'f16x3')

  def always(*args):
    calls.append(args)
    raise native.RangeError('again')
  m._predict_once = always
  with pytest.warns(RuntimeWarning), pytest.raises(native.RangeError, match='again'):
    m.predict(_batch())
  assert len(calls) == 2 and m.precision == 'bf16x3'


# ---- 2. the encode stage -------------------------------------------------------------------------------------------------
class _Stream:
  cuda_stream = 11

  def __init__(self):
    self.waited = 0

  def wait_stream(self, other):
    self.waited += 1

  def synchronize(self):
    pass


class _Native:
  def __init__(self):
    self.encoded = []

  def encode(self, *args, **kw):
    self.encoded.append((args, kw))


def _staged_model(preset='tiny_context'):
  """A bare model whose device is the host: torch's stream and device contexts do nothing, the handle records encode."""
  m = _bare_model(preset)
  m.rng, m.range_fallback, m.precision = 'philox', False, 'f16x3'
  no_context = lambda *a, **k: contextlib.nullcontext()
  m._torch = types.SimpleNamespace(Tensor=torch.Tensor, as_tensor=torch.as_tensor, float32=torch.float32,
                                   cuda=types.SimpleNamespace(device=no_context, stream=no_context, current_stream=lambda dev: None))
  m._stream, nm = _Stream(), _Native()
  m._get_native = lambda: nm
  return m, nm


REFUSALS = [
    (lambda: _batch(encoder_input_tokens=np.zeros((1, 128), np.float32)), 'Input type must be an integer or unsigned integer.'),
    (lambda: _batch(encoder_input_tokens=np.zeros((1, 127), np.int32)), r'encoder_input_tokens must be \[batch, 128\]'),
    (lambda: _batch(rows=2), 'batch 2 exceeds batch_size 1'),
    (lambda: _batch(encoder_continuous_inputs=np.zeros((1, 63, 128), np.float32)), r'encoder_continuous_inputs must be \[batch, 64, 128\]'),
    (lambda: _batch(encoder_continuous_mask=np.ones((1, 65), np.int32)), r'encoder_continuous_mask must be \[batch, 64\]'),
]


@pytest.mark.parametrize('make, match', REFUSALS, ids=['float tokens', 'token width', 'batch size', 'context shape', 'mask shape'])
@pytest.mark.parametrize('name, once, call', ENTRIES, ids=IDS)
def test_the_encode_stage_refuses_before_msd_encode(name, once, call, make, match):
  m, nm = _staged_model()
  with pytest.raises(ValueError, match=match):
    call(m, make())
  assert nm.encoded == []


def test_the_encode_stage_hands_msd_encode_the_checked_batch():
  m, nm = _staged_model()
  batch = _batch(encoder_input_tokens=np.arange(128, dtype=np.int64)[None], encoder_continuous_mask=np.ones((1, 64), bool))
  with m._encode_batch(batch) as (got_nm, b, s, t0, t1):
    assert got_nm is nm and b == 1 and s == 11 and t0 <= t1 and m._stream.waited == 1
    (args, kw), = nm.encoded
  rows, tokens, ctx, mask = args
  assert rows == 1 and kw == dict(stream=11)
  assert tokens.dtype == np.int32 and tokens.flags['C_CONTIGUOUS'] and tokens.tolist() == [list(range(128))]
  assert tuple(ctx.shape) == (1, 64, 128) and ctx.dtype == torch.float32
  assert mask.dtype == np.int32 and mask.shape == (1, 64) and mask.all()
  # a model without a context uploads none
  m, nm = _staged_model('tiny')
  with m._encode_batch({'encoder_input_tokens': np.zeros((1, 128), np.int32)}):
    pass
  assert nm.encoded[0][0][2:] == (None, None)


# ---- 3. the keys NativeModel.sample and .loss hand down ----------------------------------------------------------------
class _Lib:
  """Stands in for the loaded library: records the entry points that are called."""

  def __init__(self):
    self.calls = []

  def __getattr__(self, name):
    if not name.startswith('msd_'):
      raise AttributeError(name)

    def entry(*args):
      self.calls.append((name, args))
      return 0
    return entry


class _T:
  def __init__(self, *shape):
    self.shape = shape

  def data_ptr(self):
    return 4096


def _stub_native():
  nm = object.__new__(native.NativeModel)
  nm.lib, nm.handle = _Lib(), 1
  nm.cfg = native.MsdConfig()
  nm.cfg.cfg_weight, nm.cfg.num_steps, nm.cfg.targets_length, nm.cfg.n_dims = 5.0, 96, 64, 128
  return nm


# (seed, stream_id) -> (per_row, seeds, stream_ids) as the library receives them
KEYS = [((3, 7), (0, [3], [7])), (([3, 4], 7), (1, [3, 4], [7, 7])), ((3, [7, 8]), (1, [3, 3], [7, 8])),
        (([3, 4], [7, 8]), (1, [3, 4], [7, 8])), ((np.int64(3), np.int64(7)), (0, [3], [7])),
        ((np.asarray([3, 4]), (7, 8)), (1, [3, 4], [7, 8]))]


@pytest.mark.parametrize('keys, want', KEYS)
def test_sample_and_loss_pass_the_same_key_arrays(keys, want):
  seed, stream_id = keys
  nm = _stub_native()
  nm.sample(2, None, seed=seed, stream_id=stream_id, steps=24)   # (an entry point that takes per_row and both arrays)
  (name, a), = nm.lib.calls
  assert name == 'msd_sample_steps' and a[3] == want[0]
  for got, exp in zip(a[4:6], want[1:]):
    assert got._type_ is ctypes.c_uint64 and list(got) == exp
  nm = _stub_native()
  nm.loss(2, _T(2, 64, 128), _T(1, 1, 2, 64), [5], seed=seed, stream_id=stream_id)
  s = ctypes.cast(nm.lib.calls[0][1][1], ctypes.POINTER(native.LossArgs)).contents
  assert s.per_row == want[0]
  assert [s.seeds[k] for k in range(len(want[1]))] == want[1] and [s.stream_ids[k] for k in range(len(want[2]))] == want[2]


def test_scalar_keys_reach_the_plain_entry_points_as_scalars():
  nm = _stub_native()
  nm.sample(2, None, seed=3, stream_id=7)
  assert nm.lib.calls[0][0] == 'msd_sample' and nm.lib.calls[0][1][2:4] == (3, 7)
  nm = _stub_native()
  nm.sample(2, None, seed=[3, 4], stream_id=7, rng='threefry')
  (name, a), = nm.lib.calls
  assert name == 'msd_sample_rows' and a[2] == native.RNGS['threefry'] and list(a[3]) == [3, 4] and list(a[4]) == [7, 7]


@pytest.mark.parametrize('keys', [([1, 2, 3], 0), (0, [1]), ([1, 2], [1, 2, 3])])
def test_sample_and_loss_refuse_keys_of_another_length(keys):
  seed, stream_id = keys
  nm = _stub_native()
  with pytest.raises(ValueError, match='entries for a batch of 2'):
    nm.sample(2, None, seed=seed, stream_id=stream_id)
  with pytest.raises(ValueError, match='entries for a batch of 2'):
    nm.loss(2, _T(2, 64, 128), _T(1, 1, 2, 64), [5], seed=seed, stream_id=stream_id)
  assert nm.lib.calls == []


def test_sample_and_loss_refuse_an_unknown_generator_alike():
  nm = _stub_native()
  for call in (lambda: nm.sample(2, None, rng='jax'), lambda: nm.loss(2, _T(2, 64, 128), _T(1, 1, 2, 64), [5], rng='jax')):
    with pytest.raises(ValueError, match=r"rng must be one of \['philox', 'threefry'\]: 'jax'"):
      call()
  assert nm.lib.calls == []
