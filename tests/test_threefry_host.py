"""rng='threefry' without a GPU: the random-access form of jax's Threefry layout (jax_random.normal_at, the host
statement of what one device thread computes) against the array form, bit for bit; the three ABI 7 entry points in the
header, the binding and both built libraries; the command line; the build's scratch check."""
import os
import re

import numpy as np
import pytest

import msd_amd
from msd_amd import jax_random as jr
from msd_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 7, 4096, 32768, 98305]          # odd sizes hit the zero pad of the second half's last counter
NEW_SYMBOLS = ('msd_sample_rng', 'msd_fill_normal_threefry', 'msd_op_threefry')


def _keys():
  return [jr.prng_key(0), jr.prng_key(1701), jr.prng_key((1 << 32) + 9), jr.prng_key((7 << 32) | 0xFFFFFFFF),
          jr.fold_in(jr.prng_key(5), 0), jr.fold_in(jr.prng_key(5), 999), jr.fold_in(jr.prng_key((1 << 32) + 9), 3)]


@pytest.mark.parametrize('n_total', SIZES)
def test_normal_at_equals_the_array_draw_bit_for_bit(n_total):
  rng = np.random.default_rng(n_total)
  for key in _keys():
    full = jr.normal(key, (n_total,)).ravel()
    every = jr.normal_at(key, n_total, np.arange(n_total))
    assert every.dtype == np.float32
    np.testing.assert_array_equal(every.view(np.uint32), full.view(np.uint32))
    # random access: any subset, any order, any shape; the ends and the seam between the two halves among them
    half = (n_total + 1) // 2
    idx = np.concatenate([rng.integers(0, n_total, 64), [0, n_total - 1, half - 1, min(half, n_total - 1)]]).reshape(2, -1)
    np.testing.assert_array_equal(jr.normal_at(key, n_total, idx).view(np.uint32), full[idx].view(np.uint32))


def test_normal_at_is_a_draw_of_the_whole_array():
  """One draw covers the whole [B, T, n] array: row b of a batched call is NOT the draw of a one-row call."""
  key = jr.prng_key(5)
  three = jr.normal(key, (3, 8, 128))
  np.testing.assert_array_equal(jr.normal_at(key, three.size, np.arange(1024, 2048)), three[1].ravel())
  assert not np.array_equal(jr.normal_at(key, 1024, np.arange(1024)), three[0].ravel())
  with pytest.raises(IndexError):
    jr.normal_at(key, 8, [8])


def test_key_words_of_a_seed_beyond_32_bits():
  assert jr.prng_key((1 << 32) + 9) == (1, 9)
  a = jr.normal_at(jr.prng_key((1 << 32) + 9), 4096, np.arange(16))
  b = jr.normal_at(jr.prng_key(9), 4096, np.arange(16))
  assert not np.array_equal(a, b)                   # the high word is part of the key


def _header_functions():
  text = open(os.path.join(ROOT, 'include', 'msd_amd.h')).read()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  return set(re.findall(r'\b(msd_[a-z0-9_]+)\s*\(', text))


def test_abi7_symbols_in_header_binding_and_both_libraries():
  import __graft_entry__
  __graft_entry__.build()
  text = open(os.path.join(ROOT, 'include', 'msd_amd.h')).read()
  assert re.search(r'#define\s+MSD_AMD_ABI_VERSION\s+7\b', text) and native.ABI_VERSION == 7
  assert native.ABI_STRUCT_SIZES[7] == native.ABI_STRUCT_SIZES[6]          # entry points only: msd_config is ABI 6's
  assert re.search(r'MSD_RNG_PHILOX\s*=\s*0\s*,\s*MSD_RNG_THREEFRY\s*=\s*1', text)
  assert (native.MSD_RNG_PHILOX, native.MSD_RNG_THREEFRY) == (0, 1)
  for planes in ('f16', 'bf16'):
    lib = native.load(planes)
    assert b'abi 7' in lib.msd_version()
    for name in NEW_SYMBOLS:
      assert name in _header_functions() and name in native.EXPORTED_SYMBOLS and hasattr(lib, name), (planes, name)
  # argument checks that need no device
  lib = native.load()
  assert lib.msd_fill_normal_threefry(0, -1, None, 16, None) == 1          # MSD_ERR_INVALID_ARGUMENT: no output
  assert lib.msd_op_threefry(4, 0, -1, None, None, 16, None) == 1
  assert lib.msd_sample_rng(None, 1, native.MSD_RNG_THREEFRY, 0, 0, None, None, None, None) == 1


def test_synthesize_cli_accepts_rng_threefry(tmp_path, capsys):
  from msd_amd import synthesize
  from msd_amd.frontend import midi_io, note_sequences
  ns = note_sequences.NoteSequence()
  for k in range(8):
    ns.add_note(pitch=60 + k, velocity=90, start_time=0.5 * k, end_time=0.5 * k + 0.4, program=0)
  path = tmp_path / 'threefry.mid'
  path.write_bytes(midi_io.note_sequence_to_midi(ns, ticks_per_quarter=480))
  assert synthesize.main([str(path), '--rng', 'threefry', '--seed', '5', '--dry-run']) == 0
  assert 'segments of 256 frames' in capsys.readouterr().err
  with pytest.raises(SystemExit):
    synthesize.main([str(path), '--rng', 'mt19937', '--dry-run'])


_DESCRIPTOR = """
	.amdhsa_kernel %s
		.amdhsa_group_segment_fixed_size 0
		.amdhsa_private_segment_fixed_size %d
		.amdhsa_uses_dynamic_stack 0
	.end_amdhsa_kernel
"""


def test_build_refuses_a_sampler_or_fill_kernel_that_uses_scratch(tmp_path):
  """The build reads its own gfx950 listing (build_native.check_no_scratch): an instance of sampler_step_kernel or of
  the Threefry fill with a private segment fails it; so does a listing from which one of them is missing."""
  spec = __import__('importlib').util.spec_from_file_location(
      'msd_build_native', os.path.join(ROOT, 'music-spectrogram-diffusion_amd', 'build_native.py'))
  bn = __import__('importlib').util.module_from_spec(spec)
  spec.loader.exec_module(bn)
  names = ['_ZN3msd19sampler_step_kernelILi%dEEEvNS_13SamplerParamsE' % k for k in range(3)] + \
      ['_ZN3msd22threefry_normal_kernelEPfljjiPKj', '_ZN3msd14unscale_kernelEPKfPfiff']
  good = tmp_path / 'good.s'
  good.write_text(''.join(_DESCRIPTOR % (n, 64 if 'unscale' in n else 0) for n in names))   # other kernels are not its business
  assert bn.check_no_scratch(str(good)).startswith('OK')
  for spilled in (names[1], names[3]):
    bad = tmp_path / 'bad.s'
    bad.write_text(''.join(_DESCRIPTOR % (n, 24 if n == spilled else 0) for n in names))
    with pytest.raises(RuntimeError, match='scratch'):
      bn.check_no_scratch(str(bad))
  gone = tmp_path / 'gone.s'
  gone.write_text(''.join(_DESCRIPTOR % (n, 0) for n in names[:3]))
  with pytest.raises(RuntimeError, match='threefry_normal_kernel'):
    bn.check_no_scratch(str(gone))
