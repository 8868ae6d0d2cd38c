"""The vocoder without a GPU: its ABI surface, the float64 specification in audio_codecs.py (stft / istft /
mel_to_linear / griffin_lim) and the WAV plumbing of the command line."""
import os
import re
import sys
import wave

import numpy as np
import pytest

import msd_amd
from msd_amd import audio_codecs as ac
from msd_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import vocoder_cases as vc  # noqa: E402  (tools/vocoder_cases.py: shared with tools/vocoder_report.py)
NEW_SYMBOLS = ('msd_vocoder_create', 'msd_vocoder_destroy', 'msd_vocoder_last_error', 'msd_vocoder_stft',
               'msd_vocoder_istft', 'msd_vocoder_encode', 'msd_vocoder_decode',
               'msd_op_vocoder_phase', 'msd_op_vocoder_load_spec', 'msd_vocoder_debug_read')
F = 70


@pytest.fixture(scope='module')
def x70():
  return vc.signal(F)[None]


@pytest.fixture(scope='module')
def spec70(x70):
  return ac.stft(x70)


def test_symbols_in_header_binding_and_both_libraries():
  import __graft_entry__
  __graft_entry__.build()
  text = open(os.path.join(ROOT, 'include', 'msd_amd.h')).read()
  assert re.search(r'#define\s+MSD_AMD_ABI_VERSION\s+7\b', text) and native.ABI_VERSION == 7   # appended, no bump
  assert '(appended to ABI 7)' in text
  declared = set(re.findall(r'\b(msd_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', text, flags=re.S)))
  for planes in ('f16', 'bf16'):
    lib = native.load(planes)
    assert b'abi 7' in lib.msd_version()
    for name in NEW_SYMBOLS:
      assert name in declared and name in native.EXPORTED_SYMBOLS and hasattr(lib, name), (planes, name)
  # argument checks that need no device: MSD_ERR_INVALID_ARGUMENT = 1
  lib = native.load()
  buf = np.zeros(4, np.float32).ctypes.data
  assert lib.msd_vocoder_create(None, None, None) == 1
  assert lib.msd_vocoder_create(buf, buf, None) == 1
  assert lib.msd_vocoder_stft(None, 1, 640, buf, buf, None) == 1
  assert lib.msd_vocoder_istft(None, 1, 2, buf, buf, None) == 1
  assert lib.msd_vocoder_encode(None, 1, 640, buf, buf, None) == 1
  assert lib.msd_vocoder_decode(None, 1, 2, buf, 4, 0.99, 0, None, buf, None) == 1
  assert lib.msd_vocoder_last_error(None) == b'null vocoder'
  # ... and the test entry points: null pointers, non-positive sizes, more than 2^20 rows
  assert lib.msd_op_vocoder_phase(None, buf, buf, buf, 1, 0.5, None) == 1
  assert lib.msd_op_vocoder_phase(buf, buf, buf, None, 1, 0.5, None) == 1
  assert lib.msd_op_vocoder_phase(buf, buf, buf, buf, 0, 0.5, None) == 1
  assert lib.msd_op_vocoder_phase(buf, buf, buf, buf, 2 ** 20 + 1, 0.5, None) == 1
  assert lib.msd_op_vocoder_load_spec(None, None, buf, 1, 1, 0, None) == 1
  assert lib.msd_op_vocoder_load_spec(buf, None, None, 1, 1, 1, None) == 1
  assert lib.msd_op_vocoder_load_spec(buf, None, buf, 0, 1, 0, None) == 1
  assert lib.msd_op_vocoder_load_spec(buf, None, buf, 1, 2 ** 20, 0, None) == 1
  assert lib.msd_vocoder_debug_read(None, b'mag', buf, 4, None) == 1
  lib.msd_vocoder_destroy(None)


def test_build_checks_the_vocoder_kernels_for_scratch(tmp_path):
  """build() hands check_no_scratch every name of NO_SCRATCH_KERNELS: the vocoder's elementwise kernels are among them,
  and a listing in which one of them has a private segment, or is missing, fails."""
  import importlib.util
  spec = importlib.util.spec_from_file_location('msd_build_native', os.path.join(ROOT, 'music-spectrogram-diffusion_amd', 'build_native.py'))
  bn = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(bn)
  voc = ('voc_pad_signal_kernel', 'voc_exp_kernel', 'voc_load_spec_kernel', 'voc_ola_kernel', 'voc_phase_kernel', 'voc_magnitude_kernel')
  assert set(voc) <= set(bn.NO_SCRATCH_KERNELS) and 'vocoder.h' in bn.HEADERS
  assert 'check_no_scratch(l, NO_SCRATCH_KERNELS)' in open(bn.__file__).read()
  desc = '\t.amdhsa_kernel _ZN3msd%d%sEv\n\t\t.amdhsa_private_segment_fixed_size %d\n\t\t.amdhsa_uses_dynamic_stack 0\n\t.end_amdhsa_kernel\n'
  listing = tmp_path / 'l.s'
  listing.write_text(''.join(desc % (len(k), k, 0) for k in bn.NO_SCRATCH_KERNELS))
  assert bn.check_no_scratch(str(listing), bn.NO_SCRATCH_KERNELS).startswith('OK')
  listing.write_text(''.join(desc % (len(k), k, 16 if k == 'voc_phase_kernel' else 0) for k in bn.NO_SCRATCH_KERNELS))
  with pytest.raises(RuntimeError, match='voc_phase_kernel'):
    bn.check_no_scratch(str(listing), bn.NO_SCRATCH_KERNELS)
  listing.write_text(''.join(desc % (len(k), k, 0) for k in bn.NO_SCRATCH_KERNELS if k != 'voc_ola_kernel'))
  with pytest.raises(RuntimeError, match='voc_ola_kernel'):
    bn.check_no_scratch(str(listing), bn.NO_SCRATCH_KERNELS)


def test_vocoder_needs_a_device(monkeypatch):
  import torch
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  with pytest.raises(native.NativeLibraryError):
    msd_amd.vocoder.GriffinLimVocoder()


def test_istft_inverts_stft(x70, spec70):
  """Measured 4e-14 in float64; the first samples divide by a vanishing window (floored), so they are not restored."""
  assert spec70.shape == (1, F, 513) and spec70.dtype == np.complex128
  y = ac.istft(spec70, F)
  assert y.shape == x70.shape
  assert np.abs(y - x70)[:, 40:].max() <= 1e-12


def test_stft_magnitude_is_the_codecs(x70, spec70):
  """stft is the complex form of stft_magnitude (which frames and transforms float32 arrays): they differ by float32
  rounding, bounded elementwise by the dot-product bound of the 640-term sums."""
  x32 = x70.astype(np.float32)
  got = np.abs(ac.stft(x32.astype(np.float64)))
  want = ac.stft_magnitude(x32, 640, 320, 1024).astype(np.float64)
  bound = vc.stft_bound(x32.astype(np.float64))
  assert (np.abs(got - want) <= bound[:, :, 0] + bound[:, :, 1] + 3 * vc.U * got).all()


def test_griffin_lim_converges(spec70):
  mag = np.abs(spec70)
  phase = vc.closed_form_phase(1, F)
  sc0 = ac.spectral_convergence(ac.griffin_lim(mag, 0, init_phase=(phase[:, :, 0], phase[:, :, 1])), mag)
  sc32 = ac.spectral_convergence(ac.griffin_lim(mag, 32, init_phase=(phase[:, :, 0], phase[:, :, 1])), mag)
  print('spectral convergence: %.4f at 0 iterations, %.4f at 32' % (sc0, sc32))
  assert sc32 <= 0.25 * sc0


def test_matrix_restatement_is_the_specification(spec70):
  """The explicit-basis form the GPU tests use as float32 yardstick computes, in float64, what griffin_lim computes."""
  logmel = np.log(np.clip(np.abs(spec70) @ vc.mel_basis(), 1e-5, 1e8))
  phase = vc.closed_form_phase(1, F)
  want = ac.griffin_lim(ac.mel_to_linear(logmel), 4, init_phase=(phase[:, :, 0], phase[:, :, 1]))
  got = vc.griffin_lim_matrix(logmel, 4, 0.99, phase, np.float64)
  assert vc.rel_l2(got, want) <= 1e-9


def test_silence_decodes_to_silence():
  mag = ac.mel_to_linear(np.full((1, F, 128), np.log(1e-5)))
  assert mag.shape == (1, F, 513) and (mag >= 0).all()
  audio = ac.griffin_lim(mag, 32)
  assert audio.shape == (1, F * 320) and np.isfinite(audio).all() and np.abs(audio).max() < 1e-4


def test_unit_vector_reference_and_emulation_agree_on_the_corner_table():
  """The corner pairs fed to the device (tests/test_gpu_vocoder_edges.py), here through the float32 emulation of voc_unit with
  its reciprocal square root exact and one ulp to either side: within 6 x 2^-24 of the float64 direction, and exact where
  the table says so."""
  c = vc.unit_corners()
  assert c.shape == (18, 2) and c.dtype == np.float32
  top = np.maximum(np.abs(c[:, 0]), np.abs(c[:, 1]))
  assert sorted(set(((top.view(np.uint32) >> 23) & 0xFF)[13:].tolist())) == [252, 253, 254]   # where the clamp acts
  want_c, want_s = vc.unit_reference(c[:, 0], c[:, 1])
  assert np.allclose(want_c ** 2 + want_s ** 2, 1.0, rtol=0, atol=1e-15)
  for ulps in (-1, 0, 1):
    got_c, got_s = vc.unit_emulated(c[:, 0], c[:, 1], ulps)
    err = np.maximum(np.abs(got_c - want_c), np.abs(got_s - want_s))
    print('unit vector emulation, rsqrt %+d ulp: max %.2f x 2^-24' % (ulps, err.max() / vc.U))
    assert (err <= vc.UNIT_BOUND).all()
    assert np.array_equal(np.stack([got_c, got_s], 1)[:3], [[1, 0]] * 3)   # the zero vector, whatever its signs
    assert (got_c[6], got_s[6]) == (0, -1) and (got_c[7], got_s[7]) == (-1, 0)   # on an axis (the emulation copies the kernel's select: this keeps the table in step with it; the evidence is the device's, test_gpu_vocoder_edges.test_unit_vector_on_an_axis_is_exact)
  got_c, got_s = vc.unit_emulated(c[:, 0], c[:, 1])
  assert abs(got_c[4] + np.sqrt(0.5)) < 1e-7 and abs(got_s[4] - np.sqrt(0.5)) < 1e-7   # a denormal pair is no zero vector
  pairs = vc.unit_random(np.random.default_rng(20260101), (64, 513))   # the GPU test's block: every exponent, finite
  assert np.isfinite(pairs).all() and (np.abs(pairs).max(axis=-1) > 0).all()
  got_c, got_s = vc.unit_emulated(pairs[..., 0], pairs[..., 1], 1)
  want_c, want_s = vc.unit_reference(pairs[..., 0], pairs[..., 1])
  assert (np.maximum(np.abs(got_c - want_c), np.abs(got_s - want_s)) <= vc.UNIT_BOUND).all()


@pytest.mark.parametrize('shape', vc.EDGE_SHAPES)
def test_magnitude_bound_holds_for_the_float32_restatement(shape):
  """(128 + 2 + 4) 2^-24 (exp(logmel) . |pinv|): a float32 NumPy run of exp -> pinv product -> max(., 0) stays inside it
  on every element (measured: <= 0.06 of it), and the silent song of a batch is the floor in every bin."""
  b, f = shape
  logmel = vc.logmel_of(vc.songs(b, f))
  want = ac.mel_to_linear(logmel.astype(np.float64))
  bound = vc.mag_bound(logmel)
  err = np.abs(vc.mag_float32(logmel).astype(np.float64) - want)
  print('magnitudes %dx%d: float32 NumPy max err / bound %.4f' % (b, f, (err / np.maximum(bound, 1e-300)).max()))
  assert bound.shape == want.shape == (b, f, 513) and (err <= bound).all()
  if b > 1:
    assert (logmel[1] == np.float32(np.log(1e-5))).all() and (logmel[0] > np.float32(np.log(1e-5))).any()


def test_wav_round_trip(tmp_path):
  from msd_amd import vocoder
  x = vc.signal(4)
  path = str(tmp_path / 'a.wav')
  assert vocoder.write_wav(path, x) == 1.0                  # |x| <= 0.5: written as it is
  with wave.open(path, 'rb') as f:
    assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 16000, x.size)
  back = vocoder.read_wav(path)
  assert back.dtype == np.float32 and np.abs(back * 32768.0 / 32767.0 - x).max() <= 0.5 / 32767 + 1e-7
  gain = vocoder.write_wav(path, 3.0 * x)                  # peak 1.5 > 1: divided by the peak
  assert gain == pytest.approx(1.0 / 1.5)
  assert np.abs(vocoder.read_wav(path)).max() == pytest.approx(32767 / 32768.0)
  with pytest.raises(ValueError):
    vocoder.read_wav(path, sample_rate=44100)
  with pytest.raises(ValueError):
    vocoder.write_wav(path, np.array([0.0, np.nan]))


def test_synthesize_cli_accepts_wav(tmp_path, capsys):
  from msd_amd import synthesize
  from msd_amd.frontend import midi_io, note_sequences
  ns = note_sequences.NoteSequence()
  for k in range(8):
    ns.add_note(pitch=60 + k, velocity=90, start_time=0.5 * k, end_time=0.5 * k + 0.4, program=0)
  path = tmp_path / 'song.mid'
  path.write_bytes(midi_io.note_sequence_to_midi(ns, ticks_per_quarter=480))
  wav = tmp_path / 'x.wav'
  assert synthesize.main([str(path), '--wav', str(wav), '--vocoder-iters', '8', '--context-audio', str(wav), '--dry-run']) == 0
  assert 'segments of 256 frames' in capsys.readouterr().err and not wav.exists()


def test_codec_decode_still_raises():
  with pytest.raises(NotImplementedError):
    ac.MelGAN().decode(np.zeros((1, 4, 128), np.float32))
