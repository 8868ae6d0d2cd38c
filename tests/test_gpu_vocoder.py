"""The device vocoder (csrc/vocoder.h behind msd_vocoder_*) against its float64 specification in audio_codecs.py.

Shapes: F = 70 frames (no multiple of the 64-row GEMM tile, and more than one tile) and B = 2 songs (the row that
straddles two songs in the batched launch) -- ONE instance of the batched layout, on a signal without silence.  The other
shapes (song boundaries on tile edges, one song, one row, three songs), silent songs, sample counts on and next to a
multiple of the hop, the work buffers' layout invariants, the unit vector's corners and handle reuse across entry points:
tests/test_gpu_vocoder_edges.py.  The GEMM-shaped operations are held to the forward error bound of a
float32 dot product, |err| <= (K + 2) 2^-24 (|A| . |B|) elementwise, built here from float64 quantities
(tools/vocoder_cases.py); a wrong row, sign, window or pad column is O(1) on that scale.  Waveforms of a few Griffin-Lim
iterations are held to 16x the distance a float32 NumPy restatement keeps from float64; long runs to the spectral
convergence of the float64 run (sample values of two float32-class runs drift apart: 1.7e-3 relative at 32 iterations)."""
import os
import sys

import numpy as np
import pytest

import msd_amd
from msd_amd import audio_codecs as ac
from tests import helpers

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import vocoder_cases as vc  # noqa: E402  (tools/vocoder_cases.py: shared with tools/vocoder_report.py)

pytestmark = pytest.mark.gpu

F, B = 70, 2


@pytest.fixture(scope='module')
def voc():
  import torch
  assert torch.cuda.is_available()
  return msd_amd.vocoder.GriffinLimVocoder()


@pytest.fixture(scope='module')
def ragged():
  """float32 [2, 70 * 320 - 37]: the last frame is zero-extended; DC and Nyquist carry signal (0.01 + 0.01 (-1)^i);
  song 1 is song 0 reversed in time."""
  x = vc.two_songs(F) + 0.01 + 0.01 * (-1.0) ** np.arange(F * 320)
  return np.ascontiguousarray(x[:, :F * 320 - 37], np.float32)


@pytest.fixture(scope='module')
def case():
  """The decode case: float32 log-mel [2, 70, 128] of the two songs, explicit phases, the float64 target magnitudes."""
  logmel = np.log(np.clip(np.abs(ac.stft(vc.two_songs(F))) @ vc.mel_basis(), 1e-5, 1e8)).astype(np.float32)
  phase = vc.closed_form_phase(B, F).astype(np.float32)
  return {'logmel': logmel, 'phase': phase, 'mag': ac.mel_to_linear(logmel.astype(np.float64))}


def _reference(case, n_iters, phase=None):
  ph = (case['phase'] if phase is None else phase).astype(np.float64)
  return ac.griffin_lim(case['mag'], n_iters, 0.99, init_phase=(ph[:, :, 0], ph[:, :, 1]))


def _parity(case, got, n_iters, phase=None):
  """(distance of `got` to the float64 run, distance of the float32 NumPy restatement to it)"""
  ph = case['phase'] if phase is None else phase
  want = _reference(case, n_iters, ph)
  yard = vc.griffin_lim_matrix(case['logmel'], n_iters, 0.99, ph, np.float32)
  return vc.rel_l2(got, want), vc.rel_l2(yard, want)


def _assert_parity(case, got, n_iters, phase=None, what=''):
  dev, yard = _parity(case, got, n_iters, phase)
  print('%s %d iterations: device %.3e, float32 NumPy %.3e from float64 (ratio %.2f)' % (what, n_iters, dev, yard, dev / yard))
  assert dev <= 16.0 * yard and dev <= 1e-4, (dev, yard)


def test_stft(voc, ragged):
  got = voc.stft(ragged)
  x = ragged.astype(np.float64)
  spec = ac.stft(x)
  want = np.stack([spec.real, spec.imag], axis=2)
  bound = vc.stft_bound(x)
  assert got.shape == (B, F, 2, 513)
  err = np.abs(got - want)
  print('stft: max err / bound %.4f; bound / max|X| %.1e' % ((err / np.maximum(bound, 1e-300)).max(), bound.max() / np.abs(want).max()))
  assert (err <= bound).all()


def test_istft(voc):
  spec32 = vc.pack_spec(ac.stft(vc.two_songs(F)))
  spec = spec32[:, :, 0].astype(np.float64) + 1j * spec32[:, :, 1].astype(np.float64)
  got = voc.istft(spec32)
  want = ac.istft(spec, F)
  _, inv = vc.dft_bases()
  a_abs = np.abs(spec32.astype(np.float64)).reshape(B, F, 2 * 513)
  bound = (1026 + 2 + 4) * vc.U * vc.overlap_add(a_abs @ np.abs(inv).reshape(2 * 513, 640))   # two taps and the division: + 4
  assert got.shape == (B, F * 320)
  err = np.abs(got - want)
  print('istft: max err / bound %.4f' % (err / np.maximum(bound, 1e-300)).max())
  assert (err <= bound).all()                              # every sample, the first and the last 320 included


def _assert_mel(got_log, lin, bound, what):
  """linear domain on every bin; log domain on the bins whose float64 linear mel is >= 1e-3 (at least half of them)"""
  assert got_log.shape == lin.shape
  err = np.abs(np.exp(got_log.astype(np.float64)) - lin)
  keep = lin >= 1e-3
  err_log = np.abs(got_log.astype(np.float64) - np.log(lin))[keep]
  print('%s: max err / bound %.4f (linear), %.4f (log, %.0f %% of the bins)'
        % (what, (err / bound).max(), (err_log / (bound / lin)[keep]).max(), 100.0 * keep.mean()))
  assert (err <= bound).all()
  assert keep.mean() >= 0.5
  assert (err_log <= (bound / lin)[keep]).all()


def test_encode(voc, ragged):
  lin, bound = vc.mel_bound(ragged.astype(np.float64))
  _assert_mel(voc.encode(ragged), lin, bound, 'encode vs float64')


def test_encode_matches_the_host_codec(voc, ragged):
  """MelGAN.encode (host NumPy, float32 framing) and the device agree within the same bound."""
  _, bound = vc.mel_bound(ragged.astype(np.float64))
  host = ac.MelGAN().encode(ragged)
  _assert_mel(voc.encode(ragged), np.exp(host.astype(np.float64)), bound, 'encode vs MelGAN.encode')


@pytest.mark.parametrize('n_iters', [1, 4])
def test_decode_waveform_parity(voc, case, n_iters):
  """Measured on the MI355X (tools/vocoder_report.py -> profiles/vocoder_parity.json)."""
  got = voc.decode(case['logmel'], n_iters=n_iters, init_phase=case['phase'])
  assert got.shape == (B, F * 320) and np.isfinite(got).all()
  _assert_parity(case, got, n_iters, what='decode')


def test_decode_converges_like_float64(voc, case):
  got = voc.decode(case['logmel'], n_iters=32, init_phase=case['phase'])
  sc_dev = ac.spectral_convergence(got, case['mag'])
  sc_ref = ac.spectral_convergence(_reference(case, 32), case['mag'])
  sc_0 = ac.spectral_convergence(_reference(case, 0), case['mag'])
  print('spectral convergence after 32 iterations: device %.4f, float64 %.4f (0 iterations: %.4f)' % (sc_dev, sc_ref, sc_0))
  assert sc_dev <= 1.10 * sc_ref


def test_decode_seeds(voc, case):
  import torch
  from msd_amd import native, vocoder
  a = voc.decode(case['logmel'], n_iters=4, seed=11)
  assert np.array_equal(a, voc.decode(case['logmel'], n_iters=4, seed=11))
  assert not np.array_equal(a, voc.decode(case['logmel'], n_iters=4, seed=12))
  draws = torch.empty((B, F, 2, 513), dtype=torch.float32, device='cuda')
  native.fill_normal(draws, seed=11, stream_id=vocoder.PHASE_STREAM_ID, subseq=0)
  torch.cuda.synchronize()
  d = draws.cpu().numpy().astype(np.float64)
  phase = (d / np.sqrt((d * d).sum(axis=2, keepdims=True))).astype(np.float32)
  _assert_parity(case, a, 4, phase, what='decode(seed=11)')


def test_buffer_growth_leaves_nothing_behind(voc, case):
  """A handle that has decoded 70 frames, grown to 130 and come back gives what fresh handles give: the momentum term
  starts from Y_prev = 0 whatever the buffers held."""
  long_mel = np.log(np.clip(np.abs(ac.stft(vc.two_songs(130))) @ vc.mel_basis(), 1e-5, 1e8)).astype(np.float32)
  used = msd_amd.vocoder.GriffinLimVocoder()
  first = used.decode(case['logmel'], n_iters=4, init_phase=case['phase'])
  grown = used.decode(long_mel, n_iters=4, seed=3)
  again = used.decode(case['logmel'], n_iters=4, init_phase=case['phase'])
  assert np.array_equal(first, again)
  assert np.array_equal(first, msd_amd.vocoder.GriffinLimVocoder().decode(case['logmel'], n_iters=4, init_phase=case['phase']))
  assert np.array_equal(grown, msd_amd.vocoder.GriffinLimVocoder().decode(long_mel, n_iters=4, seed=3))
  assert np.array_equal(first, voc.decode(case['logmel'], n_iters=4, init_phase=case['phase']))


def test_arguments(voc, case):
  with pytest.raises(ValueError):
    voc.decode(case['logmel'][:, :, :64])
  with pytest.raises(ValueError):
    voc.decode(case['logmel'], init_phase=case['phase'][:, :F - 1])
  with pytest.raises(ValueError):
    voc.decode(case['logmel'], n_iters=-1)
  with pytest.raises(ValueError):
    voc.encode(np.zeros((1, 0), np.float32))
  one = voc.decode(case['logmel'][0], n_iters=1, init_phase=case['phase'][0])     # one item without the batch axis
  assert one.shape == (1, F * 320)


def test_midi_to_audio_end_to_end(tmp_path):
  """tiny_context, 2 segments, 8 steps: MIDI -> mel -> audio on the device, and audio -> mel has the shape back."""
  import dataclasses
  from msd_amd.frontend import midi_io, note_sequences
  base = msd_amd.config.preset('tiny_context', num_steps=8)
  spec = dataclasses.replace(base, t5=dataclasses.replace(base.t5, vocab_size=1536))
  model = msd_amd.InferenceModel(msd_amd.synthetic.init_params(spec, 4, norm_scale_jitter=0.1), spec, **helpers.ALL_PLANES)
  ns = note_sequences.NoteSequence()
  for k, p in enumerate([60, 64, 67, 72, 55]):
    ns.add_note(pitch=p, velocity=90, start_time=0.3 * k, end_time=0.3 * k + 1.1, program=0)
  ns.total_time = 2.4                      # 64 frames = 1.28 s per segment -> 2 segments
  path = tmp_path / 'tiny.mid'
  path.write_bytes(midi_io.note_sequence_to_midi(ns, ticks_per_quarter=500))
  mel, audio = model.synthesize_midi(str(path), seed=3, audio=True)
  assert mel.shape == (1, 2 * 64, 128) and np.array_equal(mel, model.synthesize_midi(str(path), seed=3))
  assert audio.shape == (1, mel.shape[1] * 320) and audio.dtype == np.float32 and np.isfinite(audio).all()
  assert model.vocoder is model.vocoder
  assert model.vocoder.encode(audio).shape == mel.shape
