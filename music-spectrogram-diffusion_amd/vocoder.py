"""Device vocoder: audio -> log-mel (Audio2Mel) and log-mel -> audio by fast Griffin-Lim, both on
the GPU behind the C ABI (msd_vocoder_* of include/msd_amd.h; kernels in csrc/vocoder.h).

The mel -> audio direction is a STAND-IN, not the reference's decoder: the reference runs SoundStream, a learned
vocoder shipped as a TF-Hub artifact (audio_codecs.py:249-264) that is not available here (row N2 stays "not built",
and ``AudioCodec.decode`` keeps raising).  Griffin-Lim reconstructs a phase for the magnitudes that the pseudo-inverse
of the mel filter bank gives back: intelligible, audibly "phasey", good for listening to a result and for nothing that
needs SoundStream's quality.  The specification of every operation is the float64 NumPy in audio_codecs.py
(stft / istft / mel_to_linear / griffin_lim).

  voc = GriffinLimVocoder()                 # or InferenceModel.vocoder
  mel = voc.encode(audio)                   # [B, n] -> [B, ceil(n / 320), 128]
  audio = voc.decode(mel, n_iters=32)       # [B, F, 128] -> [B, F * 320]

There is no CPU fallback: without a HIP device the constructor raises ``NativeLibraryError``."""
from __future__ import annotations

import ctypes
import wave
from typing import Optional

import numpy as np

from . import audio_codecs
from . import native

PHASE_STREAM_ID = 0x766F63   # msd_fill_normal stream of the phase draws of decode(init_phase=None) ('voc')
N_BINS = audio_codecs.FFT_LENGTH // 2 + 1


class GriffinLimVocoder:
  """Owns one ``msd_vocoder*`` on a HIP device."""

  def __init__(self, codec: Optional[audio_codecs.AudioCodec] = None, device: Optional[int] = None):
    import torch  # device memory + streams only
    codec = codec or audio_codecs.MelGAN()
    if (codec.n_dims, codec.hop_size, codec.sample_rate) != (128, audio_codecs.FRAME_STEP, 16000):
      raise ValueError('GriffinLimVocoder is built for the MelGAN geometry (128 mel bins, hop 320, 16 kHz)')
    self.codec = codec
    self.handle = ctypes.c_void_p()
    if not torch.cuda.is_available():
      raise native.NativeLibraryError('no HIP device visible: GriffinLimVocoder runs only on the GPU (no CPU fallback)')
    self.lib = native.load()
    self._torch = torch
    self.device = torch.device('cuda', torch.cuda.current_device() if device is None else device)
    basis = audio_codecs.linear_to_mel_weight_matrix(codec.n_dims, N_BINS, codec.sample_rate, 0.0, codec.sample_rate / 2.0)
    basis = np.ascontiguousarray(basis, np.float32)
    inverse = np.ascontiguousarray(audio_codecs.mel_pseudo_inverse(basis), np.float32)
    with torch.cuda.device(self.device):
      rc = self.lib.msd_vocoder_create(basis.ctypes.data, inverse.ctypes.data, ctypes.byref(self.handle))
    if rc != 0:
      msg = self.lib.msd_vocoder_last_error(self.handle).decode() if self.handle else 'invalid argument'
      self.close()
      raise native._EXC.get(rc, RuntimeError)('msd_vocoder_create failed (msd_status %d): %s' % (rc, msg))

  def close(self):
    if getattr(self, 'handle', None):
      self.lib.msd_vocoder_destroy(self.handle)
      self.handle = ctypes.c_void_p()

  def __del__(self):
    try:
      self.close()
    except Exception:  # interpreter shutdown
      pass

  def _check(self, rc, what):
    if rc:
      msg = self.lib.msd_vocoder_last_error(self.handle).decode('utf-8', 'replace')
      raise native._EXC.get(rc, RuntimeError)('%s failed (msd_status %d): %s' % (what, rc, msg))

  def _dev(self, x, ndim, what):
    torch = self._torch
    if isinstance(x, torch.Tensor):
      t = x.to(device=self.device, dtype=torch.float32)
    else:
      t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
    if t.dim() == ndim - 1:
      t = t[None]
    if t.dim() != ndim or t.numel() == 0:
      raise ValueError('%s must be a non-empty %d-d array (or one item without the batch axis)' % (what, ndim))
    return t.contiguous()

  def _run(self, fn, what, *args):
    """One entry point on the current torch stream of the device (the call synchronises it)."""
    torch = self._torch
    with torch.cuda.device(self.device):
      self._check(fn(self.handle, *args, torch.cuda.current_stream(self.device).cuda_stream), what)

  def _out(self, t, return_torch):
    return t if return_torch else t.cpu().numpy()

  # -- the STFT pair ---------------------------------------------------------------------------------------------
  def stft(self, audio, return_torch: bool = False):
    """audio [B, n] -> float32 [B, ceil(n / 320), 2, 513] (real parts, imaginary parts)."""
    a = self._dev(audio, 2, 'audio')
    b, n = a.shape
    out = self._torch.empty((b, -(-n // audio_codecs.FRAME_STEP), 2, N_BINS), dtype=self._torch.float32, device=self.device)
    self._run(self.lib.msd_vocoder_stft, 'msd_vocoder_stft', b, n, a.data_ptr(), out.data_ptr())
    return self._out(out, return_torch)

  def istft(self, spec, return_torch: bool = False):
    """spec [B, F, 2, 513] -> float32 [B, F * 320]."""
    sp = self._dev(spec, 4, 'spec')
    b, f = sp.shape[:2]
    if tuple(sp.shape[2:]) != (2, N_BINS):
      raise ValueError('spec must be [B, F, 2, %d]' % N_BINS)
    out = self._torch.empty((b, f * audio_codecs.FRAME_STEP), dtype=self._torch.float32, device=self.device)
    self._run(self.lib.msd_vocoder_istft, 'msd_vocoder_istft', b, f, sp.data_ptr(), out.data_ptr())
    return self._out(out, return_torch)

  # -- Audio2Mel / Griffin-Lim -----------------------------------------------------------------------------------
  def encode(self, audio, return_torch: bool = False):
    """audio [B, n] (NumPy or torch) -> log-mel float32 [B, ceil(n / 320), 128]: MelGAN.encode on the device."""
    a = self._dev(audio, 2, 'audio')
    b, n = a.shape
    out = self._torch.empty((b, -(-n // audio_codecs.FRAME_STEP), self.codec.n_dims), dtype=self._torch.float32,
                            device=self.device)
    self._run(self.lib.msd_vocoder_encode, 'msd_vocoder_encode', b, n, a.data_ptr(), out.data_ptr())
    return self._out(out, return_torch)

  def decode(self, mel, n_iters: int = 32, momentum: float = 0.99, seed: int = 0, init_phase=None,
             return_torch: bool = False):
    """log-mel [B, F, 128] -> audio float32 [B, F * 320] by `n_iters` fast Griffin-Lim iterations.
    init_phase: [B, F, 2, 513] (cos, sin), used as given; None: uniform phases drawn on the device from `seed`
    (pairs of native.fill_normal(seed, stream_id=PHASE_STREAM_ID, subseq=0) draws, normalised)."""
    m = self._dev(mel, 3, 'mel')
    b, f, d = m.shape
    if d != self.codec.n_dims:
      raise ValueError('mel must be [B, F, %d]' % self.codec.n_dims)
    if n_iters < 0:
      raise ValueError('n_iters must be >= 0')
    ph = None
    if init_phase is not None:
      ph = self._dev(init_phase, 4, 'init_phase')
      if tuple(ph.shape) != (b, f, 2, N_BINS):
        raise ValueError('init_phase must be [%d, %d, 2, %d]' % (b, f, N_BINS))
    out = self._torch.empty((b, f * audio_codecs.FRAME_STEP), dtype=self._torch.float32, device=self.device)
    self._run(self.lib.msd_vocoder_decode, 'msd_vocoder_decode', b, f, m.data_ptr(), int(n_iters), float(momentum),
              int(seed) & 0xFFFFFFFFFFFFFFFF, None if ph is None else ph.data_ptr(), out.data_ptr())
    return self._out(out, return_torch)

  DEBUG_BUFFERS = {'audio': 320, 'x': 1088, 'y0': 1088, 'y1': 1088, 'frames': 640, 'mag': 544}   # floats per row

  def debug_read(self, buffer: str) -> np.ndarray:
    """One work buffer as the last call left it (msd_vocoder_debug_read; for the tests): float32 [rows, floats per row],
    rows = B (F + 1) of that call."""
    if buffer not in self.DEBUG_BUFFERS:
      raise ValueError('buffer must be one of %s' % sorted(self.DEBUG_BUFFERS))
    rows = ctypes.c_int64(0)
    probe = np.zeros(1, np.float32)
    with self._torch.cuda.device(self.device):
      self._check(self.lib.msd_vocoder_debug_read(self.handle, buffer.encode(), probe.ctypes.data, 1, ctypes.byref(rows)),
                  'msd_vocoder_debug_read')
      out = np.zeros((rows.value, self.DEBUG_BUFFERS[buffer]), np.float32)
      self._check(self.lib.msd_vocoder_debug_read(self.handle, buffer.encode(), out.ctypes.data, out.size, None),
                  'msd_vocoder_debug_read')
    return out


# ---- 16-bit PCM files (the stdlib wave module; mono) -----------------------------------------------------------------
def write_wav(path: str, audio, sample_rate: int = 16000) -> float:
  """Write float samples as 16-bit PCM mono.  Samples are taken as they are unless some |x| > 1: then the whole signal
  is divided by its peak.  Returns the gain applied."""
  x = np.asarray(audio, np.float64).reshape(-1)
  if not np.isfinite(x).all():
    raise ValueError('audio has non-finite samples')
  peak = float(np.abs(x).max()) if x.size else 0.0
  gain = 1.0 / peak if peak > 1.0 else 1.0
  pcm = np.round(x * gain * 32767.0).astype('<i2')
  with wave.open(path, 'wb') as f:
    f.setnchannels(1)
    f.setsampwidth(2)
    f.setframerate(int(sample_rate))
    f.writeframes(pcm.tobytes())
  return gain


def read_wav(path: str, sample_rate: int = 16000) -> np.ndarray:
  """8- / 16- / 32-bit PCM file -> float32 [n] in [-1, 1); channels are averaged.  The rate must be `sample_rate`
  (there is no resampler here)."""
  with wave.open(path, 'rb') as f:
    ch, width, rate, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
    raw = f.readframes(n)
  if rate != sample_rate:
    raise ValueError('%s is sampled at %d Hz; the codec needs %d Hz' % (path, rate, sample_rate))
  if width == 1:
    x = (np.frombuffer(raw, np.uint8).astype(np.float32) - 128.0) / 128.0
  elif width == 2:
    x = np.frombuffer(raw, '<i2').astype(np.float32) / 32768.0
  elif width == 4:
    x = np.frombuffer(raw, '<i4').astype(np.float32) / 2147483648.0
  else:
    raise ValueError('%s: %d-byte samples are not supported' % (path, width))
  return x.reshape(-1, ch).mean(axis=1).astype(np.float32)
