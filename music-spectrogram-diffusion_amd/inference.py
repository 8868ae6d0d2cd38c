"""Drop-in mirror of the reference ``inference.py`` for the diffusion path.

Same public surface as the reference (file:line = music_spectrogram_diffusion/):
  * ``parse_training_gin_file(gin_file, gin_bindings) -> str``      inference.py:32-65
  * ``InferenceModel(checkpoint_path, gin_config, batch_size=1)``    inference.py:71-111
      .sequence_length / .inputs_length / .targets_length /
      .targets_context_length                                        inference.py:97-101
      .model.FEATURE_CONVERTER_CLS, .audio_codec, .codec, .step      inference.py:104-111,178-181
      .input_shapes / .input_types                                    inference.py:113-157
      .predict(batch, seed=0) -> (decodes, scores)                    inference.py:200-203
plus ``predict_sequence`` -- the per-song segment loop of
``InferSong.process`` (beam/evaluation.py:161-223) that BASELINE.json's
north_star names.

The compute is the HIP library behind include/msd_amd.h (native.py); there is
no fallback.  Differences that a caller can observe, all documented in
DESIGN.md: (1) the RNG is the library's Philox generator, not jax threefry
(pass ``init_z``/``noise`` for bit-identical noise across implementations);
(2) ``checkpoint_path`` accepts a T5X checkpoint directory like the reference
(checkpoints.py restates the flax-msgpack + zarr layout), and additionally
``None`` / ``'synthetic[:seed]'`` (scratch init with the reference initialisers,
as ``from_checkpoint_or_scratch`` does without a checkpoint), a ``.safetensors``
/ ``.npz`` flat dict, or an in-memory dict.  MIDI / NoteSequence input goes
through ``frontend/`` (``synthesize_midi``); ``.codec`` is the event codec the
tokeniser uses (inference.py:108-111).
"""
from __future__ import annotations

import contextlib
import dataclasses
import os
import time
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

from . import audio_codecs
from . import config as config_lib
from . import gin_lite
from . import native
from . import synthetic


def parse_training_gin_file(gin_file: str, gin_bindings: Sequence[str] = ()) -> str:
  """Parse a T5X training ``.gin`` (with includes) + extra bindings into the flat
  operative config string ``InferenceModel`` consumes (inference.py:32-65)."""
  with open(gin_file) as f:
    text = f.read()
  roots = [os.path.dirname(os.path.abspath(gin_file)), os.getcwd()]
  bindings = gin_lite.parse(text, roots)
  for b in gin_bindings:
    bindings.update(gin_lite.parse(b, roots))
  return gin_lite.to_config_str(bindings)


class _FeatureConverter:
  """Stand-in for the seqio feature-converter classes: only the names the model
  consumes matter at this boundary (models/diffusion/feature_converters.py:32-43,
  feature_converters.py:35-36)."""

  def __init__(self, model_features):
    self.MODEL_FEATURES = dict.fromkeys(model_features)


class _ModelInfo:
  """What callers read from ``InferenceModel.model`` (beam/evaluation.py:148)."""

  def __init__(self, spec: config_lib.ModelSpec):
    self.name = spec.model
    self.diffusion_config = spec.diffusion
    if spec.has_context:
      feats = ['encoder_input_tokens', 'encoder_continuous_inputs', 'encoder_continuous_mask',
               'decoder_target_tokens', 'decoder_target_mask']
    else:
      feats = ['encoder_input_tokens', 'decoder_target_tokens', 'decoder_target_mask']
    self.FEATURE_CONVERTER_CLS = _FeatureConverter(feats)


def _to_native_config(spec: config_lib.ModelSpec, codec: audio_codecs.AudioCodec,
                      batch_size: int, precision: str, attention_query_planes=None, graph_steps: int = 0,
                      weight_prefetch: Optional[bool] = None, dedup_layer0: Optional[bool] = None,
                      cross_key_split: int = 0, keep_raw_weights: bool = False,
                      kv_touch_ahead: Optional[int] = None, cross_merge_in_launch: Optional[bool] = None,
                      cross_q_fold: Optional[bool] = None, mlp_in_persistent: Optional[bool] = None,
                      touch_carrier: Optional[int] = None) -> native.MsdConfig:
  t5, d = spec.t5, spec.diffusion
  # Everything the kernels fix by construction is validated here with the
  # reference's own error type (ValueError; msd_amd.h msd_config comment).
  if t5.decoder_cross_attend_style not in ('concat_encodings', 'sum_cross_attends'):   # network.py:236-238
    raise ValueError(f'Unknown decoder_cross_attend_style: {t5.decoder_cross_attend_style}')
  if tuple(t5.mlp_activations) != ('gelu', 'linear'):
    raise NotImplementedError('only gated-GELU MLPs (mlp_activations=(gelu, linear)) are built')
  if t5.position_encoding not in ('fixed', 'fixed_permuted_offset', 'learnable_permuted_offset',
                                  'random'):
    raise ValueError(f'Unknown position_encoding: {t5.position_encoding}')
  if t5.context_positions not in ('regular', 'terminal_relative'):
    raise ValueError(f'Unknown context_positions: {t5.context_positions}')
  if d.sampler.name not in native.SAMPLERS:   # the reference's two (diffusion_utils.py:450) and 'dpmpp_2m'
    raise ValueError('Unknown sampler type: %s' % d.sampler.name)
  for sched in (d.sampler.schedule, d.train_schedule):   # diffusion_utils.py:181-202
    if sched.name not in native.SCHEDULES:
      raise ValueError('Schedule %s not identified.' % sched.name)
    if sched.name == 'linear' and (sched.start is None or sched.stop is None or not sched.num_steps):
      raise ValueError('linear schedule needs start, stop and num_steps')
  if d.model_output not in native.MODEL_OUTPUTS:       # diffusion_utils.py:288-322
    if d.model_output == 'x0_and_eps':
      raise NotImplementedError(
          'model_output="x0_and_eps" splits a 2n-channel network output (diffusion_utils.py:306-311), '
          "which the reference's own Decoder cannot produce (n_out = input channels, network.py:451-456)")
    raise ValueError('Unknown model_output: %s' % d.model_output)
  lv = d.sampler.logvar_type                            # diffusion_utils.py:141-157
  lv_frac = 0.0
  if lv == 'large':
    lv_kind = native.MSD_LOGVAR_LARGE
  elif lv == 'small':
    lv_kind = native.MSD_LOGVAR_SMALL
  elif lv.startswith('medium:'):
    lv_kind, lv_frac = native.MSD_LOGVAR_MEDIUM, float(lv.split(':')[1])
    if not 0 <= lv_frac <= 1:
      raise ValueError('logvar_type medium:<frac> needs 0 <= frac <= 1')
  else:
    raise ValueError('Unknown logvar_type: %s' % lv)
  if precision not in native.PRECISIONS:
    raise ValueError('precision must be one of %s' % sorted(native.PRECISIONS))
  lens = spec.task_feature_lengths
  cfg = native.MsdConfig()
  cfg.has_context = int(spec.has_context)
  cfg.vocab_size = t5.vocab_size
  cfg.emb_dim = t5.emb_dim
  cfg.num_heads = t5.num_heads
  cfg.head_dim = t5.head_dim
  cfg.mlp_dim = t5.mlp_dim
  cfg.num_encoder_layers = t5.num_encoder_layers
  cfg.num_decoder_layers = t5.num_decoder_layers
  cfg.inputs_length = lens['inputs']
  cfg.targets_length = lens['targets']
  cfg.context_length = lens.get('targets_context', 0) if spec.has_context else 0
  cfg.n_dims = codec.n_dims
  cfg.num_steps = d.sampler.schedule.num_steps
  cfg.sampler = native.SAMPLERS[d.sampler.name]
  cfg.clip_x0 = int(d.sampler.clip_x0)
  cfg.context_terminal_relative = int(t5.context_positions == 'terminal_relative')
  cfg.precision = native.PRECISIONS[precision]
  cfg.max_batch = batch_size
  cfg.max_decoder_noise_time = t5.max_decoder_noise_time
  cfg.cfg_weight = d.classifier_free_guidance.eval_condition_weight
  cfg.feature_min = codec.min_value
  cfg.feature_max = codec.max_value
  cfg.model_output = native.MODEL_OUTPUTS[d.model_output]
  cfg.logvar_type, cfg.logvar_frac = lv_kind, lv_frac
  ss, ts = d.sampler.schedule, d.train_schedule
  cfg.sampler_schedule = native.SCHEDULES[ss.name]
  cfg.sampler_schedule_start, cfg.sampler_schedule_stop = float(ss.start or 0.0), float(ss.stop or 0.0)
  cfg.train_schedule = native.SCHEDULES[ts.name]
  cfg.train_schedule_start, cfg.train_schedule_stop = float(ts.start or 0.0), float(ts.stop or 0.0)
  cfg.train_schedule_num_steps = int(ts.num_steps or 0)
  cfg.cross_attend_sum = int(t5.decoder_cross_attend_style == 'sum_cross_attends')
  # query side of the decoder's attentions: one number for both Q (in q.k^T) and the softmax weights (in P.V), or a
  # (q_planes, p_planes) pair; None / 0 = the library's choice
  qp = attention_query_planes
  if not isinstance(qp, (tuple, list)):
    qp = (qp, qp)
  if len(qp) != 2 or any(v not in (None, 0, 1, 2) for v in qp):
    raise ValueError('attention_query_planes must be None, 1, 2 or a (q_planes, p_planes) pair of those')
  cfg.attn_q_planes, cfg.attn_p_planes = int(qp[0] or 0), int(qp[1] or 0)
  if not 0 <= int(graph_steps) <= 64:
    raise ValueError('graph_steps must be in [0, 64] (0 = library default)')
  cfg.graph_steps = int(graph_steps)
  cfg.weight_prefetch = 0 if weight_prefetch is None else (1 if weight_prefetch else 2)
  cfg.dedup_layer0 = 0 if dedup_layer0 is None else (1 if dedup_layer0 else 2)
  if int(cross_key_split) not in (0, 1, 2, 4, 8):
    raise ValueError('cross_key_split must be 0 (chosen per segment), 1, 2, 4 or 8')
  cfg.cross_key_split = int(cross_key_split)
  cfg.keep_raw_weights = int(bool(keep_raw_weights))
  if kv_touch_ahead is not None and not 0 <= int(kv_touch_ahead) <= 16:
    raise ValueError('kv_touch_ahead must be None (library default), 0 (off) or 1 .. 16 stages')
  cfg.kv_touch_ahead = 0 if kv_touch_ahead is None else (-1 if int(kv_touch_ahead) == 0 else int(kv_touch_ahead))
  cfg.cross_merge_in_launch = 0 if cross_merge_in_launch is None else (1 if cross_merge_in_launch else 2)
  cfg.cross_q_fold = 0 if cross_q_fold is None else (1 if cross_q_fold else 2)
  cfg.mlp_in_persistent = 0 if mlp_in_persistent is None else (1 if mlp_in_persistent else 2)
  if touch_carrier is not None and int(touch_carrier) < 1:   # (the library names the values it knows: msd_create)
    raise ValueError('touch_carrier must be None (library default), 1 (in-block waves) or 2 (touch blocks)')
  cfg.touch_carrier = 0 if touch_carrier is None else int(touch_carrier)
  return cfg


def _load_checkpoint(path, spec: config_lib.ModelSpec) -> Tuple[Dict[str, np.ndarray], int]:
  if isinstance(path, Mapping):
    return dict(path), 0
  if path is None or str(path).startswith('synthetic'):
    seed = 0
    if path is not None and ':' in str(path):
      seed = int(str(path).split(':', 1)[1])
    return synthetic.init_params(spec, seed), 0
  path = str(path)
  if path.endswith('.safetensors'):
    from safetensors.numpy import load_file
    flat = load_file(path)
  elif path.endswith('.npz'):
    with np.load(path) as f:
      flat = {k: f[k] for k in f.files}
  elif os.path.isdir(path):
    # a T5X checkpoint directory, what the reference restores (inference.py:159-176)
    from . import checkpoints
    flat = checkpoints.load_t5x_checkpoint(path)
  else:
    raise ValueError(
        'checkpoint_path must be a T5X checkpoint directory, a .safetensors/.npz flat dict keyed by '
        'the Flax parameter names, or "synthetic[:seed]": %r' % path)
  step = int(np.asarray(flat.pop('__step__', 0)))
  return {k: np.asarray(v, np.float32) for k, v in flat.items()}, step


RNG_MODES = ('philox', 'threefry', 'jax')
plan_steps = native.plan_steps   # (num_steps, steps) -> (row_offset, stride) of a few-step call; ValueError names the divisors
plan_resample = native.plan_resample   # (start_step, jump, times) -> the steps and jumps of a call with resampling, in order
plan_loss_times = native.plan_loss_times   # (num_steps, times) -> the time indices of a loss call: K -> the stratified grid


def plan_region(n_frames: int, segment_frames: int, start: int, stop: int):
  """The segments a regenerated region [start, stop) of a song of n_frames touches: [(segment, mask_row)], in order;
  mask_row int32 [segment_frames], 1 = the frame lies outside the region and is KEPT.  No device needed.  The song must
  be whole segments and 0 <= start < stop <= n_frames, all integers: anything else is a ValueError."""
  vals = (n_frames, segment_frames, start, stop)
  if any(isinstance(v, bool) or int(v) != v for v in vals):
    raise ValueError('frame counts must be integers: %r' % (vals,))
  n_frames, segment_frames, start, stop = (int(v) for v in vals)
  if segment_frames <= 0 or n_frames <= 0 or n_frames % segment_frames:
    raise ValueError('the song (%d frames) is not a whole number of %d-frame segments' % (n_frames, segment_frames))
  if not 0 <= start < stop <= n_frames:
    raise ValueError('region [%d, %d) must be non-empty and inside the song\'s %d frames' % (start, stop, n_frames))
  plan = []
  for k in range(start // segment_frames, (stop - 1) // segment_frames + 1):
    lo, hi = max(start - k * segment_frames, 0), min(stop - k * segment_frames, segment_frames)
    row = np.ones((segment_frames,), np.int32)
    row[lo:hi] = 0
    plan.append((k, row))
  return plan


def region_strength(n_frames: int, segment_frames: int, start: int, stop: int, blend_frames: int):
  """plan_region with a soft edge: [(segment, strength_row)], in order; strength_row float64 [segment_frames] -- 1 inside
  the region [start, stop), 1 - d / (blend_frames + 1) at distance d = 1 .. blend_frames outside it (across segment
  boundaries, cut off at the song's ends), 0 beyond.  Every segment the region OR the ramp touches is in the plan.
  blend_frames = 0: plan_region's segments, strength_row == 1 - its mask row.  No device needed; the checks are
  plan_region's, and blend_frames must be an integer >= 0."""
  plan_region(n_frames, segment_frames, start, stop)   # (its checks)
  if isinstance(blend_frames, bool) or int(blend_frames) != blend_frames or blend_frames < 0:
    raise ValueError('blend_frames must be an integer >= 0: %r' % (blend_frames,))
  n_frames, segment_frames, start, stop, blend = (int(v) for v in (n_frames, segment_frames, start, stop, blend_frames))
  frame = np.arange(n_frames)
  dist = np.maximum(np.maximum(start - frame, frame - (stop - 1)), 0)   # 0 inside the region
  song = np.where(dist <= blend, 1.0 - dist / float(blend + 1), 0.0)
  lo, hi = max(start - blend, 0), min(stop + blend, n_frames)
  return [(k, song[k * segment_frames:(k + 1) * segment_frames].copy())
          for k in range(lo // segment_frames, (hi - 1) // segment_frames + 1)]


def plan_strength(strength, num_steps: int):
  """Edit strengths -> the sampler's release schedule.  strength [B, T] floats in [0, 1]: the share of the scan during
  which a frame is FREE -- f = floor(s * num_steps + 0.5) final steps; before them it is known (x0-replacement).  Returns
  (words int32 [B, T], start_step): word = f + 1 for f < num_steps (1 = known throughout, returned as given) and 0 for
  f == num_steps (free throughout); start_step = max f - 1 is the scan index the call starts at -- the steps above it
  have every frame known and are not run (-1: nothing to sample).  Pure: no device.  NaN, a value outside [0, 1], a
  non-float-convertible or non-2-D array, or num_steps < 1 is a ValueError."""
  if isinstance(num_steps, bool) or int(num_steps) != num_steps or num_steps < 1:
    raise ValueError('num_steps must be a positive integer: %r' % (num_steps,))
  try:
    s = np.asarray(strength, np.float64)
  except (TypeError, ValueError) as e:
    raise ValueError('strength must be an array of floats: %s' % e)
  if s.ndim != 2 or s.size == 0:
    raise ValueError('strength must be [batch, frames]: got shape %r' % (s.shape,))
  if not (np.isfinite(s).all() and (s >= 0.0).all() and (s <= 1.0).all()):
    raise ValueError('strength must lie in [0, 1] (no NaN)')
  f = np.floor(s * float(num_steps) + 0.5).astype(np.int64)
  words = np.where(f < num_steps, f + 1, 0).astype(np.int32)
  return np.ascontiguousarray(words), int(f.max()) - 1


def plan_guidance(guidance, guidance_interval, b: int, num_steps_of_call: int, model_weight: float):
  """predict's guidance / guidance_interval -> (weights float32 [b] | None, g_lo, g_hi): row r of the call combines with
  weights[r] at scan indices g_lo <= i < g_hi of its K = num_steps_of_call steps and runs the weight-1 branch (one decoder
  pass) at the others.  guidance: a finite float or [b] of them; None = the model's weight.  guidance_interval (lo, hi):
  fractions of diffusion time with 0 <= lo < hi <= 1, g = floor(x * K + 0.5) (plan_strength's rounding); None = (0, K); an
  interval that rounds to no step is a ValueError.  weights is None for THE CALL AS IT WAS -- the model's weight (or None)
  as a scalar, over the whole scan -- which runs the entry points and kernels it always ran.  Pure: no device."""
  if isinstance(num_steps_of_call, bool) or int(num_steps_of_call) != num_steps_of_call or num_steps_of_call < 1:
    raise ValueError('num_steps must be a positive integer: %r' % (num_steps_of_call,))
  k = int(num_steps_of_call)
  scalar = guidance is None or np.ndim(guidance) == 0
  w = native.check_guidance(model_weight if guidance is None else _to_numpy(guidance) if np.ndim(guidance) else guidance, b)
  g_lo, g_hi = 0, k
  if guidance_interval is not None:
    try:
      lo, hi = (float(x) for x in guidance_interval)
    except (TypeError, ValueError):
      raise ValueError('guidance_interval must be (lo, hi), two floats: %r' % (guidance_interval,))
    if not 0.0 <= lo < hi <= 1.0:   # (a NaN fails every comparison)
      raise ValueError('guidance_interval needs 0 <= lo < hi <= 1 (fractions of diffusion time): %r' % (guidance_interval,))
    g_lo, g_hi = int(np.floor(lo * k + 0.5)), int(np.floor(hi * k + 0.5))
    if g_lo == g_hi:
      raise ValueError('guidance_interval %r holds none of the call\'s %d steps (both ends round to scan index %d)'
                       % (guidance_interval, k, g_lo))
  if scalar and (g_lo, g_hi) == (0, k) and np.float32(w[0]) == np.float32(model_weight):
    return None, g_lo, g_hi
  return np.ascontiguousarray(np.broadcast_to(np.asarray(w, np.float32), (b,))), g_lo, g_hi


def plan_invert(guidance, steps, b: int, num_steps: int, model_weight: float):
  """invert's guidance / steps -> (weights, K): a list of 1 or b Python floats (float32's values) and the call's step count.
  guidance: a finite float or [b] of them; None = 1.0 -- NOT the model's weight, unlike predict: one decoder pass per step,
  and inversion under a large weight is unstable.  steps: a divisor of the model's num_steps (plan_steps); None = all of
  them.  A model created with weight 1 holds one pass's buffers and takes weight 1 only.  Pure: no device; every ValueError
  invert raises for the two is raised here."""
  k = num_steps if steps is None else steps
  plan_steps(num_steps, k)   # (its checks: a ValueError that names the divisors)
  w = native.check_guidance(1.0 if guidance is None else _to_numpy(guidance) if np.ndim(guidance) else guidance, b)
  if model_weight == 1.0 and any(x != 1.0 for x in w):
    raise ValueError('this model was created with guidance weight 1 and holds one pass\'s buffers: inversion under another '
                     'weight needs a model created with any weight != 1')
  return w, int(k)


def check_strength(strength, flags, b: int, t: int):
  """predict's strength -- a scalar, [b] or [b, t] -- as float64 [b, t], with 0 on the frames `flags` (int [b, t] or None)
  names.  A shape that is none of the three is a ValueError; the values are plan_strength's to check."""
  try:
    s = np.asarray(_to_numpy(strength), np.float64)
  except (TypeError, ValueError) as e:
    raise ValueError('strength must be a float, [batch] or [batch, %d]: %s' % (t, e))
  if s.shape == (b,):
    s = s[:, None]
  elif s.shape not in ((), (b, t)):
    raise ValueError('strength must be a scalar, [batch] = [%d] or [batch, %d]: got %r' % (b, t, s.shape))
  s = np.broadcast_to(s, (b, t)).copy()
  if flags is not None:
    s[flags != 0] = 0.0
  return s


def check_keep(keep, keep_mask, b: int, t: int, n: int):
  """The known-frame arguments of predict: both or neither; keep [b, t, n], keep_mask [b, t] bool or integer.
  Returns (keep, flags) with flags a contiguous int32 NumPy array of zeros and ones, or (None, None)."""
  if keep is None and keep_mask is None:
    return None, None
  if keep is None or keep_mask is None:
    raise ValueError('keep and keep_mask go together: one was given without the other')
  if tuple(np.shape(keep)) != (b, t, n):
    raise ValueError('keep must be [batch, %d, %d] = %r: got %r' % (t, n, (b, t, n), tuple(np.shape(keep))))
  flags = _to_numpy(keep_mask)
  if flags.dtype.kind not in 'biu':
    raise ValueError('keep_mask must be bool or integer: %s' % flags.dtype)
  if flags.shape != (b, t):
    raise ValueError('keep_mask must be [batch, %d] = %r: got %r' % (t, (b, t), flags.shape))
  return keep, np.ascontiguousarray(flags != 0, dtype=np.int32)


@dataclasses.dataclass(frozen=True)
class SampleCall:
  """The form of one sampling call, by NativeModel.sample's keyword names: known frames (keep + keep_mask), an edit
  (keep + release words + the scan index it starts at) or a few-step call (steps and / or sampler); all None = plain."""
  keep: Any = None
  keep_mask: Any = None
  release: Any = None
  start_step: Optional[int] = None
  steps: Optional[int] = None
  sampler: Optional[str] = None
  resample: Optional[Tuple[int, int]] = None   # (jump, times) of a known-frame call with resampling jumps; None = none
  guidance: Any = None                         # the call's guidance weight(s): a float, or one per row; None = the model's, as ever
  guide_range: Optional[Tuple[int, int]] = None   # the scan indices [g_lo, g_hi) it is applied at; None = all


def plan_call(keep, keep_mask, strength, steps, sampler, b: int, t: int, n: int, num_steps: int, resample=None,
              noise=None, guidance=None, guidance_interval=None, model_weight: Optional[float] = None) -> SampleCall:
  """predict's keep / keep_mask / strength / steps / sampler / resample / guidance / guidance_interval, checked and
  planned once (noise: only because resample may not be combined with it; model_weight: the model's own guidance weight,
  needed once either guidance argument is given).  Pure: no device; every ValueError predict raises for them is raised
  here, but for resample with rng='jax', which predict raises once it knows the call's generator."""
  if guidance is not None or guidance_interval is not None:
    if keep is not None or keep_mask is not None or strength is not None or resample is not None:
      raise ValueError('guidance= / guidance_interval= cannot be combined with keep= / keep_mask= / strength= / resample= '
                       '(guided edits are not built)')
    call = plan_call(None, None, None, steps, sampler, b, t, n, num_steps)
    if model_weight is None:
      raise ValueError('guidance= / guidance_interval= need the model\'s own weight (model_weight)')
    if model_weight == 1.0:
      raise ValueError('this model was created with guidance weight 1 and holds one pass\'s buffers: per-call guidance needs '
                       'a model created with any weight != 1')
    k = num_steps if call.steps is None else call.steps
    weights, g_lo, g_hi = plan_guidance(guidance, guidance_interval, b, k, model_weight)
    if weights is None:   # the call as it was
      return call
    w = [float(x) for x in weights]
    return dataclasses.replace(call, guidance=w[0] if len(set(w)) == 1 else w, guide_range=(g_lo, g_hi))
  if resample is not None:
    jump, times = native.check_resample(resample)
    if steps is not None or sampler is not None:
      raise ValueError('resample= cannot be combined with steps= / sampler= (few-step edits are not built)')
    if keep is None:
      raise ValueError('resample= needs keep: resampling jumps harmonise the free frames with known ones')
    if noise is not None:
      raise ValueError('resample= cannot be combined with noise=: the draws of the jumps and of the passes behind them are made on the device')
    call = plan_call(keep, keep_mask, strength, None, None, b, t, n, num_steps)
    return dataclasses.replace(call, resample=(jump, times))   # (times == 1: the library makes no jump; the same bits)
  if steps is not None or sampler is not None:
    if keep is not None or keep_mask is not None or strength is not None:
      raise ValueError('steps= / sampler= cannot be combined with keep= / keep_mask= / strength= (few-step edits are not built)')
    if sampler is not None and sampler not in native.SAMPLERS:
      raise ValueError('sampler must be one of %s: %r' % (sorted(native.SAMPLERS), sampler))
    if steps is not None:
      plan_steps(num_steps, steps)   # (its checks)
    return SampleCall(steps=None if steps is None else int(steps), sampler=sampler)
  if strength is None:
    keep, keep_mask = check_keep(keep, keep_mask, b, t, n)
    return SampleCall(keep=keep, keep_mask=keep_mask)
  if keep is None:
    raise ValueError('strength needs keep: the mel it is a variation of')
  keep, flags = check_keep(keep, np.zeros((b, t), np.int32) if keep_mask is None else keep_mask, b, t, n)
  words, start = plan_strength(check_strength(strength, flags, b, t), num_steps)
  return SampleCall(keep=keep, release=words, start_step=start)


class InferenceModel(object):
  """Wrapper of the HIP synthesizer with the reference's InferenceModel API."""

  def __init__(self, checkpoint_path, gin_config: Union[str, config_lib.ModelSpec],
               batch_size: int = 1, precision: str = 'f16x3', device: Optional[int] = None,
               range_fallback: bool = True, attention_query_planes=None, graph_steps: int = 0,
               weight_prefetch: Optional[bool] = None, dedup_layer0: Optional[bool] = None,
               cross_key_split: int = 0, keep_raw_weights: bool = False, kv_touch_ahead: Optional[int] = None,
               cross_merge_in_launch: Optional[bool] = None, cross_q_fold: Optional[bool] = None,
               mlp_in_persistent: Optional[bool] = None, rng: Optional[str] = None, touch_carrier: Optional[int] = None):
    """Args mirror inference.py:71-88.

    gin_config: the parsed gin string (``parse_training_gin_file``) or a typed
      ``config.ModelSpec`` preset.
    precision: 'f16x3' (default; operands as hi + lo IEEE-half planes: float32-class
      results, 5x inside the 1e-3 rms parity bar; weights must satisfy |w| < 128),
      'bf16x3' (hi + lo bfloat16 planes: float32's exponent range, 2x the error; the
      other library build), 'f16' / 'bf16' (one plane, fastest; do NOT meet the bar).
    device: HIP device index (default: torch's current device).
    attention_query_planes: planes of the query side of the decoder's attentions in the hi + lo modes (msd_config
      attn_q_planes / attn_p_planes): None = the library's choice; 1 or 2 for both Q (in q.k^T) and
      the softmax weights (in P.V), or a (q_planes, p_planes) pair.  The memory side (K, V) always keeps hi + lo.
    graph_steps: DDPM steps captured per hipGraph (0 = the library's choice, 8).
    weight_prefetch: None = the library decides from the model's size; True / False force it.
    dedup_layer0: a CFG step computes decoder layer 0's self-attention block once for both passes (exact: they are
      bit-identical up to the first cross-attention, models/diffusion/models.py:373-386); None = the library's choice
      (on), False turns it off (A/B and bitwise tests).
    cross_key_split: blocks sharing the key axis of one (head, query tile) of the decoder's cross-attention; 0 = the
      library chooses per segment from its key count, else 1, 2, 4 or 8.
    kv_touch_ahead: 128-key ring stages by which the cross-attention launches' prefetch wave touches the cached K / V
      lines ahead of their LDS-DMA (None = the library's choice, 0 = off).
    cross_merge_in_launch: a key-split cross-attention finishes inside its launch (the last block of a group merges
      the partials; no merge launch); None = the library's choice, False = the separate merge launch.  Bit-identical.
    cross_q_fold: the cross-attention's query projection has no launch of its own (folded into the QKV and the
      self-attention output projection launches by exact algebra, msd_amd.h); None = the library's choice (on)
    mlp_in_persistent: batched songs (>= 4 per call): the decoder's gated-MLP input projection as one resident block per
      CU walking its tiles (register epilogue, the next tile's operands land under it); None = the library's choice (on)
    touch_carrier: who carries the weight-prefetch touches of a one-song step: 1 = an extra wave in every compute block of
      the carrier launch, 2 = touch blocks on the CUs the carrier leaves idle (msd_amd.h; bit-identical results); None =
      the library's choice
    keep_raw_weights: keep the float32 staging copies of the packed matrices on the device (default: freed after
      packing -- 1.5 GB per handle at base_with_context).
    rng: the generator of a predict / predict_sequence call that does not name one: 'philox' (None: the library's own),
      'threefry' (the reference's draws, made on the device) or 'jax' (the same draws, made on the host); see predict.
    range_fallback: what to do when an activation leaves the range of the half planes (|x| > 65504; the
      library detects it and fails the call with native.RangeError -- the reference is float32 and has no such
      limit): True (default) switches this model to 'bf16x3' (bfloat16 planes: float32's exponent range, twice
      the rounding error), once and for good, with a RuntimeWarning, and repeats the call -- a valid workload
      never fails; False lets the error out.
    """
    import torch  # device memory + streams only
    if isinstance(gin_config, config_lib.ModelSpec):
      spec = gin_config
      self.gin_config = gin_lite.spec_to_config_str(spec)
    else:
      self.gin_config = gin_config
      spec = gin_lite.model_spec_from_bindings(gin_lite.parse(gin_config))
    self.spec = spec
    self.checkpoint_path = checkpoint_path
    self.batch_size = batch_size
    self.precision = precision
    self.range_fallback = bool(range_fallback)
    self.attention_query_planes = attention_query_planes
    self.graph_steps, self.weight_prefetch = graph_steps, weight_prefetch
    self.dedup_layer0, self.cross_key_split, self.keep_raw_weights = dedup_layer0, cross_key_split, keep_raw_weights
    self.kv_touch_ahead = kv_touch_ahead
    self.cross_merge_in_launch, self.cross_q_fold = cross_merge_in_launch, cross_q_fold
    self.mlp_in_persistent = mlp_in_persistent
    self.touch_carrier = touch_carrier
    if rng is not None and rng not in RNG_MODES:
      raise ValueError('rng must be one of %s: %r' % (RNG_MODES, rng))
    self.rng = rng or 'philox'

    self.sequence_length = dict(spec.task_feature_lengths)
    self.inputs_length = self.sequence_length['inputs']
    self.targets_length = self.sequence_length['targets']
    self.targets_context_length = self.sequence_length.get('targets_context', None)
    if spec.has_context and self.targets_context_length is None:
      raise ValueError('ContextDiffusionModel needs TASK_FEATURE_LENGTHS["targets_context"]')
    if not spec.has_context:
      self.targets_context_length = None

    self.model = _ModelInfo(spec)
    self.audio_codec = audio_codecs.get_codec(spec.audio_codec)
    # inference.py:104-111: the event codec of the tokeniser side, built from the gin's velocity bins
    from .frontend import vocabularies
    self.vocab_config = vocabularies.VocabularyConfig(num_velocity_bins=spec.num_velocity_bins)
    self.codec = vocabularies.build_codec(self.vocab_config)

    if not torch.cuda.is_available():
      raise native.NativeLibraryError(
          'no HIP device visible: InferenceModel runs only on the GPU (no CPU fallback)')
    self._torch = torch
    self.device = torch.device('cuda', torch.cuda.current_device() if device is None else device)
    self._params_np: Optional[Dict[str, np.ndarray]] = None
    self._native: Optional[native.NativeModel] = None
    self._step = 0
    self._stream = None
    self._vocoder = None
    self.last_timing: Dict[str, float] = {}

  # -- shapes / types (inference.py:113-157) -------------------------------------
  @property
  def input_shapes(self):
    shapes = {
        'encoder_input_tokens': (self.batch_size, self.inputs_length),
        'decoder_target_tokens': (self.batch_size, self.targets_length, self.audio_codec.n_dims),
    }
    if self.targets_context_length is not None:
      shapes.update({
          'encoder_continuous_inputs':
              (self.batch_size, self.targets_context_length, self.audio_codec.n_dims),
          'encoder_continuous_mask': (self.batch_size, self.targets_context_length),
      })
    if 'decoder_input_tokens' in self.model.FEATURE_CONVERTER_CLS.MODEL_FEATURES:
      shapes['decoder_input_tokens'] = shapes['decoder_target_tokens']
    return shapes

  @property
  def input_types(self):
    types = {'encoder_input_tokens': np.int32, 'decoder_target_tokens': np.float32}
    if self.targets_context_length is not None:
      types.update({'encoder_continuous_inputs': np.float32,
                    'encoder_continuous_mask': np.int32})
    if 'decoder_input_tokens' in self.model.FEATURE_CONVERTER_CLS.MODEL_FEATURES:
      types['decoder_input_tokens'] = types['decoder_target_tokens']
    return types

  # -- restore (inference.py:159-198): lazy, once per process ----------------------
  def _get_native(self) -> native.NativeModel:
    if self._native is None:
      torch = self._torch
      with torch.cuda.device(self.device):
        if self._params_np is not None:   # rebuilt after a range fallback: same weights
          params = self._params_np
        else:
          params, self._step = _load_checkpoint(self.checkpoint_path, self.spec)
        cfg = _to_native_config(self.spec, self.audio_codec, self.batch_size, self.precision,
                                self.attention_query_planes, self.graph_steps, self.weight_prefetch,
                                self.dedup_layer0, self.cross_key_split, self.keep_raw_weights, self.kv_touch_ahead,
                                self.cross_merge_in_launch, self.cross_q_fold, self.mlp_in_persistent,
                                self.touch_carrier)
        nm = native.NativeModel(cfg)   # the library build (plane format) follows from cfg.precision
        self._stream = torch.cuda.Stream(device=self.device)
        nm.load_weights(params, stream=self._stream.cuda_stream)
        self._params_np = params
        self._native = nm
    return self._native

  @property
  def step(self):
    self._get_native()
    return self._step

  @property
  def params(self) -> Dict[str, np.ndarray]:
    self._get_native()
    return self._params_np

  @property
  def vocoder(self):
    """The device vocoder of this model's codec (vocoder.GriffinLimVocoder: Audio2Mel, and Griffin-Lim as the stand-in
    for the SoundStream decoder that is not built); created on first use, one per model."""
    if self._vocoder is None:
      from . import vocoder as vocoder_lib
      self._vocoder = vocoder_lib.GriffinLimVocoder(self.audio_codec, device=self.device.index)
    return self._vocoder

  # -- predict (inference.py:200-203) -----------------------------------------------
  def predict(self, batch: Mapping[str, Any], seed: Union[int, Sequence[int]] = 0,
              segment: Union[int, Sequence[int]] = 0,
              init_z=None, noise=None, return_torch: bool = False, rng: Optional[str] = None,
              keep=None, keep_mask=None, strength=None, steps: Optional[int] = None, sampler: Optional[str] = None,
              resample=None, guidance=None, guidance_interval=None):
    """Predict one batch of 256-frame segments.

    batch: the model features of inference.py:113-136 (NumPy arrays or torch
      tensors); ``decoder_target_tokens`` is used for its shape only.
    seed / segment: key of the Philox generator (replaces PRNGKey(seed)).  Scalars key ONE draw over the whole
      [B,T,n] array (row b of a batched call is then not the draw of any one-row call).  Either may be a sequence of
      B integers (a scalar beside it is broadcast): every row is keyed by its own (seed[b], segment[b]) and draws,
      bit for bit, what the one-row call predict(row b, seed=seed[b], segment=segment[b]) draws -- independent
      segments share one call (msd_sample_rows; predict_sequence(batch_segments=) drives it).  In the 'threefry' and
      'jax' modes row b draws what the reference draws for PRNGKey(seed[b]) and a batch of one.
    init_z [B,T,n] / noise [N,B,T,n]: explicit draws (the parity contract).
    rng: None = the model's default (InferenceModel(rng=), 'philox' unless given).
      'philox': the library's device generator, one stream per segment.
      'threefry': the draws jax.random would make for PRNGKey(seed) -- init_z = normal(key), step-i noise =
      normal(fold_in(key, i)), one draw per [B,T,n] array -- made ON THE DEVICE: init_z by a fill kernel, step i's
      noise inside the sampler kernel (msd_sample_rng, MSD_RNG_THREEFRY).  No host work, no noise tensor.
      'jax': the same draws restated on the host (jax_random.py), uploaded as a [N,B,T,n] tensor
      and cached per (seed, batch): the specification the device generator is tested against (they agree to
      the rounding of log1p: <= 3 ulp on about one value in a hundred).
      Like the reference (beam/evaluation.py:209 calls predict(batch) with the default seed for EVERY segment),
      `segment` does not enter the key in the 'threefry' and 'jax' modes.
    keep [B,T,n] (mel units; NumPy or a device tensor) / keep_mask [B,T] (bool or int, non-zero = known): frames of the
      target that are KNOWN.  They come back exactly as given -- values outside the codec's range included -- and
      the other frames are sampled so that they fit them: in every step the kept elements' x0 is replaced by the
      known value (x0-replacement inside the sampler kernel, msd_sample_keep), so they carry the step's noise
      level and the free frames see them through self-attention.  The draws are those of the call without a mask
      (an all-zero mask changes nothing, bit for bit); every seed / segment / rng / init_z / noise form works.
      One without the other, or a wrong shape, is a ValueError.
    strength (with keep; a float, [B] or [B,T], each in [0, 1]): how far each frame of `keep` may move -- an
      SDEdit-style restart with a per-frame release schedule on top of the x0-replacement (plan_strength,
      msd_sample_edit).  A frame of strength s is known while the noise is high and free for the last
      f = round(s * N) steps; 0 returns it as given, 1 samples it from pure noise.  The call starts at scan index
      max f - 1 from the known mel diffused to that step's noise level (with the call's own initial draw) and costs
      max f steps, not N.  Frames named by keep_mask (optional here) get strength 0.  strength == 1 - keep_mask
      is the keep_mask call, bit for bit.  The network was never trained on known frames; the schedule is per frame
      (no per-bin map); resampling jumps are `resample`'s.  strength without keep is a ValueError.
    resample (jump, times), with keep (and keep_mask or strength): RePaint resampling jumps in the scan
      (msd_sample_resample, plan_resample).  The scan goes down `jump` steps, diffuses the state back up those steps --
      known and free frames alike, one sample of q(z_t | z_s) -- and comes down again, `times` descents per block: the free
      frames get several chances to condition on the known ones at the same noise level instead of one pass in which the
      known region is imposed from outside.  A call costs times x its steps plus (times - 1) ceil(steps / jump) jump
      launches, all enqueued at once.  Every pass behind a jump has a generator key of its own ('philox': segment +
      (p << 32), so segment < 2^32; 'threefry': fold_in(PRNGKey(seed), N + p - 1)), per row under per-row keys; init_z
      keeps its meaning for the first pass.  The draws are made on the device: not with noise= nor rng='jax'; not
      with steps= / sampler=; resample without keep, or a jump or times that is no integer >= 1, is a ValueError too, all
      raised before any device work.  None and (jump, 1) are the call without it, bit for bit.  On synthetic weights
      nothing measures whether the result sounds better; the network was still never trained on known frames.
    steps (K) / sampler ('ddpm', 'ddim', 'dpmpp_2m'): a step count and a sampler for THIS call, on the same handle
      (msd_sample_steps) -- a preview in 50 steps, the rendering in all N.  K must divide the model's N (plan_steps; a
      ValueError names the divisors).  The call is the scan of a model configured with num_steps = K -- times (j + 1) / K,
      the draws of such a model: `noise` is then [K,B,T,n] and rng='jax' draws reference_noise(seed, shape, K); with
      a cosine sampler schedule it is exactly the reference configured with K steps, with a linear one the model's own
      N-point schedule evaluated at those times.  'dpmpp_2m' is DPM-Solver++(2M), the second-order multistep solver of
      the ODE 'ddim' solves to first order: deterministic (no draw after init_z).  On a case with a closed form its
      error at 20 - 50 steps is a sixth to a seventh of DDIM's; on synthetic weights it has measured no closer to the
      1000-step DDIM result than DDIM, and nothing is known about a trained checkpoint.  None / None is the call as it always was, bit for bit.
      NOT with keep / keep_mask / strength (nor on vary / regenerate): edits on a coarse schedule, and multistep history
      across a frame's release, are a separate piece of work -- a ValueError in this version.
    guidance (a float, or [B] floats: row b takes guidance[b]) / guidance_interval ((lo, hi), 0 <= lo < hi <= 1,
      fractions of diffusion time): the classifier-free guidance weight of THIS call in the model's
      eval_condition_weight's place, on the same handle and graphs (plan_guidance, msd_sample_guided) -- a sweep of B
      weights over one set of tokens is one batched call with equal keys.  With an interval the combine is applied only
      at scan indices floor(lo K + 0.5) <= i < floor(hi K + 0.5) of the call's K steps (Kynkaanniemi et al. 2024);
      every other step is the reference's weight-1 branch: ONE decoder pass, half the rows in every launch.  A row
      whose weight is exactly 1 takes that branch at every step, so row b is always its one-row call; a scalar weight
      w gives the bits of a model created with weight w.  An interval alone uses the model's weight.  With every seed /
      segment / rng / init_z / noise form and with steps= / sampler= ('dpmpp_2m' keeps its history across the
      interval's edges).  None, or the model's own weight, over the whole scan is the call as it always was, bit for
      bit.  NOT with keep / keep_mask / strength / resample, no per-frame weights, and not on a model created with
      weight 1 (it holds one pass's buffers): ValueErrors, raised before any device work, as are a non-finite weight,
      a wrong length and an interval that is out of order, outside [0, 1] or rounds to no step.
    Returns (decodes float32 [B,T,n] in mel units, scores float32 [B] zeros).
    """
    call = plan_call(keep, keep_mask, strength, steps, sampler, np.shape(batch['encoder_input_tokens'])[0], self.targets_length,
                     self.audio_codec.n_dims, self.spec.diffusion.sampler.schedule.num_steps, resample, noise,
                     guidance, guidance_interval, self.spec.diffusion.classifier_free_guidance.eval_condition_weight)
    if rng is None:
      rng = self.rng
    if resample is not None and rng == 'jax':
      raise ValueError("resample= cannot be combined with rng='jax' (host draws): the draws of the jumps and of the passes "
                       "behind them are made on the device; use 'philox' or 'threefry'")
    return self._with_range_fallback(self._predict_once, batch, seed, segment, init_z, noise, return_torch, rng, call)

  def _with_range_fallback(self, fn, *args):
    """fn(*args), one of the _once calls.  When an activation leaves the half planes' range (native.RangeError) and
    range_fallback allows it, the model moves to the bfloat16-plane build for good and the call is repeated, once."""
    try:
      return fn(*args)
    except native.RangeError:
      if not (self.range_fallback and self.precision in ('f16x3', 'f16')):
        raise
      import warnings
      new = 'bf16x3' if self.precision == 'f16x3' else 'bf16'
      warnings.warn("an activation left the half-plane range (|x| > 65504): switching this model from precision "
                    "'%s' to '%s' (bfloat16 planes) and repeating the call" % (self.precision, new), RuntimeWarning)
      self.precision = new
      if self._native is not None:
        self._native.close()
      self._native = None
      return fn(*args)

  @contextlib.contextmanager
  def _encode_batch(self, batch):
    """The encode stage of every call that runs the decoder on an encoded state: the tokens checked, the model's stream
    ordered behind the caller's, the context and its mask uploaded and checked, msd_encode enqueued.  Yields (nm, b, s,
    t0, t1) -- the handle, the rows, the stream's handle and the stage's two timestamps -- with the model's stream current."""
    torch = self._torch
    nm = self._get_native()
    dev = self.device
    tokens = _to_numpy(batch['encoder_input_tokens'])
    if tokens.dtype.kind not in 'iu':   # layers.Embed (layers.py:546-547; layers_test.py:392-401)
      raise ValueError('Input type must be an integer or unsigned integer.')
    tokens = np.ascontiguousarray(tokens, dtype=np.int32)
    b = tokens.shape[0]
    if tokens.ndim != 2 or tokens.shape[1] != self.inputs_length:
      raise ValueError('encoder_input_tokens must be [batch, %d]' % self.inputs_length)
    if b > self.batch_size:
      raise ValueError('batch %d exceeds batch_size %d' % (b, self.batch_size))
    n = self.audio_codec.n_dims
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
      # tensors the caller produced on its own stream (e.g. the previous prediction) are consumed on
      # the model's stream: order the two
      self._stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.device(dev), torch.cuda.stream(self._stream):
      s = self._stream.cuda_stream
      ctx = mask = None
      if self.targets_context_length is not None:
        ctx = _to_device(torch, batch['encoder_continuous_inputs'], dev, torch.float32)
        if tuple(ctx.shape) != (b, self.targets_context_length, n):
          raise ValueError('encoder_continuous_inputs must be [batch, %d, %d]'
                           % (self.targets_context_length, n))
        mask = np.ascontiguousarray(_to_numpy(batch['encoder_continuous_mask']), dtype=np.int32)
        if mask.shape != (b, self.targets_context_length):   # msd_encode copies batch * C ints from it
          raise ValueError('encoder_continuous_mask must be [batch, %d]' % self.targets_context_length)
      nm.encode(b, tokens, ctx, mask, stream=s)
      yield nm, b, s, t0, time.perf_counter()

  def _check_target(self, batch, caller: str, what: str):
    """batch['decoder_target_tokens'] of invert / loss: present, and [batch, T, n] for the rows of the tokens."""
    t, n = self.targets_length, self.audio_codec.n_dims
    if 'decoder_target_tokens' not in batch:
      raise ValueError("%s() needs batch['decoder_target_tokens']: the mel to %s, [batch, %d, %d]" % (caller, what, t, n))
    b = np.shape(batch['encoder_input_tokens'])[0]
    if tuple(np.shape(batch['decoder_target_tokens'])) != (b, t, n):
      raise ValueError('decoder_target_tokens must be [batch, %d, %d] = %r: got %r'
                       % (t, n, (b, t, n), tuple(np.shape(batch['decoder_target_tokens']))))
    return b, t, n

  def _predict_once(self, batch, seed, segment, init_z, noise, return_torch, rng, call=SampleCall()):
    torch, dev = self._torch, self.device
    t, n = self.targets_length, self.audio_codec.n_dims
    with self._encode_batch(batch) as (nm, b, s, t0, t1):
      out = torch.empty((b, t, n), dtype=torch.float32, device=dev)
      per_row = not (np.isscalar(seed) and np.isscalar(segment))
      if per_row:
        seed, segment = native.row_keys(b, seed, segment)
      # the call's step count: its noise is [K, B, T, n] and its host draws are those of a K-step model
      k_steps = self.spec.diffusion.sampler.schedule.num_steps if call.steps is None else call.steps
      if rng == 'jax' and init_z is None and noise is None:
        init_z, noise = self._jax_noise_rows(seed, k_steps) if per_row else self._jax_noise(seed, b, k_steps)
      elif rng not in RNG_MODES:
        raise ValueError('rng must be one of %s: %r' % (RNG_MODES, rng))
      z0 = None if init_z is None else _to_device(torch, init_z, dev, torch.float32)
      nz = None if noise is None else _to_device(torch, noise, dev, torch.float32)
      if z0 is not None and tuple(z0.shape) != (b, t, n):
        raise ValueError('init_z must be [batch, %d, %d]' % (t, n))
      if nz is not None and tuple(nz.shape) != (k_steps, b, t, n):
        raise ValueError('noise must be [num_steps, batch, %d, %d] = %r: got %r' % (t, n, (k_steps, b, t, n), tuple(nz.shape)))
      # explicit draws keep precedence in every mode; 'jax' has none left to generate
      known = None if call.keep is None else _to_device(torch, call.keep, dev, torch.float32)
      nm.sample(b, out, seed=seed, stream_id=segment, init_z=z0, noise=nz, stream=s,
                rng='threefry' if rng == 'threefry' else 'philox', **vars(dataclasses.replace(call, keep=known)))
      self._stream.synchronize()
    t2 = time.perf_counter()
    self.last_timing = {'encode_s': t1 - t0, 'sample_s': t2 - t1, 'total_s': t2 - t0}
    scores = np.zeros((b,), np.float32)
    if return_torch:
      return out, torch.zeros((b,), dtype=torch.float32, device=dev)
    return out.cpu().numpy(), scores

  # -- inversion: the noise that renders a given mel under given tokens ----------------------------------------------
  def invert(self, batch: Mapping[str, Any], steps: Optional[int] = None, guidance=None, return_torch: bool = False):
    """Deterministic DDIM inversion on the device (msd_invert): the init_z from which
    predict(batch, init_z=, sampler='ddim', steps=K, guidance=w) renders batch['decoder_target_tokens'] again, up to the
    inversion's own error -- "same performance, other notes": invert the old mel under the old tokens, render the new tokens
    from that noise (rerender).

    batch: predict's features; the mel is ``decoder_target_tokens`` [B, T, n] in mel units, exactly as loss() takes it
      (values outside the codec's range are clipped, as the context's are); tokens and context as predict takes them.
    steps (K): the levels of the inversion, a divisor of the model's N (plan_steps; a ValueError names the divisors);
      None = N.  Step i = 0 .. K - 1 is one decoder evaluation of the state it has at time (i + 1) / K and
      z' = a_i z + b_i eps with eps frozen at that state: the exact inverse of the K-step DDIM step where the model's
      prediction does not move between the two levels (and where train and sampler schedule agree), first order in 1 / K
      otherwise.  No noise is drawn.
    guidance: a finite float or [B] floats; None = **1.0** here -- this differs from predict, whose None is the model's
      eval_condition_weight: weight 1 runs ONE decoder pass per step (half the rows in every launch), and inversion under
      a large weight is known to be unstable.  Render with the same weight you inverted with.
    The sampler's clip_x0 is ignored (the clip is not invertible where it binds), so a round trip through a clipping model
    is not exact even as K grows.  The range fallback repeats the call on the bfloat16-plane build, as predict does.
    NOT built, each a ValueError or absent: fixed-point refinement of a step, stopping below level K, inversion under DDPM
    noise or 'dpmpp_2m', keep / strength / resample, per-frame weights, K that does not divide N.
    Returns the noise float32 [B, T, n] in MODEL units (NumPy; ``return_torch``: the device tensor).  Argument errors are
    ValueErrors raised before any device work."""
    b, _, _ = self._check_target(batch, 'invert', 'invert')
    weights, k = plan_invert(guidance, steps, b, self.spec.diffusion.sampler.schedule.num_steps,
                             self.spec.diffusion.classifier_free_guidance.eval_condition_weight)
    return self._with_range_fallback(self._invert_once, batch, k, weights, return_torch)

  def _invert_once(self, batch, k, weights, return_torch):
    torch, dev = self._torch, self.device
    t, n = self.targets_length, self.audio_codec.n_dims
    with self._encode_batch(batch) as (nm, b, s, t0, t1):
      mel = _to_device(torch, batch['decoder_target_tokens'], dev, torch.float32).contiguous()
      out = torch.empty((b, t, n), dtype=torch.float32, device=dev)
      nm.invert(b, out, mel, steps=k, guidance=weights if len(weights) > 1 else weights[0], stream=s)
      self._stream.synchronize()
    t2 = time.perf_counter()
    self.last_timing = {'encode_s': t1 - t0, 'sample_s': t2 - t1, 'total_s': t2 - t0}
    return out if return_torch else out.cpu().numpy()

  def rerender(self, song, old_tokens: Sequence[np.ndarray], new_tokens: Sequence[np.ndarray], steps: Optional[int] = None,
               guidance=None, render_guidance=None, always_mask_context: bool = False, return_torch: bool = False):
    """The same performance with other notes or another instrument: every segment of `song` ([1, K * T, n], mel units;
    NumPy or a device tensor; K == len(old_tokens) == len(new_tokens)) is inverted under the tokens it was rendered from
    and rendered again from that noise under the new ones.  Per segment k:
      noise_k = invert(old tokens k, old mel k, context = OLD segment k - 1, steps=, guidance=)
      new_k   = predict(new tokens k, context = NEW segment k - 1, init_z=noise_k, sampler='ddim', steps=, guidance=render_guidance)
    (zeros and mask 0 for segment 0 and ``always_mask_context``).  guidance: invert's (None = 1.0); render_guidance:
    predict's (None = the model's own weight) -- pass the same number to both for a round trip.  rerender(song, tokens,
    tokens) at equal weights returns the song up to the inversion's error.  Returns the new song [1, K * T, n] (NumPy;
    ``return_torch``: the device tensor)."""
    t = self.targets_length
    self._check_song(song, old_tokens)
    self._check_song(song, new_tokens)
    # both directions' arguments, planned once before the first segment runs (each call plans its own again)
    n_steps, own = self.spec.diffusion.sampler.schedule.num_steps, self.spec.diffusion.classifier_free_guidance.eval_condition_weight
    plan_invert(guidance, steps, 1, n_steps, own)
    plan_call(None, None, None, steps, 'ddim', 1, t, self.audio_codec.n_dims, n_steps, guidance=render_guidance, model_weight=own)
    torch = self._torch
    old = _to_device(torch, song, self.device, torch.float32)
    outs = []
    for k, (toks_old, toks_new) in enumerate(zip(old_tokens, new_tokens)):
      no_ctx = always_mask_context or k == 0 or self.targets_context_length is None
      batch = self._segment_batch(toks_old, None if no_ctx else old[:, (k - 1) * t:k * t].clone(), no_ctx)
      batch['decoder_target_tokens'] = old[:, k * t:(k + 1) * t].clone()
      noise = self.invert(batch, steps=steps, guidance=guidance, return_torch=True)
      batch = self._segment_batch(toks_new, None if no_ctx else outs[-1].clone(), no_ctx)
      kw = {} if render_guidance is None else {'guidance': render_guidance}
      out, _ = self.predict(batch, init_z=noise, sampler='ddim', steps=steps, return_torch=True, **kw)
      outs.append(out[:1].to(self.device))
    new = torch.cat(outs, dim=1)
    return new if return_torch else new.cpu().numpy()

  def _jax_noise(self, seed: int, b: int, steps: int):
    """Device-resident (init_z, noise) of jax_random.reference_noise, cached for the last (seed, b, steps)."""
    key = (int(seed), int(b), int(steps))
    if getattr(self, '_jax_noise_key', None) != key:
      from . import jax_random
      t, n = self.targets_length, self.audio_codec.n_dims
      z, nz = jax_random.reference_noise(seed, (b, t, n), steps)
      self._jax_noise_val = (self._torch.as_tensor(z).to(self.device), self._torch.as_tensor(nz).to(self.device))
      self._jax_noise_key = key
    return self._jax_noise_val

  def _jax_noise_rows(self, seeds: Sequence[int], steps: int):
    """(init_z [B,T,n], noise [N,B,T,n]) whose row b is the one-row host draw of seeds[b]: one draw per distinct seed."""
    from . import jax_random
    torch = self._torch
    t, n = self.targets_length, self.audio_codec.n_dims
    drawn = {}
    for sd in seeds:
      if sd not in drawn:
        z, nz = jax_random.reference_noise(sd, (1, t, n), steps)
        drawn[sd] = (torch.as_tensor(z).to(self.device), torch.as_tensor(nz).to(self.device))
    return (torch.cat([drawn[sd][0] for sd in seeds], dim=0), torch.cat([drawn[sd][1] for sd in seeds], dim=1))

  # -- the denoising loss: how well a mel fits a set of tokens (models.py loss_fn as an evaluation) ---------------
  def loss(self, batch: Mapping[str, Any], times=16, seed: Union[int, Sequence[int]] = 0,
           segment: Union[int, Sequence[int]] = 0, rng: Optional[str] = None, conditioning: str = 'cond',
           loss_type: Optional[str] = None, loss_norm: Optional[str] = None, eps=None):
    """The reference's evaluation loss (models.py loss_fn over diffusion_utils.get_diffusion_training_input and
    calculate_loss) of a given mel under a given set of tokens, at time indices of the model's own step grid, on the device
    (msd_loss): diffuse the target to the time, run ONE decoder pass, compare the prediction with the noise and the
    target per element, mask and sum.

    batch: predict's features plus ``decoder_target_tokens`` (the mel, [B, T, n], mel units) and optionally
      ``decoder_target_mask`` ([B, T], any float; default ones) -- loss_fn's names.
    times: an integer K (1 <= K <= N: the stratified grid of plan_loss_times) or a sequence of time indices in [0, N);
      index i is time (i + 1) / N.  The reference draws ONE random time per row; an average over a fixed grid is the
      evaluation of the same expectation with no noise from the choice of times.
    seed / segment / rng: the keys of the eps draws, as in predict ('philox' or 'threefry'; per-row sequences work the
      same way; not 'jax': pass eps= instead).  The draw at index i is a function of (key, i): an index that appears
      twice draws the same eps twice.  eps [K, B, T, n]: explicit draws instead.
    conditioning: 'cond' (the tokens and the context as encoded), 'uncond' (the sampler's unconditional pass), or 'both'
      (the two passes of a guided step in one batched launch; not on a model created with weight 1).
    loss_type ('x0', 'eps', 'max_x0_eps', 'x0_and_eps') / loss_norm ('l1', 'l2'): calculate_loss's; None = the spec's
      (eps / l1 for every shipped configuration).  Dropout is off: this is an evaluation.
    Returns a dict of float64 NumPy values, sums taken on the host from the device's per-frame float32 sums:
      'loss' [passes] the sum over masked elements, mean over times; 'per_row' [passes, B]; 'per_frame' [passes, B, T];
      'per_time' [K, passes, B]; 'times' the indices; 'target_frames' the sum of the mask.
    The range fallback repeats the call on the bfloat16-plane build, as predict does.  Argument errors are ValueErrors
    raised before any device work."""
    n_steps = self.spec.diffusion.sampler.schedule.num_steps
    idx = native.plan_loss_times(n_steps, times)
    if rng is None:
      rng = self.rng
    if rng == 'jax' and eps is None:
      raise ValueError("loss() draws eps on the device: rng must be 'philox' or 'threefry' (or pass eps=), not 'jax'")
    if rng not in RNG_MODES:
      raise ValueError('rng must be one of %s: %r' % (RNG_MODES, rng))
    if conditioning not in native.LOSS_CONDITIONINGS:
      raise ValueError('conditioning must be one of %s: %r' % (sorted(native.LOSS_CONDITIONINGS), conditioning))
    if conditioning == 'both' and self.spec.diffusion.classifier_free_guidance.eval_condition_weight == 1.0:
      raise ValueError("conditioning='both' needs a model created with a guidance weight != 1 (a weight-1 model holds one pass's buffers)")
    loss_type = getattr(self.spec.diffusion, 'loss_type', 'eps') if loss_type is None else loss_type
    loss_norm = getattr(self.spec.diffusion, 'loss_norm', 'l1') if loss_norm is None else loss_norm
    if loss_type not in native.LOSS_TYPES:
      raise ValueError('Unknown diffusion loss_type: %r (one of %s)' % (loss_type, sorted(native.LOSS_TYPES)))
    if loss_norm not in native.LOSS_NORMS:
      raise ValueError('Unknown diffusion loss norm: %r (one of %s)' % (loss_norm, sorted(native.LOSS_NORMS)))
    b, t, n = self._check_target(batch, 'loss', 'score')
    mask = batch.get('decoder_target_mask')
    if mask is not None and tuple(np.shape(mask)) != (b, t):
      raise ValueError('decoder_target_mask must be [batch, %d]: got %r' % (t, tuple(np.shape(mask))))
    if eps is not None and tuple(np.shape(eps)) != (len(idx), b, t, n):
      raise ValueError('eps must be [times, batch, %d, %d] = %r: got %r' % (t, n, (len(idx), b, t, n), tuple(np.shape(eps))))
    return self._with_range_fallback(self._loss_once, batch, idx, seed, segment, rng, conditioning, loss_type, loss_norm, eps)

  def _loss_once(self, batch, idx, seed, segment, rng, conditioning, loss_type, loss_norm, eps):
    torch, dev = self._torch, self.device
    t = self.targets_length
    passes = 2 if conditioning == 'both' else 1
    with self._encode_batch(batch) as (nm, b, s, _, _):
      target = _to_device(torch, batch['decoder_target_tokens'], dev, torch.float32).contiguous()
      mask = batch.get('decoder_target_mask')
      mask_d = None if mask is None else _to_device(torch, mask, dev, torch.float32).contiguous()
      eps_d = None if eps is None else _to_device(torch, eps, dev, torch.float32).contiguous()
      out = torch.empty((len(idx), passes, b, t), dtype=torch.float32, device=dev)
      if not (np.isscalar(seed) and np.isscalar(segment)):
        seed, segment = native.row_keys(b, seed, segment)
      nm.loss(b, target, out, idx, seed=seed, stream_id=segment, rng='threefry' if rng == 'threefry' else 'philox',
              conditioning=conditioning, loss_type=loss_type, loss_norm=loss_norm, mask=mask_d, eps=eps_d, stream=s)
      self._stream.synchronize()
    frames = out.cpu().numpy().astype(np.float64)   # [K, passes, B, T]
    per_time = frames.sum(axis=3)
    per_frame = frames.mean(axis=0)
    per_row = per_frame.sum(axis=2)
    return {'loss': per_row.sum(axis=1), 'per_row': per_row, 'per_frame': per_frame, 'per_time': per_time,
            'times': list(idx),
            'target_frames': float(b * t) if mask is None else float(np.asarray(_to_numpy(mask), np.float64).sum())}

  def score_sequence(self, song, segments_tokens: Sequence[np.ndarray], times=16, seed: int = 0,
                     conditioning: str = 'cond', always_mask_context: bool = False, rng: Optional[str] = None):
    """The denoising loss of a whole song under its tokens, teacher-forced: segment k of `song` ([1, K * T, n], mel units;
    NumPy or a device tensor) is scored by loss() with segment k - 1 OF THE GIVEN SONG as context (zeros and mask 0 for
    segment 0 and ``always_mask_context``), keyed (seed, k); ``rng``: loss()'s ('philox' or 'threefry'; None = the model's).
    Returns {'per_frame': [passes, K * T], 'per_segment':
    [passes, K], 'loss': [passes], 'times'}: per-frame losses (mean over times) and their sums, float64."""
    t = self.targets_length
    self._check_song(song, segments_tokens)
    idx = native.plan_loss_times(self.spec.diffusion.sampler.schedule.num_steps, times)
    torch = self._torch
    mel = _to_device(torch, song, self.device, torch.float32)
    frames = []
    for k, toks in enumerate(segments_tokens):
      no_ctx = always_mask_context or k == 0 or self.targets_context_length is None
      batch = self._segment_batch(toks, None if no_ctx else mel[:, (k - 1) * t:k * t].clone(), no_ctx)
      batch['decoder_target_tokens'] = mel[:, k * t:(k + 1) * t].clone()
      frames.append(self.loss(batch, times=idx, seed=seed, segment=k, rng=rng, conditioning=conditioning)['per_frame'][:, 0])
    per_frame = np.concatenate(frames, axis=1)
    per_segment = np.stack([f.sum(axis=1) for f in frames], axis=1)
    return {'per_frame': per_frame, 'per_segment': per_segment, 'loss': per_segment.sum(axis=1), 'times': idx}

  # -- InferSong.process segment loop (beam/evaluation.py:161-223) ---------------------
  def predict_sequence(self, segments_tokens: Sequence[np.ndarray], seed: int = 0,
                       always_mask_context: bool = False, init_context: Optional[np.ndarray] = None,
                       first_segment_index: int = 0, return_timing: bool = False, rng: Optional[str] = None,
                       return_torch: bool = False, batch_segments: int = 1, steps: Optional[int] = None,
                       sampler: Optional[str] = None, guidance: Optional[float] = None, guidance_interval=None):
    """Synthesize a whole song: segments of int32 [inputs_length] (or [1, L]).

    Segment 0 runs with context zeros + mask 0 (beam/evaluation.py:195-198);
    segment i > 0 gets the previous PREDICTION (mel units) with mask 1
    (:194,199-205); ``always_mask_context`` masks every segment (:66-68).
    ``init_context`` [1, C, n] (NumPy or a device tensor; + ``first_segment_index`` > 0)
    resumes a song in the middle: the chained multi-GPU hand-off (sharding.py) uses it.
    Returns float32 [1, T*K, n] (NumPy; with ``return_torch`` the device tensor, so that the
    hand-off message never leaves the GPU); with ``return_timing`` also a dict with the
    reference's own metric (evaluation.py:217-220,244-250).

    ``batch_segments`` = B > 1 sends consecutive groups of B segments (the last group smaller) through ONE predict
    each, row j keyed (seed, first_segment_index + its index): the noise, and so the result up to the rounding of a
    batched launch, is what the loop gives that segment.  Only where the segments are independent of each other: a
    model without context (models/diffusion/models.py:167-199), or ``always_mask_context`` (the context is zeros with
    mask 0 then: a masked context contributes nothing, whatever its values).  Anything else, B > batch_size, or
    ``init_context`` with B > 1 is a ValueError.  The timing is group seconds / group rows, averaged over all groups
    but the first (the loop leaves out its first segment the same way).

    ``steps`` / ``sampler``: predict's, for every segment of the song (the batched form included).

    ``guidance`` (ONE weight for the song: a scalar) / ``guidance_interval``: predict's, for every segment as well.
    """
    if guidance is not None and (isinstance(guidance, bool) or np.ndim(guidance) != 0):
      raise ValueError('predict_sequence takes one guidance weight for the song (a scalar): %r' % (guidance,))
    few = {k: v for k, v in (('steps', steps), ('sampler', sampler), ('guidance', guidance),
                             ('guidance_interval', guidance_interval)) if v is not None}
    if batch_segments != 1:
      return self._predict_sequence_batched(segments_tokens, seed, always_mask_context, init_context,
                                            first_segment_index, return_timing, rng, return_torch, batch_segments, few)
    torch = self._torch
    n = self.audio_codec.n_dims
    c_len = self.targets_context_length
    pred = None   # (the first segment's context: zeros)
    if c_len is not None and init_context is not None:
      pred = _to_device(torch, init_context, self.device, torch.float32).reshape(1, c_len, n)
    outs, seconds = [], []
    for i, toks in enumerate(segments_tokens):
      gi = first_segment_index + i
      batch = self._segment_batch(toks, pred, always_mask_context or (i == 0 and init_context is None))
      tick = time.perf_counter()
      out, _ = self.predict(batch, seed=seed, segment=gi, return_torch=True, rng=rng, **few)
      if i != 0:
        seconds.append(time.perf_counter() - tick)
      if c_len is not None:
        pred = out[:1]
      outs.append(out[:1])
    full = torch.cat(outs, dim=1)
    if not return_torch:
      full = full.cpu().numpy()
    if not return_timing:
      return full
    return full, self._sequence_timing(seconds)

  def _check_song(self, song, segments_tokens):
    t, n = self.targets_length, self.audio_codec.n_dims
    if len(np.shape(song)) != 3 or np.shape(song)[0] != 1 or np.shape(song)[2] != n:
      raise ValueError('song must be [1, frames, %d]: got %r' % (n, tuple(np.shape(song))))
    if np.shape(song)[1] != t * len(segments_tokens) or not len(segments_tokens):
      raise ValueError('song has %d frames but %d segments of tokens (%d frames each) were given'
                       % (np.shape(song)[1], len(segments_tokens), t))

  def _segment_batch(self, tokens, context, no_ctx: bool):
    """predict's batch of one segment: its tokens and -- a model with context -- `context` [1, C, n] on the device (None =
    zeros) under a mask of ones, or of zeros when no_ctx."""
    batch = {'encoder_input_tokens': np.asarray(tokens, np.int32).reshape(1, -1)}
    c_len = self.targets_context_length
    if c_len is not None:
      if context is None:
        context = self._torch.zeros((1, c_len, self.audio_codec.n_dims), dtype=self._torch.float32, device=self.device)
      batch['encoder_continuous_inputs'] = context
      batch['encoder_continuous_mask'] = (np.zeros if no_ctx else np.ones)((1, c_len), np.int32)
    return batch

  def _edit_segment(self, new, k, tokens, always_mask_context, seed, rng, **keep_kw):
    """predict for segment k of the song `new` as it stands ([1, K * T, n] on the device): its context is segment k - 1 of
    `new` (zeros and mask 0 for segment 0 and always_mask_context), its key (seed, k), its known mel its own frames."""
    t = self.targets_length
    no_ctx = always_mask_context or k == 0 or self.targets_context_length is None
    batch = self._segment_batch(tokens, None if no_ctx else new[:, (k - 1) * t:k * t].clone(), no_ctx)
    out, _ = self.predict(batch, seed=seed, segment=k, return_torch=True, rng=rng, keep=new[:, k * t:(k + 1) * t].clone(),
                          **keep_kw)
    return out.to(self.device)

  def vary(self, song, segments_tokens: Sequence[np.ndarray], strength, seed: int = 0, always_mask_context: bool = False,
           rng: Optional[str] = None, return_torch: bool = False, resample=None):
    """A variation of a rendering: the same song at a chosen distance.

    song float32 [1, K * T, n] (mel units; NumPy or a device tensor), K == len(segments_tokens).  strength: a float in
    [0, 1], or one value per frame ([K * T] or [1, K * T]).  Every segment runs through predict(keep=its old frames,
    strength=...), keyed (seed, segment index) as predict_sequence keys it; its context is the NEW previous segment, as
    in predict_sequence.  A segment costs round(max strength * N) steps, not N: it starts part-way down the scan from its
    old frames diffused to that noise level.  strength 1.0 is predict_sequence, bit for bit; frames of strength 0 are
    the input's, bit for bit.  resample = (jump, times): predict's, for every segment.  Returns the new song
    [1, K * T, n] (NumPy; ``return_torch``: the device tensor)."""
    torch = self._torch
    t = self.targets_length
    self._check_song(song, segments_tokens)
    if resample is not None:
      native.check_resample(resample)
    frames = np.shape(song)[1]
    s = np.asarray(_to_numpy(strength), np.float64)
    if s.shape not in ((), (frames,), (1, frames)):
      raise ValueError('strength must be a float or one value per frame ([%d] or [1, %d]): got %r' % (frames, frames, s.shape))
    s = np.broadcast_to(s.reshape(-1) if s.ndim else s, (frames,))
    new = _to_device(torch, song, self.device, torch.float32).clone()
    for k, toks in enumerate(segments_tokens):
      out = self._edit_segment(new, k, toks, always_mask_context, seed, rng, strength=s[None, k * t:(k + 1) * t],
                               **({} if resample is None else {'resample': resample}))
      new[:, k * t:(k + 1) * t] = out[:1]
    return new if return_torch else new.cpu().numpy()

  def regenerate(self, song, segments_tokens: Sequence[np.ndarray], start_frame: int, stop_frame: int, seed: int = 0,
                 always_mask_context: bool = False, rng: Optional[str] = None, return_torch: bool = False,
                 blend_frames: int = 0, resample=None):
    """Sample the frames [start_frame, stop_frame) of a song again and keep the rest.

    song float32 [1, K * T, n] (mel units; NumPy or a device tensor), K == len(segments_tokens), the tokens of ALL its
    segments (after a MIDI edit: the edited ones).  Only the segments that overlap the region are sampled (plan_region),
    in order, each keyed (seed, segment index) as predict_sequence keys it and each keeping its frames outside the
    region (predict(keep=, keep_mask=)).  The context of segment k is segment k - 1 of the song AS IT STANDS --
    regenerated if the region touched it, the original otherwise --; segment 0 and ``always_mask_context`` run with
    zeros and mask 0, as in predict_sequence.  Segments behind the region are not run again: the region's last frames
    are sampled with the frames that follow them in their own segment known, and the next segment keeps the context
    it was made with.  Returns the new song [1, K * T, n] (NumPy; ``return_torch``: the device tensor); every frame
    outside the region is the input's, bit for bit.

    blend_frames = F > 0 softens the seams: the F frames on either side of the region are released to the sampler for
    the last part of the scan only -- strength 1 - d / (F + 1) at distance d (region_strength; predict(strength=)) --,
    across segment boundaries; segments that only this ramp touches are sampled too.  Frames beyond the ramp, and ramp
    frames whose share rounds to no step at all, are the input's bit for bit.  0 is the hard edge above, unchanged.

    resample = (jump, times): predict's resampling jumps (RePaint) for every segment that is sampled; None = none."""
    torch = self._torch
    if resample is not None:
      native.check_resample(resample)
    t, n = self.targets_length, self.audio_codec.n_dims
    if len(np.shape(song)) != 3 or np.shape(song)[0] != 1 or np.shape(song)[2] != n:
      raise ValueError('song must be [1, frames, %d]: got %r' % (n, tuple(np.shape(song))))
    plan = plan_region(np.shape(song)[1], t, start_frame, stop_frame)   # [(segment, mask row)]; soft: [(segment, strength row)]
    soft = blend_frames != 0
    if soft:
      plan = region_strength(np.shape(song)[1], t, start_frame, stop_frame, blend_frames)
      self._check_song(song, segments_tokens)
    elif np.shape(song)[1] != t * len(segments_tokens):
      raise ValueError('song has %d segments of %d frames but %d segments of tokens were given'
                       % (np.shape(song)[1] // t, t, len(segments_tokens)))
    new = _to_device(torch, song, self.device, torch.float32).clone()
    for k, row in plan:
      out = self._edit_segment(new, k, segments_tokens[k], always_mask_context, seed, rng,
                               **({'strength': row[None]} if soft else {'keep_mask': row[None]}),
                               **({} if resample is None else {'resample': resample}))
      free = torch.as_tensor(row > 0.0 if soft else row == 0, device=self.device)
      new[0, k * t:(k + 1) * t][free] = out[0][free]   # (the other frames of `out` are the song's already)
    return new if return_torch else new.cpu().numpy()

  def _sequence_timing(self, seconds: Sequence[float]) -> Dict[str, float]:
    seconds_per_chunk = self.targets_length * (self.audio_codec.hop_size / self.audio_codec.sample_rate)
    per_chunk = float(np.mean(seconds)) if seconds else float('nan')
    return {'prediction_seconds_per_chunk': per_chunk,
            'predictions_seconds_per_audio_second': per_chunk / seconds_per_chunk}

  def check_batch_segments(self, batch_segments: int, always_mask_context: bool = False, init_context=None):
    """ValueError unless predict_sequence(batch_segments=) may run with these options (no device needed)."""
    if int(batch_segments) != batch_segments or batch_segments < 1:
      raise ValueError('batch_segments must be a positive integer: %r' % (batch_segments,))
    if batch_segments == 1:
      return
    if self.targets_context_length is not None and not always_mask_context:
      raise ValueError('batch_segments=%d needs independent segments: this model conditions every segment on the '
                       'previous prediction; pass always_mask_context=True or use a model without context'
                       % batch_segments)
    if batch_segments > self.batch_size:
      raise ValueError('batch_segments=%d exceeds batch_size %d' % (batch_segments, self.batch_size))
    if init_context is not None:
      raise ValueError('init_context cannot be combined with batch_segments > 1 (every row runs with a masked context)')

  def _predict_sequence_batched(self, segments_tokens, seed, always_mask_context, init_context, first_segment_index,
                                return_timing, rng, return_torch, batch_segments, few=None):
    self.check_batch_segments(batch_segments, always_mask_context, init_context)
    torch = self._torch
    n = self.audio_codec.n_dims
    c_len = self.targets_context_length
    segs = [np.asarray(t, np.int32).reshape(1, -1) for t in segments_tokens]
    outs, seconds = [], []
    for g0 in range(0, len(segs), batch_segments):
      rows = segs[g0:g0 + batch_segments]
      b = len(rows)
      batch = {'encoder_input_tokens': np.concatenate(rows, axis=0)}
      if c_len is not None:
        batch['encoder_continuous_inputs'] = torch.zeros((b, c_len, n), dtype=torch.float32, device=self.device)
        batch['encoder_continuous_mask'] = np.zeros((b, c_len), np.int32)
      tick = time.perf_counter()
      out, _ = self.predict(batch, seed=seed, segment=[first_segment_index + g0 + j for j in range(b)],
                            return_torch=True, rng=rng, **(few or {}))
      if g0 != 0:
        seconds.append((time.perf_counter() - tick) / b)
      outs.append(out[:b].reshape(1, -1, n))
    full = torch.cat(outs, dim=1)
    if not return_torch:
      full = full.cpu().numpy()
    if not return_timing:
      return full
    return full, self._sequence_timing(seconds)


  # ---- MIDI in -----------------------------------------------------
  def tokenize_note_sequence(self, ns, on_too_long: str = 'error'):
    """NoteSequence -> list of int32 [1, inputs_length] segment inputs through the reference's
    full-song pipeline (frontend/tokenizer.py; tasks.py:405-464 with full_song_eval=True)."""
    from .frontend import tokenizer
    cfg = tokenizer.FrontendConfig(sample_rate=self.audio_codec.sample_rate, hop_size=self.audio_codec.hop_size,
                                   segment_frames=self.targets_length, inputs_length=self.inputs_length)
    return tokenizer.note_sequence_to_model_inputs(ns, cfg, on_too_long=on_too_long)

  def synthesize_note_sequence(self, ns, seed: int = 0, audio: bool = False, vocoder_iters: int = 32, **kw):
    """Notes -> mel frames of the whole song, float32 [1, K * targets_length, n_dims] (the tail past
    ns.total_time is the padding of the last segment).  kw: predict_sequence options (steps= / sampler= among them).
    audio=True: returns (mel, audio) -- audio float32 [1, frames * hop_size] from `vocoder_iters` Griffin-Lim
    iterations on the device (self.vocoder: a stand-in, not the reference's SoundStream); with return_timing
    (mel, audio, timing)."""
    res = self.predict_sequence(self.tokenize_note_sequence(ns), seed=seed, **kw)
    if not audio:
      return res
    mel, rest = (res[0], tuple(res[1:])) if isinstance(res, tuple) else (res, ())
    wav = self.vocoder.decode(mel, n_iters=vocoder_iters, seed=seed, return_torch=bool(kw.get('return_torch')))
    return (mel, wav) + rest

  def synthesize_midi(self, path: str, seed: int = 0, **kw):
    """Standard MIDI File -> mel frames (the reference's notebooks read MIDI with
    note_seq.midi_file_to_note_sequence; frontend/midi_io.py restates that reader).  audio=True: (mel, audio), see
    synthesize_note_sequence."""
    from .frontend import midi_io
    return self.synthesize_note_sequence(midi_io.midi_file_to_note_sequence(path), seed=seed, **kw)


def _to_numpy(x) -> np.ndarray:
  if isinstance(x, np.ndarray):
    return x
  if hasattr(x, 'detach'):
    return x.detach().cpu().numpy()
  return np.asarray(x)


def _to_device(torch, x, dev, dtype):
  if isinstance(x, torch.Tensor):
    return x.to(device=dev, dtype=dtype).contiguous()
  return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(dev)
