"""Command line: MIDI file -> mel spectrogram of the whole song (the reference's notebook flow:
note_seq.midi_file_to_note_sequence -> full-song task pipeline -> InferSong.process,
beam/evaluation.py:161-223) on the MI355X path.

  python -m msd_amd.synthesize song.mid --checkpoint /path/to/base_with_context/checkpoint_500000 \\
      --out song_mel.npy [--preset base_with_context] [--gin-file train.gin --gin-bindings ...]
      [--seed 0] [--rng threefry|jax] [--num-steps 1000] [--steps K] [--sampler ddpm|ddim|dpmpp_2m] [--dry-run]
      [--batch-segments B [--always-mask-context]]
      [--wav song.wav [--vocoder-iters 32]] [--context-audio earlier.wav]
      [--regenerate START:STOP [--blend FRAMES] (--edit-mel old_mel.npy | --edit-audio old.wav)]
      [--vary STRENGTH (--edit-mel old_mel.npy | --edit-audio old.wav)]
      [--resample JUMP:TIMES]   (with --regenerate or --vary)
      [--guidance W] [--guidance-interval LO:HI]
  python -m msd_amd.synthesize new.mid --rerender old.mid (--edit-mel old_mel.npy | --edit-audio old.wav) [--steps K] [--guidance W]
  python -m msd_amd.synthesize song.mid (--score MEL.npy | --score-audio REC.wav) [--score-times K]
      [--score-conditioning cond|uncond|both]

--score MEL.npy / --score-audio REC.wav sample nothing: they print the denoising loss of the given mel (a recording goes
through the device Audio2Mel) under the MIDI file's tokens as one JSON object with per-segment sums (a mel that ends inside a
segment is padded with the codec's pad value: 'loss_given_frames' is the sum without the padding) -- segment k scored with
segment k - 1 of the GIVEN mel as context, at --score-times K time indices spread over the model's steps
(InferenceModel.score_sequence).  No --out.

--wav writes 16-bit PCM mono at 16 kHz from the device vocoder: Griffin-Lim over the codec's STFT, a stand-in for the
reference's SoundStream decoder (which is not built).  --context-audio continues a recording: its last 256 frames are
encoded on the device and given to the first segment as context.

--batch-segments B sends B segments through every sampling call, each with the noise the one-by-one loop gives it; the
segments must be independent of each other: a preset without context, or --always-mask-context.

--regenerate START:STOP (seconds, rounded outward to whole frames) changes part of a song: the old rendering comes from
--edit-mel (the .npy a previous --out wrote) or --edit-audio (a recording, encoded on the device), the MIDI file is the
song as it should be now, and only the segments the region touches are sampled again, each keeping its frames outside
the region; every frame outside the region stays what it was.  --out / --wav write the edited song.

--blend FRAMES softens the region's edges: the FRAMES frames on either side are released to the sampler for the last part
of the scan only, less the farther they lie from the region (InferenceModel.regenerate(blend_frames=)).

--vary STRENGTH (0 .. 1) renders a variation of the old rendering: every segment starts part-way down the scan from its old
frames at the matching noise level and runs round(STRENGTH * steps) steps -- 1 is a fresh rendering, 0 the old one
(InferenceModel.vary).  An SDEdit-style restart: the network was never trained on known frames.

--resample JUMP:TIMES (with --regenerate or --vary) adds RePaint resampling jumps to the edit: the scan goes down JUMP
steps, diffuses the state back up and comes down again, TIMES descents per block, so that the sampled frames get several
chances to fit the kept ones at each noise level; a segment costs TIMES x its steps (InferenceModel.predict(resample=)).
Not with --rng jax (the extra draws are made on the device).

--steps K renders every segment in K steps (K divides --num-steps; the model keeps its num-steps tables, so the same
process could render in all of them next) and --sampler names the sampler of the run: dpmpp_2m is the second-order
DPM-Solver++(2M), deterministic after the initial draw.  Not with --regenerate / --vary.

--guidance W renders this run with the classifier-free guidance weight W in the model's (--cfg-weight) place, on the same
model; --guidance-interval LO:HI (fractions of diffusion time, 0 <= LO < HI <= 1) applies the guidance only inside that
part of the scan, and every step outside it runs one decoder pass instead of two (InferenceModel.predict(guidance=,
guidance_interval=)).  Not with --regenerate / --vary, nor with --cfg-weight 1.

--rerender OLD.mid renders the same performance with this MIDI file's notes: every segment of the old rendering (--edit-mel /
--edit-audio) is inverted under OLD.mid's tokens -- deterministic DDIM inversion on the device, --steps K levels -- and this
file's tokens are rendered with ddim in K steps from that noise (InferenceModel.rerender).  Both files must tokenise to the
same number of segments.  --guidance W is the weight of BOTH directions and defaults to 1 here (one decoder pass per step;
inversion under a large weight is unstable), not to --cfg-weight.  Not with --regenerate / --vary / --score.

--dry-run tokenises only (no GPU): prints the segment / token statistics the synthesis would see, and with --regenerate
the plan: the segments touched and the frames each keeps."""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np


def main(argv=None) -> int:
  ap = argparse.ArgumentParser(prog='msd_amd.synthesize', description=__doc__.split('\n')[0])
  ap.add_argument('midi')
  ap.add_argument('--checkpoint', default='synthetic:0',
                  help="T5X checkpoint dir, .npz/.safetensors flat dict, or 'synthetic[:seed]' (random weights)")
  ap.add_argument('--preset', default='base_with_context')
  ap.add_argument('--gin-file', default=None, help='training gin file (instead of --preset)')
  ap.add_argument('--gin-bindings', nargs='*', default=())
  ap.add_argument('--num-steps', type=int, default=1000)
  ap.add_argument('--steps', type=int, default=None, metavar='K',
                  help='sampling steps of this run; must divide the model\'s step count (--num-steps)')
  ap.add_argument('--sampler', choices=['ddpm', 'ddim', 'dpmpp_2m'], default=None,
                  help="the sampler of this run (default: the configuration's); 'dpmpp_2m' = DPM-Solver++(2M), second order")
  ap.add_argument('--cfg-weight', type=float, default=5.0)
  ap.add_argument('--guidance', type=float, default=None, metavar='W',
                  help='the guidance weight of this run (default: the model\'s, --cfg-weight)')
  ap.add_argument('--guidance-interval', default=None, metavar='LO:HI',
                  help='apply the guidance only in this part of the scan (fractions of diffusion time); one decoder pass outside')
  ap.add_argument('--seed', type=int, default=0)
  ap.add_argument('--rng', choices=['philox', 'threefry', 'jax'], default='philox',
                  help="'threefry': the reference's jax.random draws for --seed, made on the device; 'jax': the same on the host")
  ap.add_argument('--precision', choices=['f16x3', 'f16', 'bf16x3', 'bf16'], default='f16x3',
                  help="'f16x3' (default): hi + lo IEEE-half operand planes, float32-class; 'bf16x3': bfloat16 planes "
                       "(float32's exponent range, twice the rounding error); 'f16' / 'bf16': one plane, not parity-grade")
  ap.add_argument('--no-range-fallback', dest='range_fallback', action='store_false',
                  help="fail with native.RangeError when an activation leaves the half-plane range (|x| > 65504) instead "
                       "of switching to 'bf16x3' and repeating the segment (the default: a real checkpoint's residual "
                       "stream may have outlier channels; the reference is float32 and never fails on them)")
  ap.add_argument('--out', default=None, help='.npy file for the mel frames [frames, 128]')
  ap.add_argument('--wav', default=None, help='write the audio as 16-bit PCM mono (Griffin-Lim on the device; not SoundStream)')
  ap.add_argument('--vocoder-iters', type=int, default=32, help='Griffin-Lim iterations of --wav')
  ap.add_argument('--context-audio', default=None,
                  help='16 kHz PCM .wav whose last context-length frames are encoded on the device as the first segment\'s context')
  ap.add_argument('--batch-segments', type=int, default=1,
                  help='segments per sampling call (the model is built with batch_size=B); needs independent segments: '
                       'a preset without context, or --always-mask-context')
  ap.add_argument('--always-mask-context', action='store_true',
                  help='no segment sees the previous prediction (beam/evaluation.py:66-68)')
  ap.add_argument('--regenerate', default=None, metavar='START:STOP',
                  help='sample this region of the song again (seconds, rounded outward to frames) and keep the rest of '
                       '--edit-mel / --edit-audio')
  ap.add_argument('--blend', type=int, default=0, metavar='FRAMES',
                  help='with --regenerate: release this many frames on either side of the region part-way (soft seams)')
  ap.add_argument('--vary', type=float, default=None, metavar='STRENGTH',
                  help='a variation of --edit-mel / --edit-audio at this distance, 0 .. 1 (1 = a fresh rendering)')
  ap.add_argument('--resample', default=None, metavar='JUMP:TIMES',
                  help='with --regenerate / --vary: RePaint resampling jumps -- every block of JUMP steps is descended TIMES times')
  ap.add_argument('--rerender', default=None, metavar='OLD.mid',
                  help='the same performance with these notes: invert --edit-mel / --edit-audio under OLD.mid\'s tokens (DDIM '
                       'inversion on the device) and render this MIDI file from that noise; --steps K levels, --guidance W '
                       'for both directions (default 1: one decoder pass per step)')
  ap.add_argument('--edit-mel', default=None, metavar='OLD.npy', help='the old rendering as mel frames [frames, 128]')
  ap.add_argument('--edit-audio', default=None, metavar='OLD.wav',
                  help='the old rendering as a 16 kHz PCM recording (encoded on the device)')
  ap.add_argument('--score', default=None, metavar='MEL.npy',
                  help='no sampling: the denoising loss of these mel frames [frames, 128] under the MIDI file\'s tokens, per '
                       'segment, as one JSON object on stdout')
  ap.add_argument('--score-audio', default=None, metavar='REC.wav',
                  help='--score for a 16 kHz PCM recording (encoded on the device)')
  ap.add_argument('--score-times', type=int, default=16, metavar='K',
                  help='with --score / --score-audio: time indices per segment, a stratified grid over the model\'s steps')
  ap.add_argument('--score-conditioning', choices=['cond', 'uncond', 'both'], default='cond',
                  help="with --score / --score-audio: the decoder pass(es) that are scored")
  ap.add_argument('--on-too-long', choices=['error', 'truncate'], default='error')
  ap.add_argument('--dry-run', action='store_true')
  args = ap.parse_args(argv)
  scoring = bool(args.score or args.score_audio)
  if args.score and args.score_audio:
    ap.error('--score and --score-audio are two sources of the same thing: give one')
  if scoring and (args.out or args.wav):
    ap.error('--score / --score-audio sample nothing: no --out / --wav')
  if scoring and (args.regenerate or args.vary is not None or args.edit_mel or args.edit_audio or args.resample is not None):
    ap.error('--score / --score-audio do not go with --regenerate / --vary / --edit-mel / --edit-audio / --resample')
  if scoring and (args.steps is not None or args.sampler or args.guidance is not None or args.guidance_interval is not None
                  or args.batch_segments != 1 or args.context_audio):
    ap.error('--score / --score-audio sample nothing: no --steps / --sampler / --guidance / --guidance-interval / '
             '--batch-segments / --context-audio')
  if scoring and args.rng == 'jax':
    ap.error("--score / --score-audio draw on the device: --rng philox or threefry")
  if not scoring and (args.score_times != 16 or args.score_conditioning != 'cond'):
    ap.error('--score-times / --score-conditioning go with --score MEL.npy or --score-audio REC.wav')
  if args.rerender and (args.regenerate or args.vary is not None or scoring):
    ap.error('--rerender does not go with --regenerate / --vary / --score / --score-audio: give one')
  if args.rerender and not (args.edit_mel or args.edit_audio):
    ap.error('--rerender needs the old rendering: --edit-mel OLD.npy or --edit-audio OLD.wav')
  if args.rerender and (args.sampler or args.guidance_interval is not None or args.batch_segments != 1 or args.context_audio
                        or args.rng == 'jax'):
    ap.error('--rerender inverts and renders with ddim, segment by segment, and draws nothing: no --sampler / '
             '--guidance-interval / --batch-segments / --context-audio / --rng jax')
  if args.regenerate and args.vary is not None:
    ap.error('--regenerate and --vary are two edits: give one')
  if args.regenerate and not (args.edit_mel or args.edit_audio):
    ap.error('--regenerate needs the old rendering: --edit-mel OLD.npy or --edit-audio OLD.wav')
  if args.vary is not None and not (args.edit_mel or args.edit_audio):
    ap.error('--vary needs the old rendering: --edit-mel OLD.npy or --edit-audio OLD.wav')
  if args.edit_mel and args.edit_audio:
    ap.error('--edit-mel and --edit-audio are two sources of the same thing: give one')
  if (args.edit_mel or args.edit_audio) and not (args.regenerate or args.vary is not None or args.rerender):
    ap.error('--edit-mel / --edit-audio need the edit to make: --regenerate START:STOP, --vary STRENGTH or --rerender OLD.mid')
  if (args.regenerate or args.vary is not None) and (args.batch_segments != 1 or args.context_audio):
    ap.error('--regenerate / --vary sample their segments one by one with the song as context: no --batch-segments / --context-audio')
  if args.vary is not None and not 0.0 <= args.vary <= 1.0:
    ap.error('--vary wants a strength in [0, 1]: %r' % (args.vary,))
  if args.blend < 0 or (args.blend and not args.regenerate):
    ap.error('--blend FRAMES (>= 0) goes with --regenerate')
  if (args.steps is not None or args.sampler) and (args.regenerate or args.vary is not None):
    ap.error('--steps / --sampler do not go with --regenerate / --vary (few-step edits are not built)')
  if (args.guidance is not None or args.guidance_interval is not None) and (args.regenerate or args.vary is not None):
    ap.error('--guidance / --guidance-interval do not go with --regenerate / --vary (guided edits are not built)')
  if args.guidance_interval is not None:
    try:
      args.guidance_interval = interval_pair(args.guidance_interval)
    except ValueError as e:
      ap.error(str(e))

  if args.resample is not None:
    if not (args.regenerate or args.vary is not None):
      ap.error('--resample JUMP:TIMES goes with --regenerate or --vary: resampling jumps fit sampled frames to known ones')
    if args.rng == 'jax':
      ap.error("--resample does not go with --rng jax: the jumps' draws are made on the device (philox or threefry)")
    try:
      args.resample = resample_pair(args.resample)
    except ValueError as e:
      ap.error(str(e))

  import msd_amd
  from msd_amd.frontend import midi_io, tokenizer
  if args.gin_file:
    spec = msd_amd.parse_training_gin_file(args.gin_file, list(args.gin_bindings))
  else:
    spec = msd_amd.config.preset(args.preset, num_steps=args.num_steps, cfg_weight=args.cfg_weight)
  few = {}
  if args.steps is not None:
    from msd_amd import native
    try:
      native.plan_steps(spec.diffusion.sampler.schedule.num_steps, args.steps)
    except ValueError as e:
      ap.error('--steps: %s' % e)
    few['steps'] = args.steps
  if args.sampler:
    few['sampler'] = args.sampler
  if args.rerender:
    from msd_amd import inference
    try:
      inference.plan_invert(args.guidance, args.steps, 1, spec.diffusion.sampler.schedule.num_steps,
                            spec.diffusion.classifier_free_guidance.eval_condition_weight)
    except ValueError as e:
      ap.error('--rerender: %s' % e)
  elif args.guidance is not None or args.guidance_interval is not None:
    from msd_amd import inference
    k = spec.diffusion.sampler.schedule.num_steps if args.steps is None else args.steps
    w = spec.diffusion.classifier_free_guidance.eval_condition_weight
    try:
      if w == 1.0:
        raise ValueError('a model with --cfg-weight 1 holds one pass\'s buffers: give it any other weight')
      inference.plan_guidance(args.guidance, args.guidance_interval, 1, k, w)
    except ValueError as e:
      ap.error('--guidance / --guidance-interval: %s' % e)
    few.update({k_: v for k_, v in (('guidance', args.guidance), ('guidance_interval', args.guidance_interval)) if v is not None})
  if scoring:
    from msd_amd import native
    try:
      native.plan_loss_times(spec.diffusion.sampler.schedule.num_steps, args.score_times)
      if args.score_conditioning == 'both' and spec.diffusion.classifier_free_guidance.eval_condition_weight == 1.0:
        raise ValueError('a model with --cfg-weight 1 holds one pass\'s buffers: --score-conditioning cond or uncond')
    except ValueError as e:
      ap.error('--score-times / --score-conditioning: %s' % e)
  ns = midi_io.midi_file_to_note_sequence(args.midi)
  cfg = tokenizer.FrontendConfig.from_spec(spec)
  t0 = time.perf_counter()
  segments = tokenizer.note_sequence_to_model_inputs(ns, cfg, on_too_long=args.on_too_long)
  t_tok = time.perf_counter() - t0
  n_tok = [int((s > 0).sum()) for s in segments]
  print('%s: %d notes, %.2f s -> %d segments of %d frames; tokens per segment min/mean/max %d/%.0f/%d (%.3f s)'
        % (args.midi, len(ns.notes), ns.total_time, len(segments), cfg.segment_frames, min(n_tok),
           float(np.mean(n_tok)), max(n_tok), t_tok), file=sys.stderr)
  rerender = None
  if args.rerender:   # the old notes' segments and the old rendering's length, before any device work
    from msd_amd import audio_codecs, vocoder
    codec = audio_codecs.get_codec(spec.audio_codec)
    try:
      old_segments = tokenizer.note_sequence_to_model_inputs(midi_io.midi_file_to_note_sequence(args.rerender), cfg,
                                                             on_too_long=args.on_too_long)
      if len(old_segments) != len(segments):
        raise ValueError('%s has %d segments, %s has %d: --rerender keeps the performance segment by segment'
                         % (args.rerender, len(old_segments), args.midi, len(segments)))
      if args.edit_mel:
        old = np.load(args.edit_mel)
        old = old[0] if old.ndim == 3 and old.shape[0] == 1 else old
        if old.ndim != 2 or old.shape[1] != codec.n_dims:
          raise ValueError('%s must hold mel frames [frames, %d]: got %r' % (args.edit_mel, codec.n_dims, old.shape))
        old_frames = old.shape[0]
      else:
        old = vocoder.read_wav(args.edit_audio, codec.sample_rate)
        old_frames = -(-old.size // codec.hop_size)
      if old_frames > len(segments) * cfg.segment_frames:
        raise ValueError('the old rendering has %d frames, the MIDI file only %d (%d segments)'
                         % (old_frames, len(segments) * cfg.segment_frames, len(segments)))
    except (ValueError, OSError) as e:
      ap.error(str(e))
    print('rerender %d segments: %d inversion steps and %d ddim steps each, guidance %g'
          % (len(segments), args.steps or spec.diffusion.sampler.schedule.num_steps,
             args.steps or spec.diffusion.sampler.schedule.num_steps, 1.0 if args.guidance is None else args.guidance))
    rerender = (old, old_segments)
  edit = None
  if args.regenerate or args.vary is not None:
    # everything about the edit that needs no device: the region in frames, the old rendering's length, the plan
    from msd_amd import audio_codecs, inference, vocoder
    codec = audio_codecs.get_codec(spec.audio_codec)
    song_frames = len(segments) * cfg.segment_frames
    try:
      start, stop = region_frames(args.regenerate, codec.sample_rate / codec.hop_size) if args.regenerate else (0, song_frames)
      if args.edit_mel:
        old = np.load(args.edit_mel)
        old = old[0] if old.ndim == 3 and old.shape[0] == 1 else old
        if old.ndim != 2 or old.shape[1] != codec.n_dims:
          raise ValueError('%s must hold mel frames [frames, %d]: got %r' % (args.edit_mel, codec.n_dims, old.shape))
        old_frames = old.shape[0]
      else:
        old = vocoder.read_wav(args.edit_audio, codec.sample_rate)
        old_frames = -(-old.size // codec.hop_size)
      if old_frames > song_frames:
        raise ValueError('the old rendering has %d frames, the MIDI file only %d (%d segments)'
                         % (old_frames, song_frames, len(segments)))
      plan = inference.plan_region(song_frames, cfg.segment_frames, start, stop)
      soft = inference.region_strength(song_frames, cfg.segment_frames, start, stop, args.blend) if args.blend else []
      steps = spec.diffusion.sampler.schedule.num_steps
      vary_steps = None if args.vary is None else inference.plan_strength([[args.vary]], steps)[1] + 1
    except ValueError as e:
      ap.error(str(e))
    if args.vary is not None:
      print('vary %d segments at strength %g: %d of %d steps each' % (len(segments), args.vary, vary_steps, steps))
    else:
      print('regenerate frames [%d, %d) of %d (%.3f s .. %.3f s): %d of %d segments'
            % (start, stop, song_frames, start / cfg.frame_rate, stop / cfg.frame_rate, len(plan), len(segments)))
      for k, row in plan:
        free = np.nonzero(row == 0)[0]
        print('  segment %d: frames [%d, %d) sampled again, %d of %d kept'
              % (k, free[0], free[-1] + 1, int(row.sum()), row.size))
      for k, row in soft:
        words, start_step = inference.plan_strength(row[None], steps)
        part = (words[0] > 1)
        print('  blend %d, segment %d: %d frames released part-way, %d of %d steps'
              % (args.blend, k, int(part.sum()), start_step + 1, steps))
    if args.resample is not None:
      run = steps if args.vary is None else vary_steps   # (plan_resample's counts, without the list)
      jump, times = args.resample
      print('resample %d:%d: %d steps and %d jumps per full segment' % (jump, times, times * run, (times - 1) * -(-run // jump)))
    edit = (old, start, stop)
  score_mel = None
  if scoring:   # the mel's shape and length against the MIDI file's segments, before any device work
    from msd_amd import audio_codecs, vocoder
    codec = audio_codecs.get_codec(spec.audio_codec)
    try:
      if args.score:
        score_mel = np.load(args.score)
        score_mel = score_mel[0] if score_mel.ndim == 3 and score_mel.shape[0] == 1 else score_mel
        if score_mel.ndim != 2 or score_mel.shape[1] != codec.n_dims:
          raise ValueError('%s must hold mel frames [frames, %d]: got %r' % (args.score, codec.n_dims, score_mel.shape))
        got = score_mel.shape[0]
      else:
        score_mel = vocoder.read_wav(args.score_audio, codec.sample_rate)
        got = -(-score_mel.size // codec.hop_size)
      if got > len(segments) * cfg.segment_frames:
        raise ValueError('the mel to score has %d frames, the MIDI file only %d (%d segments)'
                         % (got, len(segments) * cfg.segment_frames, len(segments)))
    except (ValueError, OSError) as e:
      ap.error(str(e))
  if args.dry_run:
    return 0
  model = msd_amd.InferenceModel(args.checkpoint, spec, batch_size=max(args.batch_segments, 1), precision=args.precision,
                                 range_fallback=args.range_fallback)
  if scoring:
    return _score(args, model, segments, score_mel, cfg)
  try:   # (before any sampling, and before the context recording is read)
    model.check_batch_segments(args.batch_segments, args.always_mask_context, args.context_audio)
  except ValueError as e:
    ap.error(str(e))
  if rerender is not None:
    return _rerender(args, model, segments, rerender, ns, cfg)
  if edit is not None:
    return _regenerate(args, model, segments, edit, ns, cfg)
  init_context = None
  if args.context_audio:
    if model.targets_context_length is None:
      ap.error('--context-audio needs a model with context')
    from msd_amd import vocoder
    init_context = context_from_audio(model, vocoder.read_wav(args.context_audio, model.audio_codec.sample_rate))
  mel, timing = model.predict_sequence(segments, seed=args.seed, rng=args.rng, return_timing=True, init_context=init_context,
                                       return_torch=True, always_mask_context=args.always_mask_context,
                                       batch_segments=args.batch_segments, **few)
  mel_dev, mel = mel, mel.cpu().numpy()
  frames = int(np.ceil(ns.total_time * cfg.frame_rate))
  mel = mel[0, :max(frames, 1)]
  print('synthesised %d mel frames; %.3f s per %.2f s segment (x%.2f realtime)'
        % (mel.shape[0], timing['prediction_seconds_per_chunk'], cfg.segment_frames / cfg.frame_rate,
           1.0 / timing['predictions_seconds_per_audio_second'] if timing['predictions_seconds_per_audio_second'] == timing['predictions_seconds_per_audio_second'] else float('nan')),
        file=sys.stderr)
  _write_outputs(args, model, mel_dev, mel)
  return 0


def _score(args, model, segments, mel, cfg) -> int:
  """--score / --score-audio: InferenceModel.score_sequence of the given mel (the recording's frames made on the device,
  as --edit-audio's), padded to whole segments with the codec's pad value.  'loss' / 'per_segment' sum over whole segments,
  the padding's frames included (the decoder sees them either way); 'loss_given_frames' sums the frames that were given."""
  import json
  torch = model._torch
  if args.score:
    song = torch.as_tensor(np.ascontiguousarray(mel, np.float32)).to(model.device)[None]
  else:
    song = model.vocoder.encode(np.asarray(mel, np.float32)[None], return_torch=True)
  given = int(song.shape[1])
  song = pad_to_segments(song, len(segments) * cfg.segment_frames, model.audio_codec.pad_value)
  t0 = time.perf_counter()
  res = model.score_sequence(song, segments, times=args.score_times, seed=args.seed, conditioning=args.score_conditioning,
                             always_mask_context=args.always_mask_context, rng=args.rng)
  passes = ['cond', 'uncond'] if args.score_conditioning == 'both' else [args.score_conditioning]
  print(json.dumps({'segments': len(segments), 'frames': given, 'times': [int(i) for i in res['times']],
                    'conditioning': args.score_conditioning, 'seconds': round(time.perf_counter() - t0, 4),
                    'loss': {p: float(res['loss'][k]) for k, p in enumerate(passes)},
                    'loss_given_frames': {p: float(res['per_frame'][k, :given].sum()) for k, p in enumerate(passes)},
                    'per_segment': {p: [float(v) for v in res['per_segment'][k]] for k, p in enumerate(passes)}}))
  return 0


def _write_outputs(args, model, mel_dev, mel):
  """--out / --wav of the song `mel` [frames, 128] (`mel_dev`: the device tensor [1, >= frames, 128] it was cut from)."""
  if args.out:
    np.save(args.out, mel)
  if args.wav:
    from msd_amd import vocoder
    t0 = time.perf_counter()
    audio = model.vocoder.decode(mel_dev[:, :mel.shape[0]], n_iters=args.vocoder_iters, seed=args.seed)
    gain = vocoder.write_wav(args.wav, audio[0], model.audio_codec.sample_rate)
    print('wrote %s: %d samples, %d Griffin-Lim iterations in %.3f s%s'
          % (args.wav, audio.shape[1], args.vocoder_iters, time.perf_counter() - t0,
             '' if gain == 1.0 else ' (peak-normalised, gain %.3f)' % gain), file=sys.stderr)


def resample_pair(text: str):
  """'JUMP:TIMES' -> (jump, times), both integers >= 1; anything else is a ValueError."""
  try:
    jump, times = (int(v) for v in text.split(':'))
  except ValueError:
    raise ValueError('--resample wants JUMP:TIMES, two integers: %r' % (text,))
  if jump < 1 or times < 1:
    raise ValueError('--resample wants JUMP >= 1 and TIMES >= 1: %r' % (text,))
  return jump, times


def interval_pair(text: str):
  """'LO:HI' -> (lo, hi), floats with 0 <= lo < hi <= 1; anything else is a ValueError."""
  try:
    lo, hi = (float(v) for v in text.split(':'))
  except ValueError:
    raise ValueError('--guidance-interval wants LO:HI, two numbers: %r' % (text,))
  if not 0.0 <= lo < hi <= 1.0:
    raise ValueError('--guidance-interval wants 0 <= LO < HI <= 1: %r' % (text,))
  return lo, hi


def region_frames(text: str, frame_rate: float):
  """'START:STOP' in seconds -> (start_frame, stop_frame), rounded OUTWARD to whole frames of 1 / frame_rate seconds
  (a time that is a whole frame up to 1e-6 frames is that frame)."""
  try:
    a, b = (float(v) for v in text.split(':'))
  except ValueError:
    raise ValueError('--regenerate wants START:STOP in seconds: %r' % (text,))
  if not 0.0 <= a < b:
    raise ValueError('--regenerate wants 0 <= START < STOP: %r' % (text,))
  return int(np.floor(round(a * frame_rate, 6))), int(np.ceil(round(b * frame_rate, 6)))


def pad_to_segments(mel, n_frames: int, pad_value: float):
  """mel [1, frames, n] (device tensor) padded at its end with the codec's pad value to n_frames."""
  if mel.shape[1] >= n_frames:
    return mel[:, :n_frames]
  pad = mel.new_full((1, n_frames - mel.shape[1], mel.shape[2]), pad_value)
  import torch
  return torch.cat([mel, pad], dim=1)


def _regenerate(args, model, segments, edit, ns, cfg) -> int:
  old, start, stop = edit
  torch = model._torch
  if args.edit_mel:
    song = torch.as_tensor(np.ascontiguousarray(old, np.float32)).to(model.device)[None]
  else:   # the recording's frames, made on the device as a context recording's are (context_from_audio)
    song = model.vocoder.encode(np.asarray(old, np.float32)[None], return_torch=True)
  song = pad_to_segments(song, len(segments) * cfg.segment_frames, model.audio_codec.pad_value)
  t0 = time.perf_counter()
  kw = {} if getattr(args, 'resample', None) is None else dict(resample=tuple(args.resample))
  if args.vary is not None:
    mel_dev = model.vary(song, segments, args.vary, seed=args.seed, always_mask_context=args.always_mask_context,
                         rng=args.rng, return_torch=True, **kw)
  else:
    if args.blend:
      kw['blend_frames'] = args.blend
    mel_dev = model.regenerate(song, segments, start, stop, seed=args.seed, always_mask_context=args.always_mask_context,
                               rng=args.rng, return_torch=True, **kw)
  frames = int(np.ceil(ns.total_time * cfg.frame_rate))
  mel = mel_dev.cpu().numpy()[0, :max(frames, 1)]
  if args.vary is not None:
    print('varied %d frames at strength %g in %.3f s' % (mel.shape[0], args.vary, time.perf_counter() - t0), file=sys.stderr)
  else:
    print('regenerated frames [%d, %d) of %d in %.3f s' % (start, stop, mel.shape[0], time.perf_counter() - t0), file=sys.stderr)
  _write_outputs(args, model, mel_dev, mel)
  return 0


def _rerender(args, model, segments, rerender, ns, cfg) -> int:
  """--rerender: InferenceModel.rerender of the old rendering (padded to whole segments with the codec's pad value) from
  the old notes' tokens to this file's, one weight for both directions."""
  old, old_segments = rerender
  torch = model._torch
  if args.edit_mel:
    song = torch.as_tensor(np.ascontiguousarray(old, np.float32)).to(model.device)[None]
  else:
    song = model.vocoder.encode(np.asarray(old, np.float32)[None], return_torch=True)
  song = pad_to_segments(song, len(segments) * cfg.segment_frames, model.audio_codec.pad_value)
  w = 1.0 if args.guidance is None else args.guidance
  own = model.spec.diffusion.classifier_free_guidance.eval_condition_weight
  t0 = time.perf_counter()
  mel_dev = model.rerender(song, old_segments, segments, steps=args.steps, guidance=w,
                           render_guidance=None if w == own else w, always_mask_context=args.always_mask_context,
                           return_torch=True)
  frames = int(np.ceil(ns.total_time * cfg.frame_rate))
  mel = mel_dev.cpu().numpy()[0, :max(frames, 1)]
  print('rerendered %d frames in %.3f s' % (mel.shape[0], time.perf_counter() - t0), file=sys.stderr)
  _write_outputs(args, model, mel_dev, mel)
  return 0


def context_from_audio(model, samples):
  """The last targets_context_length frames of a recording as predict_sequence(init_context=): log-mel [1, C, 128] made on
  the device (model.vocoder.encode); a shorter recording is padded in front with the codec's pad value."""
  c_len, hop = model.targets_context_length, model.audio_codec.hop_size
  samples = np.asarray(samples, np.float32).reshape(-1)
  if samples.size == 0:
    raise ValueError('the context recording is empty')
  whole = samples[:samples.size // hop * hop] if samples.size >= hop else samples   # whole frames, so that none is half silence
  mel = model.vocoder.encode(whole[None, -c_len * hop:], return_torch=True)
  if mel.shape[1] < c_len:
    pad = mel.new_full((1, c_len - mel.shape[1], mel.shape[2]), model.audio_codec.pad_value)
    mel = model._torch.cat([pad, mel], dim=1)
  return mel[:, -c_len:]


if __name__ == '__main__':
  sys.exit(main())
