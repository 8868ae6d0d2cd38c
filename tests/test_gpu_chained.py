"""-m gpu: the chained context hand-off (BASELINE config 4; beam/evaluation.py:191-223) with the REAL
model on the device: one song cut across two ranks must be BIT-identical to the sequential song.

  * two processes on the one GPU of the test box, `sharding.chained_predict` over
    `InferenceModel.predict_sequence`, message over torch.distributed (gloo here: RCCL refuses two ranks on
    one device; on a multi-GPU node the same code path runs with comm_device=cuda over RCCL/xGMI,
    bench.py --mode chained|wavefront);
  * two handles in one process with the hand-off message kept in device memory
    (`predict_sequence(return_torch=True)` -> `init_context=<cuda tensor>`).
"""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _spec(preset, steps):
  import msd_amd
  return msd_amd.config.preset(preset, num_steps=steps)


def _segments(spec, n):
  import msd_amd
  return [msd_amd.synthetic.segment_tokens(spec, k, min_len=8, max_len=min(400, spec.task_feature_lengths['inputs'] - 2))
          for k in range(n)]


def _worker(rank, world, port, preset, steps, n_seg, q):
  import torch
  import torch.distributed as dist
  import msd_amd
  from msd_amd import sharding
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  torch.cuda.set_device(0)
  dist.init_process_group('gloo', rank=rank, world_size=world)
  try:
    spec = _spec(preset, steps)
    model = msd_amd.InferenceModel('synthetic:0', spec)
    segs = _segments(spec, n_seg)
    c = spec.task_feature_lengths['targets_context']
    local = sharding.chained_predict(model.predict_sequence, segs, (1, c, 128), rank, world, seed=4)
    full = sharding.gather_song(local, rank, world)
    wave = sharding.chained_wavefront(model.predict_sequence, [segs[:3], segs[1:]], (1, c, 128), rank, world, seed=9)
    wave_full = [sharding.gather_song(w, rank, world) for w in wave]
    if rank == 0:
      seq = model.predict_sequence(segs, seed=4)
      wseq = [model.predict_sequence(segs[:3], seed=9), model.predict_sequence(segs[1:], seed=10)]
      q.put((full, seq, wave_full, wseq))
  finally:
    dist.destroy_process_group()


@pytest.mark.parametrize('preset,steps,n_seg', [('tiny_context', 8, 5), ('base_with_context', 12, 4)])
def test_two_ranks_one_song_bit_identical_to_sequential(preset, steps, n_seg):
  import torch.multiprocessing as mp
  ctx = mp.get_context('spawn')
  q = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_worker, args=(r, 2, port, preset, steps, n_seg, q)) for r in range(2)]
  for p in procs:
    p.start()
  import queue
  import time
  result, deadline = None, time.time() + 600
  try:
    while result is None:
      try:
        result = q.get(timeout=2)
      except queue.Empty:
        dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
        assert not dead, 'a rank died with exit code %s before delivering its result' % dead
        assert time.time() < deadline, 'ranks did not finish in 600 s'
  finally:
    for p in procs:
      p.join(timeout=60)
      if p.is_alive():
        p.kill()
  full, seq, wave_full, wseq = result
  assert all(p.exitcode == 0 for p in procs)
  assert full.shape == seq.shape and np.isfinite(seq).all() and seq.std() > 0.1
  np.testing.assert_array_equal(full, seq)       # bit-for-bit: same kernels, same inputs, same noise keys
  for got, want in zip(wave_full, wseq):
    np.testing.assert_array_equal(got, want)


def test_device_resident_handoff_between_two_handles():
  """The hand-off message stays a device tensor: handle A's last prediction -> handle B's context."""
  import torch
  import msd_amd
  spec = _spec('tiny_context', 8)
  a = msd_amd.InferenceModel('synthetic:0', spec)
  b = msd_amd.InferenceModel('synthetic:0', spec)
  segs = _segments(spec, 5)
  c = spec.task_feature_lengths['targets_context']
  seq = a.predict_sequence(segs, seed=1)
  head = a.predict_sequence(segs[:2], seed=1, return_torch=True)
  assert isinstance(head, torch.Tensor) and head.is_cuda
  msg = head[:, -c:, :].contiguous()
  tail = b.predict_sequence(segs[2:], seed=1, init_context=msg, first_segment_index=2, return_torch=True)
  got = torch.cat([head, tail], dim=1).cpu().numpy()
  np.testing.assert_array_equal(got, seq)
  # and the masked-boundary mode differs exactly from the cut on (the reference's i == 0 behaviour there)
  from msd_amd import sharding
  parts = [sharding.masked_boundary_predict(a.predict_sequence, segs, r, 2, seed=1) for r in range(2)]
  cut = sharding.contiguous_chunk(len(segs), 1, 2)[0] * spec.task_feature_lengths['targets']
  masked = np.concatenate(parts, 1)
  np.testing.assert_array_equal(masked[:, :cut], seq[:, :cut])
  assert np.abs(masked[:, cut:] - seq[:, cut:]).max() > 1e-3


def test_plain_bench_command_two_ranks_real_model_handoff_leg():
  """The plain `python bench.py --gpus 2` with the REAL model (VERDICT r05 next #5b): both ranks on the one GPU of the
  test box, gloo as the transport (RCCL refuses two ranks on one device; on a multi-GPU node the same command runs over
  RCCL), one timed segment per rank, then the `handoff` leg -- BASELINE config 4's wavefront of songs x 2 segments with
  the context hand-off -- capped at 2 songs.  Checked: one JSON line, exit code 0, the leg's fields, the per-hop probe,
  the warm-up chain's cost, and that what each rank synthesized is BIT-identical to segment `rank` of the sequential
  song (digests of the float32 bytes)."""
  import hashlib
  import json
  import subprocess
  import sys
  import msd_amd
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  steps = 40
  env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
  p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--dist-backend', 'gloo', '--steps', '1',
                      '--warmup', '1', '--num-steps', str(steps), '--handoff-max-segments', '2', '--profile-steps', '1',
                      '--handoff-timeout', '300', '--full'], cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                     text=True, timeout=900)
  assert p.returncode == 0, p.stderr[-3000:]
  lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{') and l.rstrip().endswith('}')]
  assert len(lines) == 1, p.stdout[-2000:]
  d = lines[0]
  assert d['n_gpus'] == 2 and d['value'] > 0 and d['config']['mode'] == 'replicas' and d['config']['precision'] == 'f16x3'
  assert [r['rank'] for r in d['ranks_seen']] == [0, 1] and len({r['pid'] for r in d['ranks_seen']}) == 2
  hc = d['handoff_check']
  assert hc['ok'] is True and hc['hops'] == 1 and hc['message_bytes'] == 256 * 128 * 4 and hc['us_per_hop'] > 0
  assert hc['warm_up'] is not None and hc['warm_up']['p2p_chain_s'] >= 0      # the first point-to-point call was paid outside
  print('gloo hand-off on this box: %.0f us per 128 KiB hop; warm-up collective %.3f s, first point-to-point chain %.3f s'
        % (hc['us_per_hop'], hc['warm_up']['collective_s'], hc['warm_up']['p2p_chain_s']))
  h = d['handoff']
  assert h['ok'] is True and h['mode'] == 'wavefront' and h['songs'] == 2 and h['segments_per_song'] == 2 and h['segments'] == 4
  assert h['value'] > 0 and abs(h['ideal_efficiency'] - 2 / 3) < 1e-3
  rows = h['per_rank']
  assert [r['rank'] for r in rows] == [0, 1] and all(r['finite'] and len(r['segment_sha256_16']) == 2 for r in rows)
  assert all(0.0 <= r['idle_fraction'] <= 1.0 for r in rows)
  # the sequential songs, here, with the bench's own inputs: song j = segment_tokens seeds 1000 (100 + j) + k, noise seed 100 + j
  spec = msd_amd.config.preset('base_with_context', num_steps=steps)
  model = msd_amd.InferenceModel('synthetic:0', spec)
  t = spec.task_feature_lengths['targets']
  for j in range(2):
    toks = [msd_amd.synthetic.segment_tokens(spec, 1000 * (100 + j) + k) for k in range(2)]
    seq = model.predict_sequence(toks, seed=100 + j)
    for r in range(2):
      want = hashlib.sha256(np.ascontiguousarray(seq[:, r * t:(r + 1) * t], np.float32).tobytes()).hexdigest()[:16]
      assert rows[r]['segment_sha256_16'][j] == want, (j, r)


def test_plain_bench_dumps_what_its_last_timed_step_returned(tmp_path):
  """The plain `python bench.py --dump-outputs DIR` with the REAL model: DIR/mel.npy is BIT-identical to the last
  segment of the same song synthesized here through InferenceModel.predict (the bench's seeded tokens, context
  chaining, seed and segment indices), DIR/scores.npy holds predict's zeros, and the line carries no --full leg."""
  import json
  import subprocess
  import sys
  import torch
  import msd_amd
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  steps, warmup, timed = 20, 1, 2
  env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
  p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--preset', 'tiny_context',
                      '--num-steps', str(steps), '--steps', str(timed), '--warmup', str(warmup),
                      '--dump-outputs', str(tmp_path)], cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                     text=True, timeout=600)
  assert p.returncode == 0, p.stderr[-3000:]
  lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{') and l.rstrip().endswith('}')]
  assert len(lines) == 1, p.stdout[-2000:]
  d = lines[0]
  assert d['steps'] == timed and d['ms_per_step'] > 0 and d['config']['precision'] == 'f16x3'
  assert not {'roofline', 'batched', 'small', 'cpu_baseline'} & set(d)
  assert sorted(os.listdir(tmp_path)) == ['mel.npy', 'scores.npy']
  mel, scores = np.load(tmp_path / 'mel.npy'), np.load(tmp_path / 'scores.npy')
  assert mel.dtype == np.float32 and scores.dtype == np.float32 and scores.shape == (1,) and (scores == 0).all()
  spec = msd_amd.config.preset('tiny_context', num_steps=steps, cfg_weight=5.0)
  model = msd_amd.InferenceModel('synthetic:0', spec)
  c = model.targets_context_length
  pred = torch.zeros((1, c, 128), dtype=torch.float32, device=model.device)
  for k in range(warmup + timed):
    batch = {'encoder_input_tokens': msd_amd.synthetic.segment_tokens(spec, k), 'encoder_continuous_inputs': pred,
             'encoder_continuous_mask': (np.zeros if k == 0 else np.ones)((1, c), np.int32)}
    pred, _ = model.predict(batch, seed=0, segment=k, return_torch=True)
  np.testing.assert_array_equal(mel, pred.cpu().numpy())
