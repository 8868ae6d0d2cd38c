"""Generate tests/golden/small_segments_n1000.npz: the float64 oracle's 1000-step `small` segments 0 .. 3, each a
one-row run of its own, which is what a row of a batched call with per-row keys has to reproduce.

  python tests/golden/make_batch_segments_golden.py [threads]

The construction is make_golden.py's `small` case continued to four segments (the model has no context, so the
segments are independent of each other): weights synthetic.init_params(spec, 0), tokens synthetic.segment_tokens(spec, k),
noise oracle.philox.segment_noise((1, T, n), 1000, seed=0, segment=k).  Segment 0 is small_n1000.npz's `mel`
(tests/test_batch_segments_host.py checks it).  The file holds `mel` float32 [1, 4 * 256, 128] and the seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

NAME = 'small_segments_n1000.npz'
N_SEGMENTS = 4

if __name__ == '__main__':
  make_golden.song('small', N_SEGMENTS, NAME, weight_seed=0, seed=0,
                   threads=int(sys.argv[1]) if len(sys.argv) > 1 else None)
