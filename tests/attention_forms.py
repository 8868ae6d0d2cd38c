"""The forms the decoder launches attention in (csrc/msd_api.hip attention<NP>() and its callers), as cases of
msd_op_attention_launch: the case matrix, the caller-layout arrays of a case, and a Python mirror of the launcher's
block-shape rule.  Plain NumPy: tests/test_attention_forms_host.py checks this file without a GPU,
tests/test_gpu_attention_forms.py runs the cases.

Layouts
  'self'   q and k interleaved in one [segs * rows, 2J] buffer (q at column 0, k at column J), the key allocation
           exactly the segment: encoder and decoder self-attention
  'cross'  q [segs * rows, ldq] at column q_col; k [segs * k_alloc_rows, J] and v [segs, k_alloc_rows, J] caches of which
           the launch sees the WINDOW of k_rows keys from key k_row0 of every segment: cross-attention (ldq = J) and its
           folded form (ldq = 2J: two modules' un-normalised queries side by side, q_ssq row sums)
Inside the window, the keys behind n_keys[s] are LOUD but finite: K rows +-100, V rows +-1000 (both inside the half
planes' range).  Their softmax weight is exactly 0, so they must not move the output by a bit.  Outside the window (and
in the other module's query columns) the arrays hold NaN: the op never looks at them."""
import dataclasses
from typing import Optional, Tuple

import numpy as np

HEAD_DIM = 64
STAGE_KEYS = 128         # csrc/attention.h kAttStageKeys
SSQ_TILES = 24           # the decoder's D / 32 at D = 768
PREFETCH_SHAPE = (512, 768)   # rows, k of the weight target a case with `prefetch` carries
TWO_PLANE = ('f16x3', 'bf16x3')

# (k_alloc_rows, k_row0, k_rows): two regions each of a cache of 1088 and of 448 keys per segment; the windows of 64 and
# of 192 keys are no whole 128-key stages
WIN_1024, WIN_64, WIN_192, WIN_256 = (1088, 0, 1024), (1088, 1024, 64), (448, 0, 192), (448, 192, 256)
WINDOWS = (WIN_1024, WIN_64, WIN_192, WIN_256)
CACHES = ((WIN_1024, WIN_64), (WIN_192, WIN_256))   # the regions that share one allocation


@dataclasses.dataclass(frozen=True)
class Case:
  group: str               # 'encoder_self' | 'decoder_self' | 'cross' | 'touch_ahead' | 'folded'
  prec: str
  heads: int
  segs: int
  rows: int                # query rows per segment
  layout: str              # 'self' | 'cross'
  window: Tuple[int, int, int]   # (k_alloc_rows, k_row0, k_rows)
  n_keys: Tuple[int, ...]
  seed: int
  qp: int = 0
  ksplit: int = 1
  merge_in_launch: bool = False
  repeats: int = 1
  allow_qb4: bool = False
  prefetch: bool = False
  touch_ahead: int = 0
  pf_late: int = 1
  q_ld: int = 1            # ldq in units of J ('cross' layout)
  q_col: int = 0           # ... and the queries' first column in units of J
  q_ssq: bool = False      # un-normalised queries with SSQ_TILES row sums
  expect_qb: Optional[int] = None   # where the matrix NAMES the block shape (else the mirror's value)

  @property
  def J(self):
    return self.heads * HEAD_DIM

  @property
  def id(self):
    ka, r0, kr = self.window
    s = '%s-%s-h%d-s%d-r%d-w%d.%d.%d-n%s' % (self.group, self.prec, self.heads, self.segs, self.rows, ka, r0, kr,
                                            '.'.join(str(n) for n in self.n_keys))
    if self.qp: s += '-qp%d' % self.qp
    if self.ksplit > 1: s += '-ks%d%s' % (self.ksplit, 'inl' if self.merge_in_launch else 'sep')
    if self.allow_qb4: s += '-qb4'
    if self.prefetch: s += '-pf'
    if self.touch_ahead: s += '-ta%d%s' % (self.touch_ahead, '' if self.pf_late else 'early')
    if self.layout == 'cross' and self.q_ld > 1: s += '-q%dof%d' % (self.q_col, self.q_ld)
    if self.q_ssq: s += '-ssq'
    return s


# ---- the launcher's rule, mirrored (csrc/attention.h) ---------------------------------------------------------------
def attention_query_blocks(blocks64, q_rows_per_seg, planes):
  """attention_query_blocks: query blocks of 32 rows per workgroup for a launch of `blocks64` 64-row blocks."""
  if blocks64 < 128:
    return 1
  if planes == 2 and blocks64 > 256 and q_rows_per_seg % 128 == 0:
    return 4
  return 2


def ran_ksplit(ksplit):
  """launch_attention: the largest power of two <= ksplit."""
  return 1 << (int(ksplit).bit_length() - 1)


def expected_ran(case):
  """What msd_op_attention_launch reports for `case` (attention_launch_shape)."""
  planes = 2 if case.prec in TWO_PLANE else 1
  ks = ran_ksplit(case.ksplit)
  blocks64 = case.heads * (case.rows // 64) * ks * case.segs
  capped = blocks64 if (case.allow_qb4 and not case.q_ssq) else min(blocks64, 256)
  qb = attention_query_blocks(capped, case.rows, planes)
  wave = planes == 2 and case.prefetch and qb < 4
  return {'ran_qb': qb, 'ran_prefetch_wave': int(wave), 'ran_touch_ahead': int(wave and case.touch_ahead > 0),
          'ran_ksplit': ks}


def stages(n_keys, ksplit=1):
  """Key-loop stages of each split part of a segment of n_keys keys (attention_kernel: part ks takes the stages
  ks, ks + ksplit, ...)."""
  all_ = -(-n_keys // STAGE_KEYS)
  ks = ran_ksplit(ksplit)
  return [max(0, -(-(all_ - part) // ks)) for part in range(ks)]


# ---- caller-layout arrays -------------------------------------------------------------------------------------------
def loud_padding(x, n_valid, level):
  """x [keys, J] with the rows from n_valid on replaced by +level / -level (alternating by row)."""
  out = np.array(x, np.float32, copy=True)
  pad = np.arange(n_valid, out.shape[0])
  out[pad] = np.where(pad % 2 == 0, level, -level).astype(np.float32)[:, None]
  return out


def launch_fields(case):
  """The integer members of msd_attention_launch_args of `case`."""
  ka, r0, kr = case.window
  J = case.J
  f = dict(qp=case.qp, heads=case.heads, segs=case.segs, q_rows_per_seg=case.rows, repeats=case.repeats,
           ksplit=case.ksplit, merge_in_launch=int(case.merge_in_launch), allow_qb4=int(case.allow_qb4),
           k_alloc_rows=ka, k_row0=r0, k_rows=kr, touch_ahead=case.touch_ahead, pf_late=case.pf_late)
  if case.layout == 'self':
    f.update(ldq=2 * J, q_col=0, ldk=2 * J, k_col=J)
  else:
    f.update(ldq=case.q_ld * J, q_col=case.q_col * J, ldk=J, k_col=0)
  if case.prefetch:
    f.update(prefetch_rows=PREFETCH_SHAPE[0], prefetch_k=PREFETCH_SHAPE[1])
  if case.q_ssq:
    f.update(q_tiles=SSQ_TILES)
  return f


def k_windows(case):
  """[start, stop) of every segment's window, in rows of the flat [segs * k_alloc_rows] key allocation."""
  ka, r0, kr = case.window
  return [(s * ka + r0, s * ka + r0 + kr) for s in range(case.segs)]


def pack(case, q_s, k_s, v_s, ssq_s=None):
  """Per-segment contiguous q_s[s] [rows, J], k_s[s] / v_s[s] [k_rows, J] (and ssq_s[s] [rows, SSQ_TILES]) -> the op's
  arrays in the caller's layout: dict(q, k, v, n_keys[, q_ssq]); 'self': q and k are the SAME array."""
  ka, r0, kr = case.window
  J, segs, rows = case.J, case.segs, case.rows
  f = launch_fields(case)
  kp = [loud_padding(k_s[s], case.n_keys[s], 100.0) for s in range(segs)]
  vp = [loud_padding(v_s[s], case.n_keys[s], 1000.0) for s in range(segs)]
  v = np.full((segs, ka, J), np.nan, np.float32)
  for s in range(segs):
    v[s, r0:r0 + kr] = vp[s]
  if case.layout == 'self':
    assert (ka, r0, kr) == (rows, 0, rows)
    qk = np.empty((segs * rows, 2 * J), np.float32)
    for s in range(segs):
      qk[s * rows:(s + 1) * rows, :J] = q_s[s]
      qk[s * rows:(s + 1) * rows, J:] = kp[s]
    q = k = qk
  else:
    q = np.full((segs * rows, f['ldq']), np.nan, np.float32)
    k = np.full((segs * ka, f['ldk']), np.nan, np.float32)
    for s, (a, b) in enumerate(k_windows(case)):
      q[s * rows:(s + 1) * rows, f['q_col']:f['q_col'] + J] = q_s[s]
      k[a:b, f['k_col']:f['k_col'] + J] = kp[s]
  out = dict(q=q, k=k, v=v, n_keys=np.asarray(case.n_keys, np.int32))
  if ssq_s is not None:
    out['q_ssq'] = np.ascontiguousarray(np.concatenate(ssq_s, 0), np.float32)
  return out


def unpack(case, arrays):
  """The inverse of pack on the window: (q_s, k_s, v_s) per segment, the keys WITH their loud padding."""
  ka, r0, kr = case.window
  J, rows = case.J, case.rows
  f = launch_fields(case)
  q_s = [arrays['q'][s * rows:(s + 1) * rows, f['q_col']:f['q_col'] + J] for s in range(case.segs)]
  k_s = [arrays['k'][a:b, f['k_col']:f['k_col'] + J] for a, b in k_windows(case)]
  v_s = [arrays['v'][s, r0:r0 + kr] for s in range(case.segs)]
  return q_s, k_s, v_s


def split_output(case, o):
  """o [segs * rows, J] -> the segments' [rows, J]."""
  return [o[s * case.rows:(s + 1) * case.rows] for s in range(case.segs)]


def unnormalised_queries(rng, nq, j, d=32 * SSQ_TILES):
  """(q_unnorm, ssq [nq, d / 32], rstd): queries of O(1) logits times the 1/rstd of a random residual stream x [nq, d]
  whose row rms spans 1e-1 ... 1e3 (log-uniform), with rows 1e4 apart side by side in the first query block."""
  rms = 10.0 ** rng.uniform(-1, 3, nq)
  rms[:32:2], rms[1:32:2] = 0.1, 1e3
  x = rng.standard_normal((nq, d)) * rms[:, None]
  x = x.astype(np.float32).astype(np.float64)
  ssq = (x * x).reshape(nq, d // 32, 32).sum(-1).astype(np.float32)
  rstd = 1.0 / np.sqrt(ssq.astype(np.float64).sum(-1) / d + 1e-6)
  q = (rng.standard_normal((nq, j)) * 0.35 / rstd[:, None]).astype(np.float32)
  assert np.abs(q).max() < 65504
  return q, ssq, rstd


def make_inputs(case):
  """Seeded per case: q and k 0.35 N(0, 1), v N(0, 1) (tests/test_gpu_ops.py); q_ssq cases: un-normalised queries.
  -> (q_s, k_s, v_s, ssq_s or None, rstd_s or None), per segment."""
  rng = np.random.default_rng(case.seed)
  kr, J = case.window[2], case.J
  q_s, k_s, v_s, ssq_s, rstd_s = [], [], [], [], []
  for _ in range(case.segs):
    if case.q_ssq:
      q, ssq, rstd = unnormalised_queries(rng, case.rows, J)
      ssq_s.append(ssq); rstd_s.append(rstd)
    else:
      q = (rng.standard_normal((case.rows, J)) * 0.35).astype(np.float32)
    q_s.append(q)
    k_s.append((rng.standard_normal((kr, J)) * 0.35).astype(np.float32))
    v_s.append(rng.standard_normal((kr, J)).astype(np.float32))
  return q_s, k_s, v_s, (ssq_s if case.q_ssq else None), (rstd_s if case.q_ssq else None)


# ---- the matrix -----------------------------------------------------------------------------------------------------
def draw_n_keys(rng, k_rows, segs):
  """Different counts per segment from {0, 1, 33, 129, k_rows - 37, k_rows} (those that fit the window): one segment is
  full, with two or more segments one is empty."""
  pool = [n for n in (1, 33, 129, k_rows - 37) if 0 < n < k_rows]
  picked = [k_rows] + ([0] if segs >= 2 else [])
  picked += [int(n) for n in rng.choice(pool, size=segs - len(picked), replace=False)] if segs > len(picked) else []
  return tuple(int(n) for n in rng.permutation(picked))


def build_matrix():
  cases = []

  def add(**kw):
    cases.append(Case(seed=1000 + len(cases), **kw))

  # 1. encoder self-attention: one segment, q | k interleaved, ragged key counts; 192 rows with 129 keys: the second
  #    stage is clamped into the allocation
  for prec in ('f16x3', 'f16', 'bf16x3', 'bf16'):
    for rows, n in ((128, 1), (128, 33), (128, 100), (128, 128), (192, 129)):
      add(group='encoder_self', prec=prec, heads=2, segs=1, rows=rows, layout='self', window=(rows, 0, rows), n_keys=(n,))
  for qp in (1, 2, 3):
    add(group='encoder_self', prec='f16x3', heads=3, segs=1, rows=128, layout='self', window=(128, 0, 128), n_keys=(100,), qp=qp)

  # 2. decoder self-attention: segs = passes x batch, 12 heads: 96 / 144 / 384 64-row blocks -> 32-, 64-, 128-row blocks;
  #    with and without a weight target (the 128-row launch has no prefetch wave even when it is given one)
  for segs, qb, pfs in ((2, 1, (False, True)), (3, 2, (False, True)), (8, 4, (False, True))):
    for pf in pfs:
      add(group='decoder_self', prec='f16x3', heads=12, segs=segs, rows=256, layout='self', window=(256, 0, 256),
          n_keys=(256,) * segs, allow_qb4=True, prefetch=pf, expect_qb=qb, qp=3 if (segs == 3 and pf) else 0)
  add(group='decoder_self', prec='bf16x3', heads=12, segs=3, rows=256, layout='self', window=(256, 0, 256), n_keys=(256,) * 3,
      allow_qb4=True, prefetch=True, expect_qb=2)
  add(group='decoder_self', prec='f16', heads=12, segs=8, rows=256, layout='self', window=(256, 0, 256), n_keys=(256,) * 8,
      allow_qb4=True, prefetch=True, expect_qb=2)   # (one plane: no 128-row blocks, no prefetch)
  add(group='decoder_self', prec='f16x3', heads=2, segs=2, rows=256, layout='self', window=(256, 0, 256), n_keys=(256, 77),
      allow_qb4=True, prefetch=True, expect_qb=1)

  # 3. cross-attention windows: every region, 1 / 2 / 4 segments with different key counts, unsplit and key-split with
  #    the separate and the in-launch merge (three launches back to back: the counters reset); splits of 2 and 4 on the
  #    one-stage and two-stage windows leave parts without a stage.  Heads alternate between 2 and 12 (12: the block-shape
  #    thresholds: 48 x split x segs 64-row blocks); a launch of several segments may carry a weight target (the wave
  #    runs without touch-ahead, as in the batched decoder)
  rng = np.random.default_rng(2024)
  i = 0
  for window in WINDOWS:
    for segs in (1, 2, 4):
      splits = [(1, False)] + [(ks, inl) for ks in ((2, 4, 8) if window == WIN_1024 else (2, 4)) for inl in (False, True)]
      for ks, inl in splits:
        heads = 12 if i % 2 == 0 else 2
        prec = 'f16x3'
        if segs == 2 and ks == 2 and inl: prec = 'bf16x3'
        if segs == 4 and ks == 4 and inl: prec = 'f16'
        if segs == 2 and ks == 1: prec = 'bf16' if window in (WIN_64, WIN_256) else 'f16'
        add(group='cross', prec=prec, heads=heads, segs=segs, rows=256, layout='cross', window=window,
            n_keys=draw_n_keys(rng, window[2], segs), ksplit=ks, merge_in_launch=inl, repeats=3 if inl else 1,
            allow_qb4=True, prefetch=(segs > 1 and i % 3 == 0))
        i += 1

  # 4. touch-ahead: one segment, 12 heads, a weight target; the prefetch wave walks the block's stages 1 / 2 / 16 ahead of
  #    the ring and takes part in its barriers, on 0, 1, 2, 3 and 8 stages (below and above NS + ahead), unsplit (32-row
  #    blocks) and split four ways in the launch (64-row blocks)
  for window, counts in ((WIN_1024, (0, 1, 129, 257, 1000, 1024)), (WIN_192, (129, 192))):
    for ks in (1, 4):
      for n in counts:
        for ahead in (1, 2, 16):
          add(group='touch_ahead', prec='f16x3', heads=12, segs=1, rows=256, layout='cross', window=window, n_keys=(n,),
              ksplit=ks, merge_in_launch=ks > 1, allow_qb4=True, prefetch=True, touch_ahead=ahead)
  add(group='touch_ahead', prec='f16x3', heads=12, segs=1, rows=256, layout='cross', window=WIN_1024, n_keys=(1000,),
      allow_qb4=True, prefetch=True, touch_ahead=2, pf_late=0)
  add(group='touch_ahead', prec='bf16x3', heads=12, segs=1, rows=256, layout='cross', window=WIN_1024, n_keys=(1000,),
      ksplit=4, merge_in_launch=True, allow_qb4=True, prefetch=True, touch_ahead=2)

  # 5. folded cross-attention: two modules' un-normalised queries side by side (ldq = 2J), row sums per segment; one
  #    segment carries the weight target and the touch-ahead, as the decoder does at one song.  The form takes no 128-row
  #    blocks: the last case (384 64-row blocks) must run on 64-row blocks
  i = 0
  for window in (WIN_192, WIN_1024):
    for segs in (1, 2):
      for ks in (1, 2):
        for prec in TWO_PLANE:
          add(group='folded', prec=prec, heads=12 if ((i >> 1) + (i >> 2)) % 2 == 0 else 2, segs=segs, rows=256, layout='cross',
              window=window, n_keys=draw_n_keys(rng, window[2], segs), ksplit=ks, merge_in_launch=ks > 1,
              repeats=3 if ks > 1 else 1, allow_qb4=True, prefetch=segs == 1, touch_ahead=2 if segs == 1 else 0, q_ld=2,
              q_col=((i >> 1) + (i >> 3)) % 2, q_ssq=True)
          i += 1
  add(group='folded', prec='f16x3', heads=12, segs=4, rows=256, layout='cross', window=WIN_192,
      n_keys=draw_n_keys(rng, 192, 4), ksplit=2, merge_in_launch=True, repeats=3, allow_qb4=True, q_ld=2, q_col=1,
      q_ssq=True, expect_qb=2)
  add(group='folded', prec='f16x3', heads=2, segs=1, rows=256, layout='cross', window=WIN_192, n_keys=(155,), qp=1,
      allow_qb4=True, q_ld=2, q_col=0, q_ssq=True)
  return cases


MATRIX = build_matrix()
