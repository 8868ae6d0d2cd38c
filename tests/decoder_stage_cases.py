"""The wired decoder step (csrc/msd_api.hip in_proj / self_attention_block / cross_attention_block / mlp_block /
final_projection under plan_step) as cases: the model specs and their truncations, the songs, the calls, the ONE Python
statement of what a decoder evaluation leaves in the handle's per-step buffers, and the float64 reference of every such
buffer from the oracle's trace (oracle/fast.py FastModel.decoder_pass(trace=...)).  Plain NumPy:
tests/test_decoder_stage_cases_host.py checks this file without a GPU, tests/test_gpu_decoder_stages.py runs the cases.

Truncation.  The per-step buffers are overwritten layer by layer: a handle shows its LAST layer's stages only.  A depth-k
model's parameters are the full-depth parameter dict filtered to the names of the depth-k spec, so layer l of a depth-k
model IS layer l of every deeper one, and depths 1 .. 3 show layer 0 (StepPlan::self[0], fed by in_proj), a middle layer
(self[1], a fold_next producer in front and behind) and a last layer (decoder_norm gain) as a handle's last.

What survives a decoder evaluation (L = the last layer, B songs of T frames, BT = B T, pass p in rows [p BT, (p + 1) BT);
a CFG step has the conditional pass first, a single pass is pass 0; J = heads 64, F = mlp width, nq = n_cross J):
  qk    [M, 2 J]       q | k of layer L's self-attention; L = 0 under dedup_layer0 (CFG): the first BT rows only
  vt    [M / T][J][T]  v transposed, one segment per (pass, song), keys permuted per 16 (encode_cases.vt_key_pos)
  ao    [M, J]         conditional rows: module 0's cross-attention output (it overwrites the self-attention output);
                       unconditional rows: the self-attention output (not written at L = 0 under dedup)
  ao2   [Bmax T, J]    module 1's cross-attention output (sum_cross_attends with a context encoder)
  cq    folded projection: [BT, nq], the UN-normalised queries (x1 (.) gamma_cross) Wq_e of all modules side by side
        (the attention applies 1 / rms from ssq); else [Bmax T, J] per module (cq2 = module 1): the normalised q_e
  qp    [BT, nq] float32 (folded only): (x0 (.) gamma_cross) Wq_e side by side      xg  [BT, D]: x0 (.) gamma_cross
  g     [M, F]         the gated product
  x     [M, D]         x3, the residual stream after the MLP
  ssq   [M, D / 32]    partial sums of x3^2: the SUM of a row's slots is sum x3^2 (consumers add all slots); the slot
                       contents depend on the producing tile's width -- 32 columns each where D has no 48-wide tiling
  y     [M, D]         x3 (.) gamma_decoder_norm (un-normalised: the consumer applies 1 / rms)
  eps   [M, 128]
The folded projection (plan_step's `fold`) is restated in plans_fold below."""
import dataclasses
from typing import Tuple

import numpy as np

import msd_amd
from tests.encode_cases import round_up, stats, vt_key_pos  # noqa: F401 -- re-exported: ONE statement of each

N_MEL = 128
N_SONGS = 4


# ---- specs ----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class StageSpec:
  name: str
  emb: int
  heads: int
  mlp: int
  T: int
  inputs: int
  context: int
  style: str
  depths: Tuple[int, ...]
  seed: int

  @property
  def J(self):
    return self.heads * 64

  @property
  def n_cross(self):
    return 2 if self.style == 'sum_cross_attends' else 1


SPECS = {s.name: s for s in (
    StageSpec('N', 128, 2, 256, 64, 128, 64, 'concat_encodings', (1, 2), 41),
    StageSpec('M', 512, 6, 1024, 64, 256, 64, 'sum_cross_attends', (1, 2), 42),
    StageSpec('W', 768, 12, 2048, 256, 2048, 256, 'concat_encodings', (1, 2, 3), 43),
)}


def build_spec(name, depth, num_steps=5):
  """The ModelSpec of SPECS[name] with `depth` decoder layers and ONE encoder layer (the encoder has its own test:
  here it only supplies keys): dataclasses.replace of the tiny_context preset."""
  sc = SPECS[name]
  assert depth in sc.depths
  base = msd_amd.config.preset('tiny_context', num_steps=num_steps)
  t5 = dataclasses.replace(base.t5, emb_dim=sc.emb, num_heads=sc.heads, mlp_dim=sc.mlp, num_encoder_layers=1,
                           num_decoder_layers=depth, decoder_cross_attend_style=sc.style)
  return dataclasses.replace(base, t5=t5, task_feature_lengths={'inputs': sc.inputs, 'targets': sc.T,
                                                                'targets_context': sc.context})


_full_params = {}


def build_params(name, depth):
  """The FULL-depth parameters of the spec filtered to the depth-`depth` spec's names (Truncation, above)."""
  sc = SPECS[name]
  if name not in _full_params:
    _full_params[name] = msd_amd.synthetic.init_params(build_spec(name, max(sc.depths)), sc.seed, norm_scale_jitter=0.1)
  names = msd_amd.config.param_shapes(build_spec(name, depth))
  return {k: _full_params[name][k] for k in names}


# ---- songs ----------------------------------------------------------------------------------------------------------
def songs(name):
  """N_SONGS fixed songs and their z: [0] full tokens + full context, [1] 8 tokens + no context, [2] all padding + no
  context (no key at all: a zero cross update inside a batched launch; reached at B >= 3), [3] ragged.  -> (batch dict of
  the model's features, z [N_SONGS, T, 128])."""
  sc = SPECS[name]
  rng = np.random.default_rng([2046, sc.seed])
  spec = build_spec(name, sc.depths[0])
  toks = np.zeros((N_SONGS, sc.inputs), np.int32)
  mask = np.zeros((N_SONGS, sc.context), np.int32)
  toks[0, :sc.inputs - 2] = rng.integers(3, 255, sc.inputs - 2)
  toks[0, sc.inputs - 2] = 1
  mask[0] = 1
  toks[1, :8] = rng.integers(3, 255, 8)
  toks[1, 8] = 1
  toks[3] = msd_amd.synthetic.segment_tokens(spec, 303, min_len=8, max_len=sc.inputs - 2)[0]
  mask[3, :17] = 1
  batch = {'encoder_input_tokens': toks,
           'encoder_continuous_inputs': rng.uniform(-13, 5, (N_SONGS, sc.context, N_MEL)).astype(np.float32),
           'encoder_continuous_mask': mask,
           'decoder_target_tokens': np.zeros((N_SONGS, sc.T, N_MEL), np.float32)}
  return batch, rng.standard_normal((N_SONGS, sc.T, N_MEL)).astype(np.float32)


def sub_batch(batch, rows):
  return {k: np.ascontiguousarray(v[list(rows)]) for k, v in batch.items()}


# ---- calls ----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Call:
  name: str
  depth: int
  batch: int
  kind: str                 # 'single' (msd_decoder_pass on a 5-step handle) | 'cfg' (one CFG step on a 1-step handle)
  step: int = 0             # scan index
  cond: bool = True         # single passes only
  variant: str = 'default'  # 'default' | 'prefetch' | 'no_fold' | 'no_dedup'
  precision: str = 'f16x3'

  @property
  def passes(self):
    return 2 if self.kind == 'cfg' else 1

  @property
  def num_steps(self):
    return 1 if self.kind == 'cfg' else 5

  @property
  def model_kw(self):
    return {'default': {}, 'prefetch': dict(weight_prefetch=True), 'no_fold': dict(cross_q_fold=False),
            'no_dedup': dict(dedup_layer0=False)}[self.variant]

  def pass_cond(self, p):
    return (p == 0) if self.kind == 'cfg' else self.cond

  @property
  def tag(self):
    return '%s/d%d/B%d/%s%s/%s' % (self.name, self.depth, self.batch, self.kind,
                                   '' if self.kind == 'cfg' else '-i%d-%s' % (self.step, 'cond' if self.cond else 'uncond'),
                                   self.variant if self.variant != 'default' else self.precision)


SINGLE_STEPS = (0, 2, 4)
SINGLE_BATCH = {'N': 2, 'M': 2, 'W': 1}
# (spec, depth, precision) of the single-pass matrix: f16x3 everywhere, bf16x3 on N and on W at depth 2, f16 on N
SINGLE_HANDLES = tuple([(s.name, d, 'f16x3') for s in SPECS.values() for d in s.depths] +
                       [('N', 1, 'bf16x3'), ('N', 2, 'bf16x3'), ('W', 2, 'bf16x3'), ('N', 1, 'f16'), ('N', 2, 'f16')])


def single_calls(name, depth, precision):
  return [Call(name, depth, SINGLE_BATCH[name], 'single', i, cond, 'default', precision)
          for i in SINGLE_STEPS for cond in (True, False)]


# (spec, depth, batch, variant) of the CFG matrix.  By plan_step: B 1, 2 = layer-0 dedup with the folded query projection;
# W at B 3 (M = 1536) = no fold, 128-row attention blocks; W at B 4 (M = 2048) = 128-row GEMM tiles and the persistent
# gated-MLP-in loop; 'prefetch' = touch blocks on the attention launches of the truncated W (below the size rule)
CFG_CASES = tuple([(n, d, b, 'default') for n in ('N', 'M') for d in (1, 2) for b in (1, 2)] +
                  [('W', 2, b, 'default') for b in (1, 2, 3, 4)] + [('W', 1, 1, 'default'), ('W', 3, 1, 'default')] +
                  [('W', 2, 1, v) for v in ('prefetch', 'no_fold', 'no_dedup')] +
                  # two modules UN-folded: cq / cq2 per module (cq2 = the second half of cq's allocation) and ao2
                  [('M', 1, 2, 'no_fold'), ('M', 2, 2, 'no_fold')])


def cfg_call(name, depth, batch, variant):
  return Call(name, depth, batch, 'cfg', 0, True, variant)


# ---- the planner's fold decision, restated (msd_api.hip plan_step / pick_tile) --------------------------------------
def tile_cost(M, N, bm, bn):
  blocks = (M // bm) * (N // bn)
  return -(-blocks // 256) * (bm + bn)


def plans_fold(call, layer):
  """Does `layer`'s cross-attention query projection run folded (StepPlan::SelfBlock::fold of p.of(layer)) in `call`?
  Two-plane precisions, a conditional pass, M <= 1024, 64-row QKV tiles whose width divides nq, 32-column
  attention-out tiles."""
  sc = SPECS[call.name]
  if call.variant == 'no_fold' or not call.precision.endswith('x3'):
    return False
  D, J, nq, BT = sc.emb, sc.J, sc.n_cross * sc.J, call.batch * sc.T
  M = call.passes * BT
  if not (call.pass_cond(0) and M <= 1024 and BT % 64 == 0 and D // 32 <= 32 and D % 128 == 0):
    return False
  dup = call.kind == 'cfg' and call.variant != 'no_dedup' and layer == 0
  Ms = BT if dup else M
  N, align = 3 * J, 2 * J
  bn = 96 if (N % 96 == 0 and align % 96 == 0 and tile_cost(Ms, N, 64, 96) <= tile_cost(Ms, N, 64, 64)) else 64
  return nq % bn == 0   # (Ms < 2048: the QKV tile has 64 rows and the attention-out tile 32 columns)


def dedups_layer0(call):
  return call.kind == 'cfg' and call.variant != 'no_dedup'


# ---- the layout -----------------------------------------------------------------------------------------------------
def pass_rows(p, BT):
  return slice(p * BT, (p + 1) * BT)


def song_rows(p, b, B, T):
  """Rows of song b in pass p of an [M, .] buffer."""
  return slice((p * B + b) * T, (p * B + b + 1) * T)


def read_rows(flat, width, rows):
  return flat.reshape(-1, width)[rows]


def read_v(vt_flat, J, T, seg):
  """v [T, J] of segment `seg` = pass * B + song from the flat `vt` read."""
  return vt_flat.reshape(-1, J, T)[seg][:, vt_key_pos(np.arange(T))].T


def read_cq_folded(cq_flat, BT, n_cross, J, b, T, e):
  """Module e's un-normalised queries of song b from the folded projection's [BT, n_cross J]."""
  return cq_flat[:BT * n_cross * J].reshape(BT, n_cross * J)[b * T:(b + 1) * T, e * J:(e + 1) * J]


def ssq_row_sums(ssq_rows):
  """[rows, D / 32] slots -> sum x^2 per row, as every consumer adds them (float64: the reading adds no error)."""
  return np.asarray(ssq_rows, np.float64).sum(-1)


def slot_sums32(x):
  """[rows, D] -> [rows, D / 32]: sum of squares of every 32 columns (the slots of a 32-column tiling)."""
  x = np.asarray(x, np.float64)
  return (x.reshape(x.shape[0], -1, 32) ** 2).sum(-1)


def has_32_wide_slots(name):
  """No 48-column tiling of D exists (pick_tile: N % 48 == 0): every ssq slot is the sum of its own 32 columns."""
  return SPECS[name].emb % 48 != 0


# ---- the reference --------------------------------------------------------------------------------------------------
GEMM_SITES = ('self_attention/query', 'self_attention/key', 'self_attention/value', 'self_attention/out',
              'MultiHeadDotProductAttention_0/query', 'MultiHeadDotProductAttention_0/out', 'mlp/wi_0', 'mlp/wi_1', 'mlp/wo')
# the buffer (expected() key) a site's output shows in first
SITE_BUFFER = {'self_attention/query': 'q', 'self_attention/key': 'k', 'self_attention/value': 'v', 'self_attention/out': 'x1',
               'MultiHeadDotProductAttention_0/query': 'cq0', 'MultiHeadDotProductAttention_0/out': 'x2', 'mlp/wi_0': 'g',
               'mlp/wi_1': 'g', 'mlp/wo': 'x'}


def make_oracle(name, depth, dtype, precision='f32', num_steps=5, film=None, cls=None, torch_backend=False):
  """The oracle of a (spec, depth) with the decoder's input projection in the emulated precision, as the device's
  in_proj launch runs it (FastModel(in_proj_planes=True); nothing changes for precision 'f32', the reference).  torch_backend:
  the oracle's torch backend on the CPU (threaded contractions: the 2047-token songs of W)."""
  from oracle import backend, fast
  from tests import helpers
  spec = build_spec(name, depth, num_steps)
  cfg, dc = helpers.oracle_configs(spec)
  xp = backend.TorchBackend(dtype) if torch_backend else backend.NumpyBackend(dtype)
  fm = (cls or fast.FastModel)(xp, cfg, dc, build_params(name, depth), True, precision=precision, in_proj_planes=True)
  if film is not None:
    fm.set_film(film)
  return fm


def encode_songs(fm, batch, rows):
  sub = sub_batch(batch, rows)
  fm.encode(sub['encoder_input_tokens'], sub['encoder_continuous_inputs'], sub['encoder_continuous_mask'])


def expected(fm, tr, layer):
  """What the buffers hold of ONE song after a pass whose trace dict is `tr`, last layer `layer`, as float64 NumPy
  computed in fm's own arithmetic (float64 oracle: the reference; float32 emulation: the yardstick).  Keys: q k v self_ao
  x1 x2 g x ssq32 ssq y eps; on a pass with cross-attention input (conditional) also xg qp cq_fold cq<e> (normalised) and,
  for the modules with a valid key, ao<e>."""
  xp, p, c = fm.xp, fm.p, fm.cfg
  from oracle import ops
  lp = 'decoder/layers_%d' % layer
  out = {k: tr[k][layer] for k in ('q', 'k', 'v', 'self_ao', 'x1', 'x2', 'g')}
  x3 = tr['x3'][layer]
  out['x'] = x3
  sq = xp.square(x3)
  out['ssq32'] = xp.sum(xp.reshape(sq, (x3.shape[0], c.emb_dim // 32, 32)), axis=-1)
  out['ssq'] = xp.sum(sq, axis=-1)
  out['y'] = x3 * p['decoder/decoder_norm/scale']
  out['eps'] = tr['eps']
  out['has_cross'] = tr['cross_in'][layer] is not None
  n_cross = 2 if (fm.sum_style and fm.context) else 1
  gamma = p[lp + '/pre_cross_attention_layer_norm/scale']
  out['xg'] = fm.planes(tr['x0'][layer] * gamma)   # (stored as planes, and the A operand of the next product as stored)
  names = [lp + '/MultiHeadDotProductAttention_%d/query/kernel' % e for e in range(n_cross)]
  out['qp'] = xp.concatenate([fm.mm(out['xg'], n) for n in names], -1)
  out['cq_fold'] = xp.concatenate([fm.mm(tr['x1'][layer] * gamma, n) for n in names], -1)
  h = ops.rms_layer_norm(xp, tr['x1'][layer], gamma)
  for e, n in enumerate(names):
    out['cq%d' % e] = fm.rq(fm.mm(h, n))
  for e, (q, a) in tr['cross'][layer].items():
    out['ao%d' % e] = a
  return {k: (v if isinstance(v, bool) else np.asarray(xp.to_numpy(v), np.float64)) for k, v in out.items()}


def trace_song(fm, z, step, cond, row):
  """The trace dict of encoded row `row` (fm.encode ran): decoder_pass on that row alone."""
  kv = fm.kv
  try:
    fm.kv = [kv[row]]
    trace = []
    fm.decoder_pass(fm.xp.asarray(z[None]), step, cond, trace=trace)
  finally:
    fm.kv = kv
  return trace[0]


# ---- what to compare ------------------------------------------------------------------------------------------------
def stage_items(call, bufs, p, b, exp):
  """[(buffer label, device array, reference key)] of song b in pass p: everything the table at the top says the call
  leaves of that (pass, song).  bufs: name -> flat debug read; exp: expected() of that (pass, song) -- only its keys are
  read here, so that the reference and the yardstick are cut the same way."""
  sc = SPECS[call.name]
  B, T, J, D, F, nx = call.batch, sc.T, sc.J, sc.emb, sc.mlp, sc.n_cross
  BT, L = B * T, call.depth - 1
  cond = call.pass_cond(p)
  rows = song_rows(p, b, B, T)
  self_written = not (dedups_layer0(call) and L == 0 and p == 1)
  items = []
  if self_written:
    qk = read_rows(bufs['qk'], 2 * J, rows)
    items += [('qk.q', qk[:, :J], 'q'), ('qk.k', qk[:, J:], 'k'), ('vt', read_v(bufs['vt'], J, T, p * B + b), 'v')]
  if cond:
    if 'ao0' in exp:
      items.append(('ao(cross 0)', read_rows(bufs['ao'], J, rows), 'ao0'))
    if nx == 2 and 'ao1' in exp:
      items.append(('ao2', read_rows(bufs['ao2'], J, slice(b * T, (b + 1) * T)), 'ao1'))
    if plans_fold(call, L):
      for e in range(nx):
        items.append(('cq(folded %d)' % e, read_cq_folded(bufs['cq'], BT, nx, J, b, T, e), ('cq_fold', e, J)))
        items.append(('qp(%d)' % e, read_cq_folded(bufs['qp'], BT, nx, J, b, T, e), ('qp', e, J)))
      items.append(('xg', read_rows(bufs['xg'], D, slice(b * T, (b + 1) * T)), 'xg'))
    else:
      items.append(('cq', read_rows(bufs['cq'], J, slice(b * T, (b + 1) * T)), 'cq0'))
      if nx == 2:
        items.append(('cq2', read_rows(bufs['cq2'], J, slice(b * T, (b + 1) * T)), 'cq1'))
  elif self_written:
    items.append(('ao(self)', read_rows(bufs['ao'], J, rows), 'self_ao'))
  ssq = read_rows(bufs['ssq'], D // 32, rows)
  items += [('g', read_rows(bufs['g'], F, rows), 'g'), ('x', read_rows(bufs['x'], D, rows), 'x'),
            ('ssq(sum)', ssq_row_sums(ssq), 'ssq'), ('y', read_rows(bufs['y'], D, rows), 'y'),
            ('eps', read_rows(bufs['eps'], N_MEL, rows), 'eps')]
  if has_32_wide_slots(call.name):
    items.append(('ssq(slots)', ssq, 'ssq32'))
  return items


def pick(exp, key):
  """The reference array of a stage_items key."""
  if isinstance(key, tuple):
    name, e, J = key
    return exp[name][:, e * J:(e + 1) * J]
  return exp[key]


def buffer_names(call):
  sc = SPECS[call.name]
  names = ['qk', 'vt', 'ao', 'cq', 'g', 'x', 'ssq', 'y', 'eps']
  if sc.n_cross == 2:
    names += ['ao2', 'cq2']
  if plans_fold(call, call.depth - 1):
    names += ['xg', 'qp']
  return names
