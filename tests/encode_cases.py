"""The encode stage (csrc/msd_api.hip encode_impl / encoder_stack) and the load-time tables (build_tables) as cases: the
model specs, the valid-count cases of a call, the ONE Python statement of where msd_encode leaves its results (the `enc`
buffer and the cross-attention K / V^T cache) and of the gated column interleave of the `bw_mlp` table.  Plain NumPy:
tests/test_encode_cases_host.py checks this file without a GPU, tests/test_gpu_encode_stage.py runs the cases.

Layout (msd_api.hip create / encode_impl; gemm_h16.h EpiQKV)
  S_pad      = round_up(L, 64) + round_up(C, 64) key rows per (decoder layer, batch row); key_off = (0, round_up(L, 64))
  regions    concat_encodings: ONE region (e = 0) of n_tok + n_ctx keys, the context's right behind the valid tokens;
             sum_cross_attends: region 0 = the n_tok token keys, region 1 = the n_ctx context keys from key_off[1]
  cross_k    [Ld][Bmax][S_pad][J]: key i of region e in row key_off[e] + i
  cross_vt   [Ld][Bmax][J][S_pad]: key i of region e in column key_off[e] + vt_key_pos(i) -- the keys of every 16
             permuted (gemm_h16.h vt_perm16; csrc/standalone_ops.h vt_key_pos)
  enc        [S_pad][D], the LAST row of the call: the regions' encodings at the regions' rows
  bw_mlp     [N][Ld][2F]: column n of wi_<which> at (n / 16) * 32 + which * 16 + n % 16 (gemm_f32.h EpiF32StoreGated)"""
import dataclasses
from typing import Optional, Tuple

import numpy as np

import msd_amd

N_MEL = 128
BATCH = 2


def round_up(n, m):
  return -(-n // m) * m


# ---- specs ----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class SpecCase:
  name: str
  preset: str
  emb: int
  heads: int
  mlp: int
  enc_layers: int
  dec_layers: int
  inputs: int
  context: int             # 0: no context encoder
  style: str               # 'concat_encodings' | 'sum_cross_attends'
  positions: str           # context_positions
  precisions: Tuple[str, ...]
  seed: int


SPECS = {s.name: s for s in (
    SpecCase('A', 'tiny_context', 128, 2, 256, 2, 2, 128, 64, 'concat_encodings', 'terminal_relative', ('f16x3', 'f16'), 31),
    SpecCase('A_regular', 'tiny_context', 128, 2, 256, 2, 2, 128, 64, 'concat_encodings', 'regular', ('f16x3',), 31),
    SpecCase('B', 'tiny_context', 512, 6, 1024, 2, 1, 256, 64, 'sum_cross_attends', 'terminal_relative', ('f16x3',), 32),
    SpecCase('C', 'tiny_context', 768, 12, 2048, 2, 2, 256, 128, 'concat_encodings', 'terminal_relative', ('f16x3', 'bf16x3'), 33),
    SpecCase('D', 'tiny', 128, 2, 256, 2, 2, 128, 0, 'concat_encodings', 'regular', ('f16x3',), 34),
)}
HANDLES = tuple((s.name, p) for s in SPECS.values() for p in s.precisions)
TABLE_SPECS = ('A', 'C')   # the load-time table tests, at num_steps = 5
NORM_VPL = {128: 1, 512: 2, 768: 3}   # rmsnorm_film_kernel<OUT, VPL>: float4 loads per lane, D <= 256 VPL


def build_spec(name, num_steps=3):
  """The ModelSpec of SPECS[name]: dataclasses.replace of the preset, targets 64."""
  sc = SPECS[name]
  base = msd_amd.config.preset(sc.preset, num_steps=num_steps)
  t5 = dataclasses.replace(base.t5, emb_dim=sc.emb, num_heads=sc.heads, mlp_dim=sc.mlp, num_encoder_layers=sc.enc_layers,
                           num_decoder_layers=sc.dec_layers, decoder_cross_attend_style=sc.style,
                           context_positions=sc.positions)
  lengths = {'inputs': sc.inputs, 'targets': 64}
  if sc.context:
    lengths['targets_context'] = sc.context
  return dataclasses.replace(base, t5=t5, task_feature_lengths=lengths)


def build_params(name, spec):
  return msd_amd.synthetic.init_params(spec, SPECS[name].seed, norm_scale_jitter=0.1)


# ---- valid-count cases ----------------------------------------------------------------------------------------------
COUNT_CASES = ('1_C', 'L_1', '63_0', '64_63', '65_64', '0_Cm1', 'holes')
HOLES_TOKENS, HOLES_CONTEXT = 40, 20


def case_masks(case, L, C):
  """(token validity bool [L], context validity bool [C]) of a valid-count case; the counted cases are prefixes."""
  tok, ctx = np.zeros(L, bool), np.zeros(C, bool)
  if case == 'holes':
    rng = np.random.default_rng(77)
    tok[rng.choice(L - 1, HOLES_TOKENS - 1, replace=False)] = True
    tok[L - 1] = True
    if C:
      ctx[1 + rng.choice(C - 1, HOLES_CONTEXT, replace=False)] = True
    return tok, ctx
  n_tok, n_ctx = {'1_C': (1, C), 'L_1': (L, 1), '63_0': (63, 0), '64_63': (64, 63), '65_64': (65, 64),
                  '0_Cm1': (0, C - 1)}[case]
  tok[:n_tok] = True
  ctx[:max(0, min(n_ctx, C))] = True
  return tok, ctx


# a call = (case of row 0, case of row 1): every case once in each row, the two rows of a call always different
CALLS = tuple((COUNT_CASES[(i + 1) % len(COUNT_CASES)], COUNT_CASES[i]) for i in range(len(COUNT_CASES)))


def make_call(name, call, seed=0):
  """The arguments of msd_encode for `call` on spec `name`: dict(tokens int32 [B, L], ctx float32 [B, C, 128] in mel
  units, mask int32 [B, C]) (ctx / mask None without a context encoder) -- seeded by (spec, call, seed)."""
  sc = SPECS[name]
  L, C = sc.inputs, sc.context
  rng = np.random.default_rng([sc.seed, seed] + [COUNT_CASES.index(c) for c in call])
  tokens = np.zeros((len(call), L), np.int32)
  mask = np.zeros((len(call), C), np.int32)
  for b, case in enumerate(call):
    tok, ctx = case_masks(case, L, C)
    tokens[b, tok] = rng.integers(1, 256, int(tok.sum()))
    mask[b, ctx] = 1
  out = dict(tokens=tokens, ctx=None, mask=None)
  if C:
    out.update(ctx=rng.uniform(-13, 5, (len(call), C, N_MEL)).astype(np.float32), mask=mask)
  return out


def valid_counts(call_args, b):
  """(n_tok, n_ctx) of batch row b."""
  n_ctx = 0 if call_args['mask'] is None else int((call_args['mask'][b] > 0).sum())
  return int((call_args['tokens'][b] > 0).sum()), n_ctx


# ---- the layout -----------------------------------------------------------------------------------------------------
def vt_perm16(o):
  """gemm_h16.h vt_perm16: key o of a 16-key group -> its place in the group."""
  return 8 * ((o >> 2) & 1) + (o & 3) + 4 * (o >> 3)


def vt_key_pos(key):
  """csrc/standalone_ops.h vt_key_pos (vectorised)."""
  key = np.asarray(key)
  return (key & ~15) + vt_perm16(key & 15)


@dataclasses.dataclass(frozen=True)
class Layout:
  L: int
  C: int
  D: int
  J: int
  F: int
  Ld: int
  n_cross: int
  sum_style: bool
  Bmax: int = BATCH

  @classmethod
  def of(cls, name, batch=BATCH):
    sc = SPECS[name]
    sum_style = sc.style == 'sum_cross_attends'
    return cls(sc.inputs, sc.context, sc.emb, sc.heads * 64, sc.mlp, sc.dec_layers,
               2 if (sum_style and sc.context) else 1, sum_style, batch)

  @property
  def S_pad(self):
    return round_up(self.L, 64) + round_up(self.C, 64)

  @property
  def key_off(self):
    return (0, round_up(self.L, 64))

  def regions(self, n_tok, n_ctx):
    """[(e, n_keys, (token keys, context keys) of the region)] of a row; a region may hold no key."""
    if self.n_cross == 2:
      return [(0, n_tok, (n_tok, 0)), (1, n_ctx, (0, n_ctx))]
    return [(0, n_tok + n_ctx, (n_tok, n_ctx))]

  def region_rows(self, e):
    """The key rows [start, stop) region e owns in a (layer, batch row) slab."""
    start = self.key_off[e]
    return start, (self.key_off[e + 1] if e + 1 < self.n_cross else self.S_pad)

  def shape_k(self):
    return (self.Ld, self.Bmax, self.S_pad, self.J)

  def shape_vt(self):
    return (self.Ld, self.Bmax, self.J, self.S_pad)

  def read_k(self, cross_k, l, b, e, n):
    """K [n, J] of the first n keys of region e from the flat debug read."""
    return cross_k.reshape(self.shape_k())[l, b, self.key_off[e]:self.key_off[e] + n]

  def read_v(self, cross_vt, l, b, e, n):
    """V [n, J] of the first n keys of region e from the flat debug read of V^T."""
    cols = self.key_off[e] + vt_key_pos(np.arange(n))
    return cross_vt.reshape(self.shape_vt())[l, b][:, cols].T

  def valid_mask_k(self, counts):
    """bool [Ld, Bmax, S_pad, J]: the entries of cross_k that hold a valid key; counts[b] = (n_tok, n_ctx)."""
    m = np.zeros(self.shape_k(), bool)
    for b, (n_tok, n_ctx) in enumerate(counts):
      for e, n, _ in self.regions(n_tok, n_ctx):
        m[:, b, self.key_off[e]:self.key_off[e] + n] = True
    return m

  def valid_mask_vt(self, counts):
    m = np.zeros(self.shape_vt(), bool)
    for b, (n_tok, n_ctx) in enumerate(counts):
      for e, n, _ in self.regions(n_tok, n_ctx):
        m[:, b, :, self.key_off[e] + vt_key_pos(np.arange(n))] = True
    return m

  def enc_rows(self, n_tok, n_ctx):
    """(first row of the token encodings, first row of the context encodings) in `enc`."""
    return 0, (self.key_off[1] if self.n_cross == 2 else n_tok)


# ---- the gated interleave of bw_mlp ---------------------------------------------------------------------------------
def gated_column(n, which):
  """gemm_f32.h EpiF32StoreGated: where column n of wi_<which> lands in a row of 2F."""
  return (n // 16) * 32 + which * 16 + n % 16


def split_gated(bw_mlp, F):
  """[..., 2F] in the packed order -> (wi_0 part [..., F], wi_1 part [..., F])."""
  n = np.arange(F)
  return bw_mlp[..., gated_column(n, 0)], bw_mlp[..., gated_column(n, 1)]


# ---- statistics and the oracle's side -------------------------------------------------------------------------------
def stats(got, ref64):
  """(rms error, largest absolute error), both divided by the rms of the float64 array."""
  ref64 = np.asarray(ref64, np.float64)
  d = np.asarray(got, np.float64) - ref64
  scale = float(np.sqrt(np.mean(ref64 ** 2)))
  return float(np.sqrt(np.mean(d ** 2))) / scale, float(np.abs(d).max()) / scale


def oracle_encode(fm, call_args):
  """Run FastModel.encode on a call -> per batch row dict(enc=(tok or None, ctx or None), kv={e: [(K [n, J], V [n, J])
  per decoder layer]}) as float64 NumPy."""
  xp = fm.xp
  if call_args['ctx'] is None:
    fm.encode(call_args['tokens'])
  else:
    fm.encode(call_args['tokens'], call_args['ctx'], call_args['mask'])
  rows = []
  for b in range(call_args['tokens'].shape[0]):
    to64 = lambda a: None if a is None else np.asarray(xp.to_numpy(a), np.float64)
    kv = {}
    for e, layers in (fm.kv[b] or []):
      kv[e] = [(to64(k).reshape(k.shape[0], -1), to64(v).reshape(v.shape[0], -1)) for k, v in layers]
    rows.append(dict(enc=tuple(to64(a) for a in fm.enc[b]), kv=kv))
  return rows


def make_oracle(name, spec, params, dtype, precision='f32'):
  from oracle import backend, fast
  from tests import helpers
  cfg, dc = helpers.oracle_configs(spec)
  return fast.FastModel(backend.NumpyBackend(dtype), cfg, dc, params, spec.has_context, precision=precision)
