// C-ABI (include/msd_amd.h) and host runtime of the MI355X DDPM synthesizer:
// weight store + packing, step-indexed tables, encoder, the per-step kernel chain,
// hipGraph capture/replay of one DDPM step, profiling.  gfx950 only.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/msd_amd.h"
#include "attention.h"
#include "common.h"
#include "elementwise.h"
#include "gemm_h16.h"
#include "gemm_f32.h"
#include "vocoder.h"

using namespace msd;

namespace {

constexpr int kHeadDim = 64;
// Library default of the decoder attentions' query side under MSD_PREC_F16X3 (msd_config.attn_q_planes /
// attn_p_planes = 0): BOTH planes, like the memory side.  Round 3 ran Q and P on one half plane (-2.5 % step time,
// 1.05 - 1.29x the float32 oracle's error on fixtures whose attention logits are O(1)); on SHARP attention -- every
// decoder query kernel times 4: competing keys ~10 apart, what a trained model has -- one plane for Q costs 2.8x the
// float32 floor and one for P 1.25x (tests/diag/sharp_attention_study.py).  One plane stays an opt-in.
constexpr int kDefaultQPlanes = 2, kDefaultPPlanes = 2;

enum KClass { KC_NORM = 0, KC_GEMM_QKV, KC_ATTN_SELF, KC_GEMM_ATTN_OUT, KC_GEMM_CROSS_Q,
              KC_ATTN_CROSS, KC_GEMM_CROSS_OUT, KC_GEMM_MLP_IN, KC_GEMM_MLP_OUT,
              KC_FINAL_PROJ, KC_SAMPLER, KC_IN_PROJ, KC_COUNT };
const char* const kClassNames[KC_COUNT + 1] = {
    "rmsnorm_film", "gemm_qkv", "attn_self", "gemm_attn_out", "gemm_cross_q", "attn_cross",
    "gemm_cross_out", "gemm_mlp_in_geglu", "gemm_mlp_out", "final_proj_f32", "sampler_step",
    "in_proj_f32", nullptr};

struct Planes {
  h16_t* p[2] = {nullptr, nullptr};
};

struct Weight {
  std::string name;
  int64_t shape[2] = {0, 0};
  int ndim = 0;
  float* dev = nullptr;
  bool set = false;
  int64_t numel() const { return ndim == 1 ? shape[0] : shape[0] * shape[1]; }
};

struct AttnW {  // packed attention projections of one layer
  Planes wqkv;  // self: [3J, D] (q|k|v) ; encoder same
  Planes wo;    // [D, J]
};
struct MlpW {
  Planes wi;  // [2F, D] wi_0/wi_1 interleaved per 16
  Planes wo;  // [D, F]
};
struct EncLayerW {
  const float *ln_attn = nullptr, *ln_mlp = nullptr;
  AttnW attn;
  MlpW mlp;
};
struct DecLayerW {
  const float *ln_self = nullptr, *ln_cross = nullptr, *ln_mlp = nullptr;
  AttnW self;
  // one cross-attention module per key region: [0] = MultiHeadDotProductAttention_0 (concat_encodings: the
  // concatenated encodings; sum_cross_attends: the token encoder), [1] = ..._1 (sum_cross_attends: the context)
  Planes wq_cross[2];   // [J, D]
  Planes wkv_cross[2];  // [2J, D] (k|v)
  Planes wo_cross[2];   // [D, J]
  MlpW mlp;
  // folded cross-attention query projection (decoder_layers, gemm_h16.h): the modules' Wq^T stacked [n_cross J, D] (one
  // module: = wq_cross[0]) and W^T of Wo_self . diag(gamma_cross) . Wq_e stacked [n_cross J, J]
  Planes wq_fold, w2_fold;
};
struct EncoderW {
  std::vector<EncLayerW> layers;
  const float* final_ln = nullptr;
};

struct TileShape { int bm, bn; };   // a GEMM tile, BM x BN (pick_tile)

// msd_config.touch_carrier = 0: the library's choice (DESIGN.md 6 "Weight prefetch": the measurement that decides it)
constexpr int kTouchCarrierDefault = 2;
constexpr int kTouchBlocksAsk = 64;   // touch blocks a carrier launch asks for: the CUs 192 compute blocks leave idle
constexpr int kTouchDelayCrossAttn = 16;   // sleep rounds (~0.2 us each) in front of the cross-attention's touch blocks: its
                                           // compute blocks' first two K / V^T stages leave first (tools/ubench/attn_cold.hip)

// ---- the step plan -------------------------------------------------------------------------------------------------
// Everything one decoder evaluation decides about its launches, computed ONCE by plan_step and handed to in_proj and the
// blocks of decoder_layers: a launch and whoever produces its operands or warms its weights read the same value.
// P passes of `batch` songs: rows [0, BT) are the conditional pass when `cond0`, rows [BT, 2 BT) the unconditional one.
enum WarmTarget { WARM_CROSS_Q = 0, WARM_CROSS_OUT, WARM_MLP_IN };
struct StepPlan {
  int batch, P;
  // The self-attention block of layer 0 ([0]) and of layers >= 1 ([1]).  They differ under S5 (`dup`; a CFG step whose
  // input projection wrote pass 0 only): up to layer 0's first cross-attention both passes hold the same rows (same z,
  // same FiLM, same self-attention: models.py:373-386, network.py:174-193), so layer 0's QKV / self-attention /
  // attention-out run on BT rows and the attention-out epilogue writes every row twice (gemm_h16.h
  // EpiResidualNorm<NP, true>).  Exact: bit-identical to the 2 BT-row form.
  struct SelfBlock {
    int Ms, Ps;                 // rows and passes the block runs on (dup: BT, 1)
    TileShape qkv, out, out2;   // fold only: the tile of the QKV launch (both problems), of attention-out's two problems
    int warms;                  // WarmTarget: the first projection behind the block; the block warms its weights ...
    int touch_blocks;           // ... from this many touch blocks behind the self-attention's compute grid (gemm_h16.h
                                // "Touch blocks"; the launcher keeps the launch within one round of the chip); 0 = from
                                // the in-block prefetch wave
    bool warm_on_out;           // ... from the attention-out launch -- the self-attention runs 128-row blocks, which
                                // have no prefetch wave -- and not from the self-attention
    bool qb4;                   // the self-attention runs 128-row blocks (more than one round of 64-row blocks: from 3
                                // songs per handle when it carries both passes of a CFG step, from 6 on one pass's rows)
    bool dup;
    bool fold;                  // S6: the cross-attention query projection rides on the QKV and attention-out launches
  } self[2];
  const SelfBlock& of(int layer) const { return self[layer > 0]; }
  // cross-attention module e (conditional passes only): its key split; whether that makes more than one round of
  // 64-row blocks.  MLP-in's weights ride on the last module's attention launch -- unless that one runs 16 compute waves
  // per block (128-row blocks at batch: no room for a prefetch wave); its output projection carries them then.
  // (A folded layer's launch stays on 64-row blocks whatever `cross_qb4` says -- attention.h: no 128-row kernel for
  // un-normalised queries -- and its output projection still carries the target: a single pass of 4 songs.)
  int ks[2];
  // Touch-block carriers (one song per call, msd_config.touch_carrier): MLP-in's weights ride on this many touch blocks
  // of the last module's cross-attention launch, behind mlp_in_touch_delay sleep rounds, and that launch's in-block wave
  // keeps only its own K / V^T touch-ahead; 0 = on the in-block wave.
  int mlp_in_touch_blocks, mlp_in_touch_delay;
  bool cross_qb4[2];
  bool cond0, mlp_in_on_cross_out;
};
// (captured graphs are looked up by comparing plans bytewise, GraphCache: no padding bytes -- group its bools in fours)

// Instantiated graphs of a handle under keys that are compared bytewise, at most Cap of them.  The handle keeps two, the
// step graphs and msd_loss's, so that neither evicts the other's entries.  A deque: an entry stays where it is when
// another is inserted, so a caller may hold several entries at once -- as long as it makes room for all it will insert
// BEFORE its first lookup (make_room: a cache without that room is emptied, which destroys every graph in it).
template <class Key, size_t Cap>
struct GraphCache {
  static_assert(std::has_unique_object_representations<Key>::value, "a graph key (StepPlan included) must not have padding bytes");
  struct Entry { Key key; hipGraphExec_t exec = nullptr, exec1 = nullptr; };
  std::deque<Entry> entries;
  Entry* find(const Key& key) {
    for (Entry& e : entries)
      if (memcmp(&e.key, &key, sizeof(Key)) == 0) return &e;
    return nullptr;
  }
  void make_room(size_t n) {   // (a handle that cycles through more shapes than Cap re-captures)
    if (entries.size() + n > Cap) clear();
  }
  Entry* insert(const Entry& e) { entries.push_back(e); return &entries.back(); }
  void clear() {
    for (Entry& e : entries) {
      if (e.exec) (void)hipGraphExecDestroy(e.exec);
      if (e.exec1) (void)hipGraphExecDestroy(e.exec1);
    }
    entries.clear();
  }
};


struct Profiler {
  bool on = false;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double ms[KC_COUNT] = {0};
  int64_t launches[KC_COUNT] = {0};
};

}  // namespace

struct msd_model {
  msd_config cfg;
  mutable std::string err;
  int NP = 1;       // bf16 planes per operand
  int D = 0, J = 0, F = 0, H = 0, T = 0, L = 0, C = 0, ND = 0, N = 0, Ld = 0, Le = 0;
  int Bmax = 1, passes = 2;
  int S_pad = 0;    // padded key capacity of the cross-attention cache
  int Lenc_pad = 0; // padded row capacity of the encoder scratch
  bool finalized = false, encoded = false;
  int encoded_batch = 0;

  std::vector<Weight> weights;
  std::unordered_map<std::string, int> windex;
  std::vector<void*> allocs;

  EncoderW tok_enc, ctx_enc;
  std::vector<DecLayerW> dec;
  const float *dec_final_ln = nullptr, *w_spec_out = nullptr, *w_in_proj = nullptr,
              *dec_pos = nullptr, *w_ctx_in = nullptr, *ctx_pos = nullptr, *tok_emb = nullptr,
              *tok_pos = nullptr;

  // tables
  float* d_coef = nullptr;  // [N][kCoefCount]
  std::vector<float> h_coef;
  float* d_film = nullptr;  // [N][2*Ld][2D]
  // folded-norm tables (gemm_h16.h): g = gamma (.) (film_scale + 1); b.W per step
  float* d_g = nullptr;        // [N][2*Ld][D]
  float* d_bw_self = nullptr;  // [N][Ld][3J]   film_bias_self . (Wq|Wk|Wv)
  float* d_bw_mlp = nullptr;   // [N][Ld][2F]   film_bias_mlp  . (wi_0|wi_1), packed column order

  // decoder activations (rows = passes*Bmax*T)
  float* x = nullptr;
  Planes h, qk, vt, ao, cq, g;
  Planes y;                    // x (.) g of the next norm, written by the residual epilogues
  Planes zp;                   // bf16 planes of z (A operand of the folded input projection)
  float* w_out_g = nullptr;    // diag(decoder_norm scale) . spec_out_dense, fp32 [D][n]
  Planes w_in_p, w_out_p;      // packed W^T of continuous_inputs_projection [D][n] / spec_out_dense [n][D]
  float* ssq = nullptr;        // [rows][D/64] partial sums of squares of x
  float *att_part_o = nullptr, *att_part_ml = nullptr;  // key-split attention partials
  int cross_ksplit = 1;        // key split of the cross-attention at batch 1 (allocation bound)
  float* h32 = nullptr;
  float* eps = nullptr;
  float* z = nullptr;
  const float** d_noise_slot = nullptr;
  uint32_t* d_rng_key = nullptr;       // [Bmax] rows of {seed_lo, seed_hi, stream_lo, stream_hi, generator kind, PRNGKey(seed) words, per-row mode} of the current msd_sample: one row per row of z (elementwise.h SamplerParams::rng_key, kRng*)
  std::vector<uint32_t> h_rng_key;     // host staging of the rows just uploaded
  // The buffers from here to d_loss_times are made by the first call that needs them (`ensure`) or grown by a call that
  // needs more (`grow`, those with a capacity beside them), outside stream capture, and owned by the handle.
  // msd_sample_guided: the guidance weight of every row of z, [Bmax] floats beside the key table (elementwise.h
  // SamplerGuidedParams::row_wt), uploaded per call; the captured guided graphs hold a stable address and serve every
  // weight vector
  float* d_row_wt = nullptr;
  std::vector<float> h_row_wt;         // host staging of that upload
  // msd_sample_keep: the known mel in model units [Bmax][T][n] and its frame flags [Bmax][T]; the captured keep graphs hold
  // stable addresses
  float* keep_xk = nullptr;
  int32_t* keep_flags = nullptr;
  // msd_sample_resample: the key rows of every pass behind a jump, [passes][batch][kRngWords], uploaded once per call (the
  // jump kernel installs its pass's rows in d_rng_key, outside the captured graphs: the buffer may move when it grows)
  uint32_t* d_pass_keys = nullptr;
  size_t pass_keys_cap = 0;            // words
  std::vector<uint32_t> h_pass_keys;   // host staging of that upload
  // msd_sample_steps: the sampler's coefficient rows for a call of K steps (K | N), built on the first such call and kept
  // (host copy + device table; K == N is d_coef itself), and -- MSD_SAMPLER_DPMPP_2M -- the multistep side table of K and
  // the previous step's pred_x0 [Bmax][T][n] (make_step_view builds the tables); msd_invert: the inversion's side table of K
  struct StepTables { std::vector<float> h_coef; float* coef = nullptr; float* coef_ms = nullptr; float* coef_inv = nullptr; };
  std::map<int, StepTables> step_tables;
  float* x0_prev = nullptr;
  // msd_loss: the target in model units [Bmax][T][n], the per-call words of the two loss kernels (elementwise.h LossCall) and
  // the call's time rows [n_times][kLossTimeWords]; the captured loss graphs hold stable addresses.  The time rows are
  // reached THROUGH the call words: they may grow.
  float* loss_x0 = nullptr;
  LossCall* d_loss_call = nullptr;
  LossCall h_loss_call = {};           // host staging of that upload
  float* d_loss_times = nullptr;
  size_t loss_times_cap = 0;           // floats
  std::vector<float> h_loss_times;
  int* d_step = nullptr;       // [2]
  int* d_nkeys_self = nullptr; // [passes*Bmax] = T
  int* d_nkeys_cross = nullptr;// [n_cross][Bmax] valid keys per key region and song
  std::vector<int> h_nkeys_cross;
  int n_cross = 1;             // cross-attention modules per decoder layer (2: sum_cross_attends with context)
  int key_off[2] = {0, 0};     // first key row of each region in the cross cache
  Planes cq2, ao2;             // second module's query / attention output (sum_cross_attends)
  Planes kc, vtc;              // cross cache [Ld][Bmax][S_pad][J] / [Ld][Bmax][J][S_pad]

  // encoder scratch (one sequence at a time)
  float* ex = nullptr;
  Planes eh, eqk, evt, eao, eg, enc;  // enc = concatenated encodings [S_pad, D]
  int *d_tokens = nullptr, *d_pos = nullptr, *d_nkeys_enc = nullptr;
  float *ctx_scaled = nullptr, *ctx_full = nullptr;

  // instantiated step graphs, one set per step plan -- a graph bakes its launches and their grids in.  Invariant: the
  // plan of a CFG step is a function of the handle's constants, the batch and the key counts msd_encode saw (they choose
  // the cross-attention's key splits, cross_split), and the launch sequence of a step is a function of the handle's
  // constants and the plan: equal plans, same graph.
  // `keep`: the graphs of msd_sample_keep launch the sampler's keep form (other kernel, other arguments), so a plain call
  // never replays a keep graph, nor the other way round.
  // `steps`, `sampler`: msd_sample_steps' graphs bake another view of the step-indexed tables and maybe another sampler
  // kernel in; the handle's own (N, cfg.sampler) is the key every other entry point looks up, as it always did.
  // `guided`: msd_sample_guided's two-pass graphs launch the sampler's guided form (the row weights come from d_row_wt);
  // its one-pass steps replay plain graphs of the one-pass plan.  (An int like its neighbours: no padding bytes.)
  // `invert`: msd_invert's graphs launch the inversion kernel, which counts the scan index up.
  // An entry: `exec` runs graph_steps steps, `exec1` one (captured on first need).  find_graphs looks up and captures.
  struct GraphKey { StepPlan plan; int steps, sampler, keep, guided, invert; };   // ONE key, compared bytewise (GraphCache)
  using StepGraphCache = GraphCache<GraphKey, 8>;
  using StepGraphs = StepGraphCache::Entry;
  StepGraphCache graphs;
  // msd_loss's graphs: ONE evaluation (diffuse, decoder pass(es), loss) per plan in `exec` -- the conditional, the
  // unconditional and the two-pass plan differ bytewise -- in a cache of their own, so that they neither evict nor alter a
  // cached set of step graphs; msd_reset_graph empties both.
  using LossGraphCache = GraphCache<StepPlan, 6>;
  LossGraphCache loss_graphs;
  int graph_steps = 8;              // DDPM steps per graph launch (msd_config.graph_steps; 1 -> 4 -> 10: 1.2000 -> 1.1963 -> 1.1955 ms/step)
  bool prefetch = true;        // producers warm the next GEMM's weights (msd_config.weight_prefetch; default: by model size)
  bool dedup_layer0 = true;    // S5 (decoder_layers); msd_config.dedup_layer0 = 2 turns it off for A/B and bitwise tests
  int kv_touch_ahead = 2;      // attention.h kv_touch_ahead: stages the prefetch wave runs in front of the K / V^T ring (0 = off)
  bool merge_in_launch = true; // attention.h attention_inlaunch_merge (msd_config.cross_merge_in_launch = 2 turns it off)
  bool fold_q = true;          // folded cross-attention query projection (msd_config.cross_q_fold = 2 turns it off)
  bool persist_mlp_in = true;  // batched songs: persistent gated-MLP-in tile loop (msd_config.mlp_in_persistent = 2 turns it off)
  int ran_touch_blocks[2] = {0, 0};   // touch blocks of the last self- / cross-attention launch enqueued (msd_debug_read "touch_blocks")
  bool touch_blocks = kTouchCarrierDefault == 2;   // one song per call: weight touches from touch blocks (msd_config.touch_carrier; plan_step)
  Planes xg;                   // [Bmax T, D] x (.) gamma_cross of the layer about to run, conditional rows (EpiResidualNorm Y2)
  float* qp = nullptr;         // [Bmax T, n_cross J] (x0 (.) gamma) . Wq, the half of the projection that rides on the QKV launch
  int* att_tickets = nullptr;  // its arrival counters: [Bmax][T / 32][H], zero between launches
  int att_ticket_count = 0;
  int cus = 0;                 // compute units of the device
  float* d_absmax = nullptr;   // largest |w| over the packed weights (bits, pack_wt_kernel): half-plane range check
  // Query side of the DECODER's self- and cross-attention (attention.h QP bits: 1 = Q enters q.k^T as one plane,
  // 2 = the softmax weights enter P.V as one plane); from msd_config.attn_q_planes / attn_p_planes, DESIGN.md 3
  int att_qp_self = 0, att_qp_cross = 0;
  unsigned* d_sat = nullptr;   // half-plane range flag: kernel class + 1 of a conversion that saw |x| > 65504 (common.h RangeCheck)
  unsigned* h_sat = nullptr;   // pinned host copy, read after the stream sync that ends msd_encode / msd_sample
  hipStream_t own_stream = nullptr;  // used when the caller passes the (uncapturable) NULL stream
  Profiler prof;
};

namespace {

int fail(const msd_model* m, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (m) m->err = buf;
  return code;
}

#define HIP_TRY(m, expr)                                                              \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess)                                                             \
      return fail(m, MSD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                  "msd_api.hip", __LINE__); /* not __FILE__: no checkout path in the binary */ \
  } while (0)

// Synchronous copies and fills of a handle go through the handle's own NON-BLOCKING stream, never through the legacy
// (NULL) stream: a legacy-stream operation synchronises with every blocking stream of the device and FAILS while another
// thread captures a graph on one ("operation would make the legacy stream depend on a capturing blocking stream") --
// a second handle that loads its weights, or encodes, while the first one captures its step graph (round 5: found by
// tools/ab/multi_handle.py).  Handles on one device may now be created, loaded and run from different threads.
hipError_t copy_sync(const msd_model* m, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (!m || !m->own_stream) return hipMemcpy(dst, src, bytes, kind);
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, m->own_stream);
  return e != hipSuccess ? e : hipStreamSynchronize(m->own_stream);
}
hipError_t fill_sync(const msd_model* m, void* dst, int value, size_t bytes) {
  if (!m || !m->own_stream) return hipMemset(dst, value, bytes);
  const hipError_t e = hipMemsetAsync(dst, value, bytes, m->own_stream);
  return e != hipSuccess ? e : hipStreamSynchronize(m->own_stream);
}

template <class Tp>
int dalloc(msd_model* m, Tp** out, size_t count, bool zero = true) {
  void* p = nullptr;
  size_t bytes = count * sizeof(Tp);
  if (bytes == 0) bytes = 16;
  HIP_TRY(m, hipMalloc(&p, bytes));
  if (zero) HIP_TRY(m, fill_sync(m, p, 0, bytes));
  m->allocs.push_back(p);
  *out = static_cast<Tp*>(p);
  return MSD_OK;
}

int palloc(msd_model* m, Planes* pl, size_t count) {
  for (int i = 0; i < m->NP; ++i) {
    int rc = dalloc(m, &pl->p[i], count);
    if (rc) return rc;
  }
  return MSD_OK;
}

// The handle's lazily made device buffers, both outside stream capture.  ensure: allocated (zeroed) by the first call
// that needs it, each buffer on its own -- a call after a failed allocation tries again for the one that is missing.
template <class Tp>
int ensure(msd_model* m, Tp** p, size_t count) { return *p ? MSD_OK : dalloc(m, p, count); }
// grow: a buffer of *cap elements that a call needing more frees and allocates anew (the stream is idle then: every call
// that uses one ends with its synchronisation); no captured graph holds such a buffer's address
template <class Tp>
int grow(msd_model* m, Tp** p, size_t* cap, size_t count) {
  if (count <= *cap) return MSD_OK;
  if (*p) {
    auto it = std::find(m->allocs.begin(), m->allocs.end(), static_cast<void*>(*p));
    if (it != m->allocs.end()) m->allocs.erase(it);
    (void)hipFree(*p);
    *p = nullptr; *cap = 0;
  }
  if (int rc = dalloc(m, p, count)) return rc;
  *cap = count;
  return MSD_OK;
}

inline int round_up(int v, int q) { return (v + q - 1) / q * q; }

// Half-plane range flag (common.h RangeCheck): read it behind a stream sync; a set flag fails the call LOUDLY
// (round 2 clamped at 65504 and returned MSD_OK with a wrong spectrogram).  The flag is cleared for the next call.
// arm: every call that ends with check_range() starts with a clean flag (a flag raised on an error path of an earlier
// call, which returned before its own check, must not be blamed on this one)
int arm_range(msd_model* m, hipStream_t s) {
  if (kPlaneSaturates) HIP_TRY(m, hipMemsetAsync(m->d_sat, 0, sizeof(unsigned), s));
  return MSD_OK;
}
int check_range(msd_model* m, hipStream_t s, const char* what) {
  if (!kPlaneSaturates) {
    HIP_TRY(m, hipStreamSynchronize(s));
    return MSD_OK;
  }
  HIP_TRY(m, hipMemcpyAsync(m->h_sat, m->d_sat, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  HIP_TRY(m, hipStreamSynchronize(s));
  const unsigned tag = *m->h_sat;
  if (tag == 0) return MSD_OK;
  HIP_TRY(m, hipMemsetAsync(m->d_sat, 0, sizeof(unsigned), s));
  HIP_TRY(m, hipStreamSynchronize(s));
  const char* cls = (tag >= 1 && tag <= (unsigned)KC_COUNT) ? kClassNames[tag - 1] : "?";
  return fail(m, MSD_ERR_RANGE,
              "%s: an activation left the range of the IEEE-half operand planes (|x| > %g) in kernel class '%s'; the "
              "result of this call is INVALID.  Use precision 'bf16x3' (libmsd_amd_bf16.so: bfloat16 planes keep "
              "float32's exponent range at twice the rounding error)", what, (double)kPlaneMax, cls);
}

void add_weight(msd_model* m, const std::string& name, int64_t a, int64_t b = -1) {
  Weight w;
  w.name = name;
  w.shape[0] = a;
  w.shape[1] = b < 0 ? 0 : b;
  w.ndim = b < 0 ? 1 : 2;
  m->windex[name] = (int)m->weights.size();
  m->weights.push_back(w);
}

void declare_weights(msd_model* m) {
  const int D = m->D, J = m->J, F = m->F;
  auto attention = [&](const std::string& p) {
    add_weight(m, p + "/query/kernel", D, J);
    add_weight(m, p + "/key/kernel", D, J);
    add_weight(m, p + "/value/kernel", D, J);
    add_weight(m, p + "/out/kernel", J, D);
  };
  auto mlp = [&](const std::string& p) {
    add_weight(m, p + "/wi_0/kernel", D, F);
    add_weight(m, p + "/wi_1/kernel", D, F);
    add_weight(m, p + "/wo/kernel", F, D);
  };
  auto encoder_layers = [&](const std::string& p) {
    for (int l = 0; l < m->Le; ++l) {
      const std::string lp = p + "/layers_" + std::to_string(l);
      add_weight(m, lp + "/pre_attention_layer_norm/scale", D);
      attention(lp + "/attention");
      add_weight(m, lp + "/pre_mlp_layer_norm/scale", D);
      mlp(lp + "/mlp");
    }
    add_weight(m, p + "/encoder_norm/scale", D);
  };
  const std::string tok = m->cfg.has_context ? "token_encoder" : "encoder";
  add_weight(m, tok + "/token_embedder/embedding", m->cfg.vocab_size, D);
  add_weight(m, tok + "/Embed_0/embedding", m->L, D);
  encoder_layers(tok);
  if (m->cfg.has_context) {
    add_weight(m, "continuous_encoder/input_proj/kernel", m->ND, D);
    add_weight(m, "continuous_encoder/Embed_0/embedding", m->C, D);
    encoder_layers("continuous_encoder");
  }
  add_weight(m, "decoder/time_emb_dense0/kernel", D, 4 * D);
  add_weight(m, "decoder/time_emb_dense1/kernel", 4 * D, 4 * D);
  add_weight(m, "decoder/Embed_0/embedding", m->T, D);
  add_weight(m, "decoder/continuous_inputs_projection/kernel", m->ND, D);
  for (int l = 0; l < m->Ld; ++l) {
    const std::string lp = "decoder/layers_" + std::to_string(l);
    add_weight(m, lp + "/pre_self_attention_layer_norm/scale", D);
    add_weight(m, lp + "/FiLMLayer_0/DenseGeneral_0/kernel", 4 * D, 2 * D);
    attention(lp + "/self_attention");
    add_weight(m, lp + "/pre_cross_attention_layer_norm/scale", D);
    for (int e = 0; e < m->n_cross; ++e) attention(lp + "/MultiHeadDotProductAttention_" + std::to_string(e));
    add_weight(m, lp + "/pre_mlp_layer_norm/scale", D);
    add_weight(m, lp + "/FiLMLayer_1/DenseGeneral_0/kernel", 4 * D, 2 * D);
    mlp(lp + "/mlp");
  }
  add_weight(m, "decoder/decoder_norm/scale", D);
  add_weight(m, "decoder/spec_out_dense/kernel", D, m->ND);
}

const float* W(msd_model* m, const std::string& name) { return m->weights[m->windex.at(name)].dev; }

// ---- launch helpers ---------------------------------------------------------
// A sampling call's view of the handle's step-indexed tables (msd_sample_steps).  The scan index in device memory counts
// the CALL's steps, j = K - 1 .. 0; step j of a K-step call has the time of row (j + 1) N / K - 1 of the handle's N-step
// tables ((j + 1) / K and (r + 1) / N are the same rational, correctly rounded: the same float32), so every reader of a
// step-indexed table gets base + off rows and mul times the row stride, and no table or GEMM changes.  The sampler's own
// coefficients also hold s = j / K, which is no row of the N-step table: a K-row table of their own.
// make_step_view fills EVERY field for every sampling call, the handle's own (N, cfg.sampler) included; the default below is
// what a Ctx outside a sampling call reads its tables through (off, mul: the handle's rows) -- no step is enqueued on it.
struct StepView {
  int steps = 0;                    // K
  int off = 0, mul = 1;             // N / K - 1, N / K
  const float* coef = nullptr;      // [K][kCoefCount]
  const float* coef_ms = nullptr;   // [K][kMsCount], MSD_SAMPLER_DPMPP_2M only
  int sampler = 0;                  // msd_sampler_kind
  bool keep = false;                // the sampler's keep form on the handle's known-frame buffers (msd_sample_keep / _edit)
  bool guided = false;              // the sampler's guided form on the handle's row-weight table (msd_sample_guided)
  bool invert = false;              // the inversion form: the scan index counts up (msd_invert; kernel: invert_tail.h)
  const float* coef_inv = nullptr;  // [K][kInvCount], the inversion form only
};

struct Ctx {
  msd_model* m;
  hipStream_t s;
  hipError_t err = hipSuccess;
  StepView v = StepView();
  void begin(int kc) {
    if (m->prof.on) (void)hipEventRecord(m->prof.e0, s);
    (void)kc;
  }
  void latch(hipError_t e) { if (err == hipSuccess) err = e; }   // the first error of the chain is the one reported
  void end(int kc) {
    latch(hipGetLastError());
    if (m->prof.on) {
      (void)hipEventRecord(m->prof.e1, s);
      (void)hipEventSynchronize(m->prof.e1);
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, m->prof.e0, m->prof.e1);
      m->prof.ms[kc] += ms;
      m->prof.launches[kc] += 1;
    }
  }
};

template <int NP>
GemmParams gp(const Planes& a, int lda, const Planes& b, int ldb, int M, int N, int K) {
  GemmParams p;
  for (int i = 0; i < 2; ++i) {
    p.A[i] = a.p[i < NP ? i : 0];
    p.B[i] = b.p[i < NP ? i : 0];
  }
  p.lda = lda; p.ldb = ldb; p.M = M; p.N = N; p.K = K;
  return p;
}

// Kernel selection (gemm_h16.h).  The LDS-DMA variant everywhere; tile shapes from
// tools/ubench/gemm_bench.hip run with COLD weights (48 rotating copies), which is what a DDPM
// step sees: every weight matrix is touched once per ~1.4 ms and comes from HBM, so the ring
// depth has to cover HBM latency, not L2 latency.  bf16x3, M = 512, us warm -> cold:
//   QKV     N=2304 K=768 : 64x64 NS2 14.0 -> 16.6 | 64x96  NS3 (192 blocks, 1/CU) 11.2 -> 12.7
//   MLP in  N=4096 K=768 : 64x64 NS2 14.4 -> 17.3 | 64x128 NS3 (256 blocks, 1/CU)      -> 16.2
//   MLP out N=768 K=2048 : 32x32 NS4      -> 17.6 | 64x32  NS4 (192 blocks)             -> 15.4
//   N = D, K = D (attention out, cross q/out): 32x32 NS4 (384 blocks, two per CU) 5.2 .. 6.8
// At 64 x 64 the N = D projections have 96 blocks and are bound by the per-CU ingest rate
// (~31 B/clk with one block per CU), hence the small tiles there.
constexpr int kNarrowTile = 32;  // BN of every GEMM that feeds the folded-norm ssq partials
constexpr int kTallNS = 4;       // ring depth of the 64 x 32 tiles (6 measured equal in situ: 1.200 vs 1.198 ms)
constexpr int kWideNS = 3;       // 64 x 64 wide tiles: 3-deep ring (cold weights: deeper is better)
enum TileKind { TK_NARROW = 0, TK_TALL = 1, TK_QKV = 2, TK_MLP_IN = 3, TK_SQUARE = 4 };

// XCD grid (gemm_h16.h): 2 row groups x 4 column groups.  Same-box A/B over the whole step
// (tools/env_ab.sh): 1 x 8 -> 1.196 ms, 2 x 4 -> 1.167 ms, 4 x 2 -> 1.187 ms; choosing per launch by
// the bytes each L2 has to fetch (A / rx + B * rx / 8) picked 1 x 8 for the wide GEMMs and was no
// better than 1 x 8 everywhere.
void set_xcd_grid(GemmParams& p, int M, int BM) {
  p.xcd_rows = (M / BM) % 2 == 0 ? 2 : 1;
  p.xcd_walk_n = 1;
}

// launch parameters of one GEMM problem on tiles of BM rows: operands, the weight prefetch it carries, range flag, XCD grid
template <int NP>
GemmParams gp_launch(Ctx& c, int kc, const Planes& a, int lda, const Planes& b, int ldb, int M, int N, int K, int BM,
                     const WeightPrefetch& pf = WeightPrefetch()) {
  GemmParams p = gp<NP>(a, lda, b, ldb, M, N, K);
  p.pf = pf;
  p.sat = c.m->d_sat; p.sat_tag = (unsigned)kc + 1u;
  set_xcd_grid(p, M, BM);
  return p;
}

// rounds of blocks over the 256 CUs x rows of operand per K-tile: the GEMMs sit on the per-CU ingest
// path, so a launch costs about that; used to pick between tile shapes for a given (M, N)
inline long tile_cost(int M, int N, int BM, int BN) {
  const long blocks = (long)(M / BM) * (N / BN);
  return ((blocks + 255) / 256) * (BM + BN);
}

// `align` = the largest column granularity the epilogue tolerates besides N itself (QKV: the
// V^T region must start on a tile boundary).
// Batched songs (M = passes * B * T >= big_m_threshold() = 2048): every CU has several tiles anyway, so the tiles
// grow to 128 x 96/128 (2-deep ring, 128 KiB) -- half the L2->LDS re-reads per MAC
// (tools/ubench/gemm_bench_big.hip, M = 4096: QKV 85 -> 61 us, MLP-in 114 -> 95, MLP-out 68 -> 48).
constexpr int big_m_threshold() { return 2048; }   // rows from which the 128-row tiles are used

// epilogues that run on 32 x 48 tiles (gemm_h16.h EpiResidualNorm::run48)
template <class Epi> struct epi_takes_48 : std::false_type {};
template <> struct epi_takes_48<EpiResidualNorm<2>> : std::true_type {};
template <> struct epi_takes_48<EpiResidualNorm<2, false, true>> : std::true_type {};

// The tile a GEMM of kind TK runs on, (BM, BN): ONE rule for the launch below and for whoever prefetches that
// launch's weights (the prefetcher needs the consumer's column tile and XCD grid).
constexpr int kWide48 = 48;
template <int NP, int TK>
TileShape pick_tile(int M, int N, int align, bool wide48 = false, int K = 0) {
  const bool big = NP == 2 && M >= big_m_threshold() && M % 128 == 0;
  if (TK == TK_QKV) {
    if (NP == 2) {
      if (big && N % 96 == 0 && align % 96 == 0) return {128, 96};
      // 64 x 96 = one block per CU at base (192 blocks); at the small model (N = 1152: 96 blocks)
      // 64 x 64 fills the chip better
      if (N % 96 == 0 && align % 96 == 0 && tile_cost(M, N, 64, 96) <= tile_cost(M, N, 64, 64)) return {64, 96};
    }
    return {64, 64};
  }
  if (TK == TK_MLP_IN) {
    if (NP == 2) {
      if (big && N % 128 == 0) return {128, 128};
      if (N % 128 == 0 && tile_cost(M, N, 64, 128) <= tile_cost(M, N, 64, 64)) return {64, 128};
    }
    return {64, 64};
  }
  if (NP == 2 && (TK == TK_TALL || TK == TK_SQUARE) && big && N % 96 == 0) {   // N = D projections of a decoder layer
    // ... on 64 x 96 where 128 x 96 would leave CUs without a tile: the cross-attention's query / output projections run
    // on the conditional rows only -- M = 2048 at 8 songs is 128 tiles of 128 x 96 on 256 CUs (round 5)
    if (M % 64 == 0 && tile_cost(M, N, 64, 96) < tile_cost(M, N, 128, 96)) return {64, 96};
    return {128, 96};
  }
  // 32 x 48 (round 4; residual + folded-norm epilogue only): 512 x 768 outputs are 256 such tiles -- one per CU with
  // 80 operand rows per K-tile, where 32 x 32 is 384 blocks (two on half the CUs: 128 rows) and 64 x 32 is 192 (96
  // rows on three quarters of the chip)
  long best = tile_cost(M, N, kNarrowTile, kNarrowTile);
  TileShape t = {kNarrowTile, kNarrowTile};
  if (TK == TK_TALL && M % 64 == 0 && tile_cost(M, N, 64, kNarrowTile) <= best) { best = tile_cost(M, N, 64, kNarrowTile); t = {64, kNarrowTile}; }
  // ... for long K only: the tile's head and tail are heavier than the 64 x 32 tile's (256 blocks' worth of aux rows,
  // 8 lanes per row in the epilogue), its K-tile is lighter (20 KiB against 24); measured per launch at K = 768: 7.05 us
  // against 6.65 on 64 x 32, at K = 2048: 12.45 against 12.97 (profiles/r04i_*, r04j_*)
  if (NP == 2 && wide48 && K >= 1536 && N % kWide48 == 0 && tile_cost(M, N, kNarrowTile, kWide48) < best) t = {kNarrowTile, kWide48};
  return t;
}

// ---- the tile table ---------------------------------------------------------------------------------------------
// The ONLY place that names a GEMM tile (BM x BN, ring depth NS).  Dispatch (gemm, gemm_dual) walks a list in order and
// takes the entry of the shape pick_tile chose, the LAST entry otherwise; prepare_gemms opts every entry of every launch
// site into its dynamic LDS.  A new tile is one line here (and a pick_tile rule that returns its shape).  (List: common.h)
template <int BM_, int BN_, int NS_> struct Tile {
  static constexpr int BM = BM_, BN = BN_, NS = NS_;
  static bool is(TileShape t) { return t.bm == BM_ && t.bn == BN_; }
};
// Batched songs: 128-row tiles, 2-deep ring of K = 64 tiles.  A 4-deep ring of K = 32 tiles (64-byte rows, its own
// swizzle and a plain one-barrier-per-tile loop: tools/ubench/gemm_h16_k32.h) was built in round 3, is parity-green on
// the batched test and measured 10 % SLOWER end to end at 8 and 16 songs (profiles/r03m_k32_ab.log: 465 vs 516 and
// 498 vs 550 mel-frames/s; gated MLP input 1.34 vs 1.13 ms per step): twice the barriers per K and one wave per SIMD
// at 340 registers cost more than the deeper ring hides.  Not in the product build.
using BigTile = Tile<128, 96, 2>;
using BigMlpInTile = Tile<128, 128, 2>;   // EpiGeglu<2> has a persistent form on it (gemm_t)
using Wide96Tile = Tile<64, 96, 3>;
using Wide128Tile = Tile<64, 128, 3>;
using WideTile = Tile<64, 64, kWideNS>;
using TallTile = Tile<64, kNarrowTile, kTallNS>;
using Narrow96Tile = Tile<kNarrowTile, 96, 4>;   // second problem of the folded attention-out launch only
using Narrow48Tile = Tile<kNarrowTile, kWide48, 4>;
using NarrowTile = Tile<kNarrowTile, kNarrowTile, 4>;

template <class Epi> struct epi_is_y2 : std::false_type {};   // EpiResidualNorm Y2: folded layers only, never on the batched path's tiles
template <int NP> struct epi_is_y2<EpiResidualNorm<NP, false, true>> : std::true_type {};

template <int NP, int TK, class Epi>
constexpr auto tile_table() {
  if constexpr (TK == TK_QKV) {
    return list_if<NP == 2, List<BigTile, Wide96Tile>>{} + List<WideTile>{};
  } else if constexpr (TK == TK_MLP_IN) {
    return list_if<NP == 2, List<BigMlpInTile, Wide128Tile>>{} + List<WideTile>{};
  } else {
    return list_if<NP == 2 && (TK == TK_TALL || TK == TK_SQUARE) && !epi_is_y2<Epi>::value, List<BigTile, Wide96Tile>>{} +
           list_if<TK == TK_TALL, List<TallTile>>{} +
           list_if<NP == 2 && epi_takes_48<Epi>::value, List<Narrow48Tile>>{} + List<NarrowTile>{};
  }
}
template <int NP, int TK, class Epi> using TileTable = decltype(tile_table<NP, TK, Epi>());

// Dual launches of the folded cross-attention query projection (decoder_layers; two-plane modes): (problem 1's tile,
// problem 2's tile) pairs.  QKV: the same tile for both problems; attention-out: each problem its own.
template <class T1, class T2> struct TilePair { using P1 = T1; using P2 = T2; };
template <class T1, class... T2> constexpr List<TilePair<T1, T2>...> pairs_of(List<T2...>) { return {}; }
template <class... T1, class L2> constexpr auto cross(List<T1...>, L2) { return (pairs_of<T1>(L2{}) + ...); }
using FoldQkvTiles = List<TilePair<Wide96Tile, Wide96Tile>, TilePair<WideTile, WideTile>>;
using FoldOutTiles = decltype(cross(List<TallTile, NarrowTile>{}, List<Narrow96Tile, NarrowTile>{}));

// Launch sites: every (tile kind, epilogue) gemm<NP> is called with and every (pairs, epilogues) gemm_dual is.  A site
// that is missing here does not compile; one that is here has all its tiles prepared outside stream capture.
template <int TK, class Epi> struct Site {};
template <class Pairs, class Epi1, class Epi2> struct DualSite {};
template <int NP> using GemmSites = decltype(
    List<Site<TK_QKV, EpiQKV<NP>>, Site<TK_MLP_IN, EpiGeglu<NP>>, Site<TK_SQUARE, EpiResidual>, Site<TK_TALL, EpiResidual>,
         Site<TK_TALL, EpiResidualNorm<NP>>, Site<TK_TALL, EpiResidualNorm<NP, true>>, Site<TK_SQUARE, EpiResidualNorm<NP>>,
         Site<TK_SQUARE, EpiStoreH16<NP>>, Site<TK_NARROW, EpiStoreF32>, Site<TK_NARROW, EpiInProj<NP>>>{} +
    list_if<NP == 2, List<Site<TK_TALL, EpiResidualNorm<NP, false, true>>>>{});
using DualSites = List<DualSite<FoldQkvTiles, EpiQKV<2>, EpiStoreF32>,
                       DualSite<FoldOutTiles, EpiResidualNorm<2>, EpiAddStoreH16<2>>,
                       DualSite<FoldOutTiles, EpiResidualNorm<2, true>, EpiAddStoreH16<2>>>;

// EpiGeglu<2> on the batched path's tile, decoder MLP blocks: the persistent tile loop with the register epilogue
// (gemm_h16.h) -- one resident block per CU walks its 4 .. 8 tiles, the next tile's ring stages land under the current
// epilogue
template <int NP, class T, class Epi>
constexpr bool kHasPersistentForm = NP == 2 && std::is_same<T, BigMlpInTile>::value && std::is_same<Epi, EpiGeglu<2>>::value;

// does gemm_t run tile T's persistent form for this launch?  (host only; msd_op_gemm_site reports it from here too)
template <int NP, class T, class Epi>
bool runs_persistent(const msd_model* m, const GemmParams& p, const Epi& epi) {
  if constexpr (kHasPersistentForm<NP, T, Epi>) return m->persist_mlp_in && epi.rsc.ssq && epi.rsc.bias && p.K >= 2 * kGemmBK;
  else return false;
}

template <int NP, class T, class Epi>
void gemm_t(Ctx& c, int kc, const GemmParams& p, const Epi& epi) {
  c.begin(kc);
  if constexpr (kHasPersistentForm<NP, T, Epi>) {
    if (runs_persistent<NP, T, Epi>(c.m, p, epi)) {
      c.latch(launch_gemm_h16_geglu_persist<NP, T::BM, T::BN, T::NS>(p, epi, (c.m->cus > 0 ? c.m->cus : 256) / 8 * 8, c.s));
      return c.end(kc);
    }
  }
  c.latch(launch_gemm_h16_dma<NP, T::BM, T::BN, T::NS, Epi>(p, epi, c.s));
  c.end(kc);
}

// One-time opt-in to > 64 KiB dynamic LDS of everything gemm_t / gemm_dual may launch: every tile of every launch site.
// Called OUTSIDE stream capture (set_func_attrs).
template <int NP, class T, class Epi>
hipError_t prepare_tile() {
  if constexpr (kHasPersistentForm<NP, T, Epi>)
    return first_error(gemm_h16_dma_prepare<NP, T::BM, T::BN, T::NS, Epi>(), gemm_h16_geglu_persist_prepare<NP, T::BM, T::BN, T::NS>());
  else return gemm_h16_dma_prepare<NP, T::BM, T::BN, T::NS, Epi>();
}
template <int NP, class Epi, class... T> hipError_t prepare_tiles(List<T...>) { return first_error(prepare_tile<NP, T, Epi>()...); }
template <class Epi1, class Epi2, class... P>
hipError_t prepare_pairs(List<P...>) {
  return first_error(gemm_h16_dual_prepare<2, P::P1::BM, P::P1::BN, P::P1::NS, Epi1, P::P2::BM, P::P2::BN, P::P2::NS, Epi2>()...);
}
template <int NP, int... TK, class... Epi>
hipError_t prepare_sites(List<Site<TK, Epi>...>) { return first_error(prepare_tiles<NP, Epi>(TileTable<NP, TK, Epi>{})...); }
template <class... Pairs, class... Epi1, class... Epi2>
hipError_t prepare_sites(List<DualSite<Pairs, Epi1, Epi2>...>) { return first_error(prepare_pairs<Epi1, Epi2>(Pairs{})...); }
template <int NP>
hipError_t prepare_gemms() {
  if constexpr (NP == 2) return first_error(prepare_sites<NP>(GemmSites<NP>{}), prepare_sites(DualSites{}));
  else return prepare_sites<NP>(GemmSites<NP>{});
}

// opt in to > 64 KiB dynamic LDS once, outside any stream capture (msd_create).  Defined AHEAD of every other function that
// names a GEMM or attention kernel: the compiler emits kernels in the order they are first named, and the code of
// gemm_h16_dma_kernel<2, 128, 96, 2, EpiQKV<2>> was seen to differ (equivalent address arithmetic) with its place in the module
void set_func_attrs() {
  (void)attention_prepare<1>(AttnInstances<1>{});
  (void)attention_prepare<2>(AttnInstances<2>{});
  (void)prepare_gemms<1>();
  (void)prepare_gemms<2>();
}

// launches p on the list's tile of shape t; the last entry is the fall-back
template <int NP, class Epi, class T0, class... T>
void gemm_on(List<T0, T...>, TileShape t, Ctx& c, int kc, const GemmParams& p, const Epi& epi) {
  if constexpr (sizeof...(T) > 0) {
    if (!T0::is(t)) return gemm_on<NP>(List<T...>{}, t, c, kc, p, epi);
  }
  gemm_t<NP, T0, Epi>(c, kc, p, epi);
}

template <int NP, int TK, class Epi>
void gemm(Ctx& c, int kc, const Planes& a, int lda, const Planes& b, int ldb, int M, int N, int K,
          const Epi& epi, int align = 0, const WeightPrefetch& pf = WeightPrefetch()) {
  static_assert(in_list<Site<TK, Epi>>(GemmSites<NP>{}), "a new launch site: add it to GemmSites, or its kernels are never prepared");
  const TileShape t = pick_tile<NP, TK>(M, N, align, epi_takes_48<Epi>::value, K);
  gemm_on<NP>(TileTable<NP, TK, Epi>{}, t, c, kc, gp_launch<NP>(c, kc, a, lda, b, ldb, M, N, K, t.bm, pf), epi);
}

// Two GEMMs in one launch (gemm_h16.h gemm_h16_dual_kernel), problem i on the tile of shape ti; p1 carries the prefetch
template <class Epi1, class Epi2, class P0, class... P>
void gemm_dual_on(List<P0, P...>, TileShape t1, TileShape t2, Ctx& c, int kc, const GemmParams& p1, const Epi1& e1,
                  const GemmParams& p2, const Epi2& e2) {
  using T1 = typename P0::P1; using T2 = typename P0::P2;
  if constexpr (sizeof...(P) > 0) {
    if (!T1::is(t1) || !T2::is(t2)) return gemm_dual_on(List<P...>{}, t1, t2, c, kc, p1, e1, p2, e2);
  }
  c.begin(kc);
  c.latch(launch_gemm_h16_dual<2, T1::BM, T1::BN, T1::NS, Epi1, T2::BM, T2::BN, T2::NS, Epi2>(p1, e1, p2, e2, c.s));
  c.end(kc);
}
template <class Pairs, class Epi1, class Epi2>
void gemm_dual(Ctx& c, int kc, TileShape t1, const GemmParams& p1, const Epi1& e1, TileShape t2, const GemmParams& p2, const Epi2& e2) {
  static_assert(in_list<DualSite<Pairs, Epi1, Epi2>>(DualSites{}), "a new dual launch site: add it to DualSites");
  gemm_dual_on(Pairs{}, t1, t2, c, kc, p1, e1, p2, e2);
}

// Prefetch target = the packed W^T planes [N, K] of a later GEMM (gemm_h16.h PrefetchTarget)
template <int NP>
WeightPrefetch prefetch_of(const msd_model* m, const Planes& w, int N, int K) {
  WeightPrefetch pf;
  if (m->prefetch && NP == 2) pf.t.set(w.p[0], w.p[1], N, K * 2, K * 2);
  return pf;
}

// the same target on `n` touch blocks behind its carrier's compute grid (gemm_h16.h "Touch blocks"); n = 0: the in-block wave
inline WeightPrefetch on_touch_blocks(WeightPrefetch pf, int n, int delay = 0) {
  pf.touch_blocks = n; pf.touch_delay = delay;
  return pf;
}

// ---- operands and epilogues: one builder each ---------------------------------------------------------------------
// Two single-plane conventions, kept apart: OPERAND planes at an element offset keep p[1] == nullptr when NP == 1
// (planes_at); the OUTPUT pair of an epilogue aliases plane 0 then (out_pair).
template <int NP>
Planes planes_at(const Planes& base, size_t off) { return {{base.p[0] + off, NP == 2 ? base.p[1] + off : nullptr}}; }
template <int NP>
void out_pair(h16_t* (&dst)[2], const Planes& pl) { dst[0] = pl.p[0]; dst[1] = pl.p[NP - 1]; }

// rstd of the folded norm from the `tiles` partial sums of squares per row (+ the step-indexed bias.W row)
RowScale row_scale(const float* ssq, int tiles, const int* step_ptr, const float* bias = nullptr, int bias_step_stride = 0) {
  RowScale r;
  r.ssq = ssq; r.tiles = tiles; r.inv_d = 1.0f / (float)(tiles * kNarrowTile); r.bias = bias; r.bias_step_stride = bias_step_stride;
  r.step_ptr = step_ptr;
  return r;
}
// fused q|k|v (or k|v) projection: columns [0, ld_qk) row-major into `qk`, the rest as V^T [seg][vt_rows][seg_len] into `vt`
template <int NP>
EpiQKV<NP> epi_qkv(const Planes& qk, const Planes& vt, int ld_qk, int seg_len, int vt_rows, const RowScale& rsc = RowScale()) {
  EpiQKV<NP> e;
  out_pair<NP>(e.qk, qk); out_pair<NP>(e.vt, vt);
  e.ld_qk = ld_qk; e.v_start = ld_qk; e.seg_len = seg_len; e.vt_ld = seg_len; e.vt_rows = vt_rows; e.rsc = rsc;
  return e;
}
// the epilogues that store C as planes [M, ldc]: Epi = EpiStoreH16, EpiGeglu (ldc = F) ... or as float32
template <template <int> class Epi, int NP>
Epi<NP> epi_out(const Planes& out, int ldc, const RowScale& rsc = RowScale()) {
  Epi<NP> e;
  out_pair<NP>(e.out, out); e.ldc = ldc; e.rsc = rsc;
  return e;
}
EpiStoreF32 epi_store_f32(float* out, int ldc, const RowScale& rsc = RowScale()) { return {out, ldc, rsc}; }
// x += acc, partial sums of squares into `ssq`, y = x (.) g: `lo` for rows < split_row, `hi` from there.  A gain is a
// table base + its stride between steps (0: not step-indexed); a null base writes no y for its rows.
struct Gain { const float* g = nullptr; int step_stride = 0; };
template <int NP>
EpiResidualNorm<NP> epi_residual_norm(float* x, int D, const Planes& y, float* ssq, const int* step_ptr, Gain lo, Gain hi,
                                      int split_row) {
  EpiResidualNorm<NP> e;
  e.x = x; e.ldx = D; out_pair<NP>(e.y, y); e.ssq = ssq; e.tiles = D / kNarrowTile; e.step_ptr = step_ptr;
  e.g_lo = lo.g; e.g_lo_stride = lo.step_stride; e.g_hi = hi.g; e.g_hi_stride = hi.step_stride; e.split_row = split_row;
  return e;
}
// ... and its DUP / Y2 forms (gemm_h16.h): the same arguments; the caller sets dup_rows or y2 / g2 / y2_rows
template <bool DUP, bool Y2, int NP>
EpiResidualNorm<NP, DUP, Y2> residual_form(const EpiResidualNorm<NP>& e) {
  EpiResidualNorm<NP, DUP, Y2> o;
  static_cast<ResidualNormArgs&>(o) = e;
  return o;
}

// fp32 -> operand planes / back (a single-plane operand has p[1] == nullptr)
void split(const float* in, const Planes& out, int64_t n, hipStream_t s, unsigned* sat = nullptr, unsigned sat_tag = 1u) {
  hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out.p[0], out.p[1], n, sat, sat_tag);
}
void merge(const Planes& pl, float* out, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(merge_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                     (const h16_t*)pl.p[0], (const h16_t*)pl.p[1], out, n);
}

template <int NP>
void norm(Ctx& c, const float* x, const float* gamma, int rows, int D, const float* film,
          int slots, int slot, const Planes* out, float* out_f32) {
  NormParams p;
  p.x = x; p.gamma = gamma; p.film = film; p.step_ptr = c.m->d_step;
  p.film_slots = slots; p.film_slot = slot; p.rows = rows; p.D = D;
  p.out[0] = out ? out->p[0] : nullptr;
  p.out[1] = out ? out->p[NP - 1] : nullptr;
  p.out_f32 = out_f32;
  p.sat = c.m->d_sat; p.sat_tag = (unsigned)KC_NORM + 1u;
  const dim3 grid((rows + 3) / 4), block(256);
  c.begin(KC_NORM);
  const int vpl = (D + 255) / 256;
#define NORM_LAUNCH(OUT, VPL) hipLaunchKernelGGL((rmsnorm_film_kernel<OUT, VPL>), grid, block, 0, c.s, p)
  if (NP == 2) {
    if (vpl <= 1) NORM_LAUNCH(1, 1); else if (vpl <= 2) NORM_LAUNCH(1, 2); else if (vpl <= 3) NORM_LAUNCH(1, 3); else NORM_LAUNCH(1, 4);
  } else {
    if (vpl <= 1) NORM_LAUNCH(0, 1); else if (vpl <= 2) NORM_LAUNCH(0, 2); else if (vpl <= 3) NORM_LAUNCH(0, 3); else NORM_LAUNCH(0, 4);
  }
#undef NORM_LAUNCH
  c.end(KC_NORM);
}

// The memory side of an attention launch: K rows and V^T of every segment, and the segments' valid key counts
struct AttnKV {
  Planes k; int ldk; size_t k_seg_stride; int k_rows;
  Planes vt; int vt_ld; size_t vt_seg_stride; int vt_cols;   // vt_cols: AttnParams::vt_cols (0 = vt_ld)
  const int* n_keys;
};

// `qb4`: the launch may run on 128-row blocks (attention.h attention_query_blocks) -- such a launch has no prefetch wave,
// so its caller carries no weight target on it (StepPlan)
template <int NP>
void attention(Ctx& c, int kc, const Planes& q, int ldq, const AttnKV& kv, const Planes& o, int ldo, int q_rows_per_seg,
               int heads, int segs, int ksplit = 1, const WeightPrefetch& pf = WeightPrefetch(), bool qb4 = false,
               int qp = -1, const float* q_ssq = nullptr) {
  AttnParams p;
  for (int i = 0; i < 2; ++i) {
    const int j = i < NP ? i : 0;
    p.q[i] = q.p[j]; p.k[i] = kv.k.p[j]; p.vt[i] = kv.vt.p[j]; p.o[i] = o.p[j];
  }
  p.n_keys = kv.n_keys; p.ldq = ldq; p.ldk = kv.ldk; p.ldo = ldo; p.vt_ld = kv.vt_ld;
  p.q_rows_per_seg = q_rows_per_seg; p.k_seg_stride = kv.k_seg_stride;
  p.vt_seg_stride = kv.vt_seg_stride; p.k_rows = kv.k_rows; p.vt_cols = kv.vt_cols;
  p.ksplit = ksplit; p.part_o = c.m->att_part_o; p.part_ml = c.m->att_part_ml;
  p.total_rows = q_rows_per_seg * segs;
  p.pf = pf;
  p.sat = c.m->d_sat; p.sat_tag = (unsigned)kc + 1u;
  p.qp = qp >= 0 ? qp : (kc == KC_ATTN_SELF ? c.m->att_qp_self : (kc == KC_ATTN_CROSS ? c.m->att_qp_cross : 0));
  // un-normalised queries (the folded cross-attention query projection): 1/rms from the residual stream's partial sums
  p.q_ssq = q_ssq; p.q_tiles = c.m->D / kNarrowTile; p.q_inv_d = 1.0f / (float)c.m->D;
  // K / V^T touch-ahead: the decoder's cross-attention (its cache is HBM-cold at every step) at ONE song per handle,
  // where the launch is latency-bound.  Same-process A/B, ms per segment, touches off -> 2 stages ahead
  // (profiles/r05b_touch_ab*.log, r05c_touch_b{2,4}.log): one song 943.1 -> 930.1 (-1.4 %; 4 / 8 ahead: 932.8 / 931.0);
  // 2 songs +1.1 %, 4 songs +3.5 %, 8 songs +3.1 % -- batched launches are bandwidth-bound and the touches only add
  // requests -- so the library turns it on for one song only, whatever msd_config.kv_touch_ahead asks for beyond that.
  p.touch_ahead = (kc == KC_ATTN_CROSS && segs == 1) ? c.m->kv_touch_ahead : 0;
  p.pf_late = 1;   // (such a launch's prefetch wave holds its touches back until the block's first stage has landed: attention.h)
  p.allow_qb4 = qb4;
  // a key-split cross-attention merges its partials inside the launch (attention.h attention_inlaunch_merge)
  p.tickets = (kc == KC_ATTN_CROSS && ksplit > 1 && c.m->merge_in_launch) ? c.m->att_tickets : nullptr;
  if (kc == KC_ATTN_SELF || kc == KC_ATTN_CROSS) {   // what the launcher is about to run, from its own rule
    AttnParams q = p;
    q.ksplit = 1 << attention_ksplit_log2(p.ksplit);
    c.m->ran_touch_blocks[kc == KC_ATTN_CROSS] = attention_launch_shape(q, heads, segs, NP, q_ssq != nullptr).touch_y * heads * segs;
  }
  c.begin(kc);
  c.latch(launch_attention<NP>(p, heads, segs, c.s));
  c.end(kc);
  if (c.m->prof.on && ksplit > 1 && p.tickets == nullptr) c.m->prof.launches[kc] += 1;  // + attention_merge_kernel
}

template <class Epi>
void gemm32(Ctx& c, int kc, const float* A, int lda, const float* B, int ldb, int M, int N, int K,
            const Epi& epi) {
  GemmF32Params p;
  p.A = A; p.B = B; p.lda = lda; p.ldb = ldb; p.M = M; p.N = N; p.K = K;
  c.begin(kc);
  c.latch(launch_gemm_f32(p, epi, c.s));
  c.end(kc);
}

// ---- weight packing ----------------------------------------------------------
int pack(msd_model* m, hipStream_t s, const float* w, int K, int N, Planes& dst, int dst_row0,
         int mode, int ldk = 0, int k0 = 0) {
  dim3 grid((K + 63) / 64, N), block(64);
  hipLaunchKernelGGL(pack_wt_kernel, grid, block, 0, s, w, K, N, dst.p[0],
                     m->NP == 2 ? dst.p[1] : (h16_t*)nullptr, dst_row0, mode, ldk,
                     reinterpret_cast<unsigned*>(m->d_absmax), k0);
  HIP_TRY(m, hipGetLastError());
  return MSD_OK;
}

// `extra_qkv_rows` / `extra_wo_rows`: rows left free BEHIND the packed q|k|v and out matrices in the same allocation (the
// decoder's folded cross-attention query projection puts its two matrices there: one weight-prefetch target covers both)
int pack_attention(msd_model* m, hipStream_t s, const std::string& p, AttnW& a, int extra_qkv_rows = 0, int extra_wo_rows = 0) {
  const int D = m->D, J = m->J;
  int rc;
  if ((rc = palloc(m, &a.wqkv, (size_t)(3 * J + extra_qkv_rows) * D))) return rc;
  if ((rc = palloc(m, &a.wo, (size_t)(D + extra_wo_rows) * J))) return rc;
  if ((rc = pack(m, s, W(m, p + "/query/kernel"), D, J, a.wqkv, 0, 0))) return rc;
  if ((rc = pack(m, s, W(m, p + "/key/kernel"), D, J, a.wqkv, J, 0))) return rc;
  if ((rc = pack(m, s, W(m, p + "/value/kernel"), D, J, a.wqkv, 2 * J, 0))) return rc;
  return pack(m, s, W(m, p + "/out/kernel"), J, D, a.wo, 0, 0);
}

int pack_mlp(msd_model* m, hipStream_t s, const std::string& p, MlpW& w) {
  const int D = m->D, F = m->F;
  int rc;
  if ((rc = palloc(m, &w.wi, (size_t)2 * F * D))) return rc;
  if ((rc = palloc(m, &w.wo, (size_t)D * F))) return rc;
  if ((rc = pack(m, s, W(m, p + "/wi_0/kernel"), D, F, w.wi, 0, 1))) return rc;
  if ((rc = pack(m, s, W(m, p + "/wi_1/kernel"), D, F, w.wi, 0, 2))) return rc;
  return pack(m, s, W(m, p + "/wo/kernel"), F, D, w.wo, 0, 0);
}

int pack_encoder(msd_model* m, hipStream_t s, const std::string& p, EncoderW& e) {
  e.layers.resize(m->Le);
  for (int l = 0; l < m->Le; ++l) {
    const std::string lp = p + "/layers_" + std::to_string(l);
    e.layers[l].ln_attn = W(m, lp + "/pre_attention_layer_norm/scale");
    e.layers[l].ln_mlp = W(m, lp + "/pre_mlp_layer_norm/scale");
    int rc;
    if ((rc = pack_attention(m, s, lp + "/attention", e.layers[l].attn))) return rc;
    if ((rc = pack_mlp(m, s, lp + "/mlp", e.layers[l].mlp))) return rc;
  }
  e.final_ln = W(m, p + "/encoder_norm/scale");
  return MSD_OK;
}

// ---- step-indexed tables -------------------------------------------------------
// diffusion_utils.py:166-202, evaluated in float32 like the reference.  cosine: closed form;
// linear: betas = linspace(start, stop, num_steps) in float64, log-SNR of the cumulative product
// clipped to [-20, 20], then jnp.interp (float32) over linspace(0, 1, num_steps).
struct Schedule {
  int kind = MSD_SCHEDULE_COSINE;
  std::vector<float> grid;   // linear: log-SNR at the num_steps knots
  bool init(int k, double start, double stop, int n, std::string* err) {
    kind = k;
    if (k == MSD_SCHEDULE_COSINE) return true;
    if (k != MSD_SCHEDULE_LINEAR) { *err = "Schedule not identified."; return false; }
    if (n < 2) { *err = "linear schedule needs num_steps >= 2"; return false; }
    if (!(start > 0.0) || !(stop < 1.0) || !(stop >= start)) { *err = "linear schedule needs 0 < start <= stop < 1"; return false; }
    grid.resize(n);
    double ac = 1.0;
    for (int i = 0; i < n; ++i) {
      const double beta = start + (stop - start) * (double)i / (double)(n - 1);
      ac *= 1.0 - beta;
      double l = std::log(ac) - std::log1p(-ac);
      l = l < -20.0 ? -20.0 : (l > 20.0 ? 20.0 : l);
      grid[i] = (float)l;
    }
    return true;
  }
  float at(float t) const {
    if (kind == MSD_SCHEDULE_COSINE) {
      const float b = (float)std::atan(std::exp(-0.5 * 20.0));
      const float a = (float)(std::atan(std::exp(0.5 * 20.0)) - std::atan(std::exp(-0.5 * 20.0)));
      return -2.0f * std::log(std::tan(a * t + b));
    }
    const int n = (int)grid.size();
    auto xp = [&](int i) { return (float)((double)i / (double)(n - 1)); };
    if (t <= xp(0)) return grid[0];
    if (t >= xp(n - 1)) return grid[n - 1];
    int i = 1;   // first knot strictly right of t (searchsorted side='right'), clipped to [1, n-1]
    while (i < n - 1 && xp(i) <= t) ++i;
    const float dx = xp(i) - xp(i - 1), df = grid[i] - grid[i - 1], delta = t - xp(i - 1);
    return grid[i - 1] + (delta / dx) * df;
  }
};

// One row of sampler coefficients per scan index (elementwise.h kCoef*): everything in
// eval_step.body that depends only on i (diffusion_utils.py:408-452, 120-163, 205-233, 369-379).
// steps = K > 0: the rows of a K-step scan (msd_sample_steps), t = (i + 1) / K and s = i / K; the sampler schedule's FUNCTION
// stays the handle's -- for `linear` that is the cfg.num_steps-knot grid, evaluated at those times.
bool build_coef_rows(const msd_config& cfg, std::vector<float>* out, std::string* err, int steps = 0) {
  const int N = steps > 0 ? steps : cfg.num_steps;
  Schedule samp, train;
  if (!samp.init(cfg.sampler_schedule, cfg.sampler_schedule_start, cfg.sampler_schedule_stop, cfg.num_steps, err)) return false;
  if (!train.init(cfg.train_schedule, cfg.train_schedule_start, cfg.train_schedule_stop,
                  cfg.train_schedule_num_steps, err)) return false;
  if (cfg.model_output < MSD_OUTPUT_EPS || cfg.model_output > MSD_OUTPUT_V) { *err = "Unknown model_output"; return false; }
  if (cfg.logvar_type < MSD_LOGVAR_LARGE || cfg.logvar_type > MSD_LOGVAR_MEDIUM) { *err = "unknown logvar_type"; return false; }
  if (cfg.logvar_type == MSD_LOGVAR_MEDIUM && !(cfg.logvar_frac >= 0.f && cfg.logvar_frac <= 1.f)) {
    *err = "medium logvar fraction outside [0, 1]"; return false;
  }
  auto sigmoid = [](float x) { return 1.0f / (1.0f + std::exp(-x)); };
  auto log_sigmoid = [](float x) { return -(std::fmax(-x, 0.0f) + std::log1p(std::exp(-std::fabs(x)))); };
  out->assign((size_t)N * kCoefCount, 0.f);
  for (int i = 0; i < N; ++i) {
    const float t = ((float)i + 1.0f) / (float)N, s = (float)i / (float)N;
    const float lt = samp.at(t), ls = samp.at(s), lm = train.at(t);
    float* c = &(*out)[(size_t)i * kCoefCount];
    c[kCoefLogsnrT] = lt;
    c[kCoefLogsnrS] = ls;
    // predict_x0_from_eps (diffusion_utils.py:215-222)
    c[kCoefX0Scale] = std::sqrt(1.0f + std::exp(-lt));
    c[kCoefX0Eps] = 1.0f / std::sqrt(1.0f + std::exp(lt));
    // diffusion_reverse (diffusion_utils.py:120-163)
    const float alpha_st = std::sqrt((1.0f + std::exp(-lt)) / (1.0f + std::exp(-ls)));
    const float alpha_s = std::sqrt(sigmoid(ls));
    const float r = std::exp(lt - ls);
    const float one_minus_r = -std::expm1(lt - ls);
    c[kCoefMeanZ] = r * alpha_st;
    c[kCoefMeanX0] = one_minus_r * alpha_s;
    if (cfg.logvar_type == MSD_LOGVAR_LARGE) {
      c[kCoefStd] = std::sqrt(one_minus_r * sigmoid(-lt));
    } else if (cfg.logvar_type == MSD_LOGVAR_SMALL) {
      c[kCoefStd] = std::sqrt(one_minus_r * sigmoid(-ls));
    } else {  // "medium:<frac>": interpolate the log-variances (log1mexp, diffusion_utils.py:100-106)
      const float x = ls - lt;   // > 0
      const float log_one_minus_r = x > std::log(2.0f) ? std::log1p(-std::exp(-x)) : std::log(-std::expm1(-x));
      const float min_lv = log_one_minus_r + log_sigmoid(-ls), max_lv = log_one_minus_r + log_sigmoid(-lt);
      c[kCoefStd] = std::sqrt(std::exp(cfg.logvar_frac * max_lv + (1.0f - cfg.logvar_frac) * min_lv));
    }
    // predict_eps_from_x0 (diffusion_utils.py:205-212)
    c[kCoefEpsScale] = std::sqrt(1.0f + std::exp(lt));
    c[kCoefEpsX0] = 1.0f / std::sqrt(1.0f + std::exp(-lt));
    // ddim_step (diffusion_utils.py:376-378)
    c[kCoefAlphaS] = alpha_s;
    c[kCoefSigmaS] = std::sqrt(sigmoid(-ls));
    // model-output conversion at the train schedule's log-SNR (diffusion_utils.py:294-317, 225-233)
    c[kCoefMLogsnr] = lm;
    c[kCoefMX0Scale] = std::sqrt(1.0f + std::exp(-lm));
    c[kCoefMX0Eps] = 1.0f / std::sqrt(1.0f + std::exp(lm));
    c[kCoefMEpsScale] = std::sqrt(1.0f + std::exp(lm));
    c[kCoefMEpsX0] = 1.0f / std::sqrt(1.0f + std::exp(-lm));
    c[kCoefMAlpha] = std::sqrt(sigmoid(lm));
    c[kCoefMSigma] = std::sqrt(sigmoid(-lm));
  }
  return true;
}

// The multistep form's side table (multistep_tail.h, kMs*) from the K rows of build_coef_rows: with lambda = logsnr / 2 of the
// SAMPLER schedule's float32 table values, h = lambda_s - lambda_t, r = h_prev / h (h_prev = h of row i + 1, the step
// before): {sigma_s / sigma_t, -alpha_s expm1(-h), 1 / (2r)}, in double, rounded once.  Row K - 1 has no step before it: 0.
void build_multistep_rows(const std::vector<float>& rows, std::vector<float>* out) {
  const int K = (int)(rows.size() / kCoefCount);
  out->assign((size_t)K * kMsCount, 0.f);
  auto half_step = [&](int i) {
    return 0.5 * ((double)rows[(size_t)i * kCoefCount + kCoefLogsnrS] - (double)rows[(size_t)i * kCoefCount + kCoefLogsnrT]);
  };
  for (int i = 0; i < K; ++i) {
    const double lt = rows[(size_t)i * kCoefCount + kCoefLogsnrT], ls = rows[(size_t)i * kCoefCount + kCoefLogsnrS];
    const double sigma_t = std::sqrt(1.0 / (1.0 + std::exp(lt))), sigma_s = std::sqrt(1.0 / (1.0 + std::exp(ls)));
    const double alpha_s = std::sqrt(1.0 / (1.0 + std::exp(-ls)));
    const double h = half_step(i), h_prev = i + 1 < K ? half_step(i + 1) : 0.0;
    float* c = &(*out)[(size_t)i * kMsCount];
    c[kMsZ] = (float)(sigma_s / sigma_t);
    c[kMsD] = (float)(-alpha_s * std::expm1(-h));
    c[kMsHist] = h_prev > 0.0 ? (float)(h / (2.0 * h_prev)) : 0.f;
  }
}

// The inversion's side table (invert_tail.h, kInv*) from the K rows of build_coef_rows: with alpha = sqrt(sigmoid(logsnr)) and
// sigma = sqrt(sigmoid(-logsnr)) of the SAMPLER schedule's float32 table values -- level i + 1: row i's logsnr_t, level i: row
// i's logsnr_s -- {a, b} = {alpha_{i+1} / alpha_i, sigma_{i+1} - a sigma_i} for i >= 1 and {alpha_1, sigma_1} for row 0 (the
// mirror of "scan index 0 returns x0"), in double, rounded once.
void build_invert_rows(const std::vector<float>& rows, std::vector<float>* out) {
  const int K = (int)(rows.size() / kCoefCount);
  out->assign((size_t)K * kInvCount, 0.f);
  for (int i = 0; i < K; ++i) {
    const double lt = rows[(size_t)i * kCoefCount + kCoefLogsnrT], ls = rows[(size_t)i * kCoefCount + kCoefLogsnrS];
    const double alpha_t = std::sqrt(1.0 / (1.0 + std::exp(-lt))), sigma_t = std::sqrt(1.0 / (1.0 + std::exp(lt)));
    const double alpha_s = std::sqrt(1.0 / (1.0 + std::exp(-ls))), sigma_s = std::sqrt(1.0 / (1.0 + std::exp(ls)));
    const double a = i == 0 ? alpha_t : alpha_t / alpha_s;
    float* c = &(*out)[(size_t)i * kInvCount];
    c[kInvA] = (float)a;
    c[kInvB] = (float)(i == 0 ? sigma_t : sigma_t - a * sigma_s);
  }
}

// The part-way start's coefficients (diffuse_to_step_kernel): alpha = sqrt(sigmoid(logsnr_t)), sigma = sqrt(sigmoid(-logsnr_t))
// of a row's sampler log-SNR, in double, rounded once
void diffuse_coefs(float logsnr_t, float* alpha, float* sigma) {
  const double l = (double)logsnr_t;
  *alpha = (float)std::sqrt(1.0 / (1.0 + std::exp(-l)));
  *sigma = (float)std::sqrt(1.0 / (1.0 + std::exp(l)));
}

// The resampling jump's coefficients (renoise_kernel) from level `from` up to level `to` (a level = the steps still to run):
// a = alpha_to / alpha_from, b = sqrt(1 - a^2), alpha = sqrt(sigmoid(logsnr)) of the SAMPLER schedule's float32 table value
// at the level -- level L > 0: row L - 1's logsnr_t; level 0: row 0's logsnr_s --, in double, each rounded once
void renoise_coefs(const std::vector<float>& rows, int from, int to, float* a, float* b) {
  auto alpha = [&](int level) {
    const double l = level > 0 ? (double)rows[(size_t)(level - 1) * kCoefCount + kCoefLogsnrT] : (double)rows[kCoefLogsnrS];
    return std::sqrt(1.0 / (1.0 + std::exp(-l)));
  };
  const double r = alpha(to) / alpha(from);
  *a = (float)r;
  *b = (float)std::sqrt(std::max(1.0 - r * r, 0.0));
}

int build_tables(msd_model* m, hipStream_t s) {
  const int N = m->N, D = m->D;
  {
    std::string why;
    if (!build_coef_rows(m->cfg, &m->h_coef, &why)) return fail(m, MSD_ERR_INVALID_ARGUMENT, "%s", why.c_str());
  }
  HIP_TRY(m, hipMemcpyAsync(m->d_coef, m->h_coef.data(), m->h_coef.size() * sizeof(float),
                            hipMemcpyHostToDevice, s));
  // time embedding (diffusion_utils.py:69-97 via network.py:377-379), float32
  std::vector<float> sig((size_t)N * D);
  const int half = D / 2;
  const float incr = (float)(std::log((double)m->cfg.max_decoder_noise_time / 1.0) / ((double)half - 1.0));
  for (int i = 0; i < N; ++i) {
    const float t = ((float)i + 1.0f) / (float)N;
    const float pos = t * m->cfg.max_decoder_noise_time;
    for (int k = 0; k < half; ++k) {
      const float inv = std::exp((float)k * -incr);
      const float st = pos * inv;
      sig[(size_t)i * D + k] = std::sin(st);
      sig[(size_t)i * D + half + k] = std::cos(st);
    }
  }
  float *d_sig = nullptr, *d_e0 = nullptr, *d_e1 = nullptr;
  HIP_TRY(m, hipMalloc(&d_sig, sig.size() * sizeof(float)));
  HIP_TRY(m, hipMalloc(&d_e0, (size_t)N * 4 * D * sizeof(float)));
  HIP_TRY(m, hipMalloc(&d_e1, (size_t)N * 4 * D * sizeof(float)));
  HIP_TRY(m, hipMemcpyAsync(d_sig, sig.data(), sig.size() * sizeof(float), hipMemcpyHostToDevice, s));
  Ctx c{m, s};
  gemm32(c, KC_IN_PROJ, d_sig, D, W(m, "decoder/time_emb_dense0/kernel"), 4 * D, N, 4 * D, D,
         EpiF32Swish{d_e0, 4 * D});
  gemm32(c, KC_IN_PROJ, d_e0, 4 * D, W(m, "decoder/time_emb_dense1/kernel"), 4 * D, N, 4 * D, 4 * D,
         EpiF32Swish{d_e1, 4 * D});
  // FiLM scale|bias for every (step, layer, slot): film[i][2l+k][2D]
  for (int l = 0; l < m->Ld; ++l)
    for (int k = 0; k < 2; ++k) {
      const std::string name = "decoder/layers_" + std::to_string(l) + "/FiLMLayer_" +
                               std::to_string(k) + "/DenseGeneral_0/kernel";
      gemm32(c, KC_IN_PROJ, d_e1, 4 * D, W(m, name), 2 * D, N, 2 * D, 4 * D,
             EpiF32Store{m->d_film + (size_t)(2 * l + k) * 2 * D, 2 * m->Ld * 2 * D});
    }
  // folded-norm tables
  {
    const int slots = 2 * m->Ld, J = m->J, F = m->F;
    const int nthreads = N * D;
    for (int l = 0; l < m->Ld; ++l) {
      const std::string lp = "decoder/layers_" + std::to_string(l);
      hipLaunchKernelGGL(build_g_kernel, dim3((nthreads + 255) / 256), dim3(256), 0, s, m->d_film,
                         W(m, lp + "/pre_self_attention_layer_norm/scale"), m->d_g, N, slots, 2 * l, D);
      hipLaunchKernelGGL(build_g_kernel, dim3((nthreads + 255) / 256), dim3(256), 0, s, m->d_film,
                         W(m, lp + "/pre_mlp_layer_norm/scale"), m->d_g, N, slots, 2 * l + 1, D);
      const float* bias_self = m->d_film + (size_t)(2 * l) * 2 * D + D;      // row = step, lda = slots*2D
      const float* bias_mlp = m->d_film + (size_t)(2 * l + 1) * 2 * D + D;
      const char* qkv[3] = {"/self_attention/query/kernel", "/self_attention/key/kernel", "/self_attention/value/kernel"};
      for (int t = 0; t < 3; ++t)
        gemm32(c, KC_IN_PROJ, bias_self, slots * 2 * D, W(m, lp + qkv[t]), J, N, J, D,
               EpiF32Store{m->d_bw_self + (size_t)l * 3 * J + t * J, m->Ld * 3 * J});
      for (int t = 0; t < 2; ++t)
        gemm32(c, KC_IN_PROJ, bias_mlp, slots * 2 * D, W(m, lp + "/mlp/wi_" + std::to_string(t) + "/kernel"), F, N, F, D,
               EpiF32StoreGated{m->d_bw_mlp + (size_t)l * 2 * F, m->Ld * 2 * F, t});
    }
  }
  HIP_TRY(m, hipStreamSynchronize(s));
  (void)hipFree(d_sig); (void)hipFree(d_e0); (void)hipFree(d_e1);
  if (c.err != hipSuccess) return fail(m, MSD_ERR_HIP, "table build failed: %s", hipGetErrorString(c.err));
  return MSD_OK;
}

// ---- encoder ---------------------------------------------------------------------
template <int NP>
void encoder_stack(Ctx& c, const EncoderW& w, int rows, int n_valid_slot) {
  msd_model* m = c.m;
  const int D = m->D, J = m->J, F = m->F;
  for (size_t l = 0; l < w.layers.size(); ++l) {
    const EncLayerW& lw = w.layers[l];
    norm<NP>(c, m->ex, lw.ln_attn, rows, D, nullptr, 0, 0, &m->eh, nullptr);
    const EpiQKV<NP> eq = epi_qkv<NP>(m->eqk, m->evt, 2 * J, m->Lenc_pad, J);
    gemm<NP, TK_QKV>(c, KC_GEMM_QKV, m->eh, D, lw.attn.wqkv, D, rows, 3 * J, D, eq, eq.v_start);
    const AttnKV kv = {planes_at<NP>(m->eqk, J), 2 * J, 0, m->Lenc_pad, m->evt, m->Lenc_pad, 0, 0, m->d_nkeys_enc + n_valid_slot};
    attention<NP>(c, KC_ATTN_SELF, m->eqk, 2 * J, kv, m->eao, J, rows, m->H, 1, 1, WeightPrefetch(), false, /*qp=*/0);
    gemm<NP, TK_SQUARE>(c, KC_GEMM_ATTN_OUT, m->eao, J, lw.attn.wo, J, rows, D, J, EpiResidual{m->ex, D});
    norm<NP>(c, m->ex, lw.ln_mlp, rows, D, nullptr, 0, 0, &m->eh, nullptr);
    gemm<NP, TK_MLP_IN>(c, KC_GEMM_MLP_IN, m->eh, D, lw.mlp.wi, D, rows, 2 * F, D, epi_out<EpiGeglu, NP>(m->eg, F));
    gemm<NP, TK_TALL>(c, KC_GEMM_MLP_OUT, m->eg, F, lw.mlp.wo, F, rows, D, F, EpiResidual{m->ex, D});
  }
}

template <int NP>
int encode_impl(msd_model* m, int batch, const int32_t* tokens_h, const float* ctx_dev,
                const int32_t* ctx_mask_h, hipStream_t s) {
  const int D = m->D, J = m->J, L = m->L, C = m->C;
  Ctx c{m, s};
  std::vector<int> pos;
  for (int b = 0; b < batch; ++b) {
    // S3: valid token positions only (mask = tokens > 0, network.py:476/546)
    pos.clear();
    for (int i = 0; i < L; ++i)
      if (tokens_h[(size_t)b * L + i] > 0) pos.push_back(i);
    const int Lv = (int)pos.size();
    int Cv = 0;
    int nk[2] = {Lv, 0};
    Planes enc_tok = m->enc;  // rows [0, ...)
    HIP_TRY(m, hipMemsetAsync(m->enc.p[0], 0, (size_t)m->S_pad * D * sizeof(h16_t), s));
    if (NP == 2) HIP_TRY(m, hipMemsetAsync(m->enc.p[1], 0, (size_t)m->S_pad * D * sizeof(h16_t), s));
    if (Lv > 0) {
      const int rows = round_up(Lv, 64);
      HIP_TRY(m, hipMemcpyAsync(m->d_tokens, tokens_h + (size_t)b * L, L * sizeof(int), hipMemcpyHostToDevice, s));
      HIP_TRY(m, hipMemcpyAsync(m->d_pos, pos.data(), Lv * sizeof(int), hipMemcpyHostToDevice, s));
      HIP_TRY(m, hipMemcpyAsync(m->d_nkeys_enc, nk, sizeof(int), hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(embed_tokens_kernel, dim3(rows), dim3(256), 0, s, m->d_tokens, m->d_pos, Lv,
                         rows, m->tok_emb, m->tok_pos, m->ex, D);
      encoder_stack<NP>(c, m->tok_enc, rows, 0);
      norm<NP>(c, m->ex, m->tok_enc.final_ln, rows, D, nullptr, 0, 0, &enc_tok, nullptr);
      // pageable H2D copies above return after staging, but `pos` is reused below:
      HIP_TRY(m, hipStreamSynchronize(s));
    }
    if (m->cfg.has_context) {
      pos.clear();
      const int32_t* cm = ctx_mask_h + (size_t)b * C;
      for (int i = 0; i < C; ++i)
        if (cm[i] > 0) pos.push_back(i);
      Cv = (int)pos.size();
      if (Cv > 0) {
        const int rows = round_up(Cv, 64);
        // positions (network.py:327-334): arange rolled by the sequence length
        int seq_len = 0;
        bool any_zero = false;
        for (int i = 0; i < C; ++i)
          if (cm[i] == 0) { seq_len = i; any_zero = true; break; }
        if (!any_zero) seq_len = 0;
        if (seq_len == 0 && cm[0] != 0) seq_len = C;
        std::vector<int> pidx(C);
        for (int i = 0; i < C; ++i) {
          const int src = m->cfg.context_terminal_relative ? ((i - seq_len) % C + C) % C : i;
          pidx[i] = src;  // roll(arange, seq_len)[i] = arange[(i - seq_len) mod C]
        }
        int* d_pidx = m->d_tokens;  // reuse (C <= L is not guaranteed: sized max(L, C))
        HIP_TRY(m, hipMemcpyAsync(d_pidx, pidx.data(), C * sizeof(int), hipMemcpyHostToDevice, s));
        HIP_TRY(m, hipMemcpyAsync(m->d_pos, pos.data(), Cv * sizeof(int), hipMemcpyHostToDevice, s));
        nk[1] = Cv;
        HIP_TRY(m, hipMemcpyAsync(m->d_nkeys_enc + 1, nk + 1, sizeof(int), hipMemcpyHostToDevice, s));
        const int n = C * m->ND;
        hipLaunchKernelGGL(scale_clip_kernel, dim3((n + 255) / 256), dim3(256), 0, s,
                           ctx_dev + (size_t)b * n, m->ctx_scaled, n, m->cfg.feature_min, m->cfg.feature_max);
        gemm32(c, KC_IN_PROJ, m->ctx_scaled, m->ND, m->w_ctx_in, D, C, D, m->ND,
               EpiF32AddRows{m->ctx_full, m->ctx_pos, d_pidx, D});
        hipLaunchKernelGGL(gather_rows_kernel, dim3(rows), dim3(256), 0, s, m->ctx_full, m->d_pos, Cv,
                           m->ex, D);
        encoder_stack<NP>(c, m->ctx_enc, rows, 1);
        // concat_encodings: right behind the valid tokens (one compact key axis); sum_cross_attends: its own
        // key region at a fixed offset
        const size_t ctx_row = m->n_cross == 2 ? (size_t)m->key_off[1] : (size_t)Lv;
        const Planes enc_ctx = planes_at<NP>(m->enc, ctx_row * D);
        norm<NP>(c, m->ex, m->ctx_enc.final_ln, rows, D, nullptr, 0, 0, &enc_ctx, nullptr);
        HIP_TRY(m, hipStreamSynchronize(s));
      }
    }
    const int Sv = Lv + Cv;
    // rows from Sv on may hold normalised padding rows of the last encoder: zero them.  (Also when Sv is a multiple of
    // 64: one token and 63 context frames make 64 keys, and the context encoder's 64 rows, written from row 1, reach row 64.)
    if (m->n_cross == 1 && m->S_pad > Sv) {
      for (int pl = 0; pl < NP; ++pl)
        HIP_TRY(m, hipMemsetAsync(m->enc.p[pl] + (size_t)Sv * D, 0,
                                  (size_t)(m->S_pad - Sv) * D * sizeof(h16_t), s));
    }
    // S2: cross-attention K / V^T of every decoder layer, once per segment; one projection per key region
    // (concat_encodings: one region = both encodings, network.py:217-230; sum_cross_attends: a module and a
    // region per encoding, :199-216)
    const int reg_rows[2] = {m->n_cross == 2 ? Lv : Sv, Cv};
    for (int l = 0; l < m->Ld; ++l)
      for (int e = 0; e < m->n_cross; ++e) {
        if (reg_rows[e] == 0) continue;   // no valid key: the attention kernel never reads this region
        const size_t koff = ((size_t)l * m->Bmax + b) * m->S_pad * J;
        const size_t r0 = (size_t)m->key_off[e];
        const EpiQKV<NP> ek = epi_qkv<NP>(planes_at<NP>(m->kc, koff + r0 * J), planes_at<NP>(m->vtc, koff + r0), J, m->S_pad, J);
        gemm<NP, TK_QKV>(c, KC_GEMM_QKV, planes_at<NP>(m->enc, r0 * D), D, m->dec[l].wkv_cross[e], D, round_up(reg_rows[e], 64),
                         2 * J, D, ek, ek.v_start);
      }
    for (int e = 0; e < m->n_cross; ++e) m->h_nkeys_cross[(size_t)e * m->Bmax + b] = reg_rows[e];
  }
  HIP_TRY(m, hipMemcpyAsync(m->d_nkeys_cross, m->h_nkeys_cross.data(), m->h_nkeys_cross.size() * sizeof(int),
                            hipMemcpyHostToDevice, s));
  if (c.err != hipSuccess) {
    (void)hipStreamSynchronize(s);
    return fail(m, MSD_ERR_HIP, "encode failed: %s", hipGetErrorString(c.err));
  }
  return check_range(m, s, "msd_encode");   // synchronises
}


// The key split exists to fill the chip when heads x query groups alone cannot (48 blocks at one song); with
// several songs per handle the (head, query group, song) blocks already cover the CUs, and every split costs a
// partial round trip + the merge launch: split only as far as ~192 blocks need.

// ... and as far as the segment's key axis pays for: a block of a split-s launch sees n_keys / (128 s) ring stages.
// Module e's key region and the most keys any song of the encoded batch has there:
inline int cross_region(const msd_model* m, int e) {
  return (e + 1 < m->n_cross ? m->key_off[e + 1] : m->S_pad) - m->key_off[e];
}
inline int cross_keys_max(const msd_model* m, int batch, int e) {
  int k = 0;
  for (int b = 0; b < batch && b < m->Bmax; ++b) k = std::max(k, m->h_nkeys_cross[(size_t)e * m->Bmax + b]);
  return k;
}
// The key split of cross-attention module e for the batch msd_encode prepared (msd_config.cross_key_split = 0), or the
// caller's choice; always a power of two within the workspace (m->cross_ksplit) and the region's stage count.
inline int cross_split(const msd_model* m, int batch, int e) {
  const int region = cross_region(m, e), stages = std::max(1, region / kAttStageKeys);
  int want;
  if (m->cfg.cross_key_split > 0) {
    want = m->cfg.cross_key_split;
  } else {
    const int blocks = m->H * (m->T / 64) * batch;
    want = blocks > 0 ? (192 + blocks - 1) / blocks : 1;   // 1 song: 4, 2-3 songs: 2, from 4 songs: 1 ...
    // ... but 2 on a long key axis: 12 x 4 x songs blocks of ~10 ring stages each are 1.5 rounds over the 256 CUs at 8
    // songs; halves of them pack better than the merge launch costs (ms per 300 / 200 steps, split 1 -> 2: 4 songs 759.7 ->
    // 752.4, 8 songs 782.4 -> 777.5; split 4 at 8 songs: 806.3; profiles/r05c_split_b8.log, r05c_touch_b4.log)
    // -- as long as the unsplit launch is at most one round of 64-row blocks: beyond that the launcher goes to 128-row
    // blocks instead (attention.h attention_query_blocks) and a split would only undo that
    if (want < 2 && blocks <= 256 && cross_keys_max(m, batch, e) > 6 * kAttStageKeys) want = 2;
    // the key split pays only on a long key axis (the 256-frame context region runs unsplit) ...
    const int cap = region >= 1024 ? 4 : (region >= 512 ? 2 : 1);
    want = std::min(want, cap);
    // ... and only as far as THIS segment's keys go: measured per key count at one song (profiles/r05a_split_sweep.log,
    // ms per 500 steps, split 1 / 2 / 4 / 8): 385 keys 482 / 481 / 488 / 524 . 657: 505 / 491 / 495 / 525 . 957: 527 / 502 /
    // 496 / 526 . 1257: 549 / 516 / 507 / 534 . 1793: 603 / 545 / 518 / 543 -- two blocks up to ~6 stages, four beyond
    if (want > 2 && cross_keys_max(m, batch, e) <= 6 * kAttStageKeys) want = 2;
  }
  want = std::min(want, std::min(m->cross_ksplit, stages));
  int ks = 1;
  while (ks * 2 <= want) ks *= 2;
  return ks;
}

// ---- the planner of a step (StepPlan, at the top of this file) -------------------------------------------------------
// No HIP calls: safe before and during stream capture.
StepPlan plan_step(const msd_model* m, int batch, int P, bool cond0, bool dedup0) {
  const int NP = m->NP, D = m->D, J = m->J, T = m->T, BT = batch * T, M = P * BT, nq = m->n_cross * J;
  StepPlan p = {};
  p.batch = batch; p.P = P; p.cond0 = cond0;
  // S6 (round 6): a layer's cross-attention query projection runs FOLDED into its QKV and attention-out launches
  // (gemm_h16.h "The folded cross-attention query projection") in the two-plane modes (fold_q is off in the others), on
  // narrow tiles (below the batched path's threshold) and on a conditional pass only.
  // (up to two songs per call: at three -- M = 1536, several rounds of blocks per launch -- the fold measured +2.4 %,
  // profiles/r06g_fold_ab_b3.log; the batched path's 128-row tiles from four songs have no narrow epilogue anyway)
  const bool may_fold = m->fold_q && cond0 && M <= 1024 && M < big_m_threshold() && BT % 64 == 0 &&
                        D / kNarrowTile <= kAuxMaxTiles && D % 128 == 0;
  for (int i = 0; i < 2; ++i) {
    StepPlan::SelfBlock& s = p.self[i];
    s.dup = dedup0 && i == 0;
    s.Ms = s.dup ? BT : M; s.Ps = s.dup ? 1 : P;
    const TileShape tq = pick_tile<2, TK_QKV>(s.Ms, 3 * J, 2 * J), to = pick_tile<2, TK_TALL>(s.Ms, D, 0, true, J);
    s.fold = may_fold && tq.bm == 64 && nq % tq.bn == 0 && to.bn == kNarrowTile;
    if (s.fold) {
      s.qkv = tq; s.out = to; s.out2 = {kNarrowTile, nq % 96 == 0 ? 96 : kNarrowTile};
      // the attention-out launch should stay within ONE round of the chip: 32 x 32 tiles that fill it by themselves (the
      // small model: 256 blocks) leave no CU for the second problem -- 64 x 32 then (half the blocks)
      if (to.bm == kNarrowTile && s.Ms % 64 == 0 && (s.Ms / 32) * (D / 32) + (BT / 32) * (nq / s.out2.bn) > 256) s.out = {64, kNarrowTile};
    }
    s.qb4 = attention_query_blocks(m->H * (T / 64) * s.Ps * batch, T, NP) == 4;
    s.warms = !cond0 ? WARM_MLP_IN : (s.fold ? WARM_CROSS_OUT : WARM_CROSS_Q);
    s.warm_on_out = s.qb4;
  }
  for (int e = 0; e < m->n_cross && cond0; ++e) {
    p.ks[e] = cross_split(m, batch, e);
    p.cross_qb4[e] = attention_query_blocks(m->H * (T / 64) * p.ks[e] * batch, T, NP) == 4;
    if (e + 1 == m->n_cross) p.mlp_in_on_cross_out = p.cross_qb4[e];
  }
  // Touch-block carriers: ONE song per call of a CFG step, where the attentions and the cross-attention output projection
  // run 192 blocks on 256 CUs.  The batched paths (128-row blocks, several rounds of blocks per launch) keep the plan above.
  if (m->touch_blocks && m->prefetch && NP == 2 && cond0 && batch == 1 && !p.cross_qb4[m->n_cross - 1]) {
    for (int i = 0; i < 2; ++i)
      if (!p.self[i].warm_on_out) p.self[i].touch_blocks = kTouchBlocksAsk;
    p.mlp_in_touch_blocks = kTouchBlocksAsk; p.mlp_in_touch_delay = kTouchDelayCrossAttn;
  }
  return p;
}
// S5: a CFG step computes layer 0's self-attention block once for both passes
inline StepPlan plan_cfg_step(const msd_model* m, int batch) {
  return plan_step(m, batch, m->passes, true, m->passes == 2 && m->dedup_layer0);
}

// ---- the decoder's tables and buffers, named once -------------------------------------------------------------------
// (every step-indexed table of the decoder is read through c.v: row `off` first, `mul` rows per step -- StepView)
inline Gain g_tab(const Ctx& c, int slot) {
  const msd_model* m = c.m;
  const int stride = 2 * m->Ld * m->D;
  return {m->d_g + (size_t)slot * m->D + (size_t)c.v.off * stride, stride * c.v.mul};
}
inline RowScale dec_row_scale(const Ctx& c, const float* bias = nullptr, int bias_step_stride = 0) {
  const msd_model* m = c.m;
  return row_scale(m->ssq, m->D / kNarrowTile, m->d_step, bias ? bias + (size_t)c.v.off * bias_step_stride : nullptr,
                   bias_step_stride * c.v.mul);
}
template <int NP>
EpiResidualNorm<NP> dec_residual(const msd_model* m, Gain lo, Gain hi, int split_row) {
  return epi_residual_norm<NP>(m->x, m->D, m->y, m->ssq, m->d_step, lo, hi, split_row);
}
template <int NP>
WeightPrefetch mlp_in_weights(const msd_model* m, int l) { return prefetch_of<NP>(m, m->dec[l].mlp.wi, 2 * m->F, m->D); }


// Weight prefetch plan of a layer (gemm_h16.h WeightPrefetch; every producer warms a LATER GEMM's weights from a
// wave of its own): QKV -> attention-out . self-attention -> cross-q (or MLP-in on an unconditional pass) .
// cross-q -> cross-out . cross-attention -> MLP-in . MLP-in -> MLP-out . MLP-out -> next layer's QKV; the exceptions are
// StepPlan's warms / warm_on_out / mlp_in_on_cross_out.
// One song per call (msd_config.touch_carrier = 2, the library's choice; StepPlan's touch_blocks / mlp_in_touch_blocks):
// the two attention launches run 192 blocks on 256 CUs and carry their targets on TOUCH BLOCKS behind the compute grid --
// self-attention -> cross-q / cross-out from 5 (layer 0) or 2 x 2 rows of 12 blocks . cross-attention -> MLP-in from 5 rows
// of 12 blocks behind kTouchDelayCrossAttn sleep rounds, while its in-block wave keeps the K / V^T touch-ahead alone.  The
// GEMM carriers keep their waves.  (Two more moves measured slower -- MLP-in on touch blocks of the cross-attention output
// projection, layer 0's QKV on the last MLP-out -- and live in tools/ubench/exp/touch_moves.patch: DESIGN.md 12.)

// (i) self-attention block (network.py:174-193).  Layer 0 is fed by the input projection; later layers consume
// the folded-norm planes `y` written by the previous layer's MLP output projection.
template <int NP>
void self_attention_block(Ctx& c, const StepPlan& p, int l) {
  msd_model* m = c.m;
  const DecLayerW& w = m->dec[l];
  const StepPlan::SelfBlock& sb = p.of(l);
  const int D = m->D, J = m->J, T = m->T, BT = p.batch * T;
  const int nq = m->n_cross * J;              // the modules' queries, stacked
  // fused q|k|v projection (network.py:181-189 via layers.py:262-264) on the folded-norm planes y
  const EpiQKV<NP> eq = epi_qkv<NP>(m->qk, m->vt, 2 * J, T, J, dec_row_scale(c, m->d_bw_self + (size_t)l * 3 * J, m->Ld * 3 * J));
  const WeightPrefetch pf_wo = prefetch_of<NP>(m, w.self.wo, sb.fold ? D + nq : D, J);   // (folded: + W2, right behind Wo)
  if constexpr (NP == 2) {
    if (sb.fold) {   // + (x0 (.) gamma_cross) . Wq on the launch's idle CUs, left in float32 for the attention-out launch
      const GemmParams p1 = gp_launch<NP>(c, KC_GEMM_QKV, m->y, D, w.self.wqkv, D, sb.Ms, 3 * J, D, sb.qkv.bm, pf_wo);
      const GemmParams p2 = gp_launch<NP>(c, KC_GEMM_QKV, m->xg, D, w.wq_fold, D, BT, nq, D, sb.qkv.bm);
      gemm_dual<FoldQkvTiles>(c, KC_GEMM_QKV, sb.qkv, p1, eq, sb.qkv, p2, epi_store_f32(m->qp, nq));
    }
  }
  if (!sb.fold) gemm<NP, TK_QKV>(c, KC_GEMM_QKV, m->y, D, w.self.wqkv, D, sb.Ms, 3 * J, D, eq, eq.v_start, pf_wo);
  const WeightPrefetch pf_next = sb.warms == WARM_MLP_IN ? mlp_in_weights<NP>(m, l)
                               : sb.warms == WARM_CROSS_OUT ? prefetch_of<NP>(m, w.wo_cross[0], D, J)
                                                            : prefetch_of<NP>(m, w.wq_cross[0], J, D);
  const AttnKV kv = {planes_at<NP>(m->qk, J), 2 * J, (size_t)T * 2 * J, T, m->vt, T, (size_t)J * T, 0, m->d_nkeys_self};
  attention<NP>(c, KC_ATTN_SELF, m->qk, 2 * J, kv, m->ao, J, T, m->H, sb.Ps * p.batch, 1,
                sb.warm_on_out ? WeightPrefetch() : on_touch_blocks(pf_next, sb.touch_blocks), sb.qb4);
  const WeightPrefetch pf_out = sb.warm_on_out ? pf_next : WeightPrefetch();
  // out-projection + residual; produces y for the cross-attention norm (conditional rows: plain gamma) and for the
  // MLP norm (unconditional rows, which skip cross-attention: S4)
  auto out_proj = [&](const auto& epi) {
    if constexpr (NP == 2) {
      if (sb.fold) {
        // S6: the output projection and ao . (Wo diag(gamma_cross) Wq_e) in ONE launch -- same A operand; the second problem
        // adds the half the QKV launch left in `qp` and stores the UN-NORMALISED queries of all modules, [BT, n_cross J]
        const GemmParams p1 = gp_launch<NP>(c, KC_GEMM_ATTN_OUT, m->ao, J, w.self.wo, J, sb.Ms, D, J, sb.out.bm, pf_out);
        const GemmParams p2 = gp_launch<NP>(c, KC_GEMM_ATTN_OUT, m->ao, J, w.w2_fold, J, BT, nq, J, sb.out2.bm);
        EpiAddStoreH16<NP> ea;
        out_pair<NP>(ea.out, m->cq); ea.ldc = nq; ea.addend = m->qp; ea.ld_add = nq;
        return gemm_dual<FoldOutTiles>(c, KC_GEMM_ATTN_OUT, sb.out, p1, epi, sb.out2, p2, ea);
      }
    }
    gemm<NP, TK_TALL>(c, KC_GEMM_ATTN_OUT, m->ao, J, w.self.wo, J, sb.Ms, D, J, epi, 0, pf_out);
  };
  const Gain g_mlp = g_tab(c, 2 * l + 1);
  EpiResidualNorm<NP> er = dec_residual<NP>(m, p.cond0 ? Gain{w.ln_cross, 0} : g_mlp, g_mlp, p.cond0 ? BT : 0);
  if (sb.dup) {   // rows [0, BT) computed once, written as both passes: y[r] for the cross-attention norm, y[r + BT] for the MLP norm
    EpiResidualNorm<NP, true> ed = residual_form<true, false>(er);
    ed.split_row = 0; ed.dup_rows = BT;
    out_proj(ed);
  } else {
    if (sb.fold) { er.g_lo = nullptr; er.g_lo_stride = 0; }   // the conditional rows' y = x1 (.) gamma_cross has no reader any more
    out_proj(er);
  }
}

// (ii) cross-attention block, conditional rows only (S4) (network.py:196-235)
template <int NP>
void cross_attention_block(Ctx& c, const StepPlan& p, int l) {
  msd_model* m = c.m;
  const DecLayerW& w = m->dec[l];
  const bool fold = p.of(l).fold;
  const int D = m->D, J = m->J, T = m->T, BT = p.batch * T, nq = m->n_cross * J;
  const Planes* const cq[2] = {&m->cq, &m->cq2};
  const Planes* const ao[2] = {&m->ao, &m->ao2};
  // every module projects its queries from the SAME normed input (network.py:196-198), so all query
  // projections run before the first output projection rewrites y
  for (int e = 0; e < m->n_cross && !fold; ++e)
    gemm<NP, TK_SQUARE>(c, KC_GEMM_CROSS_Q, m->y, D, w.wq_cross[e], D, BT, J, D, epi_out<EpiStoreH16, NP>(*cq[e], J, dec_row_scale(c)), 0,
                        prefetch_of<NP>(m, w.wo_cross[e], D, J));
  const size_t loff = (size_t)l * m->Bmax * m->S_pad * J;
  for (int e = 0; e < m->n_cross; ++e) {
    const size_t r0 = (size_t)m->key_off[e];
    const int region = cross_region(m, e);
    const AttnKV kv = {planes_at<NP>(m->kc, loff + r0 * J), J, (size_t)m->S_pad * J, region,
                       planes_at<NP>(m->vtc, loff + r0), m->S_pad, (size_t)J * m->S_pad, region, m->d_nkeys_cross + (size_t)e * m->Bmax};
    const bool warm_mlp_in = e + 1 == m->n_cross && !p.mlp_in_on_cross_out;
    // folded: module e's columns of the stacked, un-normalised queries
    attention<NP>(c, KC_ATTN_CROSS, fold ? planes_at<NP>(m->cq, (size_t)e * J) : *cq[e], fold ? nq : J, kv, *ao[e], J, T, m->H,
                  p.batch, p.ks[e],
                  warm_mlp_in ? on_touch_blocks(mlp_in_weights<NP>(m, l), p.mlp_in_touch_blocks, p.mlp_in_touch_delay) : WeightPrefetch(),
                  true, -1, fold ? m->ssq : nullptr);
  }
  // y = x + sum_e zero_if_masked(MHA_e(...)) (network.py:199-216 / 217-235): residual adds one after the
  // other; the last one also writes the folded-norm inputs of the MLP block
  for (int e = 0; e < m->n_cross; ++e) {
    const bool last_mod = e + 1 == m->n_cross;
    const EpiResidualNorm<NP> ec = dec_residual<NP>(m, last_mod ? g_tab(c, 2 * l + 1) : Gain(), Gain(), BT);
    gemm<NP, TK_SQUARE>(c, KC_GEMM_CROSS_OUT, *ao[e], J, w.wo_cross[e], J, BT, D, J, ec, 0,
                        last_mod && p.mlp_in_on_cross_out ? mlp_in_weights<NP>(m, l) : WeightPrefetch());
  }
}

// (iii) MLP block (network.py:241-256)
template <int NP>
void mlp_block(Ctx& c, const StepPlan& p, int l) {
  msd_model* m = c.m;
  const DecLayerW& w = m->dec[l];
  const int D = m->D, J = m->J, F = m->F, BT = p.batch * m->T, M = p.P * BT;
  const bool last_layer = (l + 1 == m->Ld);
  gemm<NP, TK_MLP_IN>(c, KC_GEMM_MLP_IN, m->y, D, w.mlp.wi, D, M, 2 * F, D,
                      epi_out<EpiGeglu, NP>(m->g, F, dec_row_scale(c, m->d_bw_mlp + (size_t)l * 2 * F, m->Ld * 2 * F)), 0,
                      prefetch_of<NP>(m, w.mlp.wo, D, F));
  const Gain g_next = last_layer ? Gain{m->dec_final_ln, 0} : g_tab(c, 2 * (l + 1));   // decoder_norm has no FiLM
  const EpiResidualNorm<NP> eo = dec_residual<NP>(m, g_next, g_next, 0);
  // S6: the next layer's folded query projection reads x (.) gamma_cross of the conditional rows from this epilogue
  // (and its stacked Wq sits right behind Wq|Wk|Wv: one prefetch target)
  const bool fold_next = !last_layer && p.self[1].fold;
  const WeightPrefetch pf_qkv = last_layer ? WeightPrefetch()
                                           : prefetch_of<NP>(m, m->dec[l + 1].self.wqkv, 3 * J + (fold_next ? m->n_cross * J : 0), D);
  if constexpr (NP == 2) {   // (the fold exists in the two-plane modes only: no single-plane Y2 kernels)
    if (fold_next) {
      EpiResidualNorm<NP, false, true> e2 = residual_form<false, true>(eo);
      out_pair<NP>(e2.y2, m->xg); e2.g2 = m->dec[l + 1].ln_cross; e2.y2_rows = BT;
      return gemm<NP, TK_TALL>(c, KC_GEMM_MLP_OUT, m->g, F, w.mlp.wo, F, M, D, F, e2, 0, pf_qkv);
    }
  }
  gemm<NP, TK_TALL>(c, KC_GEMM_MLP_OUT, m->g, F, w.mlp.wo, F, M, D, F, eo, 0, pf_qkv);
}

// decoder_norm + spec_out_dense (network.py:445-456).  The reference keeps this
// projection in float32 "for stability": its output eps enters x0 = sqrt(1+e^-l)(z - s eps)
// with a gain of up to 22026 at the first steps, and with 2^-16 products the short-chain
// parity tests show 40x more clip-boundary outliers.  Parity mode therefore runs it on the
// exact-fp32 MFMA; the plain bf16 mode uses the folded bf16 GEMM like its other layers.
template <int NP>
void final_projection(Ctx& c, const StepPlan& p) {
  msd_model* m = c.m;
  const int D = m->D, M = p.P * p.batch * m->T;
  if (NP == 2) {
    FinalProjParams fp;
    fp.x = m->x; fp.wg = m->w_out_g; fp.ssq = m->ssq; fp.out = m->eps;
    fp.M = M; fp.N = m->ND; fp.K = D; fp.tiles = D / kNarrowTile; fp.inv_d = 1.0f / (float)D;
    c.begin(KC_FINAL_PROJ);
    hipLaunchKernelGGL(final_proj_f32_kernel<1>, dim3(m->ND / 32, M / 16), dim3(64 * kFinalProjWaves), 0, c.s, fp);
    c.end(KC_FINAL_PROJ);
  } else {
    gemm<NP, TK_NARROW>(c, KC_FINAL_PROJ, m->y, D, m->w_out_p, D, M, m->ND, D, epi_store_f32(m->eps, m->ND, dec_row_scale(c)));
  }
}

template <int NP>
void decoder_layers(Ctx& c, const StepPlan& p) {
  for (int l = 0; l < c.m->Ld; ++l) {
    self_attention_block<NP>(c, p, l);
    if (p.cond0) cross_attention_block<NP>(c, p, l);
    mlp_block<NP>(c, p, l);
  }
  final_projection<NP>(c, p);
}

// Decoder input (gemm_h16.h EpiInProj): x and the folded-norm inputs of layer 0's self norm (table slot 0) for the passes
// layer 0's self-attention block reads (S5: one), + x (.) gamma_cross when layer 0 folds its query projection (S6)
template <int NP>
void in_proj(Ctx& c, const StepPlan& p, bool publish_step = false) {
  msd_model* m = c.m;
  const StepPlan::SelfBlock& s0 = p.self[0];
  const int BT = p.batch * m->T;
  EpiInProj<NP> ei;
  ei.x = m->x; ei.ldx = m->D; ei.pos = m->dec_pos; ei.T = m->T; ei.pass_rows = BT; ei.passes = s0.Ps;
  out_pair<NP>(ei.y, m->y); ei.ssq = m->ssq; ei.tiles = m->D / kNarrowTile;
  const Gain g0 = g_tab(c, 0);
  ei.g = g0.g; ei.g_stride = g0.step_stride; ei.step_ptr = m->d_step;
  ei.step_copy = publish_step ? m->d_step : nullptr;
  if (s0.fold) { out_pair<NP>(ei.y2, m->xg); ei.g2 = m->dec[0].ln_cross; }
  gemm<NP, TK_NARROW>(c, KC_IN_PROJ, m->zp, m->ND, m->w_in_p, m->ND, BT, m->D, m->ND, ei, 0,
                      prefetch_of<NP>(m, m->dec[0].self.wqkv, 3 * m->J + (s0.fold ? m->n_cross * m->J : 0), m->D));
}

// one decoder evaluation: P passes from z's planes to eps
void decoder_eval(Ctx& c, const StepPlan& p, bool publish_step) {
  if (c.m->NP == 2) { in_proj<2>(c, p, publish_step); decoder_layers<2>(c, p); }
  else { in_proj<1>(c, p, publish_step); decoder_layers<1>(c, p); }
}

// z (fp32) -> bf16 planes, after z was written from outside the sampler kernel
void split_z(msd_model* m, int64_t n, hipStream_t s) { split(m->z, m->zp, n, s, m->d_sat, (unsigned)KC_SAMPLER + 1u); }

// ... and every kernel that writes z itself writes the planes and the range flag with it: the handle's z as the output of
// P -- SamplerParams and the structs derived from it, DiffuseParams, RenoiseParams, LossDiffuseParams (elementwise.h)
template <class P>
void z_out(P& p, const msd_model* m, unsigned sat_tag = (unsigned)KC_SAMPLER + 1u) {
  p.z = m->z;
  p.z_hi = m->zp.p[0];
  p.z_lo = m->NP == 2 ? m->zp.p[1] : nullptr;
  p.sat = m->d_sat; p.sat_tag = sat_tag;
}
// blocks of kRngRowBlock elements per [T, n] row of z (SamplerParams::row_blocks); a row that is no whole number of them
// keeps every block on row 0 of the key table, and the per-row calls are refused (check_encoded_call)
int row_blocks_of(const msd_model* m) { return m->T * m->ND % kRngRowBlock == 0 ? m->T * m->ND / kRngRowBlock : 1 << 30; }

// one DDPM step of the CFG sampler: the decoder on plan_cfg_step's plan, then the sampler update
// c.v: the call's view of the step-indexed tables, its coefficient rows, its sampler and whether that runs in its keep form
void enqueue_step(Ctx& c, const StepPlan& p) {
  msd_model* m = c.m;
  decoder_eval(c, p, /*publish_step=*/true);
  const int sampler = c.v.sampler;
  SamplerKeepParams sp;
  sp.eps = m->eps; sp.noise_slot = m->d_noise_slot; sp.coef = c.v.coef; sp.rng_key = m->d_rng_key;
  sp.step_ptr = m->d_step; sp.n = p.batch * m->T * m->ND; sp.passes = p.P;
  sp.row_blocks = row_blocks_of(m);
  sp.cond_wt = m->cfg.cfg_weight; sp.clip_x0 = m->cfg.clip_x0;
  sp.ddim = sampler == MSD_SAMPLER_DDIM;
  sp.model_output = m->cfg.model_output;
  z_out(sp, m);
  c.begin(KC_SAMPLER);
  sp.step_from_slot1 = 1;
  if (c.v.invert) {   // (msd_invert: no draw, no known frames; the row weights decide the passes it reads)
    SamplerInvertParams ip;
    static_cast<SamplerParams&>(ip) = sp;
    ip.row_wt = m->d_row_wt; ip.coef_inv = c.v.coef_inv;
    launch_sampler_invert(ip, c.s);
  } else if (sampler == MSD_SAMPLER_DPMPP_2M) {   // (never with keep: check_call refuses the pair)
    SamplerMultistepGuidedParams mp;
    static_cast<SamplerParams&>(mp) = sp;
    mp.x0_prev = m->x0_prev; mp.coef_ms = c.v.coef_ms;
    mp.first_step = c.v.steps - 1;
    mp.row_wt = m->d_row_wt;
    if (c.v.guided) launch_sampler_step(mp, c.s);
    else launch_sampler_step(static_cast<const SamplerMultistepParams&>(mp), c.s);
  } else if (c.v.guided) {   // (never with keep either: msd_sample_guided takes no known frames)
    SamplerGuidedParams gp;
    static_cast<SamplerParams&>(gp) = sp;
    gp.row_wt = m->d_row_wt;
    launch_sampler_step(gp, c.s);
  } else if (c.v.keep) {
    sp.xk = m->keep_xk; sp.keep = m->keep_flags; sp.n_dims = m->ND;
    launch_sampler_step(sp, c.s);
  } else {
    launch_sampler_step(static_cast<const SamplerParams&>(sp), c.s);
  }
  c.end(KC_SAMPLER);
}

// One stream capture (thread-local) on s: whatever `enqueue` puts on the stream -- it returns a status, its message set --
// instantiated as *out.  The hipGraph_t is destroyed on every path; `what` names the capture in the message.
template <class Enqueue>
int capture_graph(msd_model* m, hipStream_t s, const char* what, hipGraphExec_t* out, Enqueue enqueue) {
  hipGraph_t graph = nullptr;
  HIP_TRY(m, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue();
  const hipError_t ce = hipStreamEndCapture(s, &graph);
  if (ce != hipSuccess || rc) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc ? rc : fail(m, MSD_ERR_HIP, "%s capture failed: %s", what, hipGetErrorString(ce));
  }
  const hipError_t ie = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ie != hipSuccess) { *out = nullptr; return fail(m, MSD_ERR_HIP, "%s: hipGraphInstantiate: %s", what, hipGetErrorString(ie)); }
  return MSD_OK;
}

}  // namespace

// =============================================================================
// C ABI
// =============================================================================
extern "C" {

const char* msd_version(void) {
  static const std::string v = std::string("msd_amd 0.7.0 (gfx950, abi 7, ") + kPlaneName + ")";
  return v.c_str();
}

int msd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  return n;
}

const char* msd_last_error(const msd_model* m) { return m ? m->err.c_str() : "null model"; }

int msd_create(const msd_config* cfg, msd_model** out) {
  if (!cfg || !out) return MSD_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  // (the struct as ABI 6 / 7 first had it, without the field appended since, is taken too: the field reads as 0)
  if (cfg->struct_size != (int32_t)sizeof(msd_config) && cfg->struct_size != (int32_t)offsetof(msd_config, touch_carrier))
    return MSD_ERR_INVALID_ARGUMENT;
  msd_model* m = new msd_model();
  memset(&m->cfg, 0, sizeof(m->cfg));
  memcpy(&m->cfg, cfg, (size_t)cfg->struct_size);
  m->cfg.struct_size = (int32_t)sizeof(msd_config);
  cfg = &m->cfg;
  (void)hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking);   // first: every fill / copy below goes through it (copy_sync)
  auto bad = [&](const char* why) {
    // keep the handle alive so the caller can read the message
    m->err = why;
    *out = m;
    return MSD_ERR_INVALID_ARGUMENT;
  };
  if (cfg->head_dim != kHeadDim) { m->err = "head_dim must be 64"; *out = m; return MSD_ERR_UNSUPPORTED; }
  if (cfg->precision < MSD_PREC_F16 || cfg->precision > MSD_PREC_BF16X3) return bad("unknown precision");
  {  // the plane FORMAT is a property of the library build (common.h): refuse the other build's precisions
    const bool want_bf16 = cfg->precision == MSD_PREC_BF16 || cfg->precision == MSD_PREC_BF16X3;
    if (want_bf16 != (MSD_PLANE_BF16 != 0)) {
      m->err = std::string("this library holds operand planes in ") + (MSD_PLANE_BF16 ? "bfloat16" : "IEEE half") +
               (MSD_PLANE_BF16 ? ": it implements MSD_PREC_BF16 / MSD_PREC_BF16X3; load libmsd_amd.so for MSD_PREC_F16 / MSD_PREC_F16X3"
                               : ": it implements MSD_PREC_F16 / MSD_PREC_F16X3; load libmsd_amd_bf16.so for MSD_PREC_BF16 / MSD_PREC_BF16X3");
      *out = m;
      return MSD_ERR_UNSUPPORTED;
    }
  }
  if (cfg->sampler != MSD_SAMPLER_DDPM && cfg->sampler != MSD_SAMPLER_DDIM && cfg->sampler != MSD_SAMPLER_DPMPP_2M)
    return bad("Unknown sampler type");
  if (cfg->emb_dim % 64 || cfg->emb_dim > 1024 || cfg->emb_dim < 64) return bad("emb_dim must be a multiple of 64 in [64, 1024]");
  if (cfg->mlp_dim % 64) return bad("mlp_dim must be a multiple of 64");
  if (cfg->targets_length % 64 || cfg->targets_length <= 0) return bad("targets length must be a multiple of 64");
  if (cfg->n_dims % 64) return bad("n_dims must be a multiple of 64");
  if (cfg->num_steps <= 0 || cfg->max_batch <= 0 || cfg->num_heads <= 0) return bad("non-positive size");
  if (cfg->has_context && cfg->context_length <= 0) return bad("context model needs context_length");
  if (cfg->attn_q_planes < 0 || cfg->attn_q_planes > 2) return bad("attn_q_planes must be 0 (library default), 1 or 2");
  if (cfg->attn_p_planes < 0 || cfg->attn_p_planes > 2) return bad("attn_p_planes must be 0 (library default), 1 or 2");
  if (cfg->graph_steps < 0 || cfg->graph_steps > 64) return bad("graph_steps must be in [0, 64] (0 = library default)");
  if (cfg->weight_prefetch < 0 || cfg->weight_prefetch > 2) return bad("weight_prefetch must be 0 (by model size), 1 (on) or 2 (off)");
  if (cfg->dedup_layer0 < 0 || cfg->dedup_layer0 > 2) return bad("dedup_layer0 must be 0 (library default), 1 (on) or 2 (off)");
  if (cfg->cross_key_split != 0 && cfg->cross_key_split != 1 && cfg->cross_key_split != 2 && cfg->cross_key_split != 4 &&
      cfg->cross_key_split != 8) return bad("cross_key_split must be 0 (chosen per segment), 1, 2, 4 or 8");
  if (cfg->keep_raw_weights < 0 || cfg->keep_raw_weights > 1) return bad("keep_raw_weights must be 0 or 1");
  if (cfg->kv_touch_ahead < -1 || cfg->kv_touch_ahead > 16) return bad("kv_touch_ahead must be 0 (library default), -1 (off) or 1 .. 16 stages");
  if (cfg->cross_merge_in_launch < 0 || cfg->cross_merge_in_launch > 2) return bad("cross_merge_in_launch must be 0 (library default), 1 (on) or 2 (off)");
  if (cfg->cross_q_fold < 0 || cfg->cross_q_fold > 2) return bad("cross_q_fold must be 0 (library default), 1 (on) or 2 (off)");
  if (cfg->mlp_in_persistent < 0 || cfg->mlp_in_persistent > 2) return bad("mlp_in_persistent must be 0 (library default), 1 (on) or 2 (off)");
  if (cfg->touch_carrier < 0 || cfg->touch_carrier > 2) return bad("touch_carrier must be 0 (library default), 1 (in-block waves) or 2 (touch blocks)");
  {  // schedule / model_output / logvar_type combinations are validated by building the table once
    std::vector<float> rows;
    std::string why;
    if (!build_coef_rows(*cfg, &rows, &why)) { m->err = why; *out = m; return MSD_ERR_INVALID_ARGUMENT; }
  }
  m->NP = (cfg->precision == MSD_PREC_F16X3 || cfg->precision == MSD_PREC_BF16X3) ? 2 : 1;
  m->D = cfg->emb_dim; m->H = cfg->num_heads; m->J = cfg->num_heads * kHeadDim; m->F = cfg->mlp_dim;
  m->T = cfg->targets_length; m->L = cfg->inputs_length; m->C = cfg->has_context ? cfg->context_length : 0;
  m->ND = cfg->n_dims; m->N = cfg->num_steps; m->Ld = cfg->num_decoder_layers; m->Le = cfg->num_encoder_layers;
  m->Bmax = cfg->max_batch;
  m->passes = (cfg->cfg_weight != 1.0f) ? 2 : 1;
  if (cfg->graph_steps > 0) m->graph_steps = cfg->graph_steps;
  if (cfg->weight_prefetch) m->prefetch = cfg->weight_prefetch == 1;   // 0: msd_finalize_weights decides from the sizes
  m->dedup_layer0 = cfg->dedup_layer0 != 2;
  if (cfg->kv_touch_ahead) m->kv_touch_ahead = cfg->kv_touch_ahead < 0 ? 0 : cfg->kv_touch_ahead;
  m->merge_in_launch = cfg->cross_merge_in_launch != 2;
  m->fold_q = cfg->cross_q_fold != 2 && m->NP == 2;
  m->persist_mlp_in = cfg->mlp_in_persistent != 2;
  if (cfg->touch_carrier) m->touch_blocks = cfg->touch_carrier == 2;
  {
    // Query-side planes of the decoder's attentions (attention.h QP bit 0: Q one plane, bit 1: P one plane).  Library
    // default with half planes in the two-plane mode: kDefaultQPlanes / kDefaultPPlanes (the sharp-
    // attention study); bfloat16 planes (8-bit significands) always keep both.
    const bool can_drop = kPlaneSaturates && m->NP == 2;
    const int qpl = cfg->attn_q_planes ? cfg->attn_q_planes : (can_drop ? kDefaultQPlanes : 2);
    const int ppl = cfg->attn_p_planes ? cfg->attn_p_planes : (can_drop ? kDefaultPPlanes : 2);
    m->att_qp_self = m->att_qp_cross = m->NP == 2 ? ((qpl == 1 ? 1 : 0) | (ppl == 1 ? 2 : 0)) : 0;
  }
  {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
      m->cus = cus;
  }
  // encode_impl writes round_up(Lv, 64) token rows and then round_up(Cv, 64) context rows from row Lv
  m->S_pad = round_up(m->L, 64) + round_up(m->C, 64);
  // decoder_cross_attend_style (network.py:199-235): with one encoding both styles are the same module
  m->n_cross = (cfg->cross_attend_sum && cfg->has_context) ? 2 : 1;
  m->key_off[0] = 0; m->key_off[1] = round_up(m->L, 64);
  m->Lenc_pad = round_up(m->L > m->C ? m->L : m->C, 64);
  declare_weights(m);
  *out = m;
  set_func_attrs();

  const int D = m->D, J = m->J, F = m->F, T = m->T;
  const size_t Mmax = (size_t)m->passes * m->Bmax * T;
  int rc = MSD_OK;
#define TRY(e) do { if ((rc = (e)) != MSD_OK) return rc; } while (0)
  for (auto& w : m->weights) TRY(dalloc(m, &w.dev, (size_t)w.numel()));
  TRY(dalloc(m, &m->d_coef, (size_t)m->N * kCoefCount));
  TRY(dalloc(m, &m->d_film, (size_t)m->N * 2 * m->Ld * 2 * D));
  TRY(dalloc(m, &m->d_g, (size_t)m->N * 2 * m->Ld * D));
  TRY(dalloc(m, &m->d_bw_self, (size_t)m->N * m->Ld * 3 * J));
  TRY(dalloc(m, &m->d_bw_mlp, (size_t)m->N * m->Ld * 2 * F));
  TRY(dalloc(m, &m->x, Mmax * D));
  TRY(palloc(m, &m->y, Mmax * D));
  TRY(palloc(m, &m->zp, (size_t)m->Bmax * T * m->ND));
  TRY(dalloc(m, &m->ssq, Mmax * (D / kNarrowTile)));
  // cross-attention key split: enough blocks for the whole chip when the key axis is long
  m->cross_ksplit = m->S_pad >= 1024 ? 8 : (m->S_pad >= 512 ? 4 : (m->S_pad >= 256 ? 2 : 1));   // workspace bound
  TRY(dalloc(m, &m->att_part_o, (size_t)m->cross_ksplit * m->Bmax * T * J));
  TRY(dalloc(m, &m->att_part_ml, (size_t)m->cross_ksplit * m->Bmax * T * m->H * 2));
  m->att_ticket_count = m->Bmax * (T / 32) * m->H;
  TRY(dalloc(m, &m->att_tickets, (size_t)m->att_ticket_count));   // (zeroed)
  TRY(palloc(m, &m->h, Mmax * D));
  TRY(palloc(m, &m->qk, Mmax * 2 * J));
  TRY(palloc(m, &m->vt, Mmax * J));
  TRY(palloc(m, &m->ao, Mmax * J));
  // the modules' queries: one allocation -- [Bmax T, J] per module one after the other, or (folded projection, S6) ONE
  // [BT, n_cross J] matrix of all modules' un-normalised queries
  TRY(palloc(m, &m->cq, (size_t)m->n_cross * m->Bmax * T * J));
  if (m->n_cross == 2) {
    for (int i = 0; i < m->NP; ++i) m->cq2.p[i] = m->cq.p[i] + (size_t)m->Bmax * T * J;
    TRY(palloc(m, &m->ao2, (size_t)m->Bmax * T * J));
  }
  if (m->fold_q) {
    TRY(palloc(m, &m->xg, (size_t)m->Bmax * T * D));
    TRY(dalloc(m, &m->qp, (size_t)m->Bmax * T * m->n_cross * J));
  }
  TRY(palloc(m, &m->g, Mmax * F));
  TRY(dalloc(m, &m->h32, Mmax * D));
  TRY(dalloc(m, &m->eps, Mmax * m->ND));
  TRY(dalloc(m, &m->z, (size_t)m->Bmax * T * m->ND));
  TRY(dalloc(m, &m->d_noise_slot, 1));
  TRY(dalloc(m, &m->d_rng_key, (size_t)m->Bmax * kRngWords));
  TRY(dalloc(m, &m->d_step, 2));
  TRY(dalloc(m, &m->d_absmax, 1));
  TRY(dalloc(m, &m->d_sat, 1));
  HIP_TRY(m, hipHostMalloc(reinterpret_cast<void**>(&m->h_sat), sizeof(unsigned), hipHostMallocDefault));
  *m->h_sat = 0;
  TRY(dalloc(m, &m->d_nkeys_self, (size_t)m->passes * m->Bmax));
  TRY(dalloc(m, &m->d_nkeys_cross, (size_t)2 * m->Bmax));
  m->h_nkeys_cross.assign((size_t)m->n_cross * m->Bmax, 0);
  {
    std::vector<int> nk((size_t)m->passes * m->Bmax, T);
    HIP_TRY(m, copy_sync(m, m->d_nkeys_self, nk.data(), nk.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  TRY(palloc(m, &m->kc, (size_t)m->Ld * m->Bmax * m->S_pad * J));
  TRY(palloc(m, &m->vtc, (size_t)m->Ld * m->Bmax * m->S_pad * J));
  const size_t E = m->Lenc_pad;
  TRY(dalloc(m, &m->ex, E * D));
  TRY(palloc(m, &m->eh, E * D));
  TRY(palloc(m, &m->eqk, E * 2 * J));
  TRY(palloc(m, &m->evt, E * J));
  TRY(palloc(m, &m->eao, E * J));
  TRY(palloc(m, &m->eg, E * F));
  TRY(palloc(m, &m->enc, (size_t)m->S_pad * D));
  TRY(dalloc(m, &m->d_tokens, E));
  TRY(dalloc(m, &m->d_pos, E));
  TRY(dalloc(m, &m->d_nkeys_enc, 2));
  if (m->cfg.has_context) {
    TRY(dalloc(m, &m->ctx_scaled, (size_t)m->C * m->ND));
    TRY(dalloc(m, &m->ctx_full, (size_t)round_up(m->C, 64) * D));
  }
#undef TRY
  HIP_TRY(m, hipEventCreate(&m->prof.e0));
  HIP_TRY(m, hipEventCreate(&m->prof.e1));
  if (!m->own_stream) return fail(m, MSD_ERR_HIP, "hipStreamCreateWithFlags failed");
  return MSD_OK;
}

void msd_destroy(msd_model* m) {
  if (!m) return;
  (void)msd_reset_graph(m);
  if (m->prof.e0) (void)hipEventDestroy(m->prof.e0);
  if (m->prof.e1) (void)hipEventDestroy(m->prof.e1);
  if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
  if (m->h_sat) (void)hipHostFree(m->h_sat);
  for (void* p : m->allocs) (void)hipFree(p);
  delete m;
}

int msd_num_weights(const msd_model* m) { return m ? (int)m->weights.size() : -1; }

int msd_weight_info(const msd_model* m, int index, const char** name, int64_t shape[2], int* ndim) {
  if (!m || index < 0 || index >= (int)m->weights.size()) return MSD_ERR_INVALID_ARGUMENT;
  const Weight& w = m->weights[index];
  if (name) *name = w.name.c_str();
  if (shape) { shape[0] = w.shape[0]; shape[1] = w.shape[1]; }
  if (ndim) *ndim = w.ndim;
  return MSD_OK;
}

int msd_set_weight(msd_model* m, const char* name, const float* data, const int64_t* shape, int ndim) {
  if (!m || !name || !data || !shape) return fail(m, MSD_ERR_INVALID_ARGUMENT, "null argument");
  auto it = m->windex.find(name);
  if (it == m->windex.end()) return fail(m, MSD_ERR_UNKNOWN_WEIGHT, "unknown weight '%s'", name);
  Weight& w = m->weights[it->second];
  bool ok = ndim == w.ndim && shape[0] == w.shape[0] && (ndim == 1 || shape[1] == w.shape[1]);
  if (!ok)
    return fail(m, MSD_ERR_SHAPE_MISMATCH, "weight '%s': expected [%lld,%lld] (ndim %d)", name,
                (long long)w.shape[0], (long long)w.shape[1], w.ndim);
  // Weights are loaded ONCE per handle: after msd_finalize_weights every msd_set_weight is refused -- also for a weight
  // whose float32 copy is still resident (norm scales, embeddings, keep_raw_weights = 1): accepting it used to clear
  // `finalized` while a second msd_finalize_weights refuses ("already finalized"), which left the handle unusable and
  // the new values unused.
  if (m->dec.size() || !w.dev)
    return fail(m, MSD_ERR_BAD_STATE, "weight '%s': msd_finalize_weights has run (weights are loaded once per handle; "
                "create a new model)", name);
  HIP_TRY(m, copy_sync(m, w.dev, data, (size_t)w.numel() * sizeof(float), hipMemcpyDefault));
  w.set = true;
  m->finalized = false;
  return MSD_OK;
}

int msd_finalize_weights(msd_model* m, void* stream) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (const auto& w : m->weights)
    if (!w.set) return fail(m, MSD_ERR_BAD_STATE, "weight '%s' was never set", w.name.c_str());
  if (m->dec.size()) return fail(m, MSD_ERR_BAD_STATE, "weights already finalized (create a new model)");
  const std::string tok = m->cfg.has_context ? "token_encoder" : "encoder";
  int rc;
  if ((rc = pack_encoder(m, s, tok, m->tok_enc))) return rc;
  m->tok_emb = W(m, tok + "/token_embedder/embedding");
  m->tok_pos = W(m, tok + "/Embed_0/embedding");
  if (m->cfg.has_context) {
    if ((rc = pack_encoder(m, s, "continuous_encoder", m->ctx_enc))) return rc;
    m->w_ctx_in = W(m, "continuous_encoder/input_proj/kernel");
    m->ctx_pos = W(m, "continuous_encoder/Embed_0/embedding");
  }
  m->dec.resize(m->Ld);
  const int D = m->D, J = m->J;
  for (int l = 0; l < m->Ld; ++l) {
    const std::string lp = "decoder/layers_" + std::to_string(l);
    DecLayerW& w = m->dec[l];
    w.ln_self = W(m, lp + "/pre_self_attention_layer_norm/scale");
    w.ln_cross = W(m, lp + "/pre_cross_attention_layer_norm/scale");
    w.ln_mlp = W(m, lp + "/pre_mlp_layer_norm/scale");
    const int nq_fold = m->fold_q ? m->n_cross * J : 0;
    if ((rc = pack_attention(m, s, lp + "/self_attention", w.self, nq_fold, nq_fold))) return rc;
    for (int e = 0; e < m->n_cross; ++e) {
      const std::string cp = lp + "/MultiHeadDotProductAttention_" + std::to_string(e);
      if ((rc = palloc(m, &w.wq_cross[e], (size_t)J * D))) return rc;
      if ((rc = palloc(m, &w.wkv_cross[e], (size_t)2 * J * D))) return rc;
      if ((rc = palloc(m, &w.wo_cross[e], (size_t)D * J))) return rc;
      if ((rc = pack(m, s, W(m, cp + "/query/kernel"), D, J, w.wq_cross[e], 0, 0))) return rc;
      if ((rc = pack(m, s, W(m, cp + "/key/kernel"), D, J, w.wkv_cross[e], 0, 0))) return rc;
      if ((rc = pack(m, s, W(m, cp + "/value/kernel"), D, J, w.wkv_cross[e], J, 0))) return rc;
      if ((rc = pack(m, s, W(m, cp + "/out/kernel"), J, D, w.wo_cross[e], 0, 0))) return rc;
    }
    if ((rc = pack_mlp(m, s, lp + "/mlp", w.mlp))) return rc;
    if (m->fold_q) {
      // S6: (x1 (.) gamma) . Wq with x1 = x0 + ao . Wo  ==  (x0 (.) gamma) . Wq + ao . (Wo diag(gamma) Wq): the second
      // matrix per module, accumulated in float64, rounded once to float32 and packed like any other weight; the modules'
      // matrices are stacked along N (one launch projects the queries of all modules)
      // Both live behind the self-attention's matrices of the same row length (pack_attention left the rows free):
      // [Wq|Wk|Wv ; Wq_cross] is ONE prefetch target of the previous layer's MLP output projection, [Wo ; W2] one of the
      // QKV launch -- no launch carries a prefetch wave it did not carry before the fold.
      for (int i = 0; i < 2; ++i) {
        w.wq_fold.p[i] = w.self.wqkv.p[i] ? w.self.wqkv.p[i] + (size_t)3 * J * D : nullptr;
        w.w2_fold.p[i] = w.self.wo.p[i] ? w.self.wo.p[i] + (size_t)D * J : nullptr;
      }
      for (int e = 0; e < m->n_cross; ++e)
        if ((rc = pack(m, s, W(m, lp + "/MultiHeadDotProductAttention_" + std::to_string(e) + "/query/kernel"), D, J, w.wq_fold, e * J, 0))) return rc;
      float* w2 = nullptr;
      HIP_TRY(m, hipMalloc(&w2, (size_t)J * J * sizeof(float)));
      for (int e = 0; e < m->n_cross && rc == MSD_OK; ++e) {
        hipLaunchKernelGGL(fold_wq_kernel, dim3((J + 15) / 16, (J + 15) / 16), dim3(16, 16), 0, s,
                           W(m, lp + "/self_attention/out/kernel"), w.ln_cross,
                           W(m, lp + "/MultiHeadDotProductAttention_" + std::to_string(e) + "/query/kernel"), w2, J, D, J);
        rc = pack(m, s, w2, J, J, w.w2_fold, e * J, 0);
      }
      const hipError_t es = hipStreamSynchronize(s);
      (void)hipFree(w2);
      if (rc) return rc;
      HIP_TRY(m, es);
    }
  }
  m->dec_final_ln = W(m, "decoder/decoder_norm/scale");
  m->w_spec_out = W(m, "decoder/spec_out_dense/kernel");
  m->w_in_proj = W(m, "decoder/continuous_inputs_projection/kernel");
  m->dec_pos = W(m, "decoder/Embed_0/embedding");
  if ((rc = palloc(m, &m->w_in_p, (size_t)D * m->ND))) return rc;
  if ((rc = palloc(m, &m->w_out_p, (size_t)m->ND * D))) return rc;
  if ((rc = pack(m, s, m->w_in_proj, m->ND, D, m->w_in_p, 0, 0))) return rc;
  if ((rc = pack(m, s, m->w_spec_out, D, m->ND, m->w_out_p, 0, 0))) return rc;
  if ((rc = dalloc(m, &m->w_out_g, (size_t)D * m->ND))) return rc;
  hipLaunchKernelGGL(scale_rows_kernel, dim3((D * m->ND + 255) / 256), dim3(256), 0, s, m->w_spec_out,
                     m->dec_final_ln, m->w_out_g, D, m->ND);
  if ((rc = build_tables(m, s))) return rc;
  {
    // The weight prefetch pays only when a step streams more than the memory-side Infinity Cache (256 MB) holds:
    // base_with_context moves 396 MB of packed decoder weights + 170 MB of cached cross K/V per step, so every
    // launch used to start on HBM-cold operands (1.172 -> 1.09 ms/step with the prefetch); the `small` preset moves
    // 143 MB, its weights simply stay cached from one step to the next and the touches are pure overhead
    // (489 -> 501 ms per segment: profiles/r02_prefetch_ab.log).  msd_config.weight_prefetch overrides.
    const size_t planes = (size_t)m->NP * sizeof(h16_t);
    const size_t per_layer = ((size_t)3 * J * D + (size_t)D * J + (size_t)m->n_cross * 2 * ((size_t)J * D) +
                              (size_t)2 * m->F * D + (size_t)D * m->F) * planes;
    const size_t kv = (size_t)m->Ld * m->Bmax * m->S_pad * J * 2 * planes;
    const size_t per_step = per_layer * m->Ld + kv;
    bool decided = m->cfg.weight_prefetch != 0;
    if (!decided) m->prefetch = per_step > ((size_t)256 << 20);
  }
  HIP_TRY(m, hipStreamSynchronize(s));
  {  // half planes hold kWScale * w: |w| must stay below 65504 / kWScale (common.h)
    float top = 0.f;
    HIP_TRY(m, copy_sync(m, &top, m->d_absmax, sizeof(float), hipMemcpyDeviceToHost));
    if (!(top < kPlaneMax / kWScale))
      return fail(m, MSD_ERR_UNSUPPORTED,
                  "a projection weight has magnitude %g: the %s of this build hold |w| < %g (the bfloat16-plane build, "
                  "libmsd_amd_bf16.so / precision 'bf16x3', has no such limit)",
                  (double)top, kPlaneName, (double)(kPlaneMax / kWScale));
  }
  if (!m->cfg.keep_raw_weights) {
    // The float32 staging copy of every matrix that now lives in operand planes / tables has no reader left (finalize
    // runs once per handle): 1.5 GB of the 1.65 GB at base_with_context.  What run time still reads from the raw store
    // stays: the 1-D norm scales, the embedding / position tables and the context encoder's fp32 input projection.
    std::vector<const float*> keep = {m->tok_emb, m->tok_pos, m->w_ctx_in, m->ctx_pos, m->dec_pos};
    for (auto& w : m->weights) {
      if (w.ndim != 2 || !w.dev || std::find(keep.begin(), keep.end(), w.dev) != keep.end()) continue;
      auto it = std::find(m->allocs.begin(), m->allocs.end(), static_cast<void*>(w.dev));
      if (it != m->allocs.end()) m->allocs.erase(it);
      (void)hipFree(w.dev);
      w.dev = nullptr;
    }
    m->w_spec_out = m->w_in_proj = nullptr;   // (packed: w_out_g / w_out_p, w_in_p)
  }
  m->finalized = true;
  return MSD_OK;
}

int msd_encode(msd_model* m, int batch, const int32_t* tokens, const float* ctx_dev,
               const int32_t* ctx_mask, void* stream) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  if (!m->finalized) return fail(m, MSD_ERR_BAD_STATE, "msd_finalize_weights has not run");
  if (batch < 1 || batch > m->Bmax) return fail(m, MSD_ERR_INVALID_ARGUMENT, "batch %d outside [1, %d]", batch, m->Bmax);
  if (!tokens) return fail(m, MSD_ERR_INVALID_ARGUMENT, "tokens is null");
  if (m->cfg.has_context && (!ctx_dev || !ctx_mask))
    return fail(m, MSD_ERR_INVALID_ARGUMENT, "context model needs ctx and ctx_mask");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // tokens / mask may live on either side: stage them on the host (a few KiB).  The staging copies run on the handle's
  // own stream (copy_sync): a DEVICE-side tokens / mask buffer the caller is still writing on `stream` must be complete
  // first -- one synchronisation of the caller's stream orders it (microseconds against a ~1 s segment).
  HIP_TRY(m, hipStreamSynchronize(s));
  std::vector<int32_t> tok_h((size_t)batch * m->L), mask_h;
  HIP_TRY(m, copy_sync(m, tok_h.data(), tokens, tok_h.size() * sizeof(int32_t), hipMemcpyDefault));
  if (m->cfg.has_context) {
    mask_h.resize((size_t)batch * m->C);
    HIP_TRY(m, copy_sync(m, mask_h.data(), ctx_mask, mask_h.size() * sizeof(int32_t), hipMemcpyDefault));
  }
  for (int32_t t : tok_h)
    if (t < 0 || t >= m->cfg.vocab_size) return fail(m, MSD_ERR_INVALID_ARGUMENT, "token id %d outside [0, %d)", t, m->cfg.vocab_size);
  if (int rc0 = arm_range(m, s)) return rc0;
  int rc = m->NP == 2 ? encode_impl<2>(m, batch, tok_h.data(), ctx_dev, mask_h.data(), s)
                      : encode_impl<1>(m, batch, tok_h.data(), ctx_dev, mask_h.data(), s);
  if (rc) return rc;
  m->encoded = true;
  m->encoded_batch = batch;
  return MSD_OK;
}

int msd_fill_normal(uint64_t seed, uint64_t stream_id, uint32_t subseq, float* out_dev, int64_t n,
                    void* stream) {
  if (!out_dev || n < 0) return MSD_ERR_INVALID_ARGUMENT;
  if (n == 0) return MSD_OK;
  const int64_t blocks4 = (n + 3) / 4;
  hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)((blocks4 + 255) / 256), 1), dim3(256), 0,
                     static_cast<hipStream_t>(stream), out_dev, n, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32), subseq);
  return hipGetLastError() == hipSuccess ? MSD_OK : MSD_ERR_HIP;
}

// jax.random.normal(key, [n]) for key = PRNGKey(seed) or fold_in(PRNGKey(seed), fold); stage / bits_in: msd_op_threefry
static int threefry_fill(int stage, uint64_t seed, int64_t fold, const uint32_t* bits_in, float* out_dev, int64_t n,
                         hipStream_t s) {
  if (!out_dev || n < 0 || n > 0xFFFFFFFFll || fold > 0xFFFFFFFFll || stage < 0 || stage > 3) return MSD_ERR_INVALID_ARGUMENT;
  if (n == 0) return MSD_OK;
  uint32_t k0 = (uint32_t)(seed >> 32), k1 = (uint32_t)seed;
  if (fold >= 0) {
    uint32_t f0 = 0u, f1 = (uint32_t)fold;
    threefry2x32(k0, k1, f0, f1);
    k0 = f0; k1 = f1;
  }
  const int64_t half = (n + 1) / 2;
  hipLaunchKernelGGL(threefry_normal_kernel, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, s, out_dev, n, k0, k1,
                     stage, bits_in);
  return hipGetLastError() == hipSuccess ? MSD_OK : MSD_ERR_HIP;
}

int msd_fill_normal_threefry(uint64_t seed, int64_t fold, float* out_dev, int64_t n, void* stream) {
  return threefry_fill(2, seed, fold, nullptr, out_dev, n, static_cast<hipStream_t>(stream));
}

// the words the sampler kernel's own draw reads (one row of SamplerParams::rng_key): EVERY place that launches the step
// with a NULL noise slot writes all of them for every row of z, the generator kind and the mode included
static void fill_rng_key(uint32_t* key, int rng, uint64_t seed, uint64_t stream_id, bool per_row) {
  const uint32_t k[kRngWords] = {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32),
                                 (uint32_t)rng, (uint32_t)(seed >> 32), (uint32_t)seed, per_row ? 1u : 0u};
  memcpy(key, k, sizeof(k));
}

// The generator keys of one sampling call: ONE (seed, stream_id) for a draw over the whole [batch, T, n] array
// (msd_sample, msd_sample_rng), or one per row (msd_sample_rows; stream_ids may be NULL = zeros).
struct SampleKeys {
  uint64_t seed = 0, stream_id = 0;
  const uint64_t *seeds = nullptr, *stream_ids = nullptr;
  bool per_row() const { return seeds != nullptr; }
  uint64_t seed_of(int b) const { return seeds ? seeds[b] : seed; }
  uint64_t stream_of(int b) const { return seeds ? (stream_ids ? stream_ids[b] : 0) : stream_id; }
};

// the key table of a call over `batch` rows of z (whole-array draw: every row holds the one key)
static hipError_t upload_rng_keys(msd_model* m, int batch, int rng, const SampleKeys& keys, hipStream_t s) {
  m->h_rng_key.resize((size_t)batch * kRngWords);   // a member: the copy below may still read it when this returns
  for (int b = 0; b < batch; ++b)
    fill_rng_key(&m->h_rng_key[(size_t)b * kRngWords], rng, keys.seed_of(b), keys.stream_of(b), keys.per_row());
  return hipMemcpyAsync(m->d_rng_key, m->h_rng_key.data(), m->h_rng_key.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
}

// One sampling call as its entry point describes it to sample_body: filled once, checked once, handed down.  Every field is
// the value the call runs with: no known frames = a null `known`; steps, sampler and start_step are resolved on filling.
struct SampleCall {
  int batch, rng;                // rows of z; the msd_rng_kind of the draws that are not given
  SampleKeys keys;
  const float *init_z, *noise;   // device; null = drawn
  float* out; void* stream;
  const float* known;            // msd_sample_keep / msd_sample_edit: the caller's mel [batch, T, n] (device)
  const int32_t* mask;           // msd_sample_keep: frame flags [batch, T] (host or device)
  const int32_t* release;        // msd_sample_edit: release words [batch, T] (host, validated by the entry point)
  int start_step;                // the scan index the call starts at: steps - 1, or msd_sample_edit's
  int steps, sampler;            // K (K | N) and the msd_sampler_kind
  int jump = 1, times = 1;       // msd_sample_resample: every block of `jump` steps is descended `times` times (1 = no jump)
  // msd_sample_guided: row b combines with weights[n_weights == 1 ? 0 : b] at scan indices in [guide_lo, guide_hi) and
  // takes the cond_wt == 1 branch (one decoder pass) outside; null = the handle's own weight at every step, as ever
  const float* weights = nullptr;   // host
  int n_weights = 0, guide_lo = 0, guide_hi = 0;
  // msd_invert: the caller's mel [batch, T, n] (device); the scan starts at index 0 from it and counts up through all of
  // `steps`, every step on the two-pass plan when guide_lo < guide_hi, else on the one-pass plan; `weights` is always given
  // and `out` receives z in model units.  null = a sampling call
  const float* invert_mel = nullptr;
};

static SampleKeys sample_keys(int per_row, const uint64_t* seeds, const uint64_t* stream_ids) {
  if (per_row) return {0, 0, seeds, stream_ids};
  return {seeds[0], stream_ids ? stream_ids[0] : 0};
}

// the call of msd_sample_rng / msd_sample_rows: all of the handle's steps with its sampler, no known frames
static SampleCall plain_call(const msd_model* m, int batch, int rng, const SampleKeys& keys, const float* init_z, const float* noise, float* out, void* stream) {
  return {batch, rng, keys, init_z, noise, out, stream, nullptr, nullptr, nullptr, m->N - 1, m->N, m->cfg.sampler};
}

// "1, 2, 4, ..." -- the step counts msd_sample_steps takes on a handle of n steps
static std::string divisors_of(int n) {
  std::string out;
  for (int k = 1; k <= n; ++k)
    if (n % k == 0) out += (out.empty() ? "" : ", ") + std::to_string(k);
  return out;
}

// a call's own step count (msd_sample_steps, msd_sample_guided, msd_invert): 0 = the handle's N, or a divisor of it
static int check_num_steps(msd_model* m, int num_steps) {
  if (num_steps < 0 || (num_steps > 0 && m->N % num_steps))
    return fail(m, MSD_ERR_INVALID_ARGUMENT, "num_steps %d does not divide the handle's %d steps; it takes 0 (= %d) or one of %s",
                num_steps, m->N, m->N, divisors_of(m->N).c_str());
  return MSD_OK;
}

// The guidance weights of a call (msd_sample_guided, msd_invert; host): 1 or one per row, finite, whole sampler blocks per
// row when there is one per row; *all_one: every row takes the cond_wt == 1 branch.  A handle created with cfg_weight 1 holds
// one pass's buffers: it takes no weights at all, or -- one_pass_ok, the inversion -- none but 1.
static int check_row_weights(msd_model* m, int batch, const float* weights, int n_weights, bool one_pass_ok, bool* all_one) {
  if (!weights || (n_weights != 1 && n_weights != batch))
    return fail(m, MSD_ERR_INVALID_ARGUMENT, "guidance takes 1 weight or one per row (%d), got %d", batch, weights ? n_weights : 0);
  *all_one = true;
  for (int b = 0; b < n_weights; ++b) {
    if (!std::isfinite(weights[b])) return fail(m, MSD_ERR_INVALID_ARGUMENT, "guidance weight %d is not finite", b);
    *all_one = *all_one && weights[b] == 1.0f;
  }
  const int64_t row_n = (int64_t)m->T * m->ND;
  if (n_weights > 1 && row_n % kRngRowBlock)   // a block of the sampler launch would straddle two rows' weights
    return fail(m, MSD_ERR_UNSUPPORTED, "per-row guidance weights need targets_length * n_dims %% %d == 0 (got %lld)", (int)kRngRowBlock, (long long)row_n);
  if (m->passes == 1 && !(one_pass_ok && *all_one))
    return fail(m, MSD_ERR_UNSUPPORTED, "a handle created with cfg_weight 1 holds one pass's buffers and takes no per-call guidance: "
                "create the handle with any weight != 1");
  return MSD_OK;
}

// The view of a call of K steps with `sampler` (K | N, a known kind) in the keep form or not, every field filled, with what
// it needs built on first use: the known-frame buffers (each on its own, so that a call after a failed allocation tries
// again for the one that is missing), the K-row coefficient table (K == N: the handle's own), the multistep side table,
// x0_prev; `invert`: the inversion form (msd_invert) with its side table and the row-weight table.  Runs outside stream
// capture; every allocation is the handle's.
static int make_step_view(msd_model* m, int K, int sampler, bool keep, StepView* v, bool invert = false) {
  const int N = m->N;
  if (keep) {
    if (int rc = ensure(m, &m->keep_xk, (size_t)m->Bmax * m->T * m->ND)) return rc;
    if (int rc = ensure(m, &m->keep_flags, (size_t)m->Bmax * m->T)) return rc;
  }
  *v = StepView();
  v->steps = K; v->mul = N / K; v->off = N / K - 1; v->coef = m->d_coef; v->sampler = sampler; v->keep = keep;
  // (the kernels index base + step * stride in 64 bits; the stride itself travels as an int)
  const int64_t widest = std::max<int64_t>(std::max<int64_t>(2 * m->Ld * m->D, (int64_t)m->Ld * 3 * m->J), (int64_t)m->Ld * 2 * m->F);
  if (widest * v->mul > 0x7FFFFFFFll)
    return fail(m, MSD_ERR_UNSUPPORTED, "a stride of %d table rows does not fit the GEMM epilogues' 32-bit row stride", v->mul);
  v->invert = invert;
  if (K == N && sampler != MSD_SAMPLER_DPMPP_2M && !invert) return MSD_OK;   // the handle's own tables
  msd_model::StepTables& t = m->step_tables[K];
  if (K == N) {
    t.coef = m->d_coef;
  } else if (!t.coef) {
    std::string why;
    if (!build_coef_rows(m->cfg, &t.h_coef, &why, K)) return fail(m, MSD_ERR_INVALID_ARGUMENT, "%s", why.c_str());
    if (int rc = dalloc(m, &t.coef, t.h_coef.size())) return rc;
    HIP_TRY(m, copy_sync(m, t.coef, t.h_coef.data(), t.h_coef.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  v->coef = t.coef;
  if (sampler == MSD_SAMPLER_DPMPP_2M) {
    if (!t.coef_ms) {
      std::vector<float> ms;
      build_multistep_rows(K == N ? m->h_coef : t.h_coef, &ms);
      if (int rc = dalloc(m, &t.coef_ms, ms.size())) return rc;
      HIP_TRY(m, copy_sync(m, t.coef_ms, ms.data(), ms.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    v->coef_ms = t.coef_ms;
    if (int rc = ensure(m, &m->x0_prev, (size_t)m->Bmax * m->T * m->ND)) return rc;
  }
  if (invert) {
    if (!t.coef_inv) {
      std::vector<float> inv;
      build_invert_rows(K == N ? m->h_coef : t.h_coef, &inv);
      if (int rc = dalloc(m, &t.coef_inv, inv.size())) return rc;
      HIP_TRY(m, copy_sync(m, t.coef_inv, inv.data(), inv.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    v->coef_inv = t.coef_inv;
    if (int rc = ensure(m, &m->d_row_wt, (size_t)m->Bmax)) return rc;
  }
  return MSD_OK;
}

// What every call that runs the decoder on the encoded state refuses, sampling or loss: no encoded state, another batch
// than the encoded one, an unknown generator, per-row keys on rows that are no whole number of the sampler's blocks
static int check_encoded_call(msd_model* m, int batch, int rng, bool per_row) {
  if (!m->encoded) return fail(m, MSD_ERR_BAD_STATE, "msd_encode has not run");
  if (batch != m->encoded_batch) return fail(m, MSD_ERR_INVALID_ARGUMENT, "batch %d != encoded batch %d", batch, m->encoded_batch);
  if (rng != MSD_RNG_PHILOX && rng != MSD_RNG_THREEFRY) return fail(m, MSD_ERR_INVALID_ARGUMENT, "unknown rng %d", rng);
  const int64_t row_n = (int64_t)m->T * m->ND;
  if (per_row && row_n % kRngRowBlock)   // a block of the sampler launch would straddle two rows' keys
    return fail(m, MSD_ERR_UNSUPPORTED, "per-row keys need targets_length * n_dims %% %d == 0 (got %lld)", (int)kRngRowBlock, (long long)row_n);
  return MSD_OK;
}

// ---- the phases of a sampling call, in the order sample_body runs them ---------------------------------------------
static int check_call(msd_model* m, const SampleCall& c) {
  if (c.known && (c.steps != m->N || c.sampler == MSD_SAMPLER_DPMPP_2M))
    return fail(m, MSD_ERR_UNSUPPORTED, "known frames run on the handle's own step count with ddpm or ddim (no multistep history across a release)");
  if (c.jump < 1 || c.times < 1) return fail(m, MSD_ERR_INVALID_ARGUMENT, "resampling needs jump >= 1 and times >= 1 (got %d, %d)", c.jump, c.times);
  if (c.times > 1 && c.rng == MSD_RNG_PHILOX)   // pass p draws under (seed, stream_id + (p << 32))
    for (int b = 0; b < (c.keys.per_row() ? c.batch : 1); ++b)
      if (c.keys.stream_of(b) >> 32)
        return fail(m, MSD_ERR_INVALID_ARGUMENT, "a call with resampling needs stream_id < 2^32 (row %d: %llu)", b, (unsigned long long)c.keys.stream_of(b));
  if (int rc = check_encoded_call(m, c.batch, c.rng, c.keys.per_row())) return rc;
  if (!c.out) return fail(m, MSD_ERR_INVALID_ARGUMENT, "out is null");
  if (c.known && m->ND % 4)   // a thread of the sampler holds four consecutive elements and ONE frame flag
    return fail(m, MSD_ERR_UNSUPPORTED, "kept frames need n_dims %% 4 == 0 (got %d)", m->ND);
  return MSD_OK;
}

// The legacy NULL stream cannot be captured: the call runs on the handle's own (non-blocking) stream.  What the caller
// enqueued on the NULL stream before this call (its init_z / noise / out buffers) is ordered in front by ONE
// hipStreamSynchronize of it -- NOT hipDeviceSynchronize (round 5): that waited for every other handle's stream on the
// device as well, against the header's "handles are independent, also on one device".
static int choose_stream(msd_model* m, void* stream, hipStream_t* s) {
  *s = stream ? static_cast<hipStream_t>(stream) : m->own_stream;
  if (!stream) HIP_TRY(m, hipStreamSynchronize(nullptr));
  return MSD_OK;
}

// z, its planes and -- known frames -- xk and the frames' release words, at the scan index the call starts at
static int write_initial_state(msd_model* m, const SampleCall& c, hipStream_t s) {
  const int64_t n = (int64_t)c.batch * m->T * m->ND;
  if (c.invert_mel) {   // level 0 of the inversion: the mel as the context enters, scale_features(clip=True), and its planes
    hipLaunchKernelGGL(scale_clip_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c.invert_mel, m->z, (int)n, m->cfg.feature_min, m->cfg.feature_max);
    HIP_TRY(m, hipGetLastError());
    split_z(m, n, s);
    return MSD_OK;
  }
  if (c.init_z) {
    HIP_TRY(m, hipMemcpyAsync(m->z, c.init_z, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  } else {
    // one fill over the whole array, or -- per-row keys -- one per row over its T * n elements under its own key
    const int fills = c.keys.per_row() ? c.batch : 1;
    const int64_t fill_n = n / fills;
    for (int b = 0; b < fills; ++b) {
      float* zb = m->z + b * fill_n;
      int rc = c.rng == MSD_RNG_THREEFRY ? msd_fill_normal_threefry(c.keys.seed_of(b), -1, zb, fill_n, s)   // normal(PRNGKey(seed), [batch | 1, T, n])
                                         : msd_fill_normal(c.keys.seed_of(b), c.keys.stream_of(b), 0, zb, fill_n, s);
      if (rc) return fail(m, rc, "init_z fill failed");
    }
  }
  if (c.start_step == c.steps - 1) {
    split_z(m, n, s);
    if (c.known) {
      // the known mel enters the chain as the context does: scale_features(clip=True); init_z and the draws are untouched
      hipLaunchKernelGGL(scale_clip_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c.known, m->keep_xk, (int)n, m->cfg.feature_min, m->cfg.feature_max);
      HIP_TRY(m, hipGetLastError());
    }
  } else {
    // part-way start (msd_sample_edit): z holds the call's initial draw eps; one pass makes xk and z = alpha xk + sigma eps
    // at the start index's noise level, with z's planes and the range flag (what split_z does for the plain start)
    DiffuseParams dp;
    dp.mel = c.known; dp.eps = m->z; dp.xk = m->keep_xk;
    z_out(dp, m);
    dp.n = (int)n; dp.fmin = m->cfg.feature_min; dp.fmax = m->cfg.feature_max;
    diffuse_coefs(m->h_coef[(size_t)c.start_step * kCoefCount + kCoefLogsnrT], &dp.alpha, &dp.sigma);
    launch_diffuse_to_step(dp, s);
    HIP_TRY(m, hipGetLastError());
  }
  if (c.known) {
    // the frames' release words: msd_sample_edit's as given; msd_sample_keep's flags (host or device) as 0 / 1
    HIP_TRY(m, hipMemcpyAsync(m->keep_flags, c.release ? c.release : c.mask, (size_t)c.batch * m->T * sizeof(int32_t), hipMemcpyDefault, s));
    if (!c.release) {
      launch_normalize_flags(m->keep_flags, m->keep_flags, c.batch * m->T, s);
      HIP_TRY(m, hipGetLastError());
    }
  }
  return MSD_OK;
}

// What a step reads in device memory besides z: the key table, the noise slot and the scan index (msd_profile_steps arms
// them the same way).  Returns with the stream idle: the host temporaries are on the stack.
// noise: the caller's [K][batch, T, n] buffer, or NULL = drawn INSIDE sampler_step_kernel (elementwise.h): step i's draw is
// sub-sequence 1 + i of the (seed, stream_id) Philox stream, bit-identical to a buffer of those rows (tests/test_gpu_model.py);
// MSD_RNG_THREEFRY: normal(fold_in(PRNGKey(seed), i), [batch, T, n]), what msd_fill_normal_threefry(seed, i, ...) writes.
// Per-row keys: row b of z draws under row b of the key table what a ONE-row call (seed_b, stream_b) draws.  Kind and mode
// are words of that table, so the same captured graphs serve every combination.
// reset_tickets (a sampling call): the in-launch merge's arrival counters are zero between launches by construction (the
// reducer resets its own); once per call in case an aborted launch left a count behind.
static int arm_scan(msd_model* m, int batch, int rng, const SampleKeys& keys, const float* noise, int start_step, bool reset_tickets, hipStream_t s) {
  HIP_TRY(m, upload_rng_keys(m, batch, rng, keys, s));
  if (reset_tickets) HIP_TRY(m, hipMemsetAsync(m->att_tickets, 0, (size_t)m->att_ticket_count * sizeof(int), s));
  HIP_TRY(m, hipMemcpyAsync(m->d_noise_slot, &noise, sizeof(float*), hipMemcpyHostToDevice, s));
  const int start[2] = {start_step, start_step};
  HIP_TRY(m, hipMemcpyAsync(m->d_step, start, sizeof(start), hipMemcpyHostToDevice, s));
  HIP_TRY(m, hipStreamSynchronize(s));
  return MSD_OK;
}

// `steps` consecutive steps of the view's form, captured on s and instantiated
static int capture_steps(msd_model* m, const StepView& view, const StepPlan& plan, int steps, hipStream_t s, hipGraphExec_t* out) {
  return capture_graph(m, s, "step graph", out, [&] {
    Ctx c{m, s};
    c.v = view;
    for (int k = 0; k < steps; ++k) enqueue_step(c, plan);
    return c.err == hipSuccess ? MSD_OK : fail(m, MSD_ERR_HIP, "step graph capture failed: %s", hipGetErrorString(c.err));
  });
}

static msd_model::GraphKey step_graph_key(const StepView& view, const StepPlan& plan) {
  return {plan, view.steps, view.sampler, view.keep, view.guided, view.invert};
}

// The graphs of (plan, view), from the handle's cache or captured now.  One graph = `graph_steps` consecutive steps (the
// scan index lives in device memory, so the same graph serves every position); a second, single-step graph covers what
// a call of view.steps steps, or this call of run_steps, leaves over.
static int find_graphs(msd_model* m, const StepView& view, const StepPlan& plan, int run_steps, hipStream_t s, msd_model::StepGraphs** out) {
  const msd_model::GraphKey key = step_graph_key(view, plan);
  msd_model::StepGraphs* g = m->graphs.find(key);
  if (__builtin_expect(!g, 0)) {   // (a capture is the rare path; said so, the compiler keeps it out of line as it was inside the one long function)
    m->graphs.make_room(1);
    msd_model::StepGraphs ng = {key};
    if (int rc = capture_steps(m, view, plan, m->graph_steps, s, &ng.exec)) return rc;
    if (m->graph_steps > 1 && view.steps % m->graph_steps)
      if (int rc = capture_steps(m, view, plan, 1, s, &ng.exec1)) { (void)hipGraphExecDestroy(ng.exec); return rc; }
    g = m->graphs.insert(ng);
  }
  // (msd_sample_edit's part-way start on a handle whose N is a whole number of graphs: on first need, in the same entry)
  if (m->graph_steps > 1 && run_steps % m->graph_steps && !g->exec1)
    if (int rc = capture_steps(m, view, plan, 1, s, &g->exec1)) return rc;
  *out = g;
  return MSD_OK;
}

static int replay(msd_model* m, const msd_model::StepGraphs& g, int steps, hipStream_t s) {
  for (int i = 0; i < steps / m->graph_steps; ++i) HIP_TRY(m, hipGraphLaunch(g.exec, s));
  for (int i = 0; i < steps % m->graph_steps; ++i) HIP_TRY(m, hipGraphLaunch(m->graph_steps > 1 ? g.exec1 : g.exec, s));
  return MSD_OK;
}

// msd_sample_resample: the key rows of passes 1 .. P of the call (pass p = everything behind its p-th jump; pass 0 is the
// call as arm_scan keys it), P = (times - 1) ceil(steps / jump), as one upload in front of the call's steps.
//   Philox    (seed, stream_id + (p << 32)): the jump draws sub-sequence 0, step i sub-sequence 1 + i
//   Threefry  key_p = fold_in(PRNGKey(seed), N + p - 1), the first fold indices the plain call leaves unused: the jump draws
//             normal(key_p, ...), step i normal(fold_in(key_p, i), ...) -- the sampler kernel folds i into the table's key
static int upload_pass_keys(msd_model* m, const SampleCall& c, int steps, hipStream_t s) {
  const size_t passes = (size_t)(c.times - 1) * (size_t)((steps - 1) / c.jump + 1);   // (no steps + jump: jump may be INT_MAX, "one block")
  const size_t words = passes * c.batch * kRngWords;
  if (int rc = grow(m, &m->d_pass_keys, &m->pass_keys_cap, words)) return rc;
  m->h_pass_keys.resize(words);   // a member: the copy below may still read it when this returns
  for (size_t p = 1; p <= passes; ++p)
    for (int b = 0; b < c.batch; ++b) {
      uint32_t* row = &m->h_pass_keys[((p - 1) * c.batch + b) * kRngWords];
      if (c.rng == MSD_RNG_PHILOX) {   // the pass in the stream id's upper word
        fill_rng_key(row, c.rng, c.keys.seed_of(b), c.keys.stream_of(b) + ((uint64_t)p << 32), c.keys.per_row());
      } else {   // the pass folded into the Threefry key words (the stream id does not enter this generator's key)
        fill_rng_key(row, c.rng, c.keys.seed_of(b), c.keys.stream_of(b), c.keys.per_row());
        uint32_t f0 = 0u, f1 = (uint32_t)(m->N + p - 1);
        threefry2x32(row[kRngTfKey0], row[kRngTfKey1], f0, f1);
        row[kRngTfKey0] = f0; row[kRngTfKey1] = f1;
      }
    }
  HIP_TRY(m, hipMemcpyAsync(m->d_pass_keys, m->h_pass_keys.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  return MSD_OK;
}

// The steps of a call with resampling jumps (RePaint): blocks of c.jump steps from level `steps` down (a level = the steps
// still to run; the last block may be shorter), every block descended c.times times; after each descent but the last
// the state is diffused from the block's bottom level back to its top (renoise_kernel, which also installs the next
// pass's keys and rewinds the scan index).  times * steps steps and (times - 1) ceil(steps / jump) jumps, all enqueued.
static int replay_resampled(msd_model* m, const SampleCall& c, const msd_model::StepGraphs& g, int steps, hipStream_t s) {
  const int n = c.batch * m->T * m->ND;
  int pass = 0;
  for (int top = steps; top > 0; top -= std::min(top, c.jump)) {
    const int bottom = std::max(top - c.jump, 0);
    for (int r = 0; r < c.times; ++r) {
      if (int rc = replay(m, g, top - bottom, s)) return rc;
      if (r == c.times - 1) break;
      ++pass;
      RenoiseParams rp;
      rp.z_in = m->z; rp.n = n;
      z_out(rp, m);
      renoise_coefs(m->h_coef, bottom, top, &rp.a, &rp.b);
      rp.keys = m->d_pass_keys + (size_t)(pass - 1) * c.batch * kRngWords;
      rp.row_blocks = row_blocks_of(m);
      rp.key_table = m->d_rng_key; rp.key_words = c.batch * kRngWords;
      rp.step_ptr = m->d_step; rp.next_step = top - 1;
      launch_renoise(rp, s);
      HIP_TRY(m, hipGetLastError());
    }
  }
  return MSD_OK;
}

// The steps of a call with guidance in an interval of the scan (msd_sample_guided): up to three runs of steps -- one-pass
// above guide_hi, guided inside [guide_lo, guide_hi), one-pass below guide_lo -- each whole graphs plus singles.  The scan
// index runs on in device memory across them (both plans publish it the same way) and so do z, its planes and the multistep
// form's x0_prev; nothing synchronises with the host in between.
// The call needs TWO sets of graphs at once, and a full cache is emptied in front of a capture, which destroys the graphs in
// it.  So room for every set that is missing is made BEFORE the first lookup -- no emptying can follow -- and both sets
// are held where they lie: an insertion leaves the cache's other entries in place (GraphCache).
static int replay_guided(msd_model* m, const SampleCall& c, const StepView& view, int steps, hipStream_t s) {
  const int runs[3] = {steps - c.guide_hi, c.guide_hi - c.guide_lo, c.guide_lo};   // one-pass, guided, one-pass
  StepView one = view, two = view;
  one.guided = false; two.guided = true;
  const StepPlan plan1 = plan_step(m, c.batch, 1, true, false), plan2 = plan_cfg_step(m, c.batch);
  const bool need1 = runs[0] + runs[2] > 0, need2 = runs[1] > 0;
  m->graphs.make_room((size_t)(need1 && !m->graphs.find(step_graph_key(one, plan1))) +
                      (size_t)(need2 && !m->graphs.find(step_graph_key(two, plan2))));
  msd_model::StepGraphs *g1 = nullptr, *g2 = nullptr;
  const int gs = m->graph_steps;
  if (need1)   // (the single-step graph: needed as soon as one of the two runs is no whole number of graphs)
    if (int rc = find_graphs(m, one, plan1, (runs[0] % gs || runs[2] % gs) ? 1 : gs, s, &g1)) return rc;
  if (need2)
    if (int rc = find_graphs(m, two, plan2, runs[1], s, &g2)) return rc;
  for (int r = 0; r < 3; ++r)
    if (runs[r] > 0)
      if (int rc = replay(m, r == 1 ? *g2 : *g1, runs[r], s)) return rc;
  return MSD_OK;
}

// z -> the caller's mel units; kept frames: the caller's own values, not a round trip through model units
static int unscale(msd_model* m, const SampleCall& c, hipStream_t s) {
  const int64_t n = (int64_t)c.batch * m->T * m->ND;
  if (c.known) launch_unscale_keep(m->z, c.known, m->keep_flags, c.out, (int)n, m->ND, m->cfg.feature_min, m->cfg.feature_max, s);
  else hipLaunchKernelGGL(unscale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, m->z, c.out, (int)n, m->cfg.feature_min, m->cfg.feature_max);
  HIP_TRY(m, hipGetLastError());
  return MSD_OK;
}

// the row weights travel next to the key table (arm_scan ends with the stream idle)
static int upload_row_weights(msd_model* m, const SampleCall& c, hipStream_t s) {
  m->h_row_wt.assign((size_t)m->Bmax, c.weights[0]);   // a member: the copy may still read it when this returns
  for (int b = 0; b < c.batch && c.n_weights > 1; ++b) m->h_row_wt[b] = c.weights[b];
  HIP_TRY(m, hipMemcpyAsync(m->d_row_wt, m->h_row_wt.data(), m->h_row_wt.size() * sizeof(float), hipMemcpyHostToDevice, s));
  return MSD_OK;
}

static int sample_body(msd_model* m, const SampleCall& c) {
  if (int rc = check_call(m, c)) return rc;
  const bool invert = c.invert_mel != nullptr;
  StepView view;
  if (int rc = make_step_view(m, c.steps, c.sampler, c.known != nullptr, &view, invert)) return rc;   // (+ the handle's buffers and tables)
  hipStream_t s;
  if (int rc = choose_stream(m, c.stream, &s)) return rc;
  // the steps the call runs: all of c.steps but for msd_sample_edit's part-way start (the inversion counts up from 0)
  const int steps = invert ? c.steps : c.start_step + 1;
  if (steps <= 0) {   // (msd_sample_edit: every frame known throughout) no step runs: the caller's mel
    HIP_TRY(m, hipMemcpyAsync(c.out, c.known, (size_t)c.batch * m->T * m->ND * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(m, hipStreamSynchronize(s));
    return MSD_OK;
  }
  if (int rc = arm_range(m, s)) return rc;
  if (int rc = write_initial_state(m, c, s)) return rc;
  if (c.times > 1)
    if (int rc = upload_pass_keys(m, c, steps, s)) return rc;
  if (c.weights)
    if (int rc = upload_row_weights(m, c, s)) return rc;
  // (the inversion's key table and noise slot are written as every call writes them; its kernel reads neither)
  if (int rc = arm_scan(m, c.batch, c.rng, c.keys, c.noise, c.start_step, /*reset_tickets=*/true, s)) return rc;
  msd_model::StepGraphs* g = nullptr;
  if (c.weights && !invert) {
    if (int rc = replay_guided(m, c, view, steps, s)) return rc;
  } else if (c.times == 1) {
    // (the inversion: one form of step throughout -- its kernel reads the row weights; the plan is the passes they need)
    const bool one_pass = invert && c.guide_lo == c.guide_hi;
    if (int rc = find_graphs(m, view, one_pass ? plan_step(m, c.batch, 1, true, false) : plan_cfg_step(m, c.batch), steps, s, &g)) return rc;
    if (int rc = replay(m, *g, steps, s)) return rc;
  } else {
    // (the single-step graph: needed as soon as one block is no whole number of graphs)
    const bool singles = c.jump % m->graph_steps || steps % c.jump % m->graph_steps;
    if (int rc = find_graphs(m, view, plan_cfg_step(m, c.batch), singles ? 1 : m->graph_steps, s, &g)) return rc;
    if (int rc = replay_resampled(m, c, *g, steps, s)) return rc;
  }
  if (invert) {   // z as it stands, in model units: the init_z of the call that renders the mel again
    HIP_TRY(m, hipMemcpyAsync(c.out, m->z, (size_t)c.batch * m->T * m->ND * sizeof(float), hipMemcpyDeviceToDevice, s));
  } else if (int rc = unscale(m, c, s)) {
    return rc;
  }
  // ONE stream synchronisation ends the call (tens of microseconds against a ~1 s segment); behind it the half-plane range flag is read: a bad run fails THIS call
  return check_range(m, s, invert ? "msd_invert" : "msd_sample");
}

// ---- the entry points: each checks what only it knows, fills the call and runs it ----------------------------------
int msd_sample(msd_model* m, int batch, uint64_t seed, uint64_t stream_id, const float* init_z_dev,
               const float* noise_dev, float* out_dev, void* stream) {
  return msd_sample_rng(m, batch, MSD_RNG_PHILOX, seed, stream_id, init_z_dev, noise_dev, out_dev, stream);
}

int msd_sample_rng(msd_model* m, int batch, int rng, uint64_t seed, uint64_t stream_id, const float* init_z_dev,
                   const float* noise_dev, float* out_dev, void* stream) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  return sample_body(m, plain_call(m, batch, rng, sample_keys(0, &seed, &stream_id), init_z_dev, noise_dev, out_dev, stream));
}

int msd_sample_rows(msd_model* m, int batch, int rng, const uint64_t* seeds, const uint64_t* stream_ids,
                    const float* init_z_dev, const float* noise_dev, float* out_dev, void* stream) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  if (!seeds) return fail(m, MSD_ERR_INVALID_ARGUMENT, "seeds is null");
  return sample_body(m, plain_call(m, batch, rng, sample_keys(1, seeds, stream_ids), init_z_dev, noise_dev, out_dev, stream));
}

int msd_sample_keep(msd_model* m, int batch, int rng, int per_row, const uint64_t* seeds, const uint64_t* stream_ids,
                    const float* init_z_dev, const float* noise_dev, const float* known_dev, const int32_t* keep_mask,
                    float* out_dev, void* stream) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  if (!seeds) return fail(m, MSD_ERR_INVALID_ARGUMENT, "seeds is null");
  if (!known_dev || !keep_mask) return fail(m, MSD_ERR_INVALID_ARGUMENT, "known mel or keep mask is null");
  SampleCall c = plain_call(m, batch, rng, sample_keys(per_row, seeds, stream_ids), init_z_dev, noise_dev, out_dev, stream);
  c.known = known_dev; c.mask = keep_mask;
  return sample_body(m, c);
}

// msd_sample_edit's checks and its call (msd_sample_resample shares them)
static int edit_call(msd_model* m, int batch, int rng, int per_row, const uint64_t* seeds, const uint64_t* stream_ids,
                     const float* init_z_dev, const float* noise_dev, const float* known_dev, const int32_t* release,
                     int start_step, float* out_dev, void* stream, SampleCall* out) {
  if (!seeds) return fail(m, MSD_ERR_INVALID_ARGUMENT, "seeds is null");
  if (!known_dev || !release) return fail(m, MSD_ERR_INVALID_ARGUMENT, "known mel or release words are null");
  if (batch < 1 || batch > m->Bmax) return fail(m, MSD_ERR_INVALID_ARGUMENT, "batch %d outside [1, %d]", batch, m->Bmax);
  const int N = m->N;
  if (start_step < -1 || start_step > N - 1)
    return fail(m, MSD_ERR_INVALID_ARGUMENT, "start_step %d outside [-1, %d]", start_step, N - 1);
  // a frame must be known at every step the call skips: free below scan index v - 1 <= start_step + 1 at the most
  const int v_lo = start_step < N - 1 ? 1 : 0, v_hi = start_step < N - 1 ? start_step + 2 : N;
  for (int64_t k = 0; k < (int64_t)batch * m->T; ++k) {
    const int v = release[k];
    if (v < 0 || v > N)
      return fail(m, MSD_ERR_INVALID_ARGUMENT, "release word %d of row %d, frame %d outside [0, %d]", v, (int)(k / m->T), (int)(k % m->T), N);
    if (v < v_lo || v > v_hi)
      return fail(m, MSD_ERR_INVALID_ARGUMENT, "release word %d of row %d, frame %d: a call that starts at scan index %d needs "
                  "every frame known at the steps it skips (words in [1, %d])", v, (int)(k / m->T), (int)(k % m->T), start_step, v_hi);
  }
  SampleCall c = plain_call(m, batch, rng, sample_keys(per_row, seeds, stream_ids), init_z_dev, noise_dev, out_dev, stream);
  c.known = known_dev; c.release = release; c.start_step = start_step;
  *out = c;
  return MSD_OK;
}

int msd_sample_edit(msd_model* m, int batch, int rng, int per_row, const uint64_t* seeds, const uint64_t* stream_ids,
                    const float* init_z_dev, const float* noise_dev, const float* known_dev, const int32_t* release,
                    int start_step, float* out_dev, void* stream) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  SampleCall c;
  if (int rc = edit_call(m, batch, rng, per_row, seeds, stream_ids, init_z_dev, noise_dev, known_dev, release, start_step, out_dev, stream, &c)) return rc;
  return sample_body(m, c);
}

int msd_sample_resample(msd_model* m, int batch, int rng, int per_row, const uint64_t* seeds, const uint64_t* stream_ids,
                        const float* init_z_dev, const float* known_dev, const int32_t* release, int start_step, int jump,
                        int times, float* out_dev, void* stream) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  SampleCall c;
  if (int rc = edit_call(m, batch, rng, per_row, seeds, stream_ids, init_z_dev, nullptr, known_dev, release, start_step, out_dev, stream, &c)) return rc;
  c.jump = jump; c.times = times;   // (checked with the rest of the call: check_call)
  return sample_body(m, c);
}

// msd_sample_steps' checks of the step count and the sampler, and its call (msd_sample_guided shares them); seeds: not null
static int steps_call(msd_model* m, int batch, int rng, int per_row, const uint64_t* seeds, const uint64_t* stream_ids,
                      const float* init_z_dev, const float* noise_dev, int num_steps, int sampler, float* out_dev,
                      void* stream, SampleCall* out) {
  if (int rc = check_num_steps(m, num_steps)) return rc;
  if (sampler != -1 && sampler != MSD_SAMPLER_DDPM && sampler != MSD_SAMPLER_DDIM && sampler != MSD_SAMPLER_DPMPP_2M)
    return fail(m, MSD_ERR_INVALID_ARGUMENT, "Unknown sampler type: %d", sampler);
  SampleCall c = plain_call(m, batch, rng, sample_keys(per_row, seeds, stream_ids), init_z_dev, noise_dev, out_dev, stream);
  if (num_steps > 0) { c.steps = num_steps; c.start_step = num_steps - 1; }   // (the handle's own are (N, cfg.sampler), however they were named)
  if (sampler >= 0) c.sampler = sampler;
  *out = c;
  return MSD_OK;
}

int msd_sample_steps(msd_model* m, int batch, int rng, int per_row, const uint64_t* seeds, const uint64_t* stream_ids,
                     const float* init_z_dev, const float* noise_dev, int num_steps, int sampler, float* out_dev,
                     void* stream) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  if (!seeds) return fail(m, MSD_ERR_INVALID_ARGUMENT, "seeds is null");
  SampleCall c;
  if (int rc = steps_call(m, batch, rng, per_row, seeds, stream_ids, init_z_dev, noise_dev, num_steps, sampler, out_dev, stream, &c)) return rc;
  return sample_body(m, c);
}

int msd_sample_guided(msd_model* m, int batch, int rng, int per_row, const uint64_t* seeds, const uint64_t* stream_ids,
                      const float* init_z_dev, const float* noise_dev, int num_steps, int sampler, const float* weights_host,
                      int n_weights, int guide_lo, int guide_hi, float* out_dev, void* stream) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  if (!seeds) return fail(m, MSD_ERR_INVALID_ARGUMENT, "seeds is null");
  if (batch < 1 || batch > m->Bmax) return fail(m, MSD_ERR_INVALID_ARGUMENT, "batch %d outside [1, %d]", batch, m->Bmax);
  SampleCall c;
  if (int rc = steps_call(m, batch, rng, per_row, seeds, stream_ids, init_z_dev, noise_dev, num_steps, sampler, out_dev, stream, &c)) return rc;
  bool all_one;
  if (int rc = check_row_weights(m, batch, weights_host, n_weights, /*one_pass_ok=*/false, &all_one)) return rc;
  const int K = c.steps;
  if (guide_lo == 0 && guide_hi == 0) guide_hi = K;   // the whole scan
  if (guide_lo < 0 || guide_lo >= guide_hi || guide_hi > K)
    return fail(m, MSD_ERR_INVALID_ARGUMENT, "guidance interval [%d, %d) is not inside the call's scan indices [0, %d)", guide_lo, guide_hi, K);
  if (int rc = ensure(m, &m->d_row_wt, (size_t)m->Bmax)) return rc;
  c.weights = weights_host; c.n_weights = n_weights; c.guide_lo = guide_lo; c.guide_hi = guide_hi;
  if (all_one) c.guide_lo = c.guide_hi = 0;   // every row follows the cond_wt == 1 branch: no guided step, K one-pass steps
  return sample_body(m, c);
}

// ---- msd_invert: deterministic DDIM inversion (kernel: invert_tail.h) --------------------------------------------------
// A sampling call on a scan that counts up (sample_body): the view with the inversion's side table, level 0 written from the
// mel, the scan words armed at 0, K steps of the one plan the weights need, z copied out.  No draw is made: the keys are Philox's zeros.
int msd_invert(msd_model* m, const msd_invert_args* a, void* stream) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  if (!a || a->struct_size != (int32_t)sizeof(msd_invert_args))
    return fail(m, MSD_ERR_INVALID_ARGUMENT, "msd_invert_args.struct_size %d != %d", a ? a->struct_size : 0, (int)sizeof(msd_invert_args));
  if (!a->mel_dev || !a->out_dev) return fail(m, MSD_ERR_INVALID_ARGUMENT, "mel_dev or out_dev is null");
  if (int rc = check_num_steps(m, a->num_steps)) return rc;
  static const float kWeightOne = 1.0f;   // no weights given: ONE weight of 1 (the table is uploaded all the same)
  const bool given = a->weights_host && a->n_weights != 0;
  bool all_one = true;
  if (given)
    if (int rc = check_row_weights(m, a->batch, a->weights_host, a->n_weights, /*one_pass_ok=*/true, &all_one)) return rc;
  const int64_t row_n = (int64_t)m->T * m->ND;
  if (row_n % 4) return fail(m, MSD_ERR_UNSUPPORTED, "the inversion needs targets_length * n_dims %% 4 == 0 (got %lld)", (long long)row_n);
  SampleCall c = plain_call(m, a->batch, MSD_RNG_PHILOX, SampleKeys(), nullptr, nullptr, a->out_dev, stream);
  c.steps = a->num_steps > 0 ? a->num_steps : m->N; c.start_step = 0; c.sampler = MSD_SAMPLER_DDIM; c.invert_mel = a->mel_dev;
  c.weights = given ? a->weights_host : &kWeightOne; c.n_weights = given ? a->n_weights : 1;
  c.guide_hi = all_one ? 0 : c.steps;   // (every weight 1: the one-pass plan at every step)
  return sample_body(m, c);
}

int msd_reset_graph(msd_model* m) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  m->graphs.clear();
  m->loss_graphs.clear();
  return MSD_OK;
}

int msd_set_touch_carrier(msd_model* m, int32_t touch_carrier) {
  if (!m || touch_carrier < 0 || touch_carrier > 2) return MSD_ERR_INVALID_ARGUMENT;
  m->cfg.touch_carrier = touch_carrier;
  m->touch_blocks = (touch_carrier ? touch_carrier : kTouchCarrierDefault) == 2;
  return MSD_OK;
}

int msd_decoder_pass(msd_model* m, int batch, int step_index, const float* z_dev,
                     int include_conditioning, float* eps_out_dev, void* stream) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  if (!m->encoded) return fail(m, MSD_ERR_BAD_STATE, "msd_encode has not run");
  if (batch != m->encoded_batch) return fail(m, MSD_ERR_INVALID_ARGUMENT, "batch != encoded batch");
  if (step_index < 0 || step_index >= m->N) return fail(m, MSD_ERR_INVALID_ARGUMENT, "step_index outside [0, N)");
  if (!z_dev || !eps_out_dev) return fail(m, MSD_ERR_INVALID_ARGUMENT, "null buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)batch * m->T * m->ND;
  const int st[2] = {step_index, step_index};
  if (int rc0 = arm_range(m, s)) return rc0;
  HIP_TRY(m, hipMemcpyAsync(m->d_step, st, sizeof(st), hipMemcpyHostToDevice, s));
  HIP_TRY(m, hipMemcpyAsync(m->z, z_dev, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIP_TRY(m, hipStreamSynchronize(s));
  split_z(m, n, s);
  Ctx c{m, s};
  decoder_eval(c, plan_step(m, batch, 1, include_conditioning != 0, false), /*publish_step=*/false);
  if (c.err != hipSuccess) return fail(m, MSD_ERR_HIP, "decoder pass failed: %s", hipGetErrorString(c.err));
  HIP_TRY(m, hipMemcpyAsync(eps_out_dev, m->eps, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return check_range(m, s, "msd_decoder_pass");   // synchronises
}

// ---- msd_loss: the denoising loss at time indices of the handle's grid (kernels: loss_tail.h) --------------------------
// One evaluation = (loss_diffuse_kernel, decoder_eval(publish_step = false), diffusion_loss_kernel), captured once per plan
// and replayed once per time: the time rows, the cursor and the keys live in device memory.
static int enqueue_loss_eval(msd_model* m, const StepPlan& plan, hipStream_t s) {
  const int n = plan.batch * m->T * m->ND;
  LossDiffuseParams dp;
  dp.call = m->d_loss_call; dp.x0 = m->loss_x0;
  z_out(dp, m);
  dp.keys = m->d_rng_key; dp.row_blocks = row_blocks_of(m); dp.n = n;
  dp.fmin = m->cfg.feature_min; dp.fmax = m->cfg.feature_max;
  dp.step_ptr = m->d_step;
  Ctx c{m, s};
  c.begin(KC_SAMPLER);
  launch_loss_diffuse(dp, s);
  c.end(KC_SAMPLER);
  decoder_eval(c, plan, /*publish_step=*/false);
  LossParams lp;
  lp.call = m->d_loss_call; lp.o = m->eps; lp.z = m->z; lp.x0 = m->loss_x0; lp.coef = m->d_coef;
  lp.keys = m->d_rng_key; lp.row_blocks = dp.row_blocks; lp.n = n; lp.passes = plan.P; lp.n_dims = m->ND;
  lp.model_output = m->cfg.model_output;
  c.begin(KC_SAMPLER);
  launch_diffusion_loss(lp, s);
  c.end(KC_SAMPLER);
  if (c.err != hipSuccess) return fail(m, MSD_ERR_HIP, "loss evaluation failed: %s", hipGetErrorString(c.err));
  return MSD_OK;
}

static int find_loss_graph(msd_model* m, const StepPlan& plan, hipStream_t s, hipGraphExec_t* out) {
  msd_model::LossGraphCache::Entry* g = m->loss_graphs.find(plan);
  if (!g) {
    m->loss_graphs.make_room(1);   // (the step graphs stay)
    msd_model::LossGraphCache::Entry ng = {plan};
    if (int rc = capture_graph(m, s, "loss graph", &ng.exec, [&] { return enqueue_loss_eval(m, plan, s); })) return rc;
    g = m->loss_graphs.insert(ng);
  }
  *out = g->exec;
  return MSD_OK;
}

int msd_loss(msd_model* m, const msd_loss_args* a, void* stream) {
  if (!m) return MSD_ERR_INVALID_ARGUMENT;
  if (!a || a->struct_size != (int32_t)sizeof(msd_loss_args))
    return fail(m, MSD_ERR_INVALID_ARGUMENT, "msd_loss_args.struct_size %d != %d", a ? a->struct_size : 0, (int)sizeof(msd_loss_args));
  // every refusal in front of any device work
  if (int rc = check_encoded_call(m, a->batch, a->rng, a->per_row != 0)) return rc;
  if (a->conditioning != MSD_LOSS_COND && a->conditioning != MSD_LOSS_UNCOND && a->conditioning != MSD_LOSS_BOTH)
    return fail(m, MSD_ERR_INVALID_ARGUMENT, "unknown conditioning %d", a->conditioning);
  if (a->loss_type < MSD_LOSS_X0 || a->loss_type > MSD_LOSS_X0_AND_EPS) return fail(m, MSD_ERR_INVALID_ARGUMENT, "Unknown diffusion loss_type: %d", a->loss_type);
  if (a->loss_norm != MSD_LOSS_L1 && a->loss_norm != MSD_LOSS_L2) return fail(m, MSD_ERR_INVALID_ARGUMENT, "Unknown diffusion loss norm: %d", a->loss_norm);
  if (a->n_times < 1) return fail(m, MSD_ERR_INVALID_ARGUMENT, "n_times %d < 1", a->n_times);
  if (!a->times_host || !a->target_dev || !a->out_dev || !a->seeds)
    return fail(m, MSD_ERR_INVALID_ARGUMENT, "times_host, target_dev, out_dev or seeds is null");
  for (int j = 0; j < a->n_times; ++j)
    if (a->times_host[j] < 0 || a->times_host[j] >= m->N)
      return fail(m, MSD_ERR_INVALID_ARGUMENT, "time index %d (entry %d) outside [0, %d)", a->times_host[j], j, m->N);
  if (m->ND % 4 || 1024 % m->ND)
    return fail(m, MSD_ERR_UNSUPPORTED, "the loss needs n_dims %% 4 == 0 and 1024 %% n_dims == 0 (got %d)", m->ND);
  if (a->conditioning == MSD_LOSS_BOTH && m->passes == 1)
    return fail(m, MSD_ERR_UNSUPPORTED, "a handle created with cfg_weight 1 holds one pass's buffers and takes conditioning %d or %d, not both (%d): "
                "create the handle with any weight != 1", (int)MSD_LOSS_COND, (int)MSD_LOSS_UNCOND, (int)MSD_LOSS_BOTH);
  // the handle's buffers, each on its own (a call after a failed allocation tries again for the one that is missing)
  const size_t time_words = (size_t)a->n_times * kLossTimeWords;
  if (int rc = ensure(m, &m->loss_x0, (size_t)m->Bmax * m->T * m->ND)) return rc;
  if (int rc = ensure(m, &m->d_loss_call, 1)) return rc;
  if (int rc = grow(m, &m->d_loss_times, &m->loss_times_cap, time_words)) return rc;
  hipStream_t s;
  if (int rc = choose_stream(m, stream, &s)) return rc;
  if (int rc = arm_range(m, s)) return rc;
  // the call's words: the time rows ((alpha, sigma) of the TRAIN schedule's log-SNR at the index, in double, rounded once),
  // the caller's buffers and the loss form, the cursor at 0; members: the copies below may still read them on return
  m->h_loss_times.assign(time_words, 0.f);
  for (int j = 0; j < a->n_times; ++j) {
    float* row = &m->h_loss_times[(size_t)j * kLossTimeWords];
    const int32_t i = a->times_host[j];
    diffuse_coefs(m->h_coef[(size_t)i * kCoefCount + kCoefMLogsnr], &row[kLossTimeAlpha], &row[kLossTimeSigma]);
    memcpy(&row[kLossTimeIndex], &i, sizeof(i));
  }
  HIP_TRY(m, hipMemcpyAsync(m->d_loss_times, m->h_loss_times.data(), time_words * sizeof(float), hipMemcpyHostToDevice, s));
  m->h_loss_call = LossCall{a->target_dev, a->mask_dev, a->eps_dev, a->out_dev, m->d_loss_times, a->loss_type, a->loss_norm, {0, 0}};
  HIP_TRY(m, hipMemcpyAsync(m->d_loss_call, &m->h_loss_call, sizeof(LossCall), hipMemcpyHostToDevice, s));
  HIP_TRY(m, upload_rng_keys(m, a->batch, a->rng, sample_keys(a->per_row, a->seeds, a->stream_ids), s));
  HIP_TRY(m, hipMemsetAsync(m->att_tickets, 0, (size_t)m->att_ticket_count * sizeof(int), s));
  // (no synchronisation here: every upload above reads a member of the handle, which outlives the call)
  const StepPlan plan = a->conditioning == MSD_LOSS_BOTH ? plan_cfg_step(m, a->batch)
                                                         : plan_step(m, a->batch, 1, a->conditioning == MSD_LOSS_COND, false);
  hipGraphExec_t exec = nullptr;
  if (int rc = find_loss_graph(m, plan, s, &exec)) return rc;
  for (int j = 0; j < a->n_times; ++j) HIP_TRY(m, hipGraphLaunch(exec, s));
  return check_range(m, s, "msd_loss");   // the call's single synchronisation
}

int msd_get_schedule(const msd_model* m, float* host_out) {
  if (!m || !host_out) return MSD_ERR_INVALID_ARGUMENT;
  if (!m->finalized) return fail(m, MSD_ERR_BAD_STATE, "not finalized");
  for (int i = 0; i < m->N; ++i) {
    const float* c = &m->h_coef[(size_t)i * kCoefCount];
    float* o = host_out + (size_t)i * 8;
    o[0] = c[kCoefLogsnrT]; o[1] = c[kCoefLogsnrS]; o[2] = c[kCoefX0Scale]; o[3] = c[kCoefX0Eps];
    o[4] = c[kCoefMeanZ]; o[5] = c[kCoefMeanX0]; o[6] = c[kCoefStd]; o[7] = c[kCoefMLogsnr];
  }
  return MSD_OK;
}

int msd_debug_read(msd_model* m, const char* buffer, float* host_out, int64_t max_elems, int64_t* n_out) {
  if (!m || !buffer || !host_out) return MSD_ERR_INVALID_ARGUMENT;
  const std::string b = buffer;
  if (b == "touch_blocks") {   // host state, no device access: touch blocks of the last self- / cross-attention launch enqueued
    if (n_out) *n_out = 2;
    for (int64_t i = 0; i < 2 && i < max_elems; ++i) host_out[i] = (float)m->ran_touch_blocks[i];
    return MSD_OK;
  }
  const float* f32 = nullptr;
  const Planes* pl = nullptr;
  int64_t count = 0;
  const int64_t Mmax = (int64_t)m->passes * m->Bmax * m->T;
  if (b == "film") { f32 = m->d_film; count = (int64_t)m->N * 2 * m->Ld * 2 * m->D; }
  else if (b == "coef") { f32 = m->d_coef; count = (int64_t)m->N * kCoefCount; }
  else if (b == "g_table") { f32 = m->d_g; count = (int64_t)m->N * 2 * m->Ld * m->D; }
  else if (b == "bw_self") { f32 = m->d_bw_self; count = (int64_t)m->N * m->Ld * 3 * m->J; }
  else if (b == "bw_mlp") { f32 = m->d_bw_mlp; count = (int64_t)m->N * m->Ld * 2 * m->F; }
  else if (b == "x") { f32 = m->x; count = Mmax * m->D; }
  else if (b == "eps") { f32 = m->eps; count = Mmax * m->ND; }
  else if (b == "z") { f32 = m->z; count = (int64_t)m->Bmax * m->T * m->ND; }
  else if (b == "loss_x0" && m->loss_x0) { f32 = m->loss_x0; count = (int64_t)m->Bmax * m->T * m->ND; }
  else if (b == "ssq") { f32 = m->ssq; count = Mmax * (m->D / kNarrowTile); }
  else if (b == "y") { pl = &m->y; count = Mmax * m->D; }
  else if (b == "qk") { pl = &m->qk; count = Mmax * 2 * m->J; }
  else if (b == "vt") { pl = &m->vt; count = Mmax * m->J; }
  else if (b == "ao") { pl = &m->ao; count = Mmax * m->J; }
  else if (b == "g") { pl = &m->g; count = Mmax * m->F; }
  else if (b == "cq") { pl = &m->cq; count = (int64_t)m->n_cross * m->Bmax * m->T * m->J; }
  // the second module (sum_cross_attends): conditional rows only, [Bmax T, J] each -- ao2 is allocated that size, and cq2
  // is the second half of cq's allocation (create), which is where the un-folded projection of module 1 writes
  else if (b == "ao2" && m->n_cross == 2 && m->ao2.p[0]) { pl = &m->ao2; count = (int64_t)m->Bmax * m->T * m->J; }
  else if (b == "cq2" && m->n_cross == 2 && m->cq2.p[0]) { pl = &m->cq2; count = (int64_t)m->Bmax * m->T * m->J; }
  else if (b == "xg" && m->fold_q) { pl = &m->xg; count = (int64_t)m->Bmax * m->T * m->D; }
  else if (b == "qp" && m->fold_q) { f32 = m->qp; count = (int64_t)m->Bmax * m->T * m->n_cross * m->J; }
  else if (b == "enc") { pl = &m->enc; count = (int64_t)m->S_pad * m->D; }
  else if (b == "cross_k") { pl = &m->kc; count = (int64_t)m->Ld * m->Bmax * m->S_pad * m->J; }
  else if (b == "cross_vt") { pl = &m->vtc; count = (int64_t)m->Ld * m->Bmax * m->S_pad * m->J; }
  else return fail(m, MSD_ERR_INVALID_ARGUMENT, "unknown debug buffer '%s'", buffer);
  if (n_out) *n_out = count;
  const int64_t n = count < max_elems ? count : max_elems;
  if (n <= 0) return MSD_OK;
  // A debug entry point: waits for the whole device (whatever stream the caller ran the model on), then copies and merges
  // planes through the handle's own stream like every other synchronous copy of the library -- never through the legacy
  // stream, whose operations fail while another thread captures a step graph on a blocking stream (the
  // library's own captures are hipStreamCaptureModeThreadLocal, under which another thread's device-wide wait is legal).
  HIP_TRY(m, hipDeviceSynchronize());
  if (f32) {
    HIP_TRY(m, copy_sync(m, host_out, f32, n * sizeof(float), hipMemcpyDeviceToHost));
  } else {
    float* tmp = nullptr;
    HIP_TRY(m, hipMalloc(&tmp, n * sizeof(float)));
    merge(*pl, tmp, n, m->own_stream);
    hipError_t e = copy_sync(m, host_out, tmp, n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(tmp);
    HIP_TRY(m, e);
  }
  return MSD_OK;
}

int msd_profile_steps(msd_model* m, int batch, int n_steps, const char* const** names_out,
                      double* ms_out, int64_t* launches_out, void* stream) {
  if (!m || !ms_out || !launches_out) return MSD_ERR_INVALID_ARGUMENT;
  if (!m->encoded || batch != m->encoded_batch) return fail(m, MSD_ERR_BAD_STATE, "msd_encode (same batch) must run first");
  if (n_steps < 1 || n_steps > m->N) return fail(m, MSD_ERR_INVALID_ARGUMENT, "n_steps outside [1, N]");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)batch * m->T * m->ND;
  StepView view;   // (a handle whose own sampler is the multistep form needs its side table and history buffer)
  if (int rcv = make_step_view(m, m->N, m->cfg.sampler, /*keep=*/false, &view)) return rcv;
  if (int rc0 = arm_range(m, s)) return rc0;
  int rc = msd_fill_normal(1, 0, 0, m->z, n, s);
  if (rc) return rc;
  split_z(m, n, s);
  // the sampler kernel draws the steps' noise itself (Philox stream (1, 0): elementwise.h)
  if (int rc1 = arm_scan(m, batch, kRngPhilox, SampleKeys{1}, /*noise=*/nullptr, m->N - 1, /*reset_tickets=*/false, s)) return rc1;
  for (int k = 0; k < KC_COUNT; ++k) { m->prof.ms[k] = 0; m->prof.launches[k] = 0; }
  m->prof.on = true;
  Ctx c{m, s};
  c.v = view;
  const StepPlan plan = plan_cfg_step(m, batch);
  for (int i = 0; i < n_steps; ++i) enqueue_step(c, plan);
  m->prof.on = false;
  if (c.err != hipSuccess) { (void)hipStreamSynchronize(s); return fail(m, MSD_ERR_HIP, "profile run failed: %s", hipGetErrorString(c.err)); }
  if (int rc2 = check_range(m, s, "msd_profile_steps")) return rc2;   // synchronises; the timed steps ran with the flag armed
  for (int k = 0; k < MSD_MAX_KERNEL_CLASSES; ++k) {
    ms_out[k] = k < KC_COUNT ? m->prof.ms[k] : 0.0;
    launches_out[k] = k < KC_COUNT ? m->prof.launches[k] : 0;
  }
  if (names_out) *names_out = kClassNames;
  return MSD_OK;
}

}  // extern "C"

#include "standalone_ops.h"   // the msd_op_* unit-test entry points; belongs to this file alone (see the file)

extern "C" {

// ---- device vocoder (vocoder.h): STFT pair, Audio2Mel, fast Griffin-Lim -------------------------------------------
extern "C++" {
namespace {
int vfail(msd_vocoder* v, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  v->err = buf;
  return code;
}
// first launch error of a call (a launch wrapper's own hipGetLastError clears the runtime's copy)
struct VocErr {
  hipError_t e = hipSuccess;
  bool operator()(hipError_t x) { if (e == hipSuccess) e = x; return x == hipSuccess; }
};
inline int voc_finish(msd_vocoder* v, VocErr& err, hipStream_t s, const char* what) {
  err(hipGetLastError());
  if (err.e == hipSuccess) err(hipStreamSynchronize(s));
  if (err.e != hipSuccess) return vfail(v, MSD_ERR_HIP, "%s: %s", what, hipGetErrorString(err.e));
  return MSD_OK;
}
}  // namespace
}  // extern "C++"

const char* msd_vocoder_last_error(const msd_vocoder* v) { return v ? v->err.c_str() : "null vocoder"; }

int msd_vocoder_create(const float* mel_basis_host, const float* mel_inverse_host, msd_vocoder** out) {
  if (!mel_basis_host || !mel_inverse_host || !out) return MSD_ERR_INVALID_ARGUMENT;
  msd_vocoder* v = new msd_vocoder();
  *out = v;   // kept alive on failure so that the caller can read the message
  std::vector<float> fwd, inv, inv_norm;
  voc_host_tables(fwd, inv, inv_norm);
  std::vector<float> mel((size_t)kVocHalf * kVocMel, 0.f), mel_inv((size_t)kVocMel * kVocMelInvN, 0.f);
  memcpy(mel.data(), mel_basis_host, (size_t)kVocBins * kVocMel * sizeof(float));
  for (int r = 0; r < kVocMel; ++r)
    memcpy(&mel_inv[(size_t)r * kVocMelInvN], mel_inverse_host + (size_t)r * kVocBins, kVocBins * sizeof(float));
  struct { float** dst; const std::vector<float>* src; } up[] = {
      {&v->fwd, &fwd}, {&v->inv, &inv}, {&v->inv_norm, &inv_norm}, {&v->mel, &mel}, {&v->mel_inv, &mel_inv}};
  for (auto& u : up) {
    const size_t bytes = u.src->size() * sizeof(float);
    if (hipMalloc(reinterpret_cast<void**>(u.dst), bytes) != hipSuccess ||
        hipMemcpy(*u.dst, u.src->data(), bytes, hipMemcpyHostToDevice) != hipSuccess)
      return vfail(v, MSD_ERR_HIP, "msd_vocoder_create: %s", hipGetErrorString(hipGetLastError()));
  }
  return MSD_OK;
}

void msd_vocoder_destroy(msd_vocoder* v) {
  if (!v) return;
  voc_free_work(v);
  for (float* p : {v->fwd, v->inv, v->inv_norm, v->mel, v->mel_inv})
    if (p) (void)hipFree(p);
  delete v;
}

int msd_vocoder_stft(msd_vocoder* v, int batch, int64_t n_samples, const float* audio_dev, float* spec_out_dev, void* stream) {
  if (!v || !audio_dev || !spec_out_dev || n_samples <= 0) return MSD_ERR_INVALID_ARGUMENT;
  const int64_t frames = (n_samples + kVocHop - 1) / kVocHop;
  if (!voc_shape_ok(batch, frames)) return vfail(v, MSD_ERR_INVALID_ARGUMENT, "msd_vocoder_stft: batch %d x %lld samples", batch, (long long)n_samples);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int F = (int)frames, rows = batch * (F + 1);
  if (!voc_reserve(v, rows, s)) return vfail(v, MSD_ERR_HIP, "msd_vocoder_stft: cannot allocate %d rows", rows);
  v->last_rows = (size_t)rows;
  VocErr err;
  voc_pad(v, batch, (int)n_samples, F, audio_dev, s);
  err(voc_forward(v, rows, EpiVocSpecOut{spec_out_dev, F}, s));
  return voc_finish(v, err, s, "msd_vocoder_stft");
}

int msd_vocoder_istft(msd_vocoder* v, int batch, int n_frames, const float* spec_dev, float* audio_out_dev, void* stream) {
  if (!v || !spec_dev || !audio_out_dev) return MSD_ERR_INVALID_ARGUMENT;
  if (!voc_shape_ok(batch, n_frames)) return vfail(v, MSD_ERR_INVALID_ARGUMENT, "msd_vocoder_istft: batch %d x %d frames", batch, n_frames);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int F = n_frames, rows = batch * (F + 1);
  if (!voc_reserve(v, rows, s)) return vfail(v, MSD_ERR_HIP, "msd_vocoder_istft: cannot allocate %d rows", rows);
  v->last_rows = (size_t)rows;
  hipLaunchKernelGGL(voc_load_spec_kernel, voc_grid_rows(rows), dim3(256), 0, s, spec_dev, (const float*)nullptr, v->w[VB_X], F, rows, 0);
  VocErr err;
  err(voc_inverse(v, batch, F, audio_out_dev, false, s));
  return voc_finish(v, err, s, "msd_vocoder_istft");
}

int msd_vocoder_encode(msd_vocoder* v, int batch, int64_t n_samples, const float* audio_dev, float* logmel_out_dev, void* stream) {
  if (!v || !audio_dev || !logmel_out_dev || n_samples <= 0) return MSD_ERR_INVALID_ARGUMENT;
  const int64_t frames = (n_samples + kVocHop - 1) / kVocHop;
  if (!voc_shape_ok(batch, frames)) return vfail(v, MSD_ERR_INVALID_ARGUMENT, "msd_vocoder_encode: batch %d x %lld samples", batch, (long long)n_samples);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int F = (int)frames, rows = batch * (F + 1);
  if (!voc_reserve(v, rows, s)) return vfail(v, MSD_ERR_HIP, "msd_vocoder_encode: cannot allocate %d rows", rows);
  v->last_rows = (size_t)rows;
  VocErr err;
  voc_pad(v, batch, (int)n_samples, F, audio_dev, s);
  err(voc_forward(v, rows, EpiF32Store{v->w[VB_Y0], kVocSpec}, s));
  hipLaunchKernelGGL(voc_magnitude_kernel, voc_grid_rows(rows - 1), dim3(256), 0, s, v->w[VB_Y0], v->w[VB_MAG], rows - 1);
  err(launch_gemm_f32(voc_gemm(v->w[VB_MAG], kVocHalf, v->mel, kVocMel, rows - 1, kVocMel, kVocHalf), EpiVocLogMel{logmel_out_dev, F}, s));
  return voc_finish(v, err, s, "msd_vocoder_encode");
}

int msd_vocoder_decode(msd_vocoder* v, int batch, int n_frames, const float* logmel_dev, int n_iters, float momentum,
                       uint64_t seed, const float* init_phase_dev, float* audio_out_dev, void* stream) {
  if (!v || !logmel_dev || !audio_out_dev || n_iters < 0) return MSD_ERR_INVALID_ARGUMENT;
  if (!voc_shape_ok(batch, n_frames)) return vfail(v, MSD_ERR_INVALID_ARGUMENT, "msd_vocoder_decode: batch %d x %d frames", batch, n_frames);
  if (!(momentum >= 0.f && momentum < 1e6f)) return vfail(v, MSD_ERR_INVALID_ARGUMENT, "msd_vocoder_decode: momentum %g", (double)momentum);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int F = n_frames, rows = batch * (F + 1);
  if (!voc_reserve(v, rows, s)) return vfail(v, MSD_ERR_HIP, "msd_vocoder_decode: cannot allocate %d rows", rows);
  v->last_rows = (size_t)rows;
  // target magnitudes: max(exp(log-mel) . pinv(mel basis), 0); the straddling rows and pad columns stay zero
  const int64_t n_mel = (int64_t)batch * F * kVocMel;
  VocErr err;
  err(hipMemsetAsync(v->w[VB_MAG], 0, (size_t)rows * kVocHalf * sizeof(float), s));
  hipLaunchKernelGGL(voc_exp_kernel, dim3((unsigned)((n_mel / 4 + 255) / 256)), dim3(256), 0, s, logmel_dev, v->w[VB_LIN], n_mel / 4);
  err(launch_gemm_f32(voc_gemm(v->w[VB_LIN], kVocMel, v->mel_inv, kVocMelInvN, batch * F, kVocMelInvN, kVocMel),
                      EpiVocClampMag{v->w[VB_MAG], F}, s));
  // X = mag . phase; Y_prev = 0 (a grown or reused buffer must not leak an earlier call's spectrum into the momentum)
  const float* phase = init_phase_dev;
  if (!phase) {
    if (msd_fill_normal(seed, 0x766F63ull, 0u, v->w[VB_DRAWS], (int64_t)batch * F * 2 * kVocBins, stream) != MSD_OK)
      return vfail(v, MSD_ERR_HIP, "msd_vocoder_decode: phase draw failed");
    phase = v->w[VB_DRAWS];
  }
  hipLaunchKernelGGL(voc_load_spec_kernel, voc_grid_rows(rows), dim3(256), 0, s, phase, (const float*)v->w[VB_MAG], v->w[VB_X], F, rows,
                     init_phase_dev ? 0 : 1);
  int cur = 0;
  err(hipMemsetAsync(v->w[VB_Y1], 0, (size_t)rows * kVocSpec * sizeof(float), s));
  const float alpha = momentum / (1.0f + momentum);
  for (int it = 0; it < n_iters; ++it) {
    if (!err(voc_inverse(v, batch, F, v->w[VB_AUDIO], true, s))) break;
    if (!err(voc_forward(v, rows, EpiF32Store{v->w[VB_Y0 + cur], kVocSpec}, s))) break;
    hipLaunchKernelGGL(voc_phase_kernel, voc_grid_rows(rows - 1), dim3(256), 0, s, (const float*)v->w[VB_Y0 + cur],
                       (const float*)v->w[VB_Y0 + (cur ^ 1)], (const float*)v->w[VB_MAG], v->w[VB_X], rows - 1, alpha);
    cur ^= 1;
  }
  if (err.e == hipSuccess) err(voc_inverse(v, batch, F, audio_out_dev, false, s));
  return voc_finish(v, err, s, "msd_vocoder_decode");
}

int msd_vocoder_debug_read(msd_vocoder* v, const char* buffer, float* host_out, int64_t max_elems, int64_t* rows_out) {
  if (!v || !buffer || !host_out || max_elems <= 0) return MSD_ERR_INVALID_ARGUMENT;
  static const struct { const char* name; VocBuf buf; } kNames[] = {
      {"audio", VB_AUDIO}, {"x", VB_X}, {"y0", VB_Y0}, {"y1", VB_Y1}, {"frames", VB_FRAMES}, {"mag", VB_MAG}};
  const float* src = nullptr;
  size_t per_row = 0;
  for (const auto& n : kNames)
    if (strcmp(buffer, n.name) == 0) { src = v->w[n.buf]; per_row = kVocPerRow[n.buf]; }
  if (per_row == 0) return vfail(v, MSD_ERR_INVALID_ARGUMENT, "msd_vocoder_debug_read: unknown buffer '%s'", buffer);
  if (v->last_rows == 0 || !src) return vfail(v, MSD_ERR_BAD_STATE, "msd_vocoder_debug_read: no call has run on this handle");
  if (rows_out) *rows_out = (int64_t)v->last_rows;
  const int64_t count = (int64_t)(v->last_rows * per_row), n = count < max_elems ? count : max_elems;
  // a debug entry point: waits for the whole device (the entry points synchronise their stream themselves), then copies
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host_out, src, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
    return vfail(v, MSD_ERR_HIP, "msd_vocoder_debug_read: %s", hipGetErrorString(hipGetLastError()));
  return MSD_OK;
}

}  // extern "C"

#include "keep_frames_tail.h"   // last on purpose: see the file
#include "multistep_tail.h"     // ... and behind it, for the same reason
#include "guided_tail.h"        // ... and the guided instances behind those
#include "loss_tail.h"          // ... and the two kernels of msd_loss behind everything
#include "invert_tail.h"        // ... and the inversion's instances behind those
