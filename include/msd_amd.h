/*
 * msd_amd.h -- C ABI of the MI355X-native DDPM spectrogram synthesizer.
 *
 * Drop-in boundary for ONE path of magenta/music-spectrogram-diffusion: the
 * denoising loop reached through InferenceModel.predict
 * (music_spectrogram_diffusion/inference.py:200-203) ->
 * {Diffusion,ContextDiffusion}Model.predict_batch_with_aux
 * (models/diffusion/models.py:149-205, 340-400) ->
 * diffusion_utils.eval_scan (models/diffusion/diffusion_utils.py:456-476) over
 * network.{Transformer,ContinuousContextTransformer}.{encode,decode}
 * (models/diffusion/network.py:460-606).
 *
 * The reference is pure Python/JAX: it has no FFI.  These entry points are what
 * a maintainer would bind (ctypes stub in INTEGRATION.md) to replace the jitted
 * `predict_fn(params, batch, rng)` of inference.py:183-198 -- one call group per
 * stage of predict_batch_with_aux.
 *
 * Conventions
 *   - plain C types only; every function returns an msd_status (0 = ok) and never
 *     throws; msd_last_error() gives the message for the last failure on a handle.
 *   - one handle <-> one device <-> one caller thread at a time (not re-entrant).  Handles are independent of each
 *     other: several may be created, loaded and run concurrently from different threads, also on ONE device (the
 *     library's own synchronous copies use a non-blocking stream of the handle, never the legacy stream).  This
 *     covers every msd_* entry point that takes a handle; the stand-alone msd_op_* building blocks (unit-test entry
 *     points, csrc/standalone_ops.h: they allocate, clear and copy scratch through the legacy stream) are NOT part of that guarantee -- do
 *     not call them while another thread captures or runs a model.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all
 *     device work is enqueued on it; calls return without synchronising unless
 *     stated.
 *   - "dev" pointers are device pointers owned by the caller (e.g. torch
 *     tensor.data_ptr()); "host" pointers are host memory.  Weights, caches,
 *     tables and graph objects are owned by the library.
 *   - tensors are dense row-major; float = IEEE binary32.
 */
#ifndef MSD_AMD_H_
#define MSD_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSD_AMD_ABI_VERSION 7   /* 7: msd_sample_rng, msd_fill_normal_threefry, msd_op_threefry (the reference's Threefry draws on the
                                      device); msd_config unchanged.  Appended to ABI 7 (no version bump): the msd_vocoder_*
                                      entry points (device STFT pair, Audio2Mel, Griffin-Lim); msd_sample_rows (one
                                      generator key per row of a batched call); msd_sample_keep and
                                      msd_op_sampler_step_keep (known frames in the sampler); msd_op_gemm_site and
                                      msd_op_gemm_site_tiles, msd_op_gemm_site_name (one GEMM launch site at a time, for the tests);
                                      msd_sample_edit, msd_op_sampler_step_release and msd_op_diffuse_to_step (edit strength:
                                      per-frame release words and a part-way start of the sampler);
                                      msd_sample_steps, msd_op_sampler_step_multistep and MSD_SAMPLER_DPMPP_2M (a step
                                      count per call and a second-order multistep sampler);
                                      msd_sample_resample and msd_op_renoise (known-frame edits with RePaint resampling
                                      jumps in the sampler scan);
                                      msd_sample_guided, msd_op_sampler_step_guided and
                                      msd_op_sampler_step_multistep_guided (a guidance weight per call or per row, applied
                                      in an interval of the scan); msd_loss and msd_op_diffusion_loss;
                                      msd_invert and msd_op_invert_step (deterministic DDIM inversion);
                                      msd_op_sampler_step_planes (a sampler update of any form with its operand planes,
                                      range flag and published scan index, for the tests);
                                      msd_op_vocoder_phase, msd_op_vocoder_load_spec and msd_vocoder_debug_read (the
                                      vocoder's phase update, its row layout and its work buffers, for the tests).
                                   6: cross_merge_in_launch, cross_q_fold, mlp_in_persistent appended to msd_config.
                                   5: dedup_layer0, cross_key_split, keep_raw_weights, kv_touch_ahead appended to msd_config.
                                   4: every caller-selectable knob is a msd_config field (attn_q_planes / attn_p_planes
                                      replace ABI 3's attn_query_planes; graph_steps; weight_prefetch): the library reads
                                      NO environment variable.  3: MSD_ERR_RANGE; distinct bfloat16-plane precisions */

typedef struct msd_model msd_model; /* opaque */

typedef enum msd_status {
  MSD_OK = 0,
  MSD_ERR_INVALID_ARGUMENT = 1, /* -> ValueError (unknown sampler/schedule/...:
                                   diffusion_utils.py:202,320,450; network.py:106,237,336) */
  MSD_ERR_UNKNOWN_WEIGHT = 2,   /* -> KeyError */
  MSD_ERR_SHAPE_MISMATCH = 3,   /* -> ValueError */
  MSD_ERR_BAD_STATE = 4,        /* call order violated -> RuntimeError */
  MSD_ERR_HIP = 5,              /* HIP runtime failure -> RuntimeError */
  MSD_ERR_UNSUPPORTED = 6,      /* valid in the reference, not built here -> NotImplementedError */
  MSD_ERR_RANGE = 7             /* an ACTIVATION left the range of the IEEE-half operand planes (|x| > 65504) during
                                   this call: its result is invalid.  The reference computes in float32
                                   (gin/models/diffusion/context/t5_base.gin:72) and has no such limit; the way out is
                                   the bfloat16-plane build (MSD_PREC_BF16X3, libmsd_amd_bf16.so) -> msd RangeError
                                   (an ArithmeticError) in the Python layer */
} msd_status;

/* Arithmetic of the transformer GEMMs / attention.  Residual stream, RMSNorm
 * statistics, softmax, FiLM, input/output projections and the sampler are always
 * fp32 (network.py:454; diffusion_utils.py:461). */
typedef enum msd_precision {
  MSD_PREC_F16 = 0,    /* one IEEE-half plane per operand (v_mfma_f32_*_f16), fp32 accumulate: fast, not parity-grade */
  MSD_PREC_F16X3 = 1,  /* operands split hi + lo half planes (22 significand bits), 3 MFMAs per product
                          (hi.hi + hi.lo + lo.hi): float32-class results -- the parity mode and the default.
                          The query side of the decoder's attentions may run on one plane: msd_config.attn_q_planes /
                          attn_p_planes.
                          Weights must satisfy |w| < 128 (packed times 2^9; checked by msd_finalize_weights ->
                          MSD_ERR_UNSUPPORTED); activations |x| <= 65504 (checked on every conversion ->
                          MSD_ERR_RANGE from the call that saw it). */
  MSD_PREC_BF16 = 2,   /* one bfloat16 plane per operand */
  MSD_PREC_BF16X3 = 3  /* hi + lo bfloat16 planes (16 significand bits, float32's exponent range: no range limit) */
  /* The plane FORMAT is a property of the library build: libmsd_amd.so implements the two half precisions,
   * libmsd_amd_bf16.so (same sources, same ABI) the two bfloat16 ones; msd_create returns MSD_ERR_UNSUPPORTED for a
   * precision of the other build (ABI <= 2 aliased the names and silently ran whatever planes the library had). */
} msd_precision;

typedef enum msd_sampler_kind {
  MSD_SAMPLER_DDPM = 0, /* diffusion_utils.py:382-395 */
  MSD_SAMPLER_DDIM = 1, /* diffusion_utils.py:369-379 */
  MSD_SAMPLER_DPMPP_2M = 2 /* (appended to ABI 7; not in the reference) DPM-Solver++(2M), data-prediction form: the
                              deterministic second-order multistep solver of the ODE ddim_step solves to first order;
                              see msd_sample_steps.  Valid in msd_config.sampler and as msd_sample_steps' argument. */
} msd_sampler_kind;

typedef enum msd_schedule_kind {
  MSD_SCHEDULE_COSINE = 0, /* diffusion_utils.py:181-187 */
  MSD_SCHEDULE_LINEAR = 1  /* diffusion_utils.py:189-199: betas linspace(start, stop, num_steps) */
} msd_schedule_kind;

typedef enum msd_model_output {
  MSD_OUTPUT_EPS = 0, /* diffusion_utils.py:296-300 */
  MSD_OUTPUT_X0 = 1,  /* :301-305 */
  MSD_OUTPUT_V = 2    /* :312-317 (x0_and_eps needs a 2n-channel network output, which the
                         reference's own Decoder (network.py:451-456) cannot produce: rejected) */
} msd_model_output;

typedef enum msd_logvar_kind {
  MSD_LOGVAR_LARGE = 0, /* diffusion_utils.py:146-149 */
  MSD_LOGVAR_SMALL = 1, /* :142-145 */
  MSD_LOGVAR_MEDIUM = 2 /* :150-157, "medium:<frac>" -> logvar_frac */
} msd_logvar_kind;

/* Hyper-parameters: network.T5Config (network.py:54-72), DiffusionConfig & co
 * (diffusion_utils.py:25-59), %TASK_FEATURE_LENGTHS (inference.py:97-101) and the
 * codec range (audio_codecs.py:207-213).  Fixed by construction on this path:
 * mlp_activations=("gelu","linear"), head_dim=64; anything else is rejected by the Python layer / msd_create. */
typedef struct msd_config {
  int32_t struct_size;            /* sizeof(msd_config), ABI check */
  int32_t has_context;            /* 0 DiffusionModel, 1 ContextDiffusionModel */
  int32_t vocab_size;
  int32_t emb_dim;
  int32_t num_heads;
  int32_t head_dim;
  int32_t mlp_dim;
  int32_t num_encoder_layers;
  int32_t num_decoder_layers;
  int32_t inputs_length;          /* L  */
  int32_t targets_length;         /* T  */
  int32_t context_length;         /* C (0 without context) */
  int32_t n_dims;                 /* mel bins */
  int32_t num_steps;              /* sampler schedule num_steps */
  int32_t sampler;                /* msd_sampler_kind */
  int32_t clip_x0;
  int32_t context_terminal_relative; /* T5Config.context_positions */
  int32_t precision;              /* msd_precision */
  int32_t max_batch;              /* largest `batch` accepted by encode/sample */
  float max_decoder_noise_time;
  float cfg_weight;               /* eval_condition_weight; 1.0 = single pass */
  float feature_min;              /* codec min_value */
  float feature_max;              /* codec max_value */
  /* ABI 2: the sampler / schedule branches of diffusion_utils.py (all step-indexed table work) */
  int32_t model_output;           /* msd_model_output: DiffusionConfig.model_output */
  int32_t logvar_type;            /* msd_logvar_kind: SamplerConfig.logvar_type */
  float logvar_frac;              /* the <frac> of "medium:<frac>", in [0, 1] */
  int32_t sampler_schedule;       /* msd_schedule_kind of SamplerConfig.schedule (num_steps above) */
  float sampler_schedule_start;   /* linear only */
  float sampler_schedule_stop;
  int32_t train_schedule;         /* msd_schedule_kind of DiffusionConfig.train_schedule: the log-SNR
                                     at which the model output is converted (diffusion_utils.py:294) */
  float train_schedule_start;     /* linear only */
  float train_schedule_stop;
  int32_t train_schedule_num_steps;
  int32_t cross_attend_sum;       /* T5Config.decoder_cross_attend_style: 0 = "concat_encodings" (every shipped
                                     gin), 1 = "sum_cross_attends" (the dataclass default, network.py:199-216:
                                     one cross-attention module per encoding, outputs summed) */
  /* ABI 4: the query side of the decoder's attentions in the two-plane modes (the memory side -- K, V -- always keeps
   * hi + lo).  0 = the library's choice (DESIGN.md 3 says which and why), 1 = one 16-bit plane, 2 = hi + lo. */
  int32_t attn_q_planes;          /* Q in q.k^T: one plane perturbs a logit by ~|s| 2^-12 -- fine for O(1) logits,
                                     not for sharp (trained) attention */
  int32_t attn_p_planes;          /* the softmax weights in P.V: one plane = 2^-12 relative on each weight, whatever
                                     the logits */
  int32_t graph_steps;            /* DDPM steps captured per hipGraph (0 = the library's choice, 8) */
  int32_t weight_prefetch;        /* producers warm the next GEMM's weights: 0 = the library decides from the model's
                                     size (on when a step streams more than the 256 MB Infinity Cache holds), 1 = on,
                                     2 = off */
  /* ABI 5 */
  int32_t dedup_layer0;           /* a CFG step computes decoder layer 0's self-attention block once for both passes
                                     (they are bit-identical up to the first cross-attention: models/diffusion/models.py:
                                     373-386): 0 = the library's choice (on), 1 = on, 2 = off (A/B and bitwise tests) */
  int32_t cross_key_split;        /* blocks that share the key axis of one (head, query tile) of the decoder's
                                     cross-attention: 0 = the library chooses per msd_encode from the segment's key
                                     count and the batch, else 1, 2, 4 or 8 */
  int32_t keep_raw_weights;       /* 0 = msd_finalize_weights frees the float32 staging copy of every matrix it has
                                     packed into operand planes (1.5 GB of 1.65 at base_with_context); 1 = keep them
                                     (they have no reader; for memory-accounting A/Bs) */
  int32_t kv_touch_ahead;         /* the cross-attention launches' prefetch wave touches the cached K / V^T lines this
                                     many 128-key ring stages ahead of their LDS-DMA (they are HBM-cold at every
                                     step): 0 = the library's choice (2, with one song per handle; batched launches
                                     are bandwidth-bound and never touch), -1 = off, 1 .. 16.  The touches ride on the
                                     launch's weight-prefetch wave: a cross-attention launch WITHOUT a weight target
                                     (weight_prefetch off -- the library's choice for models whose step fits the 256 MB
                                     cache, e.g. `small` / tiny presets -- or a module other than a layer's last) never
                                     touches, whatever this field says */
  /* ABI 6 */
  int32_t cross_merge_in_launch;  /* a key-split cross-attention finishes INSIDE its launch: every block publishes its
                                     partial write-through, the last block of a (query tile, head) group to arrive merges
                                     them -- no separate merge launch (one kernel boundary less per decoder layer);
                                     bit-identical to the merge launch.  0 = the library's choice (on), 1 = on, 2 = off */
  int32_t cross_q_fold;           /* the cross-attention's query projection has no launch of its own (one kernel boundary
                                     less per decoder layer).  Exact algebra on network.py:174-198: with x1 = x0 + ao . Wo,
                                     (x1 (.) gamma) . Wq = (x0 (.) gamma) . Wq + ao . (Wo diag(gamma) Wq) -- the first term
                                     rides on the QKV launch's idle CUs, the second runs beside the self-attention output
                                     projection (same A operand), and the 1/rms of the norm moves onto the logits inside
                                     the attention kernel.  Same float32-class result, NOT bit-identical to the unfolded
                                     order (3e-7 relative on a decoder pass).  Two-plane precisions, up to 1024 decoder
                                     rows per launch: single passes of up to 4 songs per call, CFG steps (both passes'
                                     rows) of up to 2.  0 = the library's choice (on), 1 = on, 2 = off */
  int32_t mlp_in_persistent;      /* batched songs (>= 4 per call: 128 x 128 tiles, several per CU): the decoder's gated-MLP
                                     input projection runs as ONE resident block per CU that walks its tiles, with the
                                     epilogue on the accumulator registers and the next tile's operands landing under
                                     it.  Same float32-class result, not bit-identical to the per-tile launch (another
                                     contraction of the epilogue's multiply-adds).  0 = the library's choice (on), 1 = on,
                                     2 = off */
  /* appended to ABI 7 (msd_create also takes the struct WITHOUT this field, at ABI 6's size: it then reads as 0) */
  int32_t touch_carrier;          /* who carries a launch's weight-prefetch touches at one song per call:
                                     1 = one extra wave inside every compute block of the carrier launch; 2 = touch blocks
                                     -- extra blocks behind the compute grid, on CUs the launch leaves idle, that do nothing
                                     but touch and end: the self- and the cross-attention launches carry their targets
                                     that way, and the cross-attention's in-block wave keeps its own K / V^T touch-ahead
                                     only.  Bit-identical results (a touch has no reader).  0 = the library's choice (2;
                                     DESIGN.md 6 says why).  Launches of more than one song per call, and every GEMM
                                     carrier, keep the in-block waves. */
} msd_config;

const char* msd_version(void);

/* Number of visible HIP devices (<0 on failure).  */
int msd_device_count(void);

/* Create a model on the CURRENT HIP device.  Allocates weights/caches/tables. */
int msd_create(const msd_config* cfg, msd_model** out);
void msd_destroy(msd_model* m);
const char* msd_last_error(const msd_model* m);

/* Parameter tree.  Names are the Flax names of the reference modules, '/'-joined
 * (e.g. "decoder/layers_3/FiLMLayer_0/DenseGeneral_0/kernel"); shapes as stored
 * by the reference ([in, out] kernels, layers.py:430-431).  `data` may be host or
 * device memory (hipMemcpyDefault; the copy runs on the handle's own stream and the call has no stream argument, so
 * a DEVICE-side `data` must be complete -- its producer stream synchronised -- before the call).  Weights are loaded
 * ONCE per handle: after msd_finalize_weights every msd_set_weight returns MSD_ERR_BAD_STATE.  Replaces the params
 * pytree handed to predict_fn (inference.py:197-203). */
int msd_num_weights(const msd_model* m);
int msd_weight_info(const msd_model* m, int index, const char** name, int64_t shape[2], int* ndim);
int msd_set_weight(msd_model* m, const char* name, const float* data,
                   const int64_t* shape, int ndim);
/* Pack weights for the kernels and build every step-indexed table (log-SNR and
 * sampler coefficients, time-embedding MLP, FiLM scale/bias).  Synchronises. */
int msd_finalize_weights(msd_model* m, void* stream);

/* module.encode of predict_batch_with_aux (models.py:365-371; network.py:537-559 /
 * 470-482): runs the token encoder (and context encoder: clip+scale to [-1,1],
 * models.py:361-363) once and caches the decoder's cross-attention K/V.
 *   tokens   int32 [batch, L]        (host or device)
 *   ctx      float [batch, C, n]     mel units (device), NULL without context
 *   ctx_mask int32 [batch, C]        (host or device), NULL without context
 * Synchronises `stream` at entry (device-side tokens / ctx_mask written on it are staged through the host) and before
 * it returns (half-plane range flag, like msd_sample). */
int msd_encode(msd_model* m, int batch, const int32_t* tokens, const float* ctx_dev,
               const int32_t* ctx_mask, void* stream);

/* eval_scan (diffusion_utils.py:456-476) + scale_to_features (models.py:395).  SYNCHRONISES `stream` before it
 * returns (ABI 3): behind that one wait it reads the handle's half-plane range flag, so that a run whose
 * activations left the plane range fails THIS call with MSD_ERR_RANGE instead of handing back a wrong spectrogram.
 *   init_z_dev float [batch,T,n] or NULL  -> generated (Philox, see msd_fill_normal)
 *   noise_dev  float [N,batch,T,n] or NULL -> generated; noise_dev[i] is the draw
 *              used at scan index i (diffusion_utils.py:389-390).  NULL: the sampler kernel draws step i's noise
 *              itself (sub-sequence 1 + i of msd_fill_normal's generator: no [N,batch,T,n] buffer exists; the
 *              values are those msd_fill_normal(seed, stream_id, 1 + i, ...) writes, bit for bit)
 *   stream     NULL = the legacy stream: the call waits for it (hipStreamSynchronize(NULL)) and runs on the handle's
 *              own stream (the legacy stream cannot be captured); other handles' streams are not waited for
 *   seed/stream_id key the generator when a pointer is NULL (stream_id = segment)
 *   out_dev    float [batch,T,n] mel units
 * The generator is the library's own (Philox); msd_sample_rng names another.  */
int msd_sample(msd_model* m, int batch, uint64_t seed, uint64_t stream_id,
               const float* init_z_dev, const float* noise_dev, float* out_dev,
               void* stream);

/* ABI 7: the generator of the NULL pointers.  MSD_RNG_PHILOX is the library's own (msd_fill_normal);
 * MSD_RNG_THREEFRY makes the draws of the reference's `predict(batch, seed)` -- jax.random with the default
 * (non-partitionable) Threefry layout of jax <= 0.4 -- on the device, with no noise buffer and no host work. */
enum { MSD_RNG_PHILOX = 0, MSD_RNG_THREEFRY = 1 };
/* msd_sample with the generator named; msd_sample(...) == msd_sample_rng(..., MSD_RNG_PHILOX, ...).
 * MSD_RNG_THREEFRY: init_z = normal(PRNGKey(seed), [batch,T,n]), step i = normal(fold_in(PRNGKey(seed), i), [batch,T,n])
 * (inference.py:203, diffusion_utils.py:389-390,462), drawn inside the sampler kernel; the values are those
 * msd_fill_normal_threefry(seed, -1 / i, ..., batch*T*n) writes, bit for bit.  One draw covers the WHOLE [batch,T,n] array, as
 * in the reference: row b of a batched call is not the draw of a one-row call (msd_sample_rows keys every row on its
 * own).  stream_id is ignored, as the reference
 * ignores the segment (beam/evaluation.py:209-210).  An unknown rng is MSD_ERR_INVALID_ARGUMENT.  A DDIM sampler
 * uses init_z only.  The step graphs are shared by both generators (the kind lives in device memory). */
int msd_sample_rng(msd_model* m, int batch, int rng, uint64_t seed, uint64_t stream_id,
                   const float* init_z_dev, const float* noise_dev, float* out_dev, void* stream);

/* (appended to ABI 7) msd_sample_rng with one generator key PER ROW: row b of the call draws, bit for bit, what the
 * ONE-row call msd_sample_rng(m, 1, rng, seeds[b], stream_ids[b], NULL, NULL, ...) draws, whatever the other rows are
 * -- independent segments (and songs) share one call and keep their own noise.  With R = T * n_dims elements per row:
 *   MSD_RNG_PHILOX    init_z row b = msd_fill_normal(seeds[b], stream_ids[b], 0, ..., R); step i's noise of row b is what the
 *                     three-argument form msd_fill_normal(seeds[b], stream_ids[b], 1 + i, ..., R) writes: counter block
 *                     e / 4 of element e INSIDE the row, sub-sequence 1 + i
 *   MSD_RNG_THREEFRY  init_z row b = normal(PRNGKey(seeds[b]), [1,T,n]) = msd_fill_normal_threefry(seeds[b], -1, ..., R);
 *                     step i = normal(fold_in(PRNGKey(seeds[b]), i), [1,T,n]) = msd_fill_normal_threefry(seeds[b], i, ..., R)
 *   seeds      host uint64 [batch]; NULL is MSD_ERR_INVALID_ARGUMENT
 *   stream_ids host uint64 [batch] (the segment of each row), or NULL = zeros (MSD_RNG_THREEFRY ignores it)
 * init_z_dev / noise_dev, when given, take precedence exactly as in msd_sample_rng; every other argument, check and
 * status is msd_sample_rng's.  The keys travel in device memory beside the generator kind: the step graphs captured by
 * msd_sample / msd_sample_rng serve this call too and nothing is re-captured.  Rows must be a whole number of 1024
 * elements (R % 1024 == 0, true of every shipped configuration); otherwise MSD_ERR_UNSUPPORTED. */
int msd_sample_rows(msd_model* m, int batch, int rng, const uint64_t* seeds, const uint64_t* stream_ids,
                    const float* init_z_dev, const float* noise_dev, float* out_dev, void* stream);

/* (appended to ABI 7) Sampling with KNOWN frames: regenerate part of a segment and keep the rest (x0-replacement).
 *   known_dev  float [batch,T,n] mel units (device): the frames to keep; the values of the other frames are not used
 *   keep_mask  int32 [batch,T], host or device: non-zero = frame t of row b is known.  Per frame only.
 * The known mel is brought to model units as the context is (scale_features(clip=True)): xk.  In EVERY scan step, after
 * the CFG combine and after the clip_x0 branch, the kept elements get
 *     pred_x0 := xk     pred_eps := predict_eps_from_x0(z_t, xk, logsnr_t)
 * and the ordinary ddpm_step / ddim_step runs: they follow the posterior q(z_s | z_t, x0 = xk), carry the noise level of
 * their step (the free frames see them through self-attention at that level) and arrive at xk at scan index 0.  init_z
 * and every noise draw are what the call without a mask makes; resampling jumps (RePaint): msd_sample_resample.  out_dev gets the
 * CALLER's values on kept frames, bit for bit (also values outside the codec's range, which xk clips), and the sampled
 * mel on the others.  An all-zero mask gives msd_sample_rng's / msd_sample_rows' result bit for bit.
 *   per_row = 0: ONE draw over the whole array under (seeds[0], stream_ids[0]) -- msd_sample_rng's keying
 *   per_row != 0: msd_sample_rows' keying, seeds / stream_ids host uint64 [batch]
 *   stream_ids may be NULL (zeros); seeds, known_dev or keep_mask NULL is MSD_ERR_INVALID_ARGUMENT
 * Every other argument, check and status is theirs; n_dims % 4 != 0 is MSD_ERR_UNSUPPORTED.  The scaled mel and the flags
 * live in buffers the handle owns (allocated by the first such call); the step graphs of this form are captured and
 * cached beside the plain ones, by (step plan, keep): plain calls before and after replay their own graphs unchanged. */
int msd_sample_keep(msd_model* m, int batch, int rng, int per_row, const uint64_t* seeds, const uint64_t* stream_ids,
                    const float* init_z_dev, const float* noise_dev, const float* known_dev, const int32_t* keep_mask,
                    float* out_dev, void* stream);

/* (appended to ABI 7) Edit strength: msd_sample_keep with a RELEASE SCHEDULE per frame and a start part-way down the scan.
 *   release    HOST int32 [batch,T], one word v per frame, 0 <= v <= num_steps:
 *                v == 0   the frame is free at every step (msd_sample_keep's flag 0)
 *                v >= 1   the frame is known (x0-replacement, as above) at scan indices i >= v - 1 and free below: the
 *                         sampler has the last f = v - 1 steps to move it.  v == 1: known throughout (flag 1); it alone
 *                         comes back as the caller's values -- a released frame returns what the scan made of it
 *   start_step the scan index of the first step that runs, in [-1, num_steps - 1]; the call runs start_step + 1 steps
 *                start_step == num_steps - 1   z starts as init_z.  With words in {0, 1} this IS msd_sample_keep, bit for bit
 *                0 <= start_step < num_steps - 1   z starts as a direct sample of q(z_t | x0 = xk) at the start index
 *                         (the reference's diffusion_forward, diffusion_utils.py:109-117):
 *                             z = fmaf(sigma, eps, alpha * xk),  alpha = sqrt(sigmoid(logsnr_t)), sigma = sqrt(sigmoid(-logsnr_t))
 *                         of the SAMPLER schedule's logsnr_t of that index (float32 table value; alpha, sigma computed in double
 *                         and rounded once); eps = the call's own initial draw: init_z_dev if given, else what msd_sample_rng /
 *                         msd_sample_rows would have started from.  Every frame must be known at every skipped step:
 *                         1 <= v <= start_step + 2
 *                start_step == -1   only with every word 1: no step runs, out_dev = known_dev
 * Violations, and a NULL known_dev / release / seeds, are MSD_ERR_INVALID_ARGUMENT with a message.  The steps' noise is
 * indexed by scan index exactly as in the full call (noise_dev stays [num_steps][batch,T,n]).  Rows share start_step; a row
 * that should move less is held by its words.  start_step + 1 steps = whole step graphs of msd_sample_keep's set plus
 * single-step launches; the single-step graph is captured on first need.  Everything else is msd_sample_keep's. */
int msd_sample_edit(msd_model* m, int batch, int rng, int per_row, const uint64_t* seeds, const uint64_t* stream_ids,
                    const float* init_z_dev, const float* noise_dev, const float* known_dev, const int32_t* release,
                    int start_step, float* out_dev, void* stream);

/* (appended to ABI 7) msd_sample_edit with RESAMPLING JUMPS (RePaint, Lugmayr et al. 2022): the scan goes down a block of
 * steps, diffuses the state back up and comes down again, so that the free frames get several chances to condition on the
 * known frames at the same noise level.  A LEVEL is the number of steps still to run: the step with scan index i takes
 * level i + 1 to level i, and the call starts at level S = start_step + 1.
 *   jump, times  block k = 0, 1, ... has top S - k jump and bottom max(top - jump, 0) (the last block may be shorter).  Every
 *                block is descended `times` times; after each descent but the last the state is diffused from the block's
 *                bottom level s back to its top level t -- one sample of q(z_t | z_s), known and free frames alike:
 *                    z' = fmaf(b, eps, a * z),  a = alpha_t / alpha_s,  b = sqrt(1 - a^2)
 *                alpha = sqrt(sigmoid(logsnr)) of the SAMPLER schedule's float32 table value at the level (level L > 0: scan
 *                index L - 1's logsnr_t; level 0: scan index 0's logsnr_s, where z holds x0); a, b computed in double and
 *                rounded once.  The call runs times * S steps and (times - 1) ceil(S / jump) jumps.  The release words keep
 *                their meaning in every descent: known at scan indices i >= v - 1.  jump < 1 or times < 1 is
 *                MSD_ERR_INVALID_ARGUMENT; times == 1 is msd_sample_edit(..., noise_dev = NULL, ...) bit for bit, whatever jump.
 *   draws        pass p = everything behind the call's p-th jump (pass 0: the call as msd_sample_edit keys it) has a key of
 *                its own; its jump draws what that key's initial draw would be, its steps what that key's steps would draw.
 *                MSD_RNG_PHILOX: (seed, stream_id + (p << 32)) -- eps = sub-sequence 0 (msd_fill_normal's bits), step i's
 *                noise sub-sequence 1 + i; with times > 1 every stream_id must be < 2^32 (MSD_ERR_INVALID_ARGUMENT).
 *                MSD_RNG_THREEFRY: key_p = fold_in(PRNGKey(seed), num_steps + p - 1), the first fold indices the plain call
 *                does not use -- eps = normal(key_p, [batch | 1, T, n]), step i's noise normal(fold_in(key_p, i), ...).
 *                Per-row keys: row b draws, in every pass, what its one-row call draws.  The extra draws are made on the
 *                device, so there is no noise_dev; init_z_dev keeps its meaning for pass 0.
 * Nothing synchronises with the host between passes: all passes' keys are uploaded once, the jump kernel installs its
 * pass's keys and rewinds the device scan index, the descents replay msd_sample_keep's cached graphs (a jump that is a
 * multiple of graph_steps runs on whole graphs) and the call ends with its one synchronisation.  Every other argument,
 * check and status is msd_sample_edit's; an MSD_SAMPLER_DPMPP_2M handle stays MSD_ERR_UNSUPPORTED. */
int msd_sample_resample(msd_model* m, int batch, int rng, int per_row, const uint64_t* seeds, const uint64_t* stream_ids,
                        const float* init_z_dev, const float* known_dev, const int32_t* release, int start_step, int jump,
                        int times, float* out_dev, void* stream);

/* (appended to ABI 7) A step count and a sampler PER CALL: preview in 50 steps, render in 1000, on one handle.
 *   num_steps  K: 0 = the handle's N = msd_config.num_steps; else K must DIVIDE N (MSD_ERR_INVALID_ARGUMENT otherwise, with
 *              the divisors of N in the message)
 *   sampler    -1 = the handle's; else MSD_SAMPLER_DDPM, MSD_SAMPLER_DDIM or MSD_SAMPLER_DPMPP_2M
 * The call runs the scan of eval_scan (diffusion_utils.py:456-476) with sampler.schedule.num_steps = K: scan indices
 * j = K - 1 .. 0, t = (j + 1) / K, s = j / K.  Everything else is the handle's configuration: train schedule, model output,
 * CFG weight, clip, logvar type.  For the cosine sampler schedule that IS the reference configured with K steps.  For a
 * LINEAR sampler schedule it is not: the reference would rebuild its beta grid with K knots, whereas this call evaluates
 * the handle's N-knot schedule function at t = (j + 1) / K and j / K (the same noise levels as the N-step call, visited
 * more coarsely).
 *   How: the time (j + 1) / K is the time (r + 1) / N of row r = (j + 1) N / K - 1 of the handle's step-indexed tables --
 *   the same rational, correctly rounded, hence the same float32 -- so the time embedding's FiLM tables are read at row
 *   offset N / K - 1 with N / K times the row stride; no table is rebuilt.  The sampler's own K coefficient rows are
 *   built on the first call with that K and kept.  The scan index in device memory is j: the noise of step j is Philox
 *   sub-sequence 1 + j, Threefry fold_in(key, j), or row j of noise_dev -- the draws of a handle created with
 *   num_steps = K.
 *   noise_dev, when given, is [K][batch,T,n].
 * MSD_SAMPLER_DPMPP_2M, with lambda = logsnr / 2 of the sampler schedule, h = lambda_s - lambda_t, r = h_prev / h:
 *     D   = x0_t                                    on the first step of a call
 *     D   = (1 + 1/(2r)) x0_t - (1/(2r)) x0_prev    afterwards
 *     z_s = (sigma_s / sigma_t) z_t - alpha_s expm1(-h) D         scan index 0 returns x0_t
 * x0_t = the step's pred_x0 after the model-output conversion, the CFG combine and the clip.  With D = x0_t this is
 * ddim_step; no draw is made after init_z (noise_dev is ignored).  The history lives in a buffer the handle owns.
 * Keying (per_row, seeds, stream_ids), the stream rules, the range flag and the final synchronisation are
 * msd_sample_keep's.  Step graphs are cached by (step plan, keep, K, sampler), eight sets at the most; K % graph_steps
 * steps run as single-step launches.  num_steps in {0, N} with sampler in {-1, msd_config.sampler} IS msd_sample_rng /
 * msd_sample_rows: the same path, the same cached graphs, the same bits. */
int msd_sample_steps(msd_model* m, int batch, int rng, int per_row, const uint64_t* seeds, const uint64_t* stream_ids,
                     const float* init_z_dev, const float* noise_dev, int num_steps, int sampler,
                     float* out_dev, void* stream);

/* (appended to ABI 7) The classifier-free guidance weight PER CALL, per row, and in a limited interval of the scan: what
 * msd_config.cfg_weight fixes for the life of a handle becomes an argument, on one handle and one set of graphs.
 *   weights_host  n_weights finite host floats; n_weights = 1 (every row) or batch (row b takes weights_host[b])
 *   guide_lo, guide_hi   scan indices of the call's K steps, 0 <= guide_lo < guide_hi <= K; 0, 0 = the whole scan [0, K)
 *   num_steps, sampler   msd_sample_steps' (0 / -1 = the handle's own); the other arguments are that call's too
 * Row b at scan index i is eval_step.body (diffusion_utils.py:397-452) with eval_condition_weight = w[b] where
 * guide_lo <= i < guide_hi and with eval_condition_weight = 1 elsewhere (Kynkaanniemi et al. 2024, "Applying guidance in a
 * limited interval improves sample and distribution quality in diffusion models").  The == 1 branch is the reference's: ONE
 * decoder pass, no combine, pred_x0 not recomputed from eps at the sampler schedule.  A row whose weight is exactly 1
 * follows that branch inside the interval as well, so row b of any call is its one-row call.  MSD_SAMPLER_DPMPP_2M keeps
 * its x0_prev history through the interval's edges.
 *   How: inside the interval the step is the handle's two-pass step with the sampler's guided kernels, which read the
 *   row's weight from a device table the handle owns (uploaded per call next to the key table), so one captured graph
 *   serves every weight vector; a scalar weight w gives the bits of a handle created with cfg_weight = w.  Outside it the
 *   step runs the one-pass plan (msd_decoder_pass's) with the kernels the library always had: half the rows in every
 *   launch.  Up to three runs of steps (above guide_hi, inside, below guide_lo), each whole graphs plus single steps,
 *   replay without a host round trip; the call ends with its one synchronisation and range check.  All weights == 1
 *   runs K one-pass steps.
 * Not built: known frames (msd_sample_keep / _edit / _resample take no guidance), per-frame weights, and handles created
 * with cfg_weight == 1 (they hold one pass's buffers: MSD_ERR_UNSUPPORTED -- create the handle with any weight != 1).
 * Per-row weights need targets_length * n_dims % 1024 == 0 (MSD_ERR_UNSUPPORTED otherwise), as per-row keys do. */
int msd_sample_guided(msd_model* m, int batch, int rng, int per_row, const uint64_t* seeds, const uint64_t* stream_ids,
                      const float* init_z_dev, const float* noise_dev, int num_steps, int sampler,
                      const float* weights_host, int n_weights, int guide_lo, int guide_hi, float* out_dev,
                      void* stream);

/* Drop the captured hipGraph of the DDPM step; the next msd_sample captures it again. */
int msd_reset_graph(msd_model* m);

/* (appended to ABI 7) msd_config.touch_carrier of a live handle: 0 = back to the library's choice, 1, 2.  The step plan
 * -- which is the key of the captured graphs -- follows at the next sampling call; graphs of the other form stay cached
 * until msd_reset_graph.  Not while a sampling call of this handle is in flight. */
int msd_set_touch_carrier(msd_model* m, int32_t touch_carrier);

/* One decoder call of the scan body: pred_fn(z, time=(i+1)/N, include_conditioning)
 * (models.py:373-386 -> network.py:561-573).  For parity tests and profiling.
 *   z_dev float [batch,T,n]; eps_out_dev float [batch,T,n]                     */
int msd_decoder_pass(msd_model* m, int batch, int step_index, const float* z_dev,
                     int include_conditioning, float* eps_out_dev, void* stream);

/* The library's counter-based normal generator: Philox4x32-10, key
 * (seed_lo, seed_hi), counter (elem/4, stream_id_lo, stream_id_hi|..., subseq),
 * Box-Muller; documented in DESIGN.md and restated in oracle/philox.py.
 * subseq: 0 = init_z, 1 + i = step-i noise.                                   */
int msd_fill_normal(uint64_t seed, uint64_t stream_id, uint32_t subseq,
                    float* out_dev, int64_t n, void* stream);

/* jax.random.normal(key, [n]) (float32) for key = PRNGKey(seed), or fold_in(PRNGKey(seed), fold) when fold >= 0:
 * threefry2x32-20, element e < ceil(n/2) = word 0 of block (e, e + ceil(n/2)), the others word 1 (an odd n pads the
 * last counter with 0); uniform in [nextafter(-1,0), 1) by the mantissa trick; sqrt(2) * XLA's float32 erf^-1, every
 * operation rounded on its own.  Restated on the host in jax_random.py; n < 2^32, fold < 2^32. */
int msd_fill_normal_threefry(uint64_t seed, int64_t fold, float* out_dev, int64_t n, void* stream);

/* Step-indexed tables, for parity tests: copies [num_steps, 8] floats to host:
 * {logsnr_t, logsnr_s, x0_scale, x0_eps_coef, mean_z_coef, mean_x0_coef, std,
 *  logsnr of the TRAIN schedule at t (model-output conversion)}. */
int msd_get_schedule(const msd_model* m, float* host_out);

/* Read an internal buffer as float (bf16 widened) into host memory, for tests.
 * Returns the element count in *n_out; copies min(count, max_elems).  Synchronises.
 * Among the buffers: the encode stage's "enc" [S_pad][D] (the LAST encoded row's encodings), "cross_k"
 * [Ld][Bmax][S_pad][J] and "cross_vt" [Ld][Bmax][J][S_pad] (keys permuted within every 16: gemm_h16.h vt_perm16), and the
 * load-time tables "film" [N][2 Ld][2 D], "g_table" [N][2 Ld][D] = gamma (film_scale + 1), "bw_self" [N][Ld][3 J] =
 * film_bias_self . (Wq | Wk | Wv) and "bw_mlp" [N][Ld][2 F] = film_bias_mlp . (wi_0 | wi_1) in the gated projection's
 * packed column order (EpiF32StoreGated).  The decoder's per-step buffers hold what the LAST decoder evaluation's last
 * layer left (pass p in rows [p BT, (p + 1) BT)): "x" [M][D], "ssq" [M][D / 32], "y" [M][D], "qk" [M][2 J], "vt"
 * [segments][J][T], "ao" [M][J], "g" [M][F], "eps" [M][128], the conditional rows' "cq" (folded projection: [BT][n_cross J],
 * un-normalised; else [Bmax T][J] per module), "xg" [BT][D] and "qp" [BT][n_cross J] (folded projection only), and, on a
 * handle with a second cross-attention module (sum_cross_attends with a context encoder), that module's "ao2" [Bmax T][J]
 * and "cq2" [Bmax T][J] (the second half of "cq"; written by the un-folded projection only) -- on any other handle these
 * two names are unknown buffers. */
int msd_debug_read(msd_model* m, const char* buffer, float* host_out, int64_t max_elems,
                   int64_t* n_out);

/* Per-kernel-class timing of `n_steps` eagerly launched DDPM steps, measured with
 * hipEvents on `stream` around every launch (bench.py roofline leg).
 *   names_out  receives a pointer to a static NULL-terminated array of class names
 *   ms_out / launches_out  [MSD_MAX_KERNEL_CLASSES] totals over the run          */
#define MSD_MAX_KERNEL_CLASSES 16
int msd_profile_steps(msd_model* m, int batch, int n_steps, const char* const** names_out,
                      double* ms_out, int64_t* launches_out, void* stream);

/* Standalone ops (the building blocks, for unit parity tests). All device ptrs.  They synchronise and fail like the
 * model does: weights beyond the half-plane range -> MSD_ERR_UNSUPPORTED, activations beyond it -> MSD_ERR_RANGE,
 * a `precision` of the other library build -> MSD_ERR_UNSUPPORTED. */
int msd_op_gemm_h16(int precision, const float* a_dev, const float* w_dev, float* c_dev,
                    int m, int n, int k, void* stream); /* C = A[m,k] @ W[k,n] on 16-bit operand planes */
/* deprecated ABI <= 2 name of msd_op_gemm_h16 (the planes were bfloat16 then) */
int msd_op_gemm_bf16(int precision, const float* a_dev, const float* w_dev, float* c_dev,
                     int m, int n, int k, void* stream);
int msd_op_gemm_f32(const float* a_dev, const float* w_dev, float* c_dev,
                    int m, int n, int k, void* stream);
int msd_op_attention(int precision, const float* q_dev, const float* k_dev,
                     const float* v_dev, float* o_dev, int n_q, int n_keys, int n_keys_valid,
                     int heads, void* stream); /* q [n_q, heads*64] (n_q % 64 == 0), k/v [n_keys, heads*64] (n_keys % 32 == 0) */
/* The same with the query-side single-plane switches of the two-plane modes: qp bit 0 = Q enters q.k^T as ONE
 * 16-bit plane (msd_config.attn_q_planes = 1), bit 1 = the softmax weights enter P.V as one plane
 * (attn_p_planes = 1); K and V always keep hi + lo.  msd_op_attention is qp = 0. */
int msd_op_attention_qp(int precision, int qp, const float* q_dev, const float* k_dev,
                        const float* v_dev, float* o_dev, int n_q, int n_keys, int n_keys_valid,
                        int heads, void* stream);
/* ABI 6: the same with the key axis split over `ksplit` blocks per (head, query tile) (a power of two is used: 3 runs as 2)
 * and the partials merged by the separate merge launch (merge_in_launch = 0) or inside the attention launch by the last
 * block of each group to arrive (1; attention.h attention_inlaunch_merge); launched `repeats` times back to back. */
int msd_op_attention_split(int precision, int qp, int ksplit, int merge_in_launch, int repeats, const float* q_dev,
                           const float* k_dev, const float* v_dev, float* o_dev, int n_q, int n_keys,
                           int n_keys_valid, int heads, void* stream);
/* (appended to ABI 6) The same with the two launch forms only the decoder reached before.  allow_qb4 = 1 lets the launch run on
 * 128-row blocks (16 waves) when it has more than 256 64-row blocks and n_q % 128 == 0 (attention.h
 * attention_query_blocks); 0 keeps 32- / 64-row blocks, as msd_op_attention_split does.  A non-null q_ssq_dev
 * [n_q][q_tiles] (q_tiles % 4 == 0, <= 32) holds partial sums of squares of each query row's residual stream: the
 * queries are then UN-normalised and the kernel scales row r's logits by 1 / sqrt(sum_t q_ssq[r][t] / (32 q_tiles) + 1e-6)
 * (the folded cross-attention query projection; two-plane precisions only, 32- and 64-row blocks). */
int msd_op_attention_ex(int precision, int qp, int ksplit, int merge_in_launch, int repeats, int allow_qb4,
                        const float* q_ssq_dev, int q_tiles, const float* q_dev, const float* k_dev,
                        const float* v_dev, float* o_dev, int n_q, int n_keys, int n_keys_valid, int heads,
                        void* stream);


/* Standalone forms of the FUSED kernels of the step (each restates one reference function and has its
 * own parity test against the oracle, tests/test_gpu_fused_ops.py).  All device pointers, fp32. */

/* eval_step.body after the decoder calls (diffusion_utils.py:416-452): model-output conversion, CFG
 * combine, x0 / clip / eps, ddpm_step (:382-395, diffusion_reverse :120-163) or ddim_step (:369-379).
 * Uses cfg->{num_steps, sampler, clip_x0, cfg_weight, model_output, logvar_*, *_schedule*}.
 *   out_uncond_dev may be NULL iff cfg_weight == 1; noise_dev (this step's draw) may be NULL (zeros). */
int msd_op_sampler_step(const msd_config* cfg, int step_index, const float* z_dev,
                        const float* out_cond_dev, const float* out_uncond_dev,
                        const float* noise_dev, float* z_out_dev, int64_t n, void* stream);

/* (appended to ABI 7) msd_op_sampler_step with known frames (msd_sample_keep's update): element e belongs to frame
 * e / n_dims; where keep_mask_dev[frame] != 0, pred_x0 := known_scaled_dev[e] (MODEL units, [-1, 1]) and pred_eps follows
 * from it, after the CFG combine and the clip; the other elements are msd_op_sampler_step's, bit for bit.
 *   known_scaled_dev float [n]; keep_mask_dev int32 [n / n_dims] (device); n_dims % 4 == 0, n % n_dims == 0 */
int msd_op_sampler_step_keep(const msd_config* cfg, int step_index, const float* z_dev,
                             const float* out_cond_dev, const float* out_uncond_dev,
                             const float* noise_dev, const float* known_scaled_dev, const int32_t* keep_mask_dev,
                             int n_dims, float* z_out_dev, int64_t n, void* stream);

/* (appended to ABI 7) msd_op_sampler_step_keep with release words (msd_sample_edit's update): frame f is known in this
 * step iff release_dev[f] >= 1 and step_index >= release_dev[f] - 1; its elements are then msd_op_sampler_step_keep's
 * with flag 1, all others msd_op_sampler_step's, bit for bit.  At step_index 0 only words == 1 return known_scaled_dev. */
int msd_op_sampler_step_release(const msd_config* cfg, int step_index, const float* z_dev,
                                const float* out_cond_dev, const float* out_uncond_dev,
                                const float* noise_dev, const float* known_scaled_dev, const int32_t* release_dev,
                                int n_dims, float* z_out_dev, int64_t n, void* stream);

/* (appended to ABI 7) The part-way start of msd_sample_edit on its own: xk = scale_features(clip=True) of mel_dev
 * (cfg->feature_min / feature_max) and z = fmaf(sigma, eps, alpha * xk) at step_index's noise level (see msd_sample_edit).
 *   mel_dev, eps_dev float [n] in; z_out_dev, xk_out_dev float [n] out; z_planes_out_dev float [n]: z's operand planes of
 *   cfg->precision merged back to float32; n % 4 == 0.  Uses cfg->{num_steps, sampler_schedule*, feature_*, precision}. */
int msd_op_diffuse_to_step(const msd_config* cfg, int step_index, const float* mel_dev, const float* eps_dev,
                           float* z_out_dev, float* z_planes_out_dev, float* xk_out_dev, int64_t n, void* stream);

/* (appended to ABI 7) The resampling jump of msd_sample_resample on its own, with the caller's eps: z_out = fmaf(b, eps, a * z)
 * from level from_level up to level to_level, 0 <= from_level < to_level <= cfg->num_steps (see msd_sample_resample).
 *   z_dev, eps_dev float [n] in; z_out_dev float [n] out; z_planes_out_dev float [n]: z_out's operand planes of
 *   cfg->precision merged back to float32; n % 4 == 0, n <= 2^31 - 1024.  Uses cfg->{num_steps, sampler_schedule*, precision}. */
int msd_op_renoise(const msd_config* cfg, int from_level, int to_level, const float* z_dev, const float* eps_dev,
                   float* z_out_dev, float* z_planes_out_dev, int64_t n, void* stream);

/* (appended to ABI 7) One update of MSD_SAMPLER_DPMPP_2M (msd_sample_steps) at scan index step_index of cfg->num_steps:
 * x0_prev_inout_dev float [n] holds the previous step's pred_x0 on entry (not read when first != 0: D = x0_t) and this
 * step's on return.  Uses cfg->{num_steps, clip_x0, cfg_weight, model_output, *_schedule*}; cfg->sampler is not read.
 *   out_uncond_dev may be NULL iff cfg_weight == 1; n % 4 == 0. */
int msd_op_sampler_step_multistep(const msd_config* cfg, int step_index, const float* z_dev,
                                  const float* out_cond_dev, const float* out_uncond_dev,
                                  float* x0_prev_inout_dev, int first, float* z_out_dev, int64_t n, void* stream);

/* (appended to ABI 7) msd_op_sampler_step / msd_op_sampler_step_multistep in the GUIDED form (msd_sample_guided's update):
 * the arrays are `rows` rows of n / rows elements, and row b is combined with weights_host[b] (host floats, finite) in
 * cfg->cfg_weight's place; a row whose weight is exactly 1 takes the cond_wt == 1 branch.  Row b holds the bits of the
 * plain op on that row with cfg_weight = weights_host[b].  out_uncond_dev is required whatever cfg->cfg_weight is;
 * (n / rows) % 1024 == 0 (a block of the kernel reads one weight); else as the plain ops. */
int msd_op_sampler_step_guided(const msd_config* cfg, int step_index, const float* z_dev,
                               const float* out_cond_dev, const float* out_uncond_dev, const float* noise_dev,
                               const float* weights_host, int rows, float* z_out_dev, int64_t n, void* stream);
int msd_op_sampler_step_multistep_guided(const msd_config* cfg, int step_index, const float* z_dev,
                                         const float* out_cond_dev, const float* out_uncond_dev,
                                         float* x0_prev_inout_dev, int first, const float* weights_host, int rows,
                                         float* z_out_dev, int64_t n, void* stream);

/* x_out = x_in + a.w1 ; h_out = (RMSNorm(x_out; gamma) (.) (film_scale+1) + film_bias) . w2
 * (layers.py:632-666 + the Dense that follows).  folded=1: the decoder's folded-norm epilogues
 * (EpiResidualNorm producer, row-scale + tabulated bias.W consumer); folded=2: the same with the producer as the
 * 4-way split-K launch of the experiments build (tools/ubench/exp; MSD_ERR_UNSUPPORTED in the product library);
 * folded=3: the producer on the 32 x 48 tiles the decoder uses where they give one tile per CU (d % 48 == 0);
 * folded=0: separate norm kernel.
 * film_scale_dev / film_bias_dev [D] may both be NULL (plain RMSNorm).
 *   x [m,d]  a [m,k]  w1 [k,d]  gamma [d]  w2 [d,n]  x_out [m,d]  h_out [m,n]; m,k,d,n % 64 == 0 */
int msd_op_residual_norm_gemm(int folded, const float* x_in_dev, const float* a_dev,
                              const float* w1_dev, const float* gamma_dev,
                              const float* film_scale_dev, const float* film_bias_dev,
                              const float* w2_dev, float* x_out_dev, float* h_out_dev,
                              int m, int k, int d, int n, void* stream);

/* MlpBlock's gated input (layers.py:483-497): out [m,f] = gelu_tanh(a.wi0) * (a.wi1) */
int msd_op_geglu(const float* a_dev, const float* wi0_dev, const float* wi1_dev, float* out_dev,
                 int m, int k, int f, void* stream);

/* Fused q|k|v projection (layers.py:262-264) through the attention kernel's operand layouts (V^T with
 * the per-16 key permutation, per segment of seg_len rows), returned un-permuted: q,k,v [m,j]. */
int msd_op_qkv(const float* a_dev, const float* wq_dev, const float* wk_dev, const float* wv_dev,
               float* q_out_dev, float* k_out_dev, float* v_out_dev, int m, int k, int j,
               int seg_len, void* stream);

/* decoder_norm + spec_out_dense in exact fp32 (network.py:445-456): out [m,n] = RMSNorm(x; gamma).w */
int msd_op_final_proj(const float* x_dev, const float* gamma_dev, const float* w_dev, float* out_dev,
                      int m, int d, int n, void* stream);

/* The stages of msd_fill_normal_threefry's draw (seed, fold, n): stage 0 = raw bits (uint32 written into out),
 * 1 = uniform u, 2 = normal, 3 = w = -log1p(-u*u), the normal stage's one operation whose rounding the host
 * restatement does not share (a test finishes the stage on the host from it).  bits_in_dev != NULL (uint32 [n]): stages 1 / 2 applied to the caller's words instead
 * (the float stages over all 2^23 mantissas: stages 1 - 3); stage 0 then is MSD_ERR_INVALID_ARGUMENT.  Does not synchronise. */
int msd_op_threefry(int stage, uint64_t seed, int64_t fold, const uint32_t* bits_in_dev, float* out_dev, int64_t n,
                    void* stream);

/* ---- (appended to ABI 7) Device vocoder: the codec's STFT pair, Audio2Mel and a Griffin-Lim mel -> audio stage ----
 * NOT the reference's decoder: audio_codecs.py:249-264 runs SoundStream, a learned vocoder whose TF-Hub artifact is
 * not available; that stays "not built".  This is a documented stand-in -- fast Griffin-Lim (phase reconstruction with
 * momentum) over the codec's own STFT geometry -- so that a result can be listened to and a recording can be encoded
 * as context on the device.  It claims no parity with SoundStream.
 * Geometry (audio_codecs.MelGAN, :204-218): frame 640, hop 320, FFT 1024 -> 513 bins, periodic Hann window,
 * pad_end framing (frame k = samples [320k, 320k + 640) of the zero-extended signal), F = ceil(n_samples / 320)
 * frames, 128 mel bins, log-mel = log(clip(., 1e-5, 1e8)).  Specification: stft / istft / mel_to_linear /
 * griffin_lim of the package's audio_codecs.py (float64 NumPy).  All arithmetic is float32 (exact-fp32 MFMA GEMMs;
 * the plane format of the library build does not enter).
 * A handle owns its DFT / mel tables and work buffers, which grow on demand to the largest batch * n_frames seen;
 * one handle <-> one device <-> one caller thread at a time.  Every call enqueues on `stream` and SYNCHRONISES it
 * before returning, like the msd_op_* entry points.  Null pointers and zero or negative sizes give
 * MSD_ERR_INVALID_ARGUMENT without touching a device. */
typedef struct msd_vocoder msd_vocoder; /* opaque */

/* On the CURRENT HIP device.  mel_basis_host float [513, 128] (linear_to_mel_weight_matrix(128, 513, 16000, 0, 8000));
 * mel_inverse_host float [128, 513], its pseudo-inverse (taken in float64 by the caller).  On failure *out may hold a
 * handle whose msd_vocoder_last_error has the message; destroy it. */
int msd_vocoder_create(const float* mel_basis_host, const float* mel_inverse_host, msd_vocoder** out);
void msd_vocoder_destroy(msd_vocoder* v);
const char* msd_vocoder_last_error(const msd_vocoder* v);

/* tf.signal.stft(pad_end=True): audio_dev float [batch, n_samples] -> spec_out_dev float [batch, F, 2, 513], real
 * parts then imaginary parts of each frame. */
int msd_vocoder_stft(msd_vocoder* v, int batch, int64_t n_samples, const float* audio_dev, float* spec_out_dev,
                     void* stream);
/* Inverse: per frame the inverse real DFT (the imaginary parts of the DC and Nyquist bins are ignored), its first 640
 * samples times the Hann window, overlap-added, divided by max(sum of squared windows, 1e-3), cut to F * 320:
 * spec_dev float [batch, n_frames, 2, 513] -> audio_out_dev float [batch, n_frames * 320].  istft(stft(x)) = x except
 * on the first ~40 samples, where the window vanishes. */
int msd_vocoder_istft(msd_vocoder* v, int batch, int n_frames, const float* spec_dev, float* audio_out_dev,
                      void* stream);
/* Audio2Mel (audio_codecs.py:107-143, MelGAN.encode :226-247): logmel_out_dev float [batch, F, 128] =
 * log(clip(|stft| . mel_basis, 1e-5, 1e8)). */
int msd_vocoder_encode(msd_vocoder* v, int batch, int64_t n_samples, const float* audio_dev, float* logmel_out_dev,
                       void* stream);
/* Griffin-Lim: mag = max(exp(logmel) . mel_inverse, 0); X = mag . phase; n_iters times { x = istft(X); Y = stft(x);
 * U = Y - momentum / (1 + momentum) . Y_prev (Y_prev = 0 at first); X = mag . U / |U|, (1, 0) where U = 0 }; one final
 * istft.  n_iters >= 0, momentum >= 0 (0.99: Perraudin et al.'s fast form; 0: the classic iteration).
 *   logmel_dev     float [batch, n_frames, 128]
 *   init_phase_dev float [batch, n_frames, 2, 513] (cos then sin of each frame's phases, used as given), or NULL: the
 *                  phase of bin (b, f, k) is then the direction of the pair (d[b][f][0][k], d[b][f][1][k]) of
 *                  d = msd_fill_normal(seed, stream_id = 0x766F63, subseq = 0, ..., batch * n_frames * 2 * 513),
 *                  normalised to the unit circle -- uniform phases, reproducible from `seed`
 *   audio_out_dev  float [batch, n_frames * 320] */
int msd_vocoder_decode(msd_vocoder* v, int batch, int n_frames, const float* logmel_dev, int n_iters, float momentum,
                       uint64_t seed, const float* init_phase_dev, float* audio_out_dev, void* stream);

/* ---- (appended to ABI 7) One GEMM launch site of the decoder at a time (tests/test_gpu_gemm_sites.py) ----
 * Runs ONE launch site of the step (GemmSites / DualSites of csrc/msd_api.hip; the entry: csrc/standalone_ops.h SiteRun) on the caller's float32 operands through
 * the product's own dispatch: pick_tile, gp_launch / set_xcd_grid, the range flag, gemm_t's persistent switch and the
 * prefetch-wave choice are the decoder's.  Context: the entry builds a MINIMAL context of its own (no handle is passed and
 * no model is needed): the plane count of `precision`, a range flag, the device's CU count.
 * `site` is the position in GemmSites<planes> (0 .. 9, and 10 in the two-plane modes), then DualSites (11 .. 13):
 *    0 QKV             out[m][n] = q | k | v = [rstd .] (a . w) [+ bias]; n = 3 j, V^T un-permuted on the host
 *    1 MLP-in          out[m][n/2] = gelu_tanh(h0) . h1, h = [rstd .] (a . (w | w_gate)) [+ bias], bias = [steps][b0 | b1]
 *    2 residual (square kind)   3 residual (tall kind)        x[m][n] += a . w
 *    4 residual + norm inputs (tall)   5 its DUP form (tall)   6 (square)   10 its Y2 form (tall, two planes only)
 *                      x += a . w; ssq_out[row][n/32] partial sums of squares (spare slots zero); y = x (.) g, g_lo for
 *                      rows < split_row and g_hi from there, rows of a null gain are not written; DUP: every row also at
 *                      row + dup_rows (g_lo for the first copy, g_hi for the second; buffers hold dup_rows + m rows);
 *                      Y2: rows < y2_rows also y2 = x (.) g2
 *    7 store, 16-bit planes (square)   8 store, float32 (narrow)      out[m][n] = [rstd .] (a . w) [+ bias]
 *    9 in-projection   x[p][m] = a . w + pos[m % seg_len] for p < passes; y = x (.) g_lo(step); ssq_out; optional
 *                      y2 = x (.) g2 of the first pass; step_copy = the word the epilogue publishes (the scan index)
 *   11 dual, folded QKV: problem 1 as site 0, problem 2 out2[m2][n2] = a2 . w2 (float32)
 *   12 dual, folded attention-out: problem 1 as site 4, problem 2 out2 = a2 . w2 + addend2 (16-bit planes)   13: as site 5
 * rstd[m] = 1 / sqrt(sum_t ssq[m][t] / k + 1e-6) over the caller's [m][k/32] partial sums (k <= 1024); null ssq: no row
 * scale (and then no bias).  bias / g_lo / g_hi are tables of `steps` rows of n floats, read at row `step`.
 * Results that the product keeps as 16-bit planes come back merged to float32; such buffers start as NaN inside the
 * entry, so what the epilogue did not store comes back NaN.  float32 results (x, ssq_out, out of site 8, out2 of site 11)
 * are the caller's buffers as the kernel left them.
 * force_bm / force_bn (dual sites: also force_bm2 / force_bn2, required there -- the step plan, not pick_tile, names a dual
 * launch's tiles): 0 = pick_tile decides; a shape outside the site's table is MSD_ERR_INVALID_ARGUMENT, as are sizes the
 * tile that runs does not divide.  Errors otherwise as the other msd_op_* entries: MSD_ERR_UNSUPPORTED for a precision of
 * the other build and for weights beyond the half planes' range, MSD_ERR_RANGE for activations beyond it.  Synchronises. */
typedef struct msd_gemm_site_args {
  int32_t struct_size;       /* sizeof(msd_gemm_site_args) */
  int32_t precision;         /* msd_precision */
  int32_t site;
  int32_t m, n, k;
  int32_t step, steps;       /* scan index the step-indexed rows are read at; rows of those tables */
  int32_t force_bm, force_bn;
  int32_t persistent;        /* MLP-in: 0 = the product's switch (on), 2 = off (msd_config.mlp_in_persistent) */
  int32_t resident_blocks;   /* MLP-in, persistent form: 0 = the product's (one per CU), else a multiple of 8 */
  int32_t seg_len;           /* QKV: rows per V^T segment (m % seg_len == 0, seg_len % 16 == 0); in-projection: rows of pos */
  int32_t split_row, dup_rows, y2_rows, passes;
  int32_t m2, n2, k2, force_bm2, force_bn2;   /* dual sites: the second problem */
  int32_t prefetch_rows, prefetch_k;          /* shape of the prefetch target: two planes of [rows][k] 16-bit elements */
  /* out: what ran */
  int32_t ran_bm, ran_bn, ran_ns, ran_xcd_rows, ran_persistent, ran_dual, ran_prefetch;
  int32_t ran_bm2, ran_bn2, ran_ns2, ran_xcd_rows2;
  int32_t step_copy;
  /* operands (device, float32) */
  const float* a;            /* [m][k] */
  const float* w;            /* [k][n] (MLP-in: wi_0 [k][n/2]) */
  const float* w_gate;       /* MLP-in: wi_1 [k][n/2] */
  const float* ssq;
  const float* bias;
  const float* g_lo;
  const float* g_hi;
  const float* g2;           /* [n] */
  const float* pos;          /* [seg_len][n] */
  const float* a2;           /* [m2][k2] */
  const float* w2;           /* [k2][n2] */
  const float* addend2;      /* [m2][n2] */
  const void* prefetch;      /* optional weight-shaped buffer a prefetch wave touches (two-plane modes); never written */
  /* results (device, float32) */
  float* x;
  float* out;
  float* y;
  float* y2;
  float* ssq_out;
  float* out2;
} msd_gemm_site_args;
int msd_op_gemm_site(msd_gemm_site_args* args, void* stream);

/* The index-th tile (BM x BN, ring depth NS) of `site`'s table for `precision`, read from the tile table itself; bm, bn
 * and ns point to TWO ints each: [0] the tile (dual sites: the first problem's), [1] the second problem's tile of a dual
 * site's pair, 0 otherwise.  MSD_ERR_INVALID_ARGUMENT past the last tile or the last site. */
int msd_op_gemm_site_tiles(int precision, int site, int index, int32_t* bm, int32_t* bn, int32_t* ns);
/* The name of launch site `site` for `precision`, derived from the site's type (tile kind and epilogue) -- "qkv", "mlp_in",
 * "residual_square", "residual_tall", "resnorm_tall", "resnorm_tall_dup", "resnorm_square", "store_h16", "store_f32",
 * "in_proj", "resnorm_tall_y2", "dual_qkv", "dual_out", "dual_out_dup" -- or NULL past the last site. */
const char* msd_op_gemm_site_name(int precision, int site);

/* (appended to ABI 7) One attention launch the way the DECODER fills it (msd_op_attention_ex fixes the easiest form: one
 * segment, ldq = ldk = heads * 64, the key allocation exactly the key axis, no prefetch wave).  J = heads * 64; inputs are
 * float32 device arrays in the caller's own layout:
 *   q      [segs * q_rows_per_seg][ldq], head h at columns q_col + 64 h
 *   k      [segs][k_alloc_rows][ldk], head h at columns k_col + 64 h.  The launch sees the WINDOW of k_rows rows from row
 *          k_row0 of every segment (AttnParams::k_rows; segment stride k_alloc_rows * ldk).  k == q (self-attention: q and
 *          k interleaved in one buffer) needs ldk == ldq, k_row0 == 0 and k_rows == k_alloc_rows == q_rows_per_seg
 *   v      [segs][k_alloc_rows][J]; the entry builds V^T [segs][J][k_alloc_rows] with the kernel's per-16 key permutation and
 *          launches on vt = base + k_row0, vt_ld = k_alloc_rows, vt_cols = k_rows (0 when the window is the whole allocation)
 *   n_keys int32 [segs], 0 <= n_keys[s] <= k_rows
 *   q_ssq  optional [segs * q_rows_per_seg][q_tiles]: un-normalised queries, as msd_op_attention_ex
 *   o      [segs * q_rows_per_seg][J]
 * Every 16-bit plane starts as NaN and only the columns (q) and the window (k, V^T) above are filled from the caller's data:
 * a read outside them comes back as NaN through V^T, and so does an output row that nobody stored.
 * prefetch_rows, prefetch_k != 0: the launch carries a weight target of two planes [prefetch_rows][prefetch_k] (two-plane
 * precisions; prefetch_k % 64 == 0, <= 4096), so its blocks run the prefetch wave; touch_ahead (0 .. 16) and pf_late (0 / 1)
 * are AttnParams' fields.  merge_in_launch: segs * (q_rows_per_seg / 32) * heads arrival counters, zeroed once, for all
 * `repeats` launches.  ran_*: what the launcher's own rule (attention.h attention_launch_shape) chose -- query blocks per
 * workgroup (1, 2, 4), prefetch wave, touch-ahead, and the power of two the key split ran as.
 * k_row0, k_rows % 32 == 0; k_alloc_rows, ldq, ldk, q_col, k_col % 8 == 0; q_rows_per_seg % 64 == 0.  Errors as
 * msd_op_attention_ex.  Synchronises. */
typedef struct msd_attention_launch_args {
  int32_t struct_size;       /* sizeof(msd_attention_launch_args) */
  int32_t precision;         /* msd_precision */
  int32_t qp, heads, segs, q_rows_per_seg, repeats;
  int32_t ksplit, merge_in_launch, allow_qb4;
  int32_t ldq, q_col;
  int32_t ldk, k_col, k_alloc_rows, k_row0, k_rows;
  int32_t prefetch_rows, prefetch_k, touch_ahead, pf_late;
  int32_t q_tiles;
  /* out: what ran */
  int32_t ran_qb, ran_prefetch_wave, ran_touch_ahead, ran_ksplit;
  /* operands (device) */
  const float* q;
  const float* k;
  const float* v;
  const int32_t* n_keys;
  const float* q_ssq;
  /* result (device, float32) */
  float* o;
} msd_attention_launch_args;
int msd_op_attention_launch(msd_attention_launch_args* args, void* stream);

/* (appended to ABI 7) One launch WITH A WEIGHT TARGET in either carrier form (msd_config.touch_carrier).  The op makes
 * the target itself: two planes [target_rows][target_k] of 16-bit elements in ONE allocation of exactly their size, so
 * the last line a touch may read ends where the allocation ends.  `prefetch*` of the launch arguments are ignored.
 * Two-plane precisions only.  A touch has no reader: the outputs of the three forms are bit-identical. */
typedef struct msd_carrier_args {
  int32_t struct_size;
  int32_t form;                   /* 0 = no target, 1 = the in-block wave, 2 = touch blocks */
  int32_t n_touch;                /* form 2: touch blocks asked for (1 .. 1024; the launch keeps within one round of the chip) */
  int32_t delay;                  /* form 2: counted sleep rounds in front of the touches (0 .. 64, ~0.2 us each) */
  int32_t target_rows, target_k;  /* form != 0: rows and elements per row of one plane (k a multiple of 64, <= 4096) */
  /* out */
  int32_t ran_form;               /* what the launch ran: 2 only where the kernel has a touch-block form and a slot was free */
  int32_t ran_touch_blocks;
  int32_t ran_range_flag;         /* the half-plane range flag after the launch (0 = clean) */
} msd_carrier_args;
int msd_op_gemm_site_carrier(msd_gemm_site_args* args, msd_carrier_args* carrier, void* stream);
int msd_op_attention_launch_carrier(msd_attention_launch_args* args, msd_carrier_args* carrier, void* stream);
/* Host only, no GPU call: how a target of `target_bytes` -- rows of `row_bytes` bytes (<= 8192), `row_pitch` bytes apart,
 * the last row ending the target -- is dealt over `waves` touching waves, by the function both device forms use.
 * Each touch is evaluated lane by lane with the predicate the device waves use; the target is ONE plane (the device deals a
 * two-plane target as 2 x rows rows, plane 1 behind plane 0, with the same predicate).
 * ranges[(w * R + u) * 3 + {0, 1, 2}] = first row, rows, and 128-byte lines per row of touch u of wave w (rows 0 = nothing),
 * R = the return value (touches per wave).  Negative: -msd_status (bad arguments, `capacity` int32 words too few, or
 * MSD_ERR_UNSUPPORTED: more rows than the waves cover in R touches each). */
int msd_op_touch_deal(int64_t target_bytes, int32_t row_bytes, int32_t row_pitch, int32_t waves, int32_t* ranges, int32_t capacity);

/* ---- the denoising loss (appended to ABI 7): how well a mel fits the encoded tokens --------------------------------------
 * The evaluation loss of the reference (models.py loss_fn over diffusion_utils.get_diffusion_training_input and
 * calculate_loss) at time indices of the handle's own grid, on the device, with no host round trip between evaluations.
 * One EVALUATION at index i (row i of the handle's step tables, time (i + 1) / num_steps, as msd_decoder_pass), for the
 * rows of the encoded batch:
 *   x0    = scale_features(target, clip=True)                      the context path's expression and bits
 *   z_t   = fmaf(sigma, eps, alpha * x0)                           (alpha, sigma) = sqrt(sigmoid(+-logsnr)) of the TRAIN
 *                                                                  schedule at the index (msd_get_schedule word 7), computed
 *                                                                  in double and rounded once -- not the sampler schedule
 *                                                                  of msd_sample_edit's part-way start
 *   eps   = eps_dev[j] (the j-th entry of the call's time list), or drawn under the call's keys: MSD_RNG_PHILOX
 *           sub-sequence 1 + i of (seed, stream_id) = msd_fill_normal(seed, stream_id, 1 + i, ...); MSD_RNG_THREEFRY
 *           normal(fold_in(PRNGKey(seed), i), [batch | 1, T, n]) = msd_fill_normal_threefry(seed, i, ...); per-row keys as
 *           in msd_sample_rows.  The draw is a function of the index: an index that appears twice in one call draws the SAME
 *           eps twice, and its two output rows are equal.
 *   o     = one decoder pass on z_t, conditional (MSD_LOSS_COND) or unconditional (MSD_LOSS_UNCOND), or both passes in the
 *           two-pass plan of a guided step (MSD_LOSS_BOTH; MSD_ERR_UNSUPPORTED on a handle created with cfg_weight 1).
 *           Dropout is off: this is an evaluation (the reference's loss_fn passes enable_dropout=True even in eval; that
 *           quirk is not restated), and loss_fn's own draws of the time and of the condition drop are the caller's business.
 *   (eps_hat, x0_hat) = the model-output conversion of the sampler, at the train schedule's log-SNR, for every pass
 *   element loss = |d| (MSD_LOSS_L1) or d * d (MSD_LOSS_L2) of d_x0 = x0_hat - x0 (MSD_LOSS_X0), d_eps = eps_hat - eps
 *           (MSD_LOSS_EPS), the larger of the two (MSD_LOSS_MAX_X0_EPS; a NaN stays a NaN) or eps loss + x0 loss
 *           (MSD_LOSS_X0_AND_EPS), times mask[b, t] (float, any value; NULL = ones)
 *   out_dev[j][pass][b][t] = the sum over the frame's n_dims elements, float32: a thread sums its four consecutive
 *           elements left to right, the frame's n_dims / 4 thread sums are added as a pairwise tree (level s = 1, 2, 4, ...:
 *           thread t with t % 2s == 0 adds the sum of thread t + s).  passes = 2 for MSD_LOSS_BOTH (0 = conditional), else 1.
 *           Sums over frames, rows and times are the caller's, in whatever precision it likes.
 * times_host: n_times >= 1 indices in [0, num_steps), any order, repeats allowed.  loss_type / loss_norm are arguments of
 * the call, not of msd_config.  Needs msd_encode; batch must be the encoded batch; n_dims % 4 == 0 and 1024 % n_dims == 0
 * (MSD_ERR_UNSUPPORTED otherwise; every shipped configuration has 128); per-row keys need targets_length * n_dims % 1024 == 0.
 * Every refusal comes before any device work, names the offending value and leaves the handle usable.  The call ends
 * with one synchronisation and the half-plane range check (MSD_ERR_RANGE).  It overwrites the sampler's state (z, the scan
 * index, the key table), which every sampling call writes afresh; its captured graphs are the handle's (msd_reset_graph
 * drops them) and are kept apart from the step graphs. */
enum { MSD_LOSS_COND = 0, MSD_LOSS_UNCOND = 1, MSD_LOSS_BOTH = 2 };
enum { MSD_LOSS_X0 = 0, MSD_LOSS_EPS = 1, MSD_LOSS_MAX_X0_EPS = 2, MSD_LOSS_X0_AND_EPS = 3 };
enum { MSD_LOSS_L1 = 0, MSD_LOSS_L2 = 1 };
typedef struct msd_loss_args {
  int32_t struct_size;         /* sizeof(msd_loss_args) */
  int32_t batch;               /* rows; = the encoded batch */
  int32_t rng;                 /* MSD_RNG_*: the generator of eps when eps_dev is NULL */
  int32_t per_row;             /* 0: seeds[0] / stream_ids[0] key one draw over [batch, T, n]; else one key per row */
  const uint64_t* seeds;       /* host [per_row ? batch : 1] */
  const uint64_t* stream_ids;  /* host, same length, or NULL = zeros */
  const float* target_dev;     /* [batch, T, n] the mel, mel units */
  const float* mask_dev;       /* [batch, T] float, or NULL = ones */
  const float* eps_dev;        /* [n_times][batch, T, n], or NULL = drawn */
  const int32_t* times_host;   /* [n_times] time indices */
  int32_t n_times;
  int32_t conditioning;        /* MSD_LOSS_COND / _UNCOND / _BOTH */
  int32_t loss_type;           /* MSD_LOSS_X0 / _EPS / _MAX_X0_EPS / _X0_AND_EPS */
  int32_t loss_norm;           /* MSD_LOSS_L1 / _L2 */
  float* out_dev;              /* [n_times][passes][batch][T] */
} msd_loss_args;
int msd_loss(msd_model* m, const msd_loss_args* args, void* stream);
/* The loss kernel alone (unit test): out_dev[n / n_dims] = the per-frame loss of ONE pass's model output o_dev at step_index
 * of cfg's tables, over the caller's z, x0 (model units), eps and mask (float [n / n_dims] or NULL), all device [n].
 * n % n_dims == 0, n_dims as above.  Synchronises. */
int msd_op_diffusion_loss(const msd_config* cfg, int step_index, int loss_type, int loss_norm, const float* o_dev,
                          const float* z_dev, const float* x0_dev, const float* eps_dev, const float* mask_dev, int n_dims,
                          float* out_dev, int64_t n, void* stream);

/* ---- deterministic DDIM inversion (appended to ABI 7): from a mel and the encoded tokens to the noise that renders it -----
 * A call of K steps (K | num_steps) has levels 0 .. K; level l has time l / K, logsnr_l of the SAMPLER schedule, alpha_l =
 * sqrt(sigmoid(logsnr_l)) and sigma_l = sqrt(sigmoid(-logsnr_l)).  Level 0 is scale_features(mel, clip=True) (the context
 * path's expression and bits); step i = 0 .. K - 1 takes level i to level i + 1 with ONE decoder evaluation of the state it
 * has, at the UPPER level's time (i + 1) / K (table row (i + 1) num_steps / K - 1, as scan index i of msd_sample_steps), and
 * no draw:
 *   eps  = the model output -> eps at the TRAIN schedule's log-SNR (the sampler's conversion), combined as
 *          w eps_cond + (1 - w) eps_uncond when the row's weight w != 1 (two rounded products and a sum)
 *   z_up = fmaf(b_i, eps, a_i * z)      a_i = alpha_{i+1} / alpha_i, b_i = sigma_{i+1} - a_i sigma_i  (i >= 1)
 *                                       a_0 = alpha_1, b_0 = sigma_1   (the mirror of "scan index 0 returns x0")
 * a and b are computed in double from the float32 log-SNRs of the call's K coefficient rows and rounded once.  This is the
 * exact inverse of the DDIM step of msd_sample_steps(MSD_SAMPLER_DDIM, K) with eps frozen -- taken at the state below, not
 * above -- where the train and the sampler schedule agree at the time; with a linear sampler schedule, or different train
 * and sampler schedules, the step is what these lines say.  msd_config.clip_x0 is IGNORED: the clip is not invertible where
 * it binds.  out_dev is z at level K: float32 [batch, T, n] in MODEL units (not unscaled), an init_z_dev for msd_sample_steps.
 * num_steps: 0 = the handle's; K must divide it.  weights_host / n_weights: NULL or 0 = weight 1 for every row; else 1 or
 * `batch` finite floats, per-row weights need targets_length * n_dims % 1024 == 0.  Every weight == 1 runs the one-pass plan
 * (half the rows in every launch); a handle created with cfg_weight 1 holds one pass's buffers and takes nothing else
 * (MSD_ERR_UNSUPPORTED).  Needs msd_encode; batch must be the encoded batch.  Every refusal comes before any device work
 * and leaves the handle usable.  The call ends with one synchronisation and the half-plane range check (MSD_ERR_RANGE).
 * It overwrites the sampler's state (z, the scan index, the key table, the row weights), which every sampling call writes
 * afresh; its graphs live in the handle's step-graph cache under a key of their own.
 * NOT built: fixed-point refinement of a step, stopping below level K, inversion under DDPM noise or the multistep sampler,
 * known frames, per-frame weights, K that does not divide num_steps. */
typedef struct msd_invert_args {
  int32_t struct_size;         /* sizeof(msd_invert_args) */
  int32_t batch;               /* rows; = the encoded batch */
  const float* mel_dev;        /* [batch, T, n] the mel, mel units */
  int32_t num_steps;           /* K; 0 = the handle's */
  int32_t n_weights;           /* 0, 1 or batch */
  const float* weights_host;   /* [n_weights] guidance weights, or NULL = 1 */
  float* out_dev;              /* [batch, T, n] z at level K, model units */
} msd_invert_args;
int msd_invert(msd_model* m, const msd_invert_args* args, void* stream);
/* One inversion update alone (unit test): z_out_dev = fmaf(b, eps, a * z_dev) at step_index of cfg's tables (cfg->num_steps
 * is the call's K) from the model outputs of the passes, row r of `rows` rows of n / rows elements (a multiple of 1024)
 * with weights_host[r]; z_planes_out_dev = z_out's operand planes of cfg->precision merged back to float32.
 * out_uncond_dev may be NULL if and only if every weight is 1.  cfg->cfg_weight and cfg->clip_x0 are not read.  Synchronises. */
int msd_op_invert_step(const msd_config* cfg, int step_index, const float* z_dev, const float* out_cond_dev,
                       const float* out_uncond_dev, const float* weights_host, int rows, float* z_out_dev,
                       float* z_planes_out_dev, int64_t n, void* stream);

/* (appended to ABI 7) One sampler update in ANY form of the msd_op_sampler_step* entry points above, with what those leave
 * out: the launch also writes z_out's operand planes of cfg->precision and feeds the half-plane range flag, as every step
 * of a sampling call does (unit test of the kernels' plane tails: tests/test_gpu_sampler_planes.py).
 * The form follows from the pointers, which mean what they mean above: weights_host != NULL = guided (`rows` rows, with
 * either update); x0_prev_inout_dev != NULL = the multistep update (noise_dev is not read); known_scaled_dev != NULL = known
 * frames (plain update only, not guided: MSD_ERR_INVALID_ARGUMENT otherwise), keep_dev holding msd_op_sampler_step_keep's
 * flags when keep_is_flags != 0 and msd_op_sampler_step_release's words otherwise.  z_out_dev holds the bits of the
 * corresponding entry point above.  z_planes_out_dev float [n]: the planes merged back to float32.
 * MSD_ERR_UNSUPPORTED: cfg->precision is a precision of the other library build.  MSD_ERR_RANGE: the half-plane range flag
 * was set (|z_out| > 65504 somewhere; half-plane build only); the outputs and the ran_* fields are written all the same.
 * Synchronises. */
typedef struct msd_sampler_planes_args {
  int32_t struct_size;            /* sizeof(msd_sampler_planes_args) */
  int32_t step_index;             /* scan index, 0 .. cfg->num_steps - 1 */
  int32_t n_dims;                 /* known frames: elements per frame (% 4 == 0, n % n_dims == 0) */
  int32_t keep_is_flags;          /* known frames: keep_dev holds flags (any non-zero = known throughout), not release words */
  int32_t first;                  /* multistep: != 0 = the call's first step (x0_prev is not read) */
  int32_t rows;                   /* guided: rows of z = entries of weights_host; (n / rows) % 1024 == 0 */
  /* out */
  int32_t ran_range_flag;         /* the half-plane range flag after the launch (0 = clean) */
  int32_t ran_next_step;          /* the scan index the launch published for the next step: step_index - 1 */
  int64_t n;                      /* elements of z; % 4 == 0 */
  const msd_config* cfg;
  /* operands (device, float32 [n] unless said otherwise) */
  const float* z_dev;
  const float* out_cond_dev;
  const float* out_uncond_dev;    /* may be NULL iff one pass is read (not guided and cfg_weight == 1) */
  const float* noise_dev;         /* this step's draw, or NULL = zeros */
  const float* known_scaled_dev;  /* or NULL */
  const int32_t* keep_dev;        /* int32 [n / n_dims] */
  float* x0_prev_inout_dev;       /* or NULL */
  const float* weights_host;      /* HOST floats [rows], or NULL */
  /* results (device, float32 [n]) */
  float* z_out_dev;
  float* z_planes_out_dev;
} msd_sampler_planes_args;
int msd_op_sampler_step_planes(msd_sampler_planes_args* args, void* stream);

/* ---- (appended to ABI 7) The vocoder's layout and unit-vector kernels on their own (tests/test_gpu_vocoder_edges.py) ----
 * Host code around kernels the msd_vocoder_* entry points launch already.  A spectrum row is 1088 floats (real parts at
 * [0, 513), imaginary parts at [544, 1057), zeros between), a magnitude row 544 (513 bins, zeros behind); a call of
 * `batch` songs of F frames has batch (F + 1) rows, row b (F + 1) + k = frame k of song b, the rows k = F straddle two
 * songs.  All three synchronise; null pointers, non-positive sizes and more than 2^20 rows give
 * MSD_ERR_INVALID_ARGUMENT before any device work. */
/* The phase update of one Griffin-Lim iteration, launched as msd_vocoder_decode launches it: U = Y - alpha Y_prev,
 * X = mag U / |U|, (mag, 0) where U = 0.  y_dev, yprev_dev, x_out_dev float [rows, 1088]; mag_dev float [rows, 544]. */
int msd_op_vocoder_phase(const float* y_dev, const float* yprev_dev, const float* mag_dev, float* x_out_dev, int rows,
                         float alpha, void* stream);
/* The caller's spectrum (or phases) into spectrum rows, as msd_vocoder_istft and msd_vocoder_decode launch it:
 * src_dev float [batch, n_frames, 2, 513]; mag_dev float [batch (n_frames + 1), 544] or NULL (= ones);
 * x_out_dev float [batch (n_frames + 1), 1088] = mag . src, with normalise != 0: mag . src / |src| per (re, im) pair,
 * (mag, 0) for the zero pair.  Straddling rows and pad columns come out zero. */
int msd_op_vocoder_load_spec(const float* src_dev, const float* mag_dev, float* x_out_dev, int batch, int n_frames,
                             int normalise, void* stream);
/* One work buffer of the handle as its LAST call left it (in the spirit of msd_debug_read): `buffer` is "audio"
 * (320 floats per row: the padded signals), "x", "y0", "y1" (1088), "frames" (640) or "mag" (544); *rows_out (may be
 * NULL) = rows of that call, batch (F + 1); min(rows . floats per row, max_elems) floats are copied to host_out.
 * MSD_ERR_BAD_STATE: no call has run on the handle.  Waits for the whole device. */
int msd_vocoder_debug_read(msd_vocoder* v, const char* buffer, float* host_out, int64_t max_elems, int64_t* rows_out);

#ifdef __cplusplus
}
#endif
#endif /* MSD_AMD_H_ */
