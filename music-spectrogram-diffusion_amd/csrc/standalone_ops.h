// The msd_op_* entry points: the library's building blocks one at a time, for the unit tests (tests/test_gpu_ops.py,
// test_gpu_fused_ops.py, test_gpu_gemm_sites.py, test_gpu_attention_forms.py (+ attention_forms.py, test_attention_forms_host.py), test_gpu_keep_frames.py, test_gpu_edit_strength.py, test_gpu_few_steps.py, test_gpu_threefry.py, test_gpu_invert.py, test_gpu_sampler_planes.py, test_gpu_vocoder_edges.py).  Host code only, and no
// part of the product's paths; the file belongs to msd_api.hip alone, which includes it behind its own entry points and
// in front of the vocoder's.
// Every GEMM here runs through the product's dispatch (gemm / gemm_on on a site's TileTable), so its tile is an entry of
// the tile table and its kernel one that set_func_attrs has named already; the single exception is launch_wide_store_f32
// below.  The kernel instances this file can reach, and the order the compiler emits them in (the order of their first
// use: set_func_attrs, keep_frames_tail.h), are checked, not assumed: when this file changes, compile the library before
// and after with the build's own command line and compare the gfx950 code object and its listing byte for byte.
#pragma once
namespace {
// planes per operand of an op's `precision` argument; -1: not a precision of THIS build's plane format
int op_planes(int precision) {
  const bool bf = precision == MSD_PREC_BF16 || precision == MSD_PREC_BF16X3;
  if (precision < MSD_PREC_F16 || precision > MSD_PREC_BF16X3 || bf != (MSD_PLANE_BF16 != 0)) return -1;
  return (precision == MSD_PREC_F16X3 || precision == MSD_PREC_BF16X3) ? 2 : 1;
}

// key -> its place in a row of V^T: the per-16 key permutation of the attention kernel's V operand.  The host mirror of
// vt_perm16 (gemm_h16.h), which is what EpiQKV stores by and the attention kernel reads by.
int vt_key_pos(int key) {
  const int o = key & 15;
  return (key & ~15) + 8 * ((o >> 2) & 1) + (o & 3) + 4 * (o >> 3);
}

template <class T> constexpr TileShape shape_of() { return {T::BM, T::BN}; }

// What every op needs around its launches, in ONE place: device scratch (zeroed, freed when the op returns), operands as
// planes of the op's plane count, the range flags, and a MINIMAL launch context -- an msd_model of which Ctx, gp_launch,
// gemm_t and prefetch_of read the plane count, the range flag, the CU count and the persistent / prefetch switches;
// it has no weights, tables or buffers.
// Range flags: device words [0] = bits of the largest packed |w| (pack_wt_kernel), [1] = the activation range flag
// (common.h RangeCheck).  The ops fail like the model does: weights beyond the half-plane range -> MSD_ERR_UNSUPPORTED
// (msd_finalize_weights), activations beyond it -> MSD_ERR_RANGE.
struct OpKit {
  hipStream_t s;
  int np;   // planes per operand
  int rc = MSD_OK;   // the first failure of a helper below
  msd_model ctx_model;
  Ctx c;
  unsigned* flags = nullptr;
  unsigned range_flag = 0;   // the activation range flag as finish() read it
  std::vector<void*> owned;

  OpKit(hipStream_t s_, int planes_) : s(s_), np(planes_), c{&ctx_model, s_} { ctx_model.NP = planes_; }
  OpKit(const OpKit&) = delete;   // (c points into this object)
  ~OpKit() { for (void* q : owned) (void)hipFree(q); }

  bool ok(hipError_t e) {
    if (e != hipSuccess && rc == MSD_OK) rc = MSD_ERR_HIP;
    return e == hipSuccess;
  }
  template <class Tp> Tp* get(size_t n) {
    void* q = nullptr;
    if (!ok(hipMalloc(&q, n * sizeof(Tp) + 16))) return nullptr;
    (void)hipMemset(q, 0, n * sizeof(Tp) + 16);
    (void)hipStreamSynchronize(nullptr);   // the ops run on the caller's (possibly non-blocking) stream
    owned.push_back(q);
    return static_cast<Tp*>(q);
  }
  // n host elements as new scratch; synchronises (the source may be a temporary).  nullptr on failure.
  template <class Tp> Tp* put(const Tp* host, size_t n) {
    Tp* q = get<Tp>(n);
    const bool done = q && ok(hipMemcpyAsync(q, host, n * sizeof(Tp), hipMemcpyHostToDevice, s)) && ok(hipStreamSynchronize(s));
    return done ? q : nullptr;
  }

  // zeroed planes (one when np == 1: p[1] stays null, the operand convention); `nan`: every element a NaN instead
  bool planes(size_t n, Planes* out, bool nan = false) {
    for (int i = 0; i < np; ++i) {
      out->p[i] = get<h16_t>(n);
      if (!out->p[i]) return false;
      if (nan && !ok(hipMemsetAsync(out->p[i], 0xFF, n * sizeof(h16_t), s))) return false;
    }
    return true;
  }
  // an fp32 array as new planes
  bool operand(const float* in, size_t n, Planes* out) {
    if (!planes(n, out)) return false;
    split(in, *out, (int64_t)n, s, sat());
    return true;
  }
  // W fp32 [K, N] (reference layout) -> rows [row0, row0 + N) of packed W^T planes [rows, K], allocated on first use
  bool weight(const float* w, int K, int N, int mode, int row0, Planes* out, int rows) {
    if (!out->p[0] && !planes((size_t)rows * K, out)) return false;
    dim3 grid((K + 63) / 64, N), block(64);
    hipLaunchKernelGGL(pack_wt_kernel, grid, block, 0, s, w, K, N, out->p[0], out->p[1], row0, mode, 0, absmax());
    return ok(hipGetLastError());
  }
  // planes -> fp32
  void back(const Planes& pl, float* out, size_t n) { merge(pl, out, (int64_t)n, s); }

  // p on tile T of launch site (TK, Epi), through the product's dispatch (gemm_on on the site's tile table); skipped after
  // an error, which c.err keeps
  template <int TK, class T, class Epi> void launch_on(int kc, const GemmParams& p, const Epi& epi) {
    static_assert(in_list<Site<TK, Epi>>(GemmSites<2>{}) && in_list<T>(TileTable<2, TK, Epi>{}), "not a tile of a launch site");
    if (c.err == hipSuccess) gemm_on<2>(TileTable<2, TK, Epi>{}, shape_of<T>(), c, kc, p, epi);
  }

  // The weight target of a carrier op (msd_op_*_carrier): two planes [rows][k] in ONE allocation of exactly their size --
  // the last line a touch may read ends at the allocation's end -- in the form the caller asks for.  form 0: no target.
  bool carrier_target(const msd_carrier_args* ca, WeightPrefetch* pf) {
    *pf = WeightPrefetch();
    if (ca->form == 0) return true;
    void* q = nullptr;
    const size_t plane = (size_t)ca->target_rows * ca->target_k * sizeof(h16_t);
    if (!ok(hipMalloc(&q, 2 * plane))) return false;
    owned.push_back(q);
    if (!ok(hipMemsetAsync(q, 0, 2 * plane, s))) return false;
    Planes w;
    w.p[0] = static_cast<h16_t*>(q); w.p[1] = w.p[0] + (size_t)ca->target_rows * ca->target_k;
    *pf = prefetch_of<2>(&ctx_model, w, ca->target_rows, ca->target_k);
    if (ca->form == 2) { pf->touch_blocks = ca->n_touch; pf->touch_delay = ca->delay; }
    return true;
  }

  // the range flags: init_flags() before the first operand, arm() every launch that should report, finish() at the end
  bool init_flags() {
    flags = get<unsigned>(2);
    ctx_model.d_sat = sat();
    return flags != nullptr;
  }
  unsigned* absmax() const { return flags; }
  unsigned* sat() const { return flags ? flags + 1 : nullptr; }
  template <class P> void arm(P& p) const { p.sat = sat(); p.sat_tag = 1; }
  // z and planes `zp` of this kit as the output of p, armed: the product's filler (z_out) on the kit's own context
  template <class P> void z_out_to(P& p, float* z, const Planes& zp) {
    ctx_model.z = z; ctx_model.zp = zp;
    z_out(p, &ctx_model, 1u);
  }
  int finish() {   // synchronises
    unsigned h[2] = {0, 0};
    if (hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return MSD_ERR_HIP;
    range_flag = h[1];
    if (kPlaneSaturates) {
      float top;
      memcpy(&top, &h[0], sizeof(top));
      if (!(top < kPlaneMax / kWScale)) return MSD_ERR_UNSUPPORTED;
      if (h[1]) return MSD_ERR_RANGE;
    }
    return MSD_OK;
  }
};

// The one GEMM instance here that is NOT in the tile table, a test-only one: the float32 store on the wide square tile
// (the decoder stores float32 from narrow tiles only), msd_op_gemm_h16's kernel and the consumer of
// msd_op_residual_norm_gemm.
template <int NP>
hipError_t launch_wide_store_f32(const GemmParams& p, const EpiStoreF32& epi, hipStream_t s) {
  return launch_gemm_h16_dma<NP, WideTile::BM, WideTile::BN, WideTile::NS>(p, epi, s);
}

// ---- one GEMM launch site at a time, through the product's dispatcher (tests/test_gpu_gemm_sites.py) ----------------
struct TileInfo { int bm = 0, bn = 0, ns = 0; };
template <class... T> std::vector<TileInfo> tiles_of(List<T...>) { return {TileInfo{T::BM, T::BN, T::NS}...}; }
template <class... P> std::vector<TileInfo> first_tiles_of(List<P...>) { return {TileInfo{P::P1::BM, P::P1::BN, P::P1::NS}...}; }
template <class... P> std::vector<TileInfo> second_tiles_of(List<P...>) { return {TileInfo{P::P2::BM, P::P2::BN, P::P2::NS}...}; }
const TileInfo* find_tile(const std::vector<TileInfo>& v, TileShape t) {
  for (const TileInfo& x : v)
    if (x.bm == t.bm && x.bn == t.bn) return &x;
  return nullptr;
}
template <int NP, class Epi, class... T>
bool persistent_on(List<T...>, TileShape t, const msd_model* m, const GemmParams& p, const Epi& epi) {
  return ((T::is(t) && runs_persistent<NP, T, Epi>(m, p, epi)) || ...);
}
template <int NP, class Epi, class... T>
int touch_blocks_on(List<T...>, TileShape t, const GemmParams& p) {
  int n = 0;
  ((T::is(t) ? (void)(n = gemm_touch_blocks<NP, T::BM, T::BN, T::NS, Epi>(p)) : (void)0), ...);
  return n;
}
// the launch sites by name, from their types (msd_op_gemm_site_name)
template <int TK, int NP> const char* site_name(Site<TK, EpiQKV<NP>>) { return "qkv"; }
template <int TK, int NP> const char* site_name(Site<TK, EpiGeglu<NP>>) { return "mlp_in"; }
template <int TK> const char* site_name(Site<TK, EpiResidual>) { return TK == TK_TALL ? "residual_tall" : "residual_square"; }
template <int TK, int NP, bool DUP, bool Y2> const char* site_name(Site<TK, EpiResidualNorm<NP, DUP, Y2>>) {
  return TK == TK_TALL ? (DUP ? "resnorm_tall_dup" : (Y2 ? "resnorm_tall_y2" : "resnorm_tall")) : "resnorm_square";
}
template <int TK, int NP> const char* site_name(Site<TK, EpiStoreH16<NP>>) { return "store_h16"; }
template <int TK> const char* site_name(Site<TK, EpiStoreF32>) { return "store_f32"; }
template <int TK, int NP> const char* site_name(Site<TK, EpiInProj<NP>>) { return "in_proj"; }
template <class Pairs> const char* site_name(DualSite<Pairs, EpiQKV<2>, EpiStoreF32>) { return "dual_qkv"; }
template <class Pairs, bool DUP> const char* site_name(DualSite<Pairs, EpiResidualNorm<2, DUP>, EpiAddStoreH16<2>>) {
  return DUP ? "dual_out_dup" : "dual_out";
}

// f(S{}) for the index-th entry of a list of (empty) site types; false: no such entry
template <class F, class... S>
bool visit_at(List<S...>, int index, F&& f) {
  int i = 0;
  return ((i++ == index ? (f(S{}), true) : false) || ...);
}
template <class... S> constexpr int list_size(List<S...>) { return (int)sizeof...(S); }
// f(site) for the site at position `index` of GemmSites<NP>, then (two-plane modes) of DualSites; false: no such site
template <int NP, class F>
bool visit_site(int index, F&& f) {
  if (visit_at(GemmSites<NP>{}, index, f)) return true;
  if constexpr (NP == 2) return visit_at(DualSites{}, index - list_size(GemmSites<NP>{}), f);
  else return false;
}

template <int NP> struct SiteTiles {
  std::vector<TileInfo> first, second;   // second: dual sites only
  template <int TK, class Epi> void operator()(Site<TK, Epi>) { first = tiles_of(TileTable<NP, TK, Epi>{}); }
  template <class Pairs, class E1, class E2> void operator()(DualSite<Pairs, E1, E2>) {
    first = first_tiles_of(Pairs{});
    second = second_tiles_of(Pairs{});
  }
};

// One site launch: the caller's msd_gemm_site_args on an OpKit of NP planes.
template <int NP>
struct SiteRun : OpKit {
  msd_gemm_site_args* g;
  msd_carrier_args* carrier;   // msd_op_gemm_site_carrier: the target and its form come from here, not from g->prefetch
  int* step = nullptr;

  SiteRun(msd_gemm_site_args* g_, hipStream_t s_, msd_carrier_args* ca = nullptr) : OpKit(s_, NP), g(g_), carrier(ca) {}

  bool bad() { rc = MSD_ERR_INVALID_ARGUMENT; return false; }

  bool init() {
    if (!init_flags()) return false;
    step = get<int>(2);
    if (!step) return false;
    const int st[2] = {g->step, -1};
    if (!ok(hipMemcpyAsync(step, st, sizeof(st), hipMemcpyHostToDevice, s)) || !ok(hipStreamSynchronize(s))) return false;
    ctx_model.persist_mlp_in = g->persistent != 2;
    ctx_model.prefetch = true;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
      ctx_model.cus = cus;
    if (g->resident_blocks > 0) ctx_model.cus = g->resident_blocks;
    return true;
  }
  int finish() {
    int st[2] = {0, 0};
    if (!ok(hipGetLastError()) || !ok(hipMemcpyAsync(st, step, sizeof(st), hipMemcpyDeviceToHost, s))) return rc;
    const int frc = OpKit::finish();   // synchronises
    g->step_copy = st[1];
    return frc;
  }
  // folded-norm row scale of a consumer site: rstd from the caller's [M][K / 32] partial sums, + the step-indexed bias row
  bool row_scale_of(int K, const float* bias, int N, RowScale* out) {
    *out = RowScale();
    if (!g->ssq) return bias ? bad() : true;
    if (K / kNarrowTile > kAuxMaxTiles) return bad();
    *out = row_scale(g->ssq, K / kNarrowTile, step, bias, bias ? N : 0);
    return true;
  }
  WeightPrefetch pf_target() {
    WeightPrefetch pf;
    if (carrier) {
      if constexpr (NP == 2) (void)carrier_target(carrier, &pf);
      return pf;
    }
    if (!g->prefetch) return pf;
    Planes w;
    w.p[0] = static_cast<h16_t*>(const_cast<void*>(g->prefetch));
    w.p[1] = w.p[0] + (size_t)g->prefetch_rows * g->prefetch_k;
    pf = prefetch_of<NP>(&ctx_model, w, g->prefetch_rows, g->prefetch_k);
    return pf;
  }
  bool common_ok(int M, int N, int K, const float* a, const float* w) {
    if (M <= 0 || N <= 0 || K <= 0 || K % kGemmBK || !a || !w) return bad();
    if (g->prefetch && (g->prefetch_rows <= 0 || g->prefetch_k <= 0 || g->prefetch_k % kGemmBK || g->prefetch_k > 4096)) return bad();
    if (g->resident_blocks < 0 || g->resident_blocks % 8) return bad();
    return true;
  }

  // The launch of a single site: the product's gemm<NP, TK, Epi> when no tile is forced; gemm_on on the forced tile, with
  // gemm's own launch parameters, otherwise.  Reported: the table's entry of that shape, or its last one (the fall-back).
  template <int TK, class Epi>
  bool launch(int kc, const Planes& a, const Planes& w, int M, int N, int K, const Epi& epi, int align) {
    using Tab = TileTable<NP, TK, Epi>;
    const std::vector<TileInfo> tiles = tiles_of(Tab{});
    TileShape t = {g->force_bm, g->force_bn};
    const bool forced = t.bm != 0 || t.bn != 0;
    if (!forced) t = pick_tile<NP, TK>(M, N, align, epi_takes_48<Epi>::value, K);
    const TileInfo* ti = find_tile(tiles, t);
    if (!ti) {
      if (forced) return bad();
      ti = &tiles.back();
    }
    if (M % ti->bm || M % t.bm || N % ti->bn || align % ti->bn) return bad();
    const WeightPrefetch pf = pf_target();
    GemmParams probe;
    set_xcd_grid(probe, M, t.bm);
    g->ran_bm = ti->bm; g->ran_bn = ti->bn; g->ran_ns = ti->ns; g->ran_xcd_rows = probe.xcd_rows;
    const GemmParams lp = gp_launch<NP>(c, kc, a, K, w, K, M, N, K, t.bm, pf);
    // both reports come from the predicates the launch itself uses (gemm_t, launch_gemm_h16_dma / _geglu_persist)
    g->ran_persistent = persistent_on<NP, Epi>(Tab{}, TileShape{ti->bm, ti->bn}, &ctx_model, lp, epi);
    g->ran_prefetch = g->ran_persistent ? lp.pf.active() : gemm_carries_prefetch<NP, Epi>(lp);
    if (carrier) {   // the launcher's own rule, on the tile that runs (gemm_h16.h gemm_touch_blocks)
      const int n_touch = g->ran_persistent ? 0 : touch_blocks_on<NP, Epi>(Tab{}, TileShape{ti->bm, ti->bn}, lp);
      carrier->ran_touch_blocks = n_touch;
      carrier->ran_form = n_touch > 0 ? 2 : (g->ran_prefetch ? 1 : 0);
    }
    if (forced) gemm_on<NP>(Tab{}, t, c, kc, lp, epi);
    else gemm<NP, TK>(c, kc, a, K, w, K, M, N, K, epi, align, pf);
    return ok(c.err);
  }
  template <class Pairs, class E1, class E2>
  bool launch_dual(int kc, const Planes& a1, const Planes& w1, int M1, int N1, int K1, const E1& e1, int align1,
                   const Planes& a2, const Planes& w2, int M2, int N2, int K2, const E2& e2) {
    const std::vector<TileInfo> t1s = first_tiles_of(Pairs{}), t2s = second_tiles_of(Pairs{});
    const TileShape t1 = {g->force_bm, g->force_bn}, t2 = {g->force_bm2, g->force_bn2};
    const TileInfo *i1 = nullptr, *i2 = nullptr;
    for (size_t i = 0; i < t1s.size() && !i1; ++i)
      if (t1s[i].bm == t1.bm && t1s[i].bn == t1.bn && t2s[i].bm == t2.bm && t2s[i].bn == t2.bn) { i1 = &t1s[i]; i2 = &t2s[i]; }
    if (!i1) return bad();   // the step plan names both tiles of a dual launch: there is nothing to pick here
    if (M1 % t1.bm || N1 % t1.bn || align1 % t1.bn || M2 % t2.bm || N2 % t2.bn) return bad();
    const WeightPrefetch pf = pf_target();
    const GemmParams p1 = gp_launch<NP>(c, kc, a1, K1, w1, K1, M1, N1, K1, t1.bm, pf);
    const GemmParams p2 = gp_launch<NP>(c, kc, a2, K2, w2, K2, M2, N2, K2, t2.bm);
    g->ran_bm = i1->bm; g->ran_bn = i1->bn; g->ran_ns = i1->ns; g->ran_xcd_rows = p1.xcd_rows;
    g->ran_bm2 = i2->bm; g->ran_bn2 = i2->bn; g->ran_ns2 = i2->ns; g->ran_xcd_rows2 = p2.xcd_rows;
    g->ran_dual = 1;
    g->ran_prefetch = p1.pf.active();   // (launch_gemm_h16_dual's own test)
    gemm_dual<Pairs>(c, kc, t1, p1, e1, t2, p2, e2);
    return ok(c.err);
  }

  // ---- operands and results of each epilogue ----
  struct QkvIo { Planes a, w, qk, vt; int J = 0; };
  bool qkv_prepare(QkvIo* io, EpiQKV<NP>* e) {
    const int M = g->m, N = g->n, K = g->k, J = N / 3;
    if (!common_ok(M, N, K, g->a, g->w) || N % 3 || J % 16 || !g->out || g->seg_len <= 0 || g->seg_len % 16 || M % g->seg_len)
      return bad();
    RowScale rs;
    if (!row_scale_of(K, g->bias, N, &rs)) return false;
    io->J = J;
    if (!operand(g->a, (size_t)M * K, &io->a) || !weight(g->w, K, N, 0, 0, &io->w, N) ||
        !planes((size_t)M * 2 * J, &io->qk, true) || !planes((size_t)M * J, &io->vt, true))
      return false;
    *e = epi_qkv<NP>(io->qk, io->vt, 2 * J, g->seg_len, J, rs);
    return true;
  }
  // q | k row-major and V^T[seg][j][vt_key_pos(key)] -> out [M][3J] = q | k | v.  The ONLY un-permutation (msd_op_qkv
  // runs this site).
  bool qkv_collect(const QkvIo& io) {
    const int M = g->m, J = io.J, L = g->seg_len;
    float* f32 = get<float>((size_t)M * 2 * J);
    if (!f32) return false;
    std::vector<float> h((size_t)M * 2 * J), o((size_t)M * 3 * J);
    back(io.qk, f32, (size_t)M * 2 * J);
    if (!ok(hipMemcpyAsync(h.data(), f32, h.size() * sizeof(float), hipMemcpyDeviceToHost, s)) || !ok(hipStreamSynchronize(s)))
      return false;
    for (int m = 0; m < M; ++m)
      memcpy(&o[(size_t)m * 3 * J], &h[(size_t)m * 2 * J], (size_t)2 * J * sizeof(float));
    back(io.vt, f32, (size_t)M * J);
    if (!ok(hipMemcpyAsync(h.data(), f32, (size_t)M * J * sizeof(float), hipMemcpyDeviceToHost, s)) || !ok(hipStreamSynchronize(s)))
      return false;
    for (int m = 0; m < M; ++m) {
      const int seg = m / L, kp = vt_key_pos(m % L);
      for (int j = 0; j < J; ++j) o[(size_t)m * 3 * J + 2 * J + j] = h[((size_t)seg * J + j) * L + kp];
    }
    return ok(hipMemcpyAsync(g->out, o.data(), o.size() * sizeof(float), hipMemcpyHostToDevice, s)) && ok(hipStreamSynchronize(s));
  }

  struct ResNormIo { Planes a, w, y, y2; int rows = 0; };
  template <bool DUP, bool Y2>
  bool resnorm_prepare(ResNormIo* io, EpiResidualNorm<NP, DUP, Y2>* e) {
    const int M = g->m, N = g->n, K = g->k;
    if (!common_ok(M, N, K, g->a, g->w) || N % kNarrowTile || !g->x || !g->y || !g->ssq_out || g->split_row < 0) return bad();
    if (DUP && (g->dup_rows < M || !g->g_lo || !g->g_hi)) return bad();   // (the duplicating form reads both gain rows)
    if (Y2 && (!g->y2 || !g->g2 || g->y2_rows < 0 || g->y2_rows > M)) return bad();
    io->rows = DUP ? g->dup_rows + M : M;
    if (!operand(g->a, (size_t)M * K, &io->a) || !weight(g->w, K, N, 0, 0, &io->w, N) ||
        !planes((size_t)io->rows * N, &io->y, true))
      return false;
    const EpiResidualNorm<NP> base = epi_residual_norm<NP>(g->x, N, io->y, g->ssq_out, step, Gain{g->g_lo, g->g_lo ? N : 0},
                                                           Gain{g->g_hi, g->g_hi ? N : 0}, g->split_row);
    *e = residual_form<DUP, Y2>(base);
    if (DUP) { e->split_row = 0; e->dup_rows = g->dup_rows; }
    if constexpr (Y2) {
      if (!planes((size_t)M * N, &io->y2, true)) return false;
      out_pair<NP>(e->y2, io->y2); e->g2 = g->g2; e->y2_rows = g->y2_rows;
    }
    return true;
  }
  bool resnorm_collect(const ResNormIo& io, bool y2) {
    back(io.y, g->y, (size_t)io.rows * g->n);
    if (y2) back(io.y2, g->y2, (size_t)g->m * g->n);
    return true;
  }

  // ---- the sites ----
  template <int TK> void run(Site<TK, EpiQKV<NP>>) {
    QkvIo io;
    EpiQKV<NP> e;
    if (qkv_prepare(&io, &e) && launch<TK>(KC_GEMM_QKV, io.a, io.w, g->m, g->n, g->k, e, e.v_start)) qkv_collect(io);
  }
  template <int TK> void run(Site<TK, EpiGeglu<NP>>) {
    const int M = g->m, N = g->n, K = g->k, F = N / 2;
    if (!common_ok(M, N, K, g->a, g->w) || N % 32 || !g->w_gate || !g->out) return (void)bad();
    Planes a, wi, o;
    const float* bias = nullptr;
    if (g->bias) {   // natural order [steps][wi_0 columns | wi_1 columns] -> the packed column order of the weights
      if (g->steps <= 0) return (void)bad();
      std::vector<float> h((size_t)g->steps * N), p((size_t)g->steps * N);
      float* d = get<float>(p.size());
      if (!d || !ok(hipMemcpyAsync(h.data(), g->bias, h.size() * sizeof(float), hipMemcpyDeviceToHost, s)) || !ok(hipStreamSynchronize(s)))
        return;
      for (int r = 0; r < g->steps; ++r)
        for (int j = 0; j < F; ++j) {
          p[(size_t)r * N + (j / 16) * 32 + j % 16] = h[(size_t)r * N + j];
          p[(size_t)r * N + (j / 16) * 32 + 16 + j % 16] = h[(size_t)r * N + F + j];
        }
      if (!ok(hipMemcpyAsync(d, p.data(), p.size() * sizeof(float), hipMemcpyHostToDevice, s)) || !ok(hipStreamSynchronize(s))) return;
      bias = d;
    }
    RowScale rs;
    if (!row_scale_of(K, bias, N, &rs)) return;
    if (!operand(g->a, (size_t)M * K, &a) || !weight(g->w, K, F, 1, 0, &wi, N) || !weight(g->w_gate, K, F, 2, 0, &wi, N) ||
        !planes((size_t)M * F, &o, true))
      return;
    if (launch<TK>(KC_GEMM_MLP_IN, a, wi, M, N, K, epi_out<EpiGeglu, NP>(o, F, rs), 0)) back(o, g->out, (size_t)M * F);
  }
  template <int TK> void run(Site<TK, EpiResidual>) {
    const int M = g->m, N = g->n, K = g->k;
    if (!common_ok(M, N, K, g->a, g->w) || !g->x) return (void)bad();
    Planes a, w;
    if (!operand(g->a, (size_t)M * K, &a) || !weight(g->w, K, N, 0, 0, &w, N)) return;
    launch<TK>(KC_GEMM_MLP_OUT, a, w, M, N, K, EpiResidual{g->x, N}, 0);
  }
  template <int TK, bool DUP, bool Y2> void run(Site<TK, EpiResidualNorm<NP, DUP, Y2>>) {
    ResNormIo io;
    EpiResidualNorm<NP, DUP, Y2> e;
    if (resnorm_prepare<DUP, Y2>(&io, &e) && launch<TK>(KC_GEMM_ATTN_OUT, io.a, io.w, g->m, g->n, g->k, e, 0)) resnorm_collect(io, Y2);
  }
  template <int TK> void run(Site<TK, EpiStoreH16<NP>>) {
    const int M = g->m, N = g->n, K = g->k;
    if (!common_ok(M, N, K, g->a, g->w) || !g->out) return (void)bad();
    RowScale rs;
    Planes a, w, o;
    if (!row_scale_of(K, g->bias, N, &rs) || !operand(g->a, (size_t)M * K, &a) || !weight(g->w, K, N, 0, 0, &w, N) ||
        !planes((size_t)M * N, &o, true))
      return;
    if (launch<TK>(KC_GEMM_CROSS_Q, a, w, M, N, K, epi_out<EpiStoreH16, NP>(o, N, rs), 0)) back(o, g->out, (size_t)M * N);
  }
  template <int TK> void run(Site<TK, EpiStoreF32>) {
    const int M = g->m, N = g->n, K = g->k;
    if (!common_ok(M, N, K, g->a, g->w) || !g->out) return (void)bad();
    RowScale rs;
    Planes a, w;
    if (!row_scale_of(K, g->bias, N, &rs) || !operand(g->a, (size_t)M * K, &a) || !weight(g->w, K, N, 0, 0, &w, N)) return;
    launch<TK>(KC_FINAL_PROJ, a, w, M, N, K, epi_store_f32(g->out, N, rs), 0);
  }
  template <int TK> void run(Site<TK, EpiInProj<NP>>) {
    const int M = g->m, N = g->n, K = g->k, P = g->passes;
    if (!common_ok(M, N, K, g->a, g->w) || N % kNarrowTile || !g->pos || !g->g_lo || !g->x || !g->y || !g->ssq_out ||
        g->seg_len <= 0 || P < 1 || P > 2 || (g->g2 != nullptr) != (g->y2 != nullptr))
      return (void)bad();
    Planes a, w, y, y2;
    if (!operand(g->a, (size_t)M * K, &a) || !weight(g->w, K, N, 0, 0, &w, N) || !planes((size_t)P * M * N, &y, true)) return;
    EpiInProj<NP> ei;
    ei.x = g->x; ei.ldx = N; ei.pos = g->pos; ei.T = g->seg_len; ei.pass_rows = M; ei.passes = P;
    out_pair<NP>(ei.y, y); ei.ssq = g->ssq_out; ei.tiles = N / kNarrowTile;
    ei.g = g->g_lo; ei.g_stride = N; ei.step_ptr = step; ei.step_copy = step;
    if (g->g2) {
      if (!planes((size_t)M * N, &y2, true)) return;
      out_pair<NP>(ei.y2, y2); ei.g2 = g->g2;
    }
    if (!launch<TK>(KC_IN_PROJ, a, w, M, N, K, ei, 0)) return;
    back(y, g->y, (size_t)P * M * N);
    if (g->g2) back(y2, g->y2, (size_t)M * N);
  }
  // dual sites (two-plane modes): problem 1 as its single site, problem 2 from a2 / w2 (/ addend2) into out2
  bool second_operands(Planes* a2, Planes* w2) {
    if (g->m2 <= 0 || g->n2 <= 0 || g->k2 <= 0 || g->k2 % kGemmBK || !g->a2 || !g->w2 || !g->out2) return bad();
    return operand(g->a2, (size_t)g->m2 * g->k2, a2) && weight(g->w2, g->k2, g->n2, 0, 0, w2, g->n2);
  }
  template <class Pairs> void run(DualSite<Pairs, EpiQKV<2>, EpiStoreF32>) {
    if constexpr (NP == 2) {
      QkvIo io;
      EpiQKV<NP> e;
      Planes a2, w2;
      if (!qkv_prepare(&io, &e) || !second_operands(&a2, &w2)) return;
      if (launch_dual<Pairs>(KC_GEMM_QKV, io.a, io.w, g->m, g->n, g->k, e, e.v_start, a2, w2, g->m2, g->n2, g->k2,
                             epi_store_f32(g->out2, g->n2)))
        qkv_collect(io);
    }
  }
  template <class Pairs, bool DUP> void run(DualSite<Pairs, EpiResidualNorm<2, DUP>, EpiAddStoreH16<2>>) {
    if constexpr (NP == 2) {
      ResNormIo io;
      EpiResidualNorm<NP, DUP> e;
      Planes a2, w2, o2;
      if (!resnorm_prepare<DUP, false>(&io, &e) || !second_operands(&a2, &w2) || !g->addend2) return (void)(rc = rc ? rc : MSD_ERR_INVALID_ARGUMENT);
      if (!planes((size_t)g->m2 * g->n2, &o2, true)) return;
      EpiAddStoreH16<NP> ea;
      out_pair<NP>(ea.out, o2); ea.ldc = g->n2; ea.addend = g->addend2; ea.ld_add = g->n2;
      if (!launch_dual<Pairs>(KC_GEMM_ATTN_OUT, io.a, io.w, g->m, g->n, g->k, e, 0, a2, w2, g->m2, g->n2, g->k2, ea)) return;
      resnorm_collect(io, false);
      back(o2, g->out2, (size_t)g->m2 * g->n2);
    }
  }
};

// the site of type S on the caller's arguments
template <int NP, class S>
int run_site(msd_gemm_site_args* g, hipStream_t s, S site, msd_carrier_args* ca = nullptr) {
  SiteRun<NP> r(g, s, ca);
  if (!r.init()) return r.rc;
  r.run(site);
  const int frc = r.finish();
  if (ca) ca->ran_range_flag = (int32_t)r.range_flag;
  return r.rc ? r.rc : frc;
}
// ... and the site at position g->site
template <int NP>
int run_gemm_site(msd_gemm_site_args* g, hipStream_t s, msd_carrier_args* ca = nullptr) {
  int rc = MSD_ERR_INVALID_ARGUMENT;   // no such site
  visit_site<NP>(g->site, [&](auto site) { rc = run_site<NP>(g, s, site, ca); });
  return rc;
}
// arguments of a site run that the library itself makes (msd_op_geglu, msd_op_qkv): two planes, one step, a forced tile
msd_gemm_site_args forced_site_args(TileShape tile, int M, int N, int K) {
  msd_gemm_site_args g = {};
  g.struct_size = (int32_t)sizeof(g);
  g.m = M; g.n = N; g.k = K; g.steps = 1; g.force_bm = tile.bm; g.force_bn = tile.bn;
  return g;
}

// The form of a stand-alone sampler launch, as its entry point (msd_op_sampler_step*) describes it: the forms combine as
// the product's do (enqueue_step) -- guided with either update, known frames with the plain update only.
struct SamplerOpForm {
  const float* noise = nullptr;      // the plain update's draw of this step; NULL = zeros.  (The multistep update draws nothing.)
  const float* known = nullptr;      // != NULL: the keep form on the known mel in model units, with
  const int32_t* keep = nullptr;     // ... its frames' release words, or -- flags -- msd_sample_keep's flags (any non-zero =
  int n_dims = 0;                    //     known throughout)
  bool flags = false;
  float* x0_prev = nullptr;          // != NULL: the multistep update with this history, at the call's first step or not
  int first = 0;
  bool guided = false;               // the guided form: `rows` finite host weights, one per row of n / rows elements, each
  const float* weights = nullptr;    // a whole number of the sampler's blocks (a block reads ONE weight)
  int rows = 0;
};

// What msd_op_sampler_step_planes asks of the launch beyond z, and what it returns
struct SamplerOpPlanes {
  float* planes_out = nullptr;   // device [n]: z_out's operand planes of cfg->precision, merged back to float32
  unsigned range_flag = 0;       // the activation range flag as finish() read it
  int next_step = 0;             // the scan index the launch published
};

// One launch of the sampler update on the caller's arrays, in form f.  What the forms share, in ONE place: the argument
// checks, the coefficient rows of cfg, the staged operands -- the passes of the model output side by side (the guided forms
// stage the unconditional output whatever cfg->cfg_weight is: their weights come from a table), z copied into z_out (the
// kernel updates in place), the scan index in both slots -- and the SamplerParams every form starts from (no planes).
// Then the draw (noise, slot, key rows) or the multistep side table, staged once each, and the launch of the form's arguments.
// With `po` (msd_op_sampler_step_planes) the launch also writes z_out's operand planes of cfg->precision and feeds the range
// flag, as the product's launches do (z_out), and the op returns what it would otherwise leave behind: the planes merged
// back to float32, the flag word and the scan index the launch published (slot 0: step_from_slot1).
int op_sampler_step(const msd_config* cfg, int step_index, const float* z_dev, const float* out_cond_dev,
                    const float* out_uncond_dev, float* z_out_dev, int64_t n, void* stream, const SamplerOpForm& f,
                    SamplerOpPlanes* po = nullptr) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int NP = po && cfg && cfg->struct_size == (int32_t)sizeof(msd_config) ? op_planes(cfg->precision) : 1;
  if (NP < 0) return MSD_ERR_UNSUPPORTED;
  OpKit kit(s, NP);
  SamplerMultistepGuidedParams sp;   // the widest form's arguments; the other forms' are its bases
  if (f.guided) {
    if (!f.weights || f.rows < 1 || n <= 0 || n % f.rows || (n / f.rows) % kRngRowBlock) return MSD_ERR_INVALID_ARGUMENT;
    for (int b = 0; b < f.rows; ++b)
      if (!std::isfinite(f.weights[b])) return MSD_ERR_INVALID_ARGUMENT;
    sp.row_wt = kit.put(f.weights, (size_t)f.rows);
    if (!sp.row_wt) return MSD_ERR_HIP;
    sp.row_blocks = (int)(n / f.rows / kRngRowBlock);
  }
  if (!cfg || cfg->struct_size != (int32_t)sizeof(msd_config) || !z_dev || !out_cond_dev || !z_out_dev ||
      n <= 0 || n % 4 || n > 0x7FFFFFFFll || step_index < 0 || step_index >= cfg->num_steps)
    return MSD_ERR_INVALID_ARGUMENT;
  const int passes = (f.guided || cfg->cfg_weight != 1.0f) ? 2 : 1;
  if (passes == 2 && !out_uncond_dev) return MSD_ERR_INVALID_ARGUMENT;
  std::vector<float> rows, ms;
  std::string why;
  if (!build_coef_rows(*cfg, &rows, &why)) return MSD_ERR_INVALID_ARGUMENT;
  Planes zp;
  if (po && !po->planes_out) return MSD_ERR_INVALID_ARGUMENT;
  if (po && (!kit.init_flags() || !kit.planes((size_t)n, &zp))) return MSD_ERR_HIP;
  const int st[2] = {step_index, step_index};
  float* eps = kit.get<float>((size_t)passes * n);
  sp.coef = kit.put(rows.data(), rows.size());
  sp.step_ptr = kit.put(st, 2);
  if (!eps || !sp.coef || !sp.step_ptr) return MSD_ERR_HIP;
  if (hipMemcpyAsync(eps, out_cond_dev, n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess ||
      (passes == 2 && hipMemcpyAsync(eps + n, out_uncond_dev, n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) ||
      hipMemcpyAsync(z_out_dev, z_dev, n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return MSD_ERR_HIP;
  sp.eps = eps; sp.z = z_out_dev; sp.noise_slot = nullptr;
  sp.n = (int)n; sp.passes = passes; sp.cond_wt = cfg->cfg_weight; sp.clip_x0 = cfg->clip_x0;
  sp.ddim = 0; sp.model_output = cfg->model_output;
  sp.z_hi = nullptr; sp.z_lo = nullptr; sp.step_from_slot1 = 1;
  if (po) kit.z_out_to(sp, z_out_dev, zp);   // (every form below starts from a copy of sp)
  if (f.x0_prev) {   // (noise_slot / rng_key stay null: the form makes no draw and reads neither)
    build_multistep_rows(rows, &ms);
    sp.coef_ms = kit.put(ms.data(), ms.size());
    if (!sp.coef_ms) return MSD_ERR_HIP;
    sp.x0_prev = f.x0_prev; sp.first_step = f.first ? step_index : -1;
  } else {
    float* noise = kit.get<float>((size_t)n);   // one step's draw (zeros) when the caller gives none
    // the kernel fetches the words of its own draw up front, used or not: one (zero) row per row of z (not guided: table
    // row 0 only, SamplerParams::row_blocks' default)
    sp.rng_key = kit.get<uint32_t>((size_t)(f.guided ? f.rows : 1) * kRngWords);
    if (!noise || !sp.rng_key) return MSD_ERR_HIP;
    // the kernel indexes noise as base + i * n: hand it base = draw - i * n
    const float* base = (f.noise ? f.noise : noise) - (size_t)step_index * n;
    sp.noise_slot = kit.put(&base, 1);
    if (!sp.noise_slot) return MSD_ERR_HIP;
    sp.ddim = cfg->sampler == MSD_SAMPLER_DDIM;
  }
  if (f.x0_prev) {
    if (f.guided) launch_sampler_step(sp, s);
    else launch_sampler_step(static_cast<const SamplerMultistepParams&>(sp), s);
  } else if (f.guided) {
    SamplerGuidedParams gp;
    static_cast<SamplerParams&>(gp) = sp;
    gp.row_wt = sp.row_wt;
    launch_sampler_step(gp, s);
  } else if (f.known) {
    SamplerKeepParams kp;
    static_cast<SamplerParams&>(kp) = sp;
    kp.xk = f.known; kp.keep = f.keep; kp.n_dims = f.n_dims;
    if (f.flags) {
      int32_t* words = kit.get<int32_t>((size_t)(n / f.n_dims));
      if (!words) return MSD_ERR_HIP;
      launch_normalize_flags(f.keep, words, (int)(n / f.n_dims), s);
      kp.keep = words;
    }
    launch_sampler_step(kp, s);
  } else {
    launch_sampler_step(static_cast<const SamplerParams&>(sp), s);
  }
  if (hipGetLastError() != hipSuccess) return MSD_ERR_HIP;
  if (!po) return hipStreamSynchronize(s) == hipSuccess ? MSD_OK : MSD_ERR_HIP;
  kit.back(zp, po->planes_out, (size_t)n);
  int published[2] = {0, 0};
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(published, sp.step_ptr, sizeof(published), hipMemcpyDeviceToHost, s) != hipSuccess)
    return MSD_ERR_HIP;
  const int frc = kit.finish();   // synchronises
  po->range_flag = kit.range_flag; po->next_step = published[0];
  return frc;
}

// ---- one attention launch the way the decoder fills it (tests/test_gpu_attention_forms.py) ---------------------------
// The caller's float32 arrays become planes that are NaN wherever the launch has no business: the operands are gathered
// dense, split (the range flag sees the caller's values only), and scattered into their place of all-NaN planes.
template <int NP>
struct AttnLaunchRun : OpKit {
  msd_attention_launch_args* g;
  msd_carrier_args* carrier;   // msd_op_attention_launch_carrier

  AttnLaunchRun(msd_attention_launch_args* g_, hipStream_t s_, msd_carrier_args* ca = nullptr) : OpKit(s_, NP), g(g_), carrier(ca) {}

  // `blocks` blocks of `rows` rows of `width` floats, block b from src + b * block_stride, row pitch ld -> dense planes
  bool gather(const float* src, size_t block_stride, int ld, int blocks, int rows, int width, Planes* out) {
    float* dense = get<float>((size_t)blocks * rows * width);
    if (!dense) return false;
    for (int b = 0; b < blocks; ++b)
      if (!ok(hipMemcpy2DAsync(dense + (size_t)b * rows * width, (size_t)width * sizeof(float), src + b * block_stride,
                               (size_t)ld * sizeof(float), (size_t)width * sizeof(float), rows, hipMemcpyDeviceToDevice, s)))
        return false;
    return operand(dense, (size_t)blocks * rows * width, out);
  }
  // dense planes [blocks][rows][width] -> block b at off + b * block_stride, row pitch ld, of new planes of `total`
  // elements, NaN everywhere else
  bool scatter(const Planes& dense, size_t total, size_t off, size_t block_stride, int ld, int blocks, int rows, int width,
               Planes* out) {
    if (!planes(total, out, true)) return false;
    for (int i = 0; i < np; ++i)
      for (int b = 0; b < blocks; ++b)
        if (!ok(hipMemcpy2DAsync(out->p[i] + off + b * block_stride, (size_t)ld * sizeof(h16_t),
                                 dense.p[i] + (size_t)b * rows * width, (size_t)width * sizeof(h16_t),
                                 (size_t)width * sizeof(h16_t), rows, hipMemcpyDeviceToDevice, s)))
          return false;
    return true;
  }

  int run() {
    const int heads = g->heads, segs = g->segs, rows = g->q_rows_per_seg, J = heads * kHeadDim;
    const int ka = g->k_alloc_rows, r0 = g->k_row0, kr = g->k_rows;
    const size_t total_rows = (size_t)segs * rows;
    const bool self = g->k == g->q;
    // n_keys: the kernel clamps its reads into the window whatever the count says, but a count beyond the window is no launch
    // of the decoder's
    std::vector<int32_t> nk(segs);
    if (!ok(hipMemcpy(nk.data(), g->n_keys, nk.size() * sizeof(int32_t), hipMemcpyDeviceToHost))) return rc;
    for (int32_t n : nk)
      if (n < 0 || n > kr) return MSD_ERR_INVALID_ARGUMENT;
    if (!init_flags()) return rc;
    ctx_model.prefetch = true;

    Planes q, k, vt, o, dense;
    if (self) {   // q | k interleaved in one buffer: split once, the whole of it is the launch's
      if (!operand(g->q, total_rows * g->ldq, &q)) return rc;
      k = q;
    } else {
      if (!gather(g->q + g->q_col, 0, g->ldq, 1, (int)total_rows, J, &dense) ||
          !scatter(dense, total_rows * g->ldq, (size_t)g->q_col, 0, g->ldq, 1, (int)total_rows, J, &q))
        return rc;
      if (!gather(g->k + (size_t)r0 * g->ldk + g->k_col, (size_t)ka * g->ldk, g->ldk, segs, kr, J, &dense) ||
          !scatter(dense, (size_t)segs * ka * g->ldk, (size_t)r0 * g->ldk + g->k_col, (size_t)ka * g->ldk, g->ldk, segs, kr, J, &k))
        return rc;
    }
    {   // the window of V -> V^T [segs][J][k_rows] with the per-16 key permutation (host copy, as msd_op_attention_ex),
        // then columns [k_row0, k_row0 + k_rows) of V^T [segs][J][k_alloc_rows]
      std::vector<float> vh((size_t)segs * ka * J), vth((size_t)segs * J * kr);
      if (!ok(hipMemcpy(vh.data(), g->v, vh.size() * sizeof(float), hipMemcpyDeviceToHost))) return rc;
      for (int sg = 0; sg < segs; ++sg)
        for (int key = 0; key < kr; ++key) {
          const int kp = vt_key_pos(key);
          const float* src = &vh[((size_t)sg * ka + r0 + key) * J];
          for (int j = 0; j < J; ++j) vth[((size_t)sg * J + j) * kr + kp] = src[j];
        }
      float* vt32 = get<float>(vth.size());
      if (!vt32 || !ok(hipMemcpy(vt32, vth.data(), vth.size() * sizeof(float), hipMemcpyHostToDevice)) ||
          !operand(vt32, vth.size(), &dense) ||
          !scatter(dense, (size_t)segs * J * ka, (size_t)r0, 0, ka, 1, segs * J, kr, &vt))
        return rc;
    }
    if (!planes(total_rows * J, &o, true)) return rc;

    AttnParams p;
    arm(p);
    p.qp = g->qp;
    p.allow_qb4 = g->allow_qb4 != 0;
    if (g->q_ssq) { p.q_ssq = g->q_ssq; p.q_tiles = g->q_tiles; p.q_inv_d = 1.0f / (float)(kNarrowTile * g->q_tiles); }
    const size_t k_off = (size_t)r0 * g->ldk + g->k_col;
    for (int i = 0; i < 2; ++i) {
      const int j = i < NP ? i : 0;
      p.q[i] = q.p[j] + g->q_col; p.k[i] = k.p[j] + k_off; p.vt[i] = vt.p[j] + r0; p.o[i] = o.p[j];
    }
    p.n_keys = g->n_keys; p.ldq = g->ldq; p.ldk = g->ldk; p.ldo = J; p.vt_ld = ka; p.q_rows_per_seg = rows;
    p.k_seg_stride = (size_t)ka * g->ldk; p.vt_seg_stride = (size_t)J * ka; p.k_rows = kr;
    p.vt_cols = (r0 == 0 && kr == ka) ? 0 : kr;
    p.ksplit = g->ksplit; p.part_o = nullptr; p.part_ml = nullptr; p.total_rows = (int)total_rows;
    p.touch_ahead = g->touch_ahead; p.pf_late = g->pf_late;
    if (carrier) {
      if constexpr (NP == 2) { if (!carrier_target(carrier, &p.pf)) return rc; }
    } else if (g->prefetch_rows) {
      Planes w;
      if (!planes((size_t)g->prefetch_rows * g->prefetch_k, &w)) return rc;
      p.pf = prefetch_of<NP>(&ctx_model, w, g->prefetch_rows, g->prefetch_k);
    }
    AttnParams ran = p;   // as launch_attention will see it: the split a power of two
    ran.ksplit = 1 << attention_ksplit_log2(p.ksplit);
    if (ran.ksplit > 1) {
      p.part_o = get<float>((size_t)ran.ksplit * total_rows * J);
      p.part_ml = get<float>((size_t)ran.ksplit * total_rows * heads * 2);
      if (!p.part_o || !p.part_ml) return rc;
      if (g->merge_in_launch) {   // one (zeroed) arrival counter per (segment, 32-row query block, head): enough for every block shape
        p.tickets = get<int>((size_t)segs * (rows / 32) * heads);
        if (!p.tickets) return rc;
      }
    }
    const AttnLaunchShape shape = attention_launch_shape(ran, heads, segs, NP, g->q_ssq != nullptr);
    g->ran_qb = shape.qb; g->ran_prefetch_wave = shape.pf_wave; g->ran_touch_ahead = shape.touch_ahead; g->ran_ksplit = ran.ksplit;
    if (carrier) {
      carrier->ran_touch_blocks = shape.touch_y * heads * segs;
      carrier->ran_form = shape.touch_y > 0 ? 2 : (shape.prefetch ? 1 : 0);
    }
    hipError_t e = hipSuccess;
    for (int r = 0; r < g->repeats && e == hipSuccess; ++r)   // back to back: the counters must be zero again after every launch
      e = launch_attention<NP>(p, heads, segs, s);
    if (e != hipSuccess) return MSD_ERR_HIP;
    back(o, g->o, total_rows * J);
    const int frc = finish();
    if (carrier) carrier->ran_range_flag = (int32_t)range_flag;
    return rc ? rc : frc;
  }
};

bool carrier_args_ok(const msd_carrier_args* ca) {
  if (!ca || ca->struct_size != (int32_t)sizeof(msd_carrier_args) || ca->form < 0 || ca->form > 2) return false;
  if (ca->form == 0) return true;
  if (ca->target_rows <= 0 || ca->target_rows > (1 << 20) || ca->target_k <= 0 || ca->target_k % kGemmBK || ca->target_k > 4096) return false;
  return ca->form == 1 || (ca->n_touch >= 1 && ca->n_touch <= 1024 && ca->delay >= 0 && ca->delay <= kTouchDelayMax);
}
}  // namespace

extern "C" {
int msd_op_gemm_h16(int precision, const float* a_dev, const float* w_dev, float* c_dev, int M,
                    int N, int K, void* stream) {
  if (M % 64 || N % 64 || K % 64 || M <= 0 || N <= 0 || K <= 0) return MSD_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int NP = op_planes(precision);
  if (NP < 0) return MSD_ERR_UNSUPPORTED;
  OpKit kit(s, NP);
  Planes a, w;
  if (!kit.init_flags() || !kit.operand(a_dev, (size_t)M * K, &a) || !kit.weight(w_dev, K, N, 0, 0, &w, N)) return MSD_ERR_HIP;
  hipError_t e;
  if (NP == 2) e = launch_wide_store_f32<2>(gp<2>(a, K, w, K, M, N, K), epi_store_f32(c_dev, N), s);
  else e = launch_wide_store_f32<1>(gp<1>(a, K, w, K, M, N, K), epi_store_f32(c_dev, N), s);
  if (e != hipSuccess) return MSD_ERR_HIP;
  return kit.finish();
}

/* ABI <= 2 name of msd_op_gemm_h16 (the planes were bfloat16 then); kept so that old bindings keep linking */
int msd_op_gemm_bf16(int precision, const float* a_dev, const float* w_dev, float* c_dev, int M,
                     int N, int K, void* stream) {
  return msd_op_gemm_h16(precision, a_dev, w_dev, c_dev, M, N, K, stream);
}

int msd_op_gemm_f32(const float* a_dev, const float* w_dev, float* c_dev, int M, int N, int K,
                    void* stream) {
  if (N % 64 || K % 16 || M <= 0) return MSD_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  GemmF32Params p;
  p.A = a_dev; p.B = w_dev; p.lda = K; p.ldb = N; p.M = M; p.N = N; p.K = K;
  if (launch_gemm_f32(p, EpiF32Store{c_dev, N}, s) != hipSuccess) return MSD_ERR_HIP;
  return hipStreamSynchronize(s) == hipSuccess ? MSD_OK : MSD_ERR_HIP;
}

int msd_op_attention(int precision, const float* q_dev, const float* k_dev, const float* v_dev,
                     float* o_dev, int n_q, int n_keys, int n_keys_valid, int heads, void* stream) {
  return msd_op_attention_qp(precision, 0, q_dev, k_dev, v_dev, o_dev, n_q, n_keys, n_keys_valid, heads, stream);
}

int msd_op_attention_qp(int precision, int qp, const float* q_dev, const float* k_dev, const float* v_dev,
                        float* o_dev, int n_q, int n_keys, int n_keys_valid, int heads, void* stream) {
  // (long key axes exercise the key-split path + the merge LAUNCH: a split of 3 runs as 2)
  return msd_op_attention_split(precision, qp, n_keys >= 512 ? 3 : 1, 0, 1, q_dev, k_dev, v_dev, o_dev, n_q, n_keys, n_keys_valid,
                                heads, stream);
}

int msd_op_attention_split(int precision, int qp, int ksplit, int merge_in_launch, int repeats, const float* q_dev,
                           const float* k_dev, const float* v_dev, float* o_dev, int n_q, int n_keys, int n_keys_valid,
                           int heads, void* stream) {
  return msd_op_attention_ex(precision, qp, ksplit, merge_in_launch, repeats, 0, nullptr, 0, q_dev, k_dev, v_dev, o_dev, n_q,
                             n_keys, n_keys_valid, heads, stream);
}

int msd_op_attention_ex(int precision, int qp, int ksplit, int merge_in_launch, int repeats, int allow_qb4,
                        const float* q_ssq_dev, int q_tiles, const float* q_dev, const float* k_dev, const float* v_dev,
                        float* o_dev, int n_q, int n_keys, int n_keys_valid, int heads, void* stream) {
  if (qp < 0 || qp > 3 || ksplit < 1 || ksplit > 8 || repeats < 1 || repeats > 1000) return MSD_ERR_INVALID_ARGUMENT;
  if (n_q % 64 || n_keys % 32 || n_q <= 0 || n_keys <= 0 || heads <= 0 || n_keys_valid < 0 ||
      n_keys_valid > n_keys)
    return MSD_ERR_INVALID_ARGUMENT;
  if (q_ssq_dev != nullptr && (q_tiles <= 0 || q_tiles > kAuxMaxTiles || q_tiles % 4)) return MSD_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int NP = op_planes(precision);
  if (NP < 0) return MSD_ERR_UNSUPPORTED;
  if (q_ssq_dev != nullptr && NP != 2) return MSD_ERR_UNSUPPORTED;   // (un-normalised queries: two-plane kernels only)
  const int J = heads * kHeadDim;
  OpKit kit(s, NP);
  Planes q, k, vt, o;
  int* d_nk = kit.get<int>(1);
  float* vt32 = kit.get<float>((size_t)J * n_keys);
  if (!kit.init_flags() || !d_nk || !vt32 || !kit.planes((size_t)n_q * J, &o)) return MSD_ERR_HIP;
  (void)hipMemcpyAsync(d_nk, &n_keys_valid, sizeof(int), hipMemcpyHostToDevice, s);
  if (!kit.operand(q_dev, (size_t)n_q * J, &q) || !kit.operand(k_dev, (size_t)n_keys * J, &k)) return MSD_ERR_HIP;
  // V -> V^T with the per-16 key permutation, via the GEMM epilogue's own rule (host copy)
  std::vector<float> vh((size_t)n_keys * J), vth((size_t)J * n_keys);
  if (hipMemcpy(vh.data(), v_dev, vh.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return MSD_ERR_HIP;
  for (int key = 0; key < n_keys; ++key) {
    const int kp = vt_key_pos(key);
    for (int j = 0; j < J; ++j) vth[(size_t)j * n_keys + kp] = vh[(size_t)key * J + j];
  }
  if (hipMemcpy(vt32, vth.data(), vth.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return MSD_ERR_HIP;
  if (!kit.operand(vt32, (size_t)J * n_keys, &vt)) return MSD_ERR_HIP;
  AttnParams p;
  kit.arm(p);
  p.qp = qp;
  p.allow_qb4 = allow_qb4 != 0;
  if (q_ssq_dev != nullptr) { p.q_ssq = q_ssq_dev; p.q_tiles = q_tiles; p.q_inv_d = 1.0f / (float)(kNarrowTile * q_tiles); }
  for (int i = 0; i < 2; ++i) {
    const int j = i < NP ? i : 0;
    p.q[i] = q.p[j]; p.k[i] = k.p[j]; p.vt[i] = vt.p[j]; p.o[i] = o.p[j];
  }
  p.n_keys = d_nk; p.ldq = J; p.ldk = J; p.ldo = J; p.vt_ld = n_keys; p.q_rows_per_seg = n_q;
  p.k_seg_stride = 0; p.vt_seg_stride = 0; p.k_rows = n_keys;
  p.ksplit = 1; p.part_o = nullptr; p.part_ml = nullptr; p.total_rows = n_q;
  float *po = nullptr, *pml = nullptr;
  if (ksplit > 1) {
    p.ksplit = ksplit;
    po = kit.get<float>((size_t)ksplit * n_q * J);
    pml = kit.get<float>((size_t)ksplit * n_q * heads * 2);
    if (!po || !pml) return MSD_ERR_HIP;
    p.part_o = po; p.part_ml = pml;
    if (merge_in_launch) {   // attention.h attention_inlaunch_merge: one (zeroed) arrival counter per (query block, head)
      p.tickets = kit.get<int>((size_t)(n_q / 32) * heads);
      if (!p.tickets) return MSD_ERR_HIP;
    }
  }
  hipError_t e = hipSuccess;
  for (int r = 0; r < repeats && e == hipSuccess; ++r)   // back to back: the counters must be zero again after every launch
    e = NP == 2 ? launch_attention<2>(p, heads, 1, s) : launch_attention<1>(p, heads, 1, s);
  if (e != hipSuccess) return MSD_ERR_HIP;
  kit.back(o, o_dev, (size_t)n_q * J);
  return kit.finish();
}

static int attention_launch_op(msd_attention_launch_args* g, msd_carrier_args* ca, void* stream) {
  if (!g || g->struct_size != (int32_t)sizeof(msd_attention_launch_args)) return MSD_ERR_INVALID_ARGUMENT;
  g->ran_qb = g->ran_prefetch_wave = g->ran_touch_ahead = g->ran_ksplit = 0;
  if (g->qp < 0 || g->qp > 3 || g->ksplit < 1 || g->ksplit > 8 || g->repeats < 1 || g->repeats > 1000) return MSD_ERR_INVALID_ARGUMENT;
  if (g->heads <= 0 || g->heads > 64 || g->segs <= 0 || g->segs > 1024 || g->q_rows_per_seg <= 0 || g->q_rows_per_seg % 64 ||
      g->q_rows_per_seg > 65536 || !g->q || !g->k || !g->v || !g->n_keys || !g->o)
    return MSD_ERR_INVALID_ARGUMENT;
  const int J = g->heads * kHeadDim;
  // the window lies inside the allocation; whole 32-key blocks (the plain op's rule) from a 32-key boundary (the V^T
  // permutation works on 16 keys, a DMA lane moves 8 elements: rows of K and of V^T start on 16 bytes)
  if (g->k_alloc_rows <= 0 || g->k_alloc_rows > (1 << 20) || g->k_alloc_rows % 8 || g->k_rows <= 0 || g->k_rows % 32 ||
      g->k_row0 < 0 || g->k_row0 % 32 || (int64_t)g->k_row0 + g->k_rows > g->k_alloc_rows)
    return MSD_ERR_INVALID_ARGUMENT;
  // the heads' columns fit the rows of q and of k
  if (g->ldq <= 0 || g->ldq > (1 << 20) || g->ldq % 8 || g->q_col < 0 || g->q_col % 8 || (int64_t)g->q_col + J > g->ldq ||
      g->ldk <= 0 || g->ldk > (1 << 20) || g->ldk % 8 || g->k_col < 0 || g->k_col % 8 || (int64_t)g->k_col + J > g->ldk)
    return MSD_ERR_INVALID_ARGUMENT;
  if (g->k == g->q && (g->ldk != g->ldq || g->k_row0 != 0 || g->k_rows != g->k_alloc_rows || g->k_rows != g->q_rows_per_seg))
    return MSD_ERR_INVALID_ARGUMENT;
  if (g->touch_ahead < 0 || g->touch_ahead > 16 || g->pf_late < 0 || g->pf_late > 1) return MSD_ERR_INVALID_ARGUMENT;
  if ((g->prefetch_rows != 0) != (g->prefetch_k != 0) || g->prefetch_rows < 0 || g->prefetch_rows > (1 << 20) ||
      g->prefetch_k < 0 || g->prefetch_k % kGemmBK || g->prefetch_k > 4096)
    return MSD_ERR_INVALID_ARGUMENT;
  // the kernels index rows, partials and planes with 32-bit offsets
  const int64_t total_rows = (int64_t)g->segs * g->q_rows_per_seg, lim = 0x7FFFFFFFll;
  if (total_rows * g->ldq > lim || (int64_t)g->segs * g->k_alloc_rows * (g->ldk > J ? g->ldk : J) > lim ||
      total_rows * J * 8 * (int64_t)sizeof(float) > lim)
    return MSD_ERR_INVALID_ARGUMENT;
  if (g->q_ssq != nullptr && (g->q_tiles <= 0 || g->q_tiles > kAuxMaxTiles || g->q_tiles % 4)) return MSD_ERR_INVALID_ARGUMENT;
  const int NP = op_planes(g->precision);
  if (NP < 0) return MSD_ERR_UNSUPPORTED;
  if (g->q_ssq != nullptr && NP != 2) return MSD_ERR_UNSUPPORTED;   // (un-normalised queries: two-plane kernels only)
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (ca && NP != 2) return MSD_ERR_UNSUPPORTED;   // (the single-plane modes never carry a target)
  if (NP == 2) return AttnLaunchRun<2>(g, s, ca).run();
  return AttnLaunchRun<1>(g, s).run();
}
int msd_op_attention_launch(msd_attention_launch_args* g, void* stream) { return attention_launch_op(g, nullptr, stream); }
int msd_op_attention_launch_carrier(msd_attention_launch_args* g, msd_carrier_args* ca, void* stream) {
  if (!carrier_args_ok(ca)) return MSD_ERR_INVALID_ARGUMENT;
  ca->ran_form = ca->ran_touch_blocks = ca->ran_range_flag = 0;
  return attention_launch_op(g, ca, stream);
}

// (ONE plane: a two-plane target is dealt as 2 x rows rows, plane 1 behind plane 0 -- the same predicate with planes = 2.)
// Host only (no HIP call): how a target of `target_bytes` -- rows of `row_bytes` bytes, `row_pitch` bytes apart -- is dealt
// over `waves` touching waves, by the function both device forms use (gemm_h16.h touch_first_row / prefetch_wave).
// ranges[(w * kTouchesPerWave + u) * 3 + {0, 1, 2}] = first row, rows and 128-byte lines per row of touch u of wave w (rows
// = 0: that touch covers nothing).  Returns the touches per wave (> 0), or a negative msd_status: bad arguments, a
// `capacity` (in int32 words) too small, or a target the waves cannot cover in their kTouchesPerWave touches each.
int msd_op_touch_deal(int64_t target_bytes, int32_t row_bytes, int32_t row_pitch, int32_t waves, int32_t* ranges, int32_t capacity) {
  if (target_bytes <= 0 || row_bytes <= 0 || row_bytes > 64 * 128 || row_pitch < row_bytes || waves <= 0 || waves > (1 << 16) || !ranges)
    return -MSD_ERR_INVALID_ARGUMENT;
  if ((target_bytes - row_bytes) % row_pitch) return -MSD_ERR_INVALID_ARGUMENT;   // whole rows; the last one ends the target
  const int64_t rows64 = (target_bytes - row_bytes) / row_pitch + 1;
  if (rows64 > (1 << 24) || (int64_t)waves * kTouchesPerWave * 3 > capacity) return -MSD_ERR_INVALID_ARGUMENT;
  PrefetchTarget t;
  t.set(nullptr, nullptr, (int)rows64, row_pitch, row_bytes);
  const int rpt = 64 >> t.lg;
  if ((int64_t)waves * kTouchesPerWave * rpt < rows64) return -MSD_ERR_UNSUPPORTED;
  for (int w = 0; w < waves; ++w)
    for (int u = 0; u < kTouchesPerWave; ++u) {
      // the 64 lanes of the touch, through the device's own predicate (gemm_h16.h touch_lane_in): lane = (sub, line)
      const int r0 = touch_first_row(w, waves, u, rpt);
      int first = -1, last = -1, lines = 0;
      for (int lane = 0; lane < 64; ++lane) {
        const int sub = lane >> t.lg, line = lane & ((1 << t.lg) - 1);
        int pl, row0;
        if (!touch_lane_in(r0, sub, line, t.rows, /*planes=*/1, t.lpr, &pl, &row0)) continue;
        if (first < 0) first = row0 + sub;
        last = row0 + sub;
        if (row0 + sub == first) ++lines;
      }
      int32_t* o = ranges + ((size_t)w * kTouchesPerWave + u) * 3;
      o[0] = first < 0 ? r0 : first; o[1] = first < 0 ? 0 : last - first + 1; o[2] = first < 0 ? t.lpr : lines;
    }
  return kTouchesPerWave;
}

int msd_op_threefry(int stage, uint64_t seed, int64_t fold, const uint32_t* bits_in_dev, float* out_dev, int64_t n,
                    void* stream) {
  if (bits_in_dev && stage == 0) return MSD_ERR_INVALID_ARGUMENT;
  return threefry_fill(stage, seed, fold, bits_in_dev, out_dev, n, static_cast<hipStream_t>(stream));
}

// the sampler update's entry points: each checks what only it takes and names its form (op_sampler_step)
int msd_op_sampler_step(const msd_config* cfg, int step_index, const float* z_dev, const float* out_cond_dev,
                        const float* out_uncond_dev, const float* noise_dev, float* z_out_dev, int64_t n,
                        void* stream) {
  SamplerOpForm f;
  f.noise = noise_dev;
  return op_sampler_step(cfg, step_index, z_dev, out_cond_dev, out_uncond_dev, z_out_dev, n, stream, f);
}

int msd_op_sampler_step_keep(const msd_config* cfg, int step_index, const float* z_dev, const float* out_cond_dev,
                             const float* out_uncond_dev, const float* noise_dev, const float* known_scaled_dev,
                             const int32_t* keep_mask_dev, int n_dims, float* z_out_dev, int64_t n, void* stream) {
  if (!known_scaled_dev || !keep_mask_dev || n_dims <= 0 || n_dims % 4 || n <= 0 || n % n_dims)
    return MSD_ERR_INVALID_ARGUMENT;
  SamplerOpForm f;
  f.noise = noise_dev; f.known = known_scaled_dev; f.keep = keep_mask_dev; f.n_dims = n_dims; f.flags = true;
  return op_sampler_step(cfg, step_index, z_dev, out_cond_dev, out_uncond_dev, z_out_dev, n, stream, f);
}

int msd_op_sampler_step_release(const msd_config* cfg, int step_index, const float* z_dev, const float* out_cond_dev,
                                const float* out_uncond_dev, const float* noise_dev, const float* known_scaled_dev,
                                const int32_t* release_dev, int n_dims, float* z_out_dev, int64_t n, void* stream) {
  if (!known_scaled_dev || !release_dev || n_dims <= 0 || n_dims % 4 || n <= 0 || n % n_dims)
    return MSD_ERR_INVALID_ARGUMENT;
  SamplerOpForm f;
  f.noise = noise_dev; f.known = known_scaled_dev; f.keep = release_dev; f.n_dims = n_dims;
  return op_sampler_step(cfg, step_index, z_dev, out_cond_dev, out_uncond_dev, z_out_dev, n, stream, f);
}

int msd_op_sampler_step_multistep(const msd_config* cfg, int step_index, const float* z_dev, const float* out_cond_dev,
                                  const float* out_uncond_dev, float* x0_prev_inout_dev, int first, float* z_out_dev,
                                  int64_t n, void* stream) {
  if (!x0_prev_inout_dev) return MSD_ERR_INVALID_ARGUMENT;
  SamplerOpForm f;
  f.x0_prev = x0_prev_inout_dev; f.first = first;
  return op_sampler_step(cfg, step_index, z_dev, out_cond_dev, out_uncond_dev, z_out_dev, n, stream, f);
}

int msd_op_sampler_step_guided(const msd_config* cfg, int step_index, const float* z_dev, const float* out_cond_dev,
                               const float* out_uncond_dev, const float* noise_dev, const float* weights_host, int rows,
                               float* z_out_dev, int64_t n, void* stream) {
  SamplerOpForm f;
  f.noise = noise_dev; f.guided = true; f.weights = weights_host; f.rows = rows;
  return op_sampler_step(cfg, step_index, z_dev, out_cond_dev, out_uncond_dev, z_out_dev, n, stream, f);
}

int msd_op_sampler_step_multistep_guided(const msd_config* cfg, int step_index, const float* z_dev, const float* out_cond_dev,
                                         const float* out_uncond_dev, float* x0_prev_inout_dev, int first,
                                         const float* weights_host, int rows, float* z_out_dev, int64_t n, void* stream) {
  if (!x0_prev_inout_dev) return MSD_ERR_INVALID_ARGUMENT;
  SamplerOpForm f;
  f.x0_prev = x0_prev_inout_dev; f.first = first; f.guided = true; f.weights = weights_host; f.rows = rows;
  return op_sampler_step(cfg, step_index, z_dev, out_cond_dev, out_uncond_dev, z_out_dev, n, stream, f);
}

// any of the forms above with z_out's planes, the range flag and the published scan index (tests/test_gpu_sampler_planes.py):
// the form follows from the pointers, each checked as its own entry point checks it
int msd_op_sampler_step_planes(msd_sampler_planes_args* a, void* stream) {
  if (!a || a->struct_size != (int32_t)sizeof(msd_sampler_planes_args) || !a->z_planes_out_dev) return MSD_ERR_INVALID_ARGUMENT;
  SamplerOpForm f;
  f.noise = a->noise_dev;
  if (a->weights_host) { f.guided = true; f.weights = a->weights_host; f.rows = a->rows; }
  if (a->x0_prev_inout_dev) { f.x0_prev = a->x0_prev_inout_dev; f.first = a->first; f.noise = nullptr; }
  if (a->known_scaled_dev) {
    if (f.guided || f.x0_prev || !a->keep_dev || a->n_dims <= 0 || a->n_dims % 4 || a->n <= 0 || a->n % a->n_dims)
      return MSD_ERR_INVALID_ARGUMENT;
    f.known = a->known_scaled_dev; f.keep = a->keep_dev; f.n_dims = a->n_dims; f.flags = a->keep_is_flags != 0;
  }
  SamplerOpPlanes po;
  po.planes_out = a->z_planes_out_dev;
  const int rc = op_sampler_step(a->cfg, a->step_index, a->z_dev, a->out_cond_dev, a->out_uncond_dev, a->z_out_dev, a->n,
                                 stream, f, &po);
  a->ran_range_flag = (int32_t)po.range_flag; a->ran_next_step = po.next_step;
  return rc;
}

// sampler_invert_kernel alone (tests/test_gpu_invert.py): one step up the scan on the caller's arrays, the row weights from
// the caller's host floats, z and its planes out.  No draw: no noise slot, no key table.
int msd_op_invert_step(const msd_config* cfg, int step_index, const float* z_dev, const float* out_cond_dev,
                       const float* out_uncond_dev, const float* weights_host, int rows, float* z_out_dev,
                       float* z_planes_out_dev, int64_t n, void* stream) {
  if (!cfg || cfg->struct_size != (int32_t)sizeof(msd_config) || !z_dev || !out_cond_dev || !z_out_dev || !z_planes_out_dev ||
      !weights_host || rows < 1 || n <= 0 || n % 4 || n > 0x7FFFFFFFll - 1023 || n % rows || (n / rows) % kRngRowBlock ||
      step_index < 0 || step_index >= cfg->num_steps)
    return MSD_ERR_INVALID_ARGUMENT;   // (n: the last block's element index, blocks of 1024, stays an int)
  bool all_one = true;
  for (int b = 0; b < rows; ++b) {
    if (!std::isfinite(weights_host[b])) return MSD_ERR_INVALID_ARGUMENT;
    all_one = all_one && weights_host[b] == 1.0f;
  }
  if (all_one != (out_uncond_dev == nullptr)) return MSD_ERR_INVALID_ARGUMENT;
  const int NP = op_planes(cfg->precision);
  if (NP < 0) return MSD_ERR_UNSUPPORTED;
  std::vector<float> coef, inv;
  std::string why;
  if (!build_coef_rows(*cfg, &coef, &why)) return MSD_ERR_INVALID_ARGUMENT;
  build_invert_rows(coef, &inv);
  hipStream_t s = static_cast<hipStream_t>(stream);
  OpKit kit(s, NP);
  Planes zp;
  if (!kit.init_flags() || !kit.planes((size_t)n, &zp)) return MSD_ERR_HIP;
  const int passes = all_one ? 1 : 2;
  const int st[2] = {step_index, step_index};
  SamplerInvertParams ip;
  float* eps = kit.get<float>((size_t)passes * n);
  ip.coef = kit.put(coef.data(), coef.size());
  ip.coef_inv = kit.put(inv.data(), inv.size());
  ip.row_wt = kit.put(weights_host, (size_t)rows);
  ip.step_ptr = kit.put(st, 2);
  if (!eps || !ip.coef || !ip.coef_inv || !ip.row_wt || !ip.step_ptr) return MSD_ERR_HIP;
  if (hipMemcpyAsync(eps, out_cond_dev, n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess ||
      (passes == 2 && hipMemcpyAsync(eps + n, out_uncond_dev, n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) ||
      hipMemcpyAsync(z_out_dev, z_dev, n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return MSD_ERR_HIP;
  ip.eps = eps; ip.noise_slot = nullptr; ip.rng_key = nullptr;   // (the form makes no draw and reads neither)
  ip.row_blocks = (int)(n / rows / kRngRowBlock);
  ip.n = (int)n; ip.passes = passes; ip.cond_wt = 1.0f; ip.clip_x0 = cfg->clip_x0; ip.ddim = 1;
  ip.model_output = cfg->model_output; ip.step_from_slot1 = 1;
  kit.z_out_to(ip, z_out_dev, zp);   // (the kernel updates z in place: z_out_dev holds the caller's z)
  launch_sampler_invert(ip, s);
  if (hipGetLastError() != hipSuccess) return MSD_ERR_HIP;
  kit.back(zp, z_planes_out_dev, (size_t)n);
  return kit.finish();
}

int msd_op_diffuse_to_step(const msd_config* cfg, int step_index, const float* mel_dev, const float* eps_dev,
                           float* z_out_dev, float* z_planes_out_dev, float* xk_out_dev, int64_t n, void* stream) {
  if (!cfg || cfg->struct_size != (int32_t)sizeof(msd_config) || !mel_dev || !eps_dev || !z_out_dev || !z_planes_out_dev ||
      !xk_out_dev || n <= 0 || n % 4 || n > 0x7FFFFFFFll || step_index < 0 || step_index >= cfg->num_steps)
    return MSD_ERR_INVALID_ARGUMENT;
  const int NP = op_planes(cfg->precision);
  if (NP < 0) return MSD_ERR_UNSUPPORTED;
  std::vector<float> rows;
  std::string why;
  if (!build_coef_rows(*cfg, &rows, &why)) return MSD_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  OpKit kit(s, NP);
  Planes zp;
  if (!kit.init_flags() || !kit.planes((size_t)n, &zp)) return MSD_ERR_HIP;
  DiffuseParams dp;
  dp.mel = mel_dev; dp.eps = eps_dev; dp.xk = xk_out_dev;
  kit.z_out_to(dp, z_out_dev, zp);
  dp.n = (int)n; dp.fmin = cfg->feature_min; dp.fmax = cfg->feature_max;
  diffuse_coefs(rows[(size_t)step_index * kCoefCount + kCoefLogsnrT], &dp.alpha, &dp.sigma);
  launch_diffuse_to_step(dp, s);
  if (hipGetLastError() != hipSuccess) return MSD_ERR_HIP;
  kit.back(zp, z_planes_out_dev, (size_t)n);
  return kit.finish();
}

int msd_op_renoise(const msd_config* cfg, int from_level, int to_level, const float* z_dev, const float* eps_dev,
                   float* z_out_dev, float* z_planes_out_dev, int64_t n, void* stream) {
  if (!cfg || cfg->struct_size != (int32_t)sizeof(msd_config) || !z_dev || !eps_dev || !z_out_dev || !z_planes_out_dev ||
      n <= 0 || n % 4 || n > 0x7FFFFFFFll - 1023 || from_level < 0 || to_level <= from_level || to_level > cfg->num_steps)
    return MSD_ERR_INVALID_ARGUMENT;   // (n: the last block's element index, blocks of 1024, stays an int)
  const int NP = op_planes(cfg->precision);
  if (NP < 0) return MSD_ERR_UNSUPPORTED;
  std::vector<float> rows;
  std::string why;
  if (!build_coef_rows(*cfg, &rows, &why)) return MSD_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  OpKit kit(s, NP);
  Planes zp;
  if (!kit.init_flags() || !kit.planes((size_t)n, &zp)) return MSD_ERR_HIP;
  RenoiseParams rp;   // (no keys, no key table, no scan index: the caller's eps, and nothing armed behind the jump)
  rp.z_in = z_dev; rp.eps = eps_dev; rp.n = (int)n;
  kit.z_out_to(rp, z_out_dev, zp);
  renoise_coefs(rows, from_level, to_level, &rp.a, &rp.b);
  launch_renoise(rp, s);
  if (hipGetLastError() != hipSuccess) return MSD_ERR_HIP;
  kit.back(zp, z_planes_out_dev, (size_t)n);
  return kit.finish();
}

// diffusion_loss_kernel alone (tests/test_gpu_loss.py): one pass, the caller's eps, a one-row time list at cursor 0
int msd_op_diffusion_loss(const msd_config* cfg, int step_index, int loss_type, int loss_norm, const float* o_dev,
                          const float* z_dev, const float* x0_dev, const float* eps_dev, const float* mask_dev, int n_dims,
                          float* out_dev, int64_t n, void* stream) {
  if (!cfg || cfg->struct_size != (int32_t)sizeof(msd_config) || !o_dev || !z_dev || !x0_dev || !eps_dev || !out_dev ||
      n_dims <= 0 || n <= 0 || n % n_dims || n > 0x7FFFFFFFll - 1023 || step_index < 0 || step_index >= cfg->num_steps ||
      loss_type < MSD_LOSS_X0 || loss_type > MSD_LOSS_X0_AND_EPS || (loss_norm != MSD_LOSS_L1 && loss_norm != MSD_LOSS_L2))
    return MSD_ERR_INVALID_ARGUMENT;   // (n: the last block's element index, blocks of 1024, stays an int)
  if (n_dims % 4 || 1024 % n_dims) return MSD_ERR_UNSUPPORTED;
  std::vector<float> rows;
  std::string why;
  if (!build_coef_rows(*cfg, &rows, &why)) return MSD_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  OpKit kit(s, 1);
  float* coef = kit.get<float>(rows.size());
  float* times = kit.get<float>(kLossTimeWords);
  LossCall* call = kit.get<LossCall>(1);
  if (!coef || !times || !call) return MSD_ERR_HIP;
  float row[kLossTimeWords] = {0.f, 0.f, 0.f, 0.f};
  const int32_t i = step_index;
  memcpy(&row[kLossTimeIndex], &i, sizeof(i));
  const LossCall lc = {nullptr, mask_dev, eps_dev, out_dev, times, loss_type, loss_norm, {0, 0}};
  if (hipMemcpyAsync(coef, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(times, row, sizeof(row), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(call, &lc, sizeof(lc), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return MSD_ERR_HIP;
  LossParams lp;   // (no keys: the caller's eps)
  lp.call = call; lp.o = o_dev; lp.z = z_dev; lp.x0 = x0_dev; lp.coef = coef; lp.keys = nullptr; lp.n = (int)n; lp.passes = 1;
  lp.n_dims = n_dims; lp.model_output = cfg->model_output;
  launch_diffusion_loss(lp, s);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return MSD_ERR_HIP;
  return MSD_OK;
}

// x_out = x_in + a . w1 ;  h_out = (RMSNorm(x_out; gamma) (.) (film_scale + 1) + film_bias) . w2
// folded != 0: the product's path -- EpiResidualNorm (y = x (.) g planes + partial sums of squares)
// then a consumer GEMM whose epilogue applies rstd and the tabulated bias.W2;
// folded == 0: residual GEMM, rmsnorm_film_kernel, plain GEMM.
// The one test that hands a producer's planes `y` straight to a consumer (no round trip through float32).
int msd_op_residual_norm_gemm(int folded, const float* x_in_dev, const float* a_dev, const float* w1_dev,
                              const float* gamma_dev, const float* film_scale_dev, const float* film_bias_dev,
                              const float* w2_dev, float* x_out_dev, float* h_out_dev, int M, int K, int D, int N,
                              void* stream) {
  if (M % 64 || K % 64 || D % 64 || N % 64 || M <= 0 || D > 1024 || !x_in_dev || !a_dev || !w1_dev || !gamma_dev ||
      !w2_dev || !x_out_dev || !h_out_dev || (!film_scale_dev) != (!film_bias_dev))
    return MSD_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  OpKit kit(s, 2);
  Ctx& c = kit.c;
  Planes a, w1, w2, y;
  if (!kit.init_flags() || !kit.operand(a_dev, (size_t)M * K, &a) || !kit.weight(w1_dev, K, D, 0, 0, &w1, D) ||
      !kit.weight(w2_dev, D, N, 0, 0, &w2, N))
    return MSD_ERR_HIP;
  const int tiles = D / kNarrowTile;
  float* ssq = kit.get<float>((size_t)M * tiles);
  float* film = kit.get<float>((size_t)2 * D);   // one-step, one-slot table: scale | bias
  float* g = kit.get<float>((size_t)D);
  float* bw = kit.get<float>((size_t)N);
  int* step = kit.get<int>(2);
  if (!kit.planes((size_t)M * D, &y) || !ssq || !film || !g || !bw || !step) return MSD_ERR_HIP;
  if (hipMemcpyAsync(x_out_dev, x_in_dev, (size_t)M * D * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
    return MSD_ERR_HIP;
  if (film_scale_dev) {
    (void)hipMemcpyAsync(film, film_scale_dev, D * sizeof(float), hipMemcpyDeviceToDevice, s);
    (void)hipMemcpyAsync(film + D, film_bias_dev, D * sizeof(float), hipMemcpyDeviceToDevice, s);
  }
  const GemmParams p2 = gp<2>(y, D, w2, D, M, N, D);
  if (folded) {
    hipLaunchKernelGGL(build_g_kernel, dim3((D + 255) / 256), dim3(256), 0, s, film, gamma_dev, g, 1, 1, 0, D);
    GemmF32Params bp;   // bias . W2 : one row
    bp.A = film + D; bp.B = w2_dev; bp.lda = D; bp.ldb = N; bp.M = 1; bp.N = N; bp.K = D;
    c.latch(launch_gemm_f32(bp, EpiF32Store{bw, N}, s));
    const EpiResidualNorm<2> er = epi_residual_norm<2>(x_out_dev, D, y, ssq, step, Gain{g, 0}, Gain{g, 0}, M / 2);
    GemmParams p1 = gp<2>(a, K, w1, K, M, D, K);
    p1.xcd_rows = 2; p1.xcd_walk_n = 1;
    kit.arm(p1);
    if (folded == 2) {   // (was: the split-K producer of the frozen experiments build, tools/ubench/exp -- not in the product)
      return MSD_ERR_UNSUPPORTED;
    } else if (folded == 3) {   // the producer on 32 x 48 tiles (one partial sum per row and tile + zeroed spare slots)
      if (D % kWide48 || M % 32) return MSD_ERR_INVALID_ARGUMENT;
      kit.launch_on<TK_TALL, Narrow48Tile>(KC_GEMM_MLP_OUT, p1, er);
    } else kit.launch_on<TK_TALL, NarrowTile>(KC_GEMM_MLP_OUT, p1, er);
    if (c.err == hipSuccess) c.latch(launch_wide_store_f32<2>(p2, epi_store_f32(h_out_dev, N, row_scale(ssq, tiles, step, bw, 0)), s));
  } else {
    kit.launch_on<TK_SQUARE, NarrowTile>(KC_GEMM_MLP_OUT, gp<2>(a, K, w1, K, M, D, K), EpiResidual{x_out_dev, D});
    NormParams np;
    np.x = x_out_dev; np.gamma = gamma_dev; np.film = film_scale_dev ? film : nullptr; np.step_ptr = step;
    np.film_slots = 1; np.film_slot = 0; np.rows = M; np.D = D; np.out[0] = y.p[0]; np.out[1] = y.p[1]; np.out_f32 = nullptr;
    kit.arm(np);
    hipLaunchKernelGGL((rmsnorm_film_kernel<1, 4>), dim3((M + 3) / 4), dim3(256), 0, s, np);
    if (c.err == hipSuccess) c.latch(launch_wide_store_f32<2>(p2, epi_store_f32(h_out_dev, N), s));
  }
  if (c.err != hipSuccess || hipGetLastError() != hipSuccess) return MSD_ERR_HIP;
  return kit.finish();
}

// out[M, F] = gelu_tanh(a . wi0) * (a . wi1)   (layers.py:483-497): interleaved wi_0/wi_1 packing + EpiGeglu.  Site
// mlp_in without a row scale, on the 64 x 128 tile the decoder uses at one song.
int msd_op_geglu(const float* a_dev, const float* wi0_dev, const float* wi1_dev, float* out_dev, int M, int K, int F,
                 void* stream) {
  if (M % 64 || K % 64 || F % 64 || M <= 0 || !a_dev || !wi0_dev || !wi1_dev || !out_dev) return MSD_ERR_INVALID_ARGUMENT;
  msd_gemm_site_args g = forced_site_args(shape_of<Wide128Tile>(), M, 2 * F, K);
  g.a = a_dev; g.w = wi0_dev; g.w_gate = wi1_dev; g.out = out_dev;
  return run_site<2>(&g, static_cast<hipStream_t>(stream), Site<TK_MLP_IN, EpiGeglu<2>>{});
}

// Fused q|k|v projection with the attention kernel's operand layouts (EpiQKV): q, k row-major, V^T per
// segment with the per-16 key permutation; returned un-permuted as q, k, v [M, J].  Site qkv on wq | wk | wv, on the
// 64 x 96 tile where it fits the q|k and the V^T regions and on 64 x 64 otherwise.
int msd_op_qkv(const float* a_dev, const float* wq_dev, const float* wk_dev, const float* wv_dev, float* q_out_dev,
               float* k_out_dev, float* v_out_dev, int M, int K, int J, int seg_len, void* stream) {
  if (M % 64 || K % 64 || J % 64 || M <= 0 || seg_len <= 0 || seg_len % 64 || M % seg_len || !a_dev || !wq_dev ||
      !wk_dev || !wv_dev || !q_out_dev || !k_out_dev || !v_out_dev)
    return MSD_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  OpKit kit(s, 2);
  float* w = kit.get<float>((size_t)K * 3 * J);     // [K][3J] = wq | wk | wv
  float* qkv = kit.get<float>((size_t)M * 3 * J);   // [M][3J] = q | k | v
  if (!w || !qkv) return MSD_ERR_HIP;
  const size_t col = (size_t)J * sizeof(float);
  const float* const w_in[3] = {wq_dev, wk_dev, wv_dev};
  float* const out[3] = {q_out_dev, k_out_dev, v_out_dev};
  for (int i = 0; i < 3; ++i)
    if (hipMemcpy2DAsync(w + (size_t)i * J, 3 * col, w_in[i], col, col, K, hipMemcpyDeviceToDevice, s) != hipSuccess) return MSD_ERR_HIP;
  const bool wide96 = (3 * J) % Wide96Tile::BN == 0 && (2 * J) % Wide96Tile::BN == 0;
  msd_gemm_site_args g = forced_site_args(wide96 ? shape_of<Wide96Tile>() : shape_of<WideTile>(), M, 3 * J, K);
  g.a = a_dev; g.w = w; g.out = qkv; g.seg_len = seg_len;
  if (const int rc = run_site<2>(&g, s, Site<TK_QKV, EpiQKV<2>>{})) return rc;
  for (int i = 0; i < 3; ++i)
    if (hipMemcpy2DAsync(out[i], col, qkv + (size_t)i * J, 3 * col, col, M, hipMemcpyDeviceToDevice, s) != hipSuccess) return MSD_ERR_HIP;
  return hipStreamSynchronize(s) == hipSuccess ? MSD_OK : MSD_ERR_HIP;
}

// out[M, n] = RMSNorm(x; gamma) . w in exact fp32 (network.py:445-456): final_proj_f32_kernel with the
// decoder_norm folded in (w pre-multiplied by gamma, rstd from the partial sums of squares that the
// residual epilogue of the last MLP writes -- produced here by the same epilogue with a zero update)
int msd_op_final_proj(const float* x_dev, const float* gamma_dev, const float* w_dev, float* out_dev, int M, int D,
                      int n, void* stream) {
  if (M % 64 || D % 64 || n % 32 || M <= 0 || D > 1024 || !x_dev || !gamma_dev || !w_dev || !out_dev)
    return MSD_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  OpKit kit(s, 2);
  const int tiles = D / kNarrowTile;
  float* x = kit.get<float>((size_t)M * D);
  float* ssq = kit.get<float>((size_t)M * tiles);
  float* wg = kit.get<float>((size_t)D * n);
  int* step = kit.get<int>(2);
  Planes za, zw;   // zero operands of the zero-update residual GEMM: one K-tile
  if (!x || !ssq || !wg || !step || !kit.planes((size_t)M * kGemmBK, &za) || !kit.planes((size_t)D * kGemmBK, &zw)) return MSD_ERR_HIP;
  if (hipMemcpyAsync(x, x_dev, (size_t)M * D * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return MSD_ERR_HIP;
  const EpiResidualNorm<2> er = epi_residual_norm<2>(x, D, Planes(), ssq, step, Gain(), Gain(), 0);
  kit.launch_on<TK_TALL, NarrowTile>(KC_GEMM_MLP_OUT, gp<2>(za, kGemmBK, zw, kGemmBK, M, D, kGemmBK), er);
  if (kit.c.err != hipSuccess) return MSD_ERR_HIP;
  hipLaunchKernelGGL(scale_rows_kernel, dim3((D * n + 255) / 256), dim3(256), 0, s, w_dev, gamma_dev, wg, D, n);
  FinalProjParams fp;
  fp.x = x; fp.wg = wg; fp.ssq = ssq; fp.out = out_dev; fp.M = M; fp.N = n; fp.K = D; fp.tiles = tiles;
  fp.inv_d = 1.0f / (float)D;
  hipLaunchKernelGGL(final_proj_f32_kernel<1>, dim3(n / 32, M / 16), dim3(64 * kFinalProjWaves), 0, s, fp);
  if (hipGetLastError() != hipSuccess) return MSD_ERR_HIP;
  return hipStreamSynchronize(s) == hipSuccess ? MSD_OK : MSD_ERR_HIP;
}

int msd_op_gemm_site(msd_gemm_site_args* args, void* stream) {
  if (!args || args->struct_size != (int32_t)sizeof(msd_gemm_site_args) || args->site < 0 || args->step < 0 ||
      args->steps <= 0 || args->step >= args->steps)
    return MSD_ERR_INVALID_ARGUMENT;
  const int NP = op_planes(args->precision);
  if (NP < 0) return MSD_ERR_UNSUPPORTED;
  args->ran_bm = args->ran_bn = args->ran_ns = args->ran_xcd_rows = args->ran_persistent = args->ran_dual = 0;
  args->ran_prefetch = args->ran_bm2 = args->ran_bn2 = args->ran_ns2 = args->ran_xcd_rows2 = 0;
  args->step_copy = -1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return NP == 2 ? run_gemm_site<2>(args, s) : run_gemm_site<1>(args, s);
}

int msd_op_gemm_site_carrier(msd_gemm_site_args* args, msd_carrier_args* ca, void* stream) {
  if (!args || args->struct_size != (int32_t)sizeof(msd_gemm_site_args) || args->site < 0 || args->step < 0 ||
      args->steps <= 0 || args->step >= args->steps || !carrier_args_ok(ca))
    return MSD_ERR_INVALID_ARGUMENT;
  if (op_planes(args->precision) != 2) return MSD_ERR_UNSUPPORTED;   // (the single-plane modes never carry a target)
  args->ran_bm = args->ran_bn = args->ran_ns = args->ran_xcd_rows = args->ran_persistent = args->ran_dual = 0;
  args->ran_prefetch = args->ran_bm2 = args->ran_bn2 = args->ran_ns2 = args->ran_xcd_rows2 = 0;
  args->step_copy = -1;
  ca->ran_form = ca->ran_touch_blocks = ca->ran_range_flag = 0;
  return run_gemm_site<2>(args, static_cast<hipStream_t>(stream), ca);
}

const char* msd_op_gemm_site_name(int precision, int site) {
  const int NP = op_planes(precision);
  const char* name = nullptr;
  auto f = [&](auto s) { name = site_name(s); };
  if (NP == 2) visit_site<2>(site, f);
  else if (NP == 1) visit_site<1>(site, f);
  return name;
}

int msd_op_gemm_site_tiles(int precision, int site, int index, int32_t* bm, int32_t* bn, int32_t* ns) {
  if (!bm || !bn || !ns || site < 0 || index < 0) return MSD_ERR_INVALID_ARGUMENT;
  const int NP = op_planes(precision);
  if (NP < 0) return MSD_ERR_UNSUPPORTED;
  std::vector<TileInfo> first, second;
  bool found;
  if (NP == 2) { SiteTiles<2> t; found = visit_site<2>(site, t); first = t.first; second = t.second; }
  else { SiteTiles<1> t; found = visit_site<1>(site, t); first = t.first; second = t.second; }
  if (!found || index >= (int)first.size()) return MSD_ERR_INVALID_ARGUMENT;
  bm[0] = first[index].bm; bn[0] = first[index].bn; ns[0] = first[index].ns;
  bm[1] = bn[1] = ns[1] = 0;
  if (!second.empty()) { bm[1] = second[index].bm; bn[1] = second[index].bn; ns[1] = second[index].ns; }
  return MSD_OK;
}

// ---- the vocoder's two elementwise kernels with a unit vector in them, on the caller's rows (tests/test_gpu_vocoder_edges.py)
// voc_phase_kernel as msd_vocoder_decode launches it: Y, Y_prev, X [rows, 1088], mag [rows, 544]
int msd_op_vocoder_phase(const float* y_dev, const float* yprev_dev, const float* mag_dev, float* x_out_dev, int rows,
                         float alpha, void* stream) {
  if (!y_dev || !yprev_dev || !mag_dev || !x_out_dev || rows <= 0 || rows > kVocMaxRows) return MSD_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(voc_phase_kernel, voc_grid_rows(rows), dim3(256), 0, s, y_dev, yprev_dev, mag_dev, x_out_dev, rows, alpha);
  if (hipGetLastError() != hipSuccess) return MSD_ERR_HIP;
  return hipStreamSynchronize(s) == hipSuccess ? MSD_OK : MSD_ERR_HIP;
}

// voc_load_spec_kernel as msd_vocoder_istft and msd_vocoder_decode launch it: src [B, F, 2, 513], mag [B (F + 1), 544] or
// NULL, X [B (F + 1), 1088]
int msd_op_vocoder_load_spec(const float* src_dev, const float* mag_dev, float* x_out_dev, int batch, int n_frames,
                             int normalise, void* stream) {
  if (!src_dev || !x_out_dev || !voc_shape_ok(batch, n_frames)) return MSD_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rows = batch * (n_frames + 1);
  hipLaunchKernelGGL(voc_load_spec_kernel, voc_grid_rows(rows), dim3(256), 0, s, src_dev, mag_dev, x_out_dev, n_frames, rows,
                     normalise ? 1 : 0);
  if (hipGetLastError() != hipSuccess) return MSD_ERR_HIP;
  return hipStreamSynchronize(s) == hipSuccess ? MSD_OK : MSD_ERR_HIP;
}
}  // extern "C"
