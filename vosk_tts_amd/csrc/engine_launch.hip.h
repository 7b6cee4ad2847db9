// engine_launch.hip.h -- launch helpers: the conv executors behind launch_conv (which kernel: plan_conv, engine_convplan.hip.h), and the
// attention / LayerNorm selection and launches.
// Part of the ONE translation unit engine.hip (included there, in order; not a standalone header): split out in round 6 so that the
// planner / launch selection / stages / host paths can be read on their own.
#pragma once
// ------------------------------------------------------------------------------------ launch helpers
// Test hook (vits_debug_launch_log / vits_debug_launch_count): while on, every ProfScope counts its launch under "op|kernel", process-wide,
// so a test can assert WHICH kernel a launch took and not only what it computed.  Off (default): one relaxed load per launch.
static std::atomic<int> g_launch_log{0};
static std::mutex g_launch_log_mu;
static std::map<std::string, int> g_launch_counts;
struct ProfScope {
  vits_session* s; bool on; bool log; const char* op; std::string lk;
  ProfScope(vits_session* s_, const char* name, double flops, const char* kernel = "-")
      : s(s_), on(s_->profile), log(g_launch_log.load(std::memory_order_relaxed) != 0), op(name) {
    if (log) lk = kernel;
    if (!on) return;
    ProfRec r; r.name = name; r.kernel = kernel; r.flops = flops;
    hipEventCreate(&r.e0); hipEventCreate(&r.e1);
    hipEventRecord(r.e0, s->stream);
    s->prof.push_back(r);
  }
  void set_kernel(const char* k) { if (on) s->prof.back().kernel = k; if (log) lk = k; }
  ~ProfScope() {
    if (on) hipEventRecord(s->prof.back().e1, s->stream);
    if (log) { std::lock_guard<std::mutex> g(g_launch_log_mu); ++g_launch_counts[std::string(op) + "|" + lk]; }
  }
};


// ---- one persistent step program (persist.hip.h) as ONE launch of P = #CUs workgroups
static bool big_lds_needed(std::atomic<unsigned long long>& done);
static void persist_launch(vits_session* s, vits_session::PersistProg& pp, const char* name, const float* d_noise = nullptr, float nsw = 0.f,
                           uint64_t seed = 0, const int64_t* d_ids = nullptr, const int* d_forced = nullptr, float length_scale = 1.f,
                           float noise_scale = 0.f) {
  vits_model* m = s->m;
  ProfScope ps(s, name, pp.flops, "persist_kernel");
  PCall c;
  c.ctl = s->ps_ctl; c.ids = reinterpret_cast<const long long*>(d_ids); c.noise = d_noise; c.nsw = nsw; c.seed = seed;
  c.solo = s->solo ? 1 : 0; c.dv = s->dv; c.item_seeds = s->item_seeds; c.trace = nullptr;
  c.dbg = m->ps_dbg;
  c.forced = d_forced; c.length_scale = length_scale; c.noise_scale = noise_scale; c.noise_prior = nullptr; c.noise_stride = 0;
  static const char* trace_path = getenv("VITS_PS_TRACE");  // tools/ps_trace.py: per-worker, per-step cycle stamps of an EAGER forward
  static const char* trace_name = getenv("VITS_PS_TRACE_PROG");  // which program ("dp.persist" by default)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const bool want_trace = trace_path && !strcmp(name, trace_name ? trace_name : "dp.persist");
  if (want_trace) hipStreamIsCapturing(s->stream, &cap);
  const size_t trace_n = (size_t)m->n_cu * PS_MAX_STEPS * 8;
  if (want_trace && cap == hipStreamCaptureStatusNone) {
    hipMalloc((void**)&c.trace, trace_n * sizeof(long long));
    hipMemsetAsync(c.trace, 0, trace_n * sizeof(long long), s->stream);
  }
  g_ps_last_steps.store(pp.h.n_steps, std::memory_order_relaxed);
  if (pp.fused) hipLaunchKernelGGL(persist_kernel_fz, dim3(m->n_cu), dim3(PS_THREADS), 0, s->stream, pp.d, c);
  else hipLaunchKernelGGL(persist_kernel, dim3(m->n_cu), dim3(PS_THREADS), 0, s->stream, pp.d, c);
  if (c.trace) {
    std::vector<long long> h(trace_n);
    hipMemcpyAsync(h.data(), c.trace, trace_n * sizeof(long long), hipMemcpyDeviceToHost, s->stream);
    hipStreamSynchronize(s->stream);
    hipFree(c.trace);
    if (FILE* f = fopen(trace_path, "wb")) {
      const int hdr[4] = {m->n_cu, PS_MAX_STEPS, pp.h.n_steps, pp.h.T};
      fwrite(hdr, sizeof hdr, 1, f);
      for (int i = 0; i < pp.h.n_steps; ++i) fwrite(&pp.kinds[i], sizeof(int), 1, f);
      fwrite(h.data(), sizeof(long long), trace_n, f);
      fclose(f);
    }
  }
}

// compact tile map for a ragged launch (see conv_decode_block); nullptr when no table slot is left
static const int* tile_table(vits_session* s, const int* len, int mul, int add, int cap, int tile, int has_cap = 0, int cap_add = 0) {
  auto key = std::make_tuple(len, mul, add + 100000 * cap_add, cap, tile);
  for (size_t i = 0; i < s->tile_keys.size(); ++i)
    if (s->tile_keys[i] == key) return s->tile_tabs + i * (s->B + 1);
  if (s->tile_keys.size() >= 32) return nullptr;
  int* tab = s->tile_tabs + s->tile_keys.size() * (s->B + 1);
  s->tile_keys.push_back(key);
  hipLaunchKernelGGL(ragged_tiles_kernel, dim3(1), dim3(64), 0, s->stream, len, s->B, mul, add, cap, tile, tab, has_cap, cap_add);
  return tab;
}

static void attach_tile_table(vits_session* s, ConvParams& P, int N_T) {
  P.tile_start = nullptr;
  if (!s || !s->arena || s->B == 1) return;  // a single utterance in a padded bucket: the few dead tiles exit early instead
  if (P.rag) P.tile_start = tile_table(s, P.rag, P.rag_out_mul, P.rag_tab_add > P.rag_out_add ? P.rag_tab_add : P.rag_out_add, P.Tout, N_T, 1, P.rag_out_cap_add);  // (tiles the map lists beyond this launch's own limit exit at once)  // (the decoder's rag array carries its cap in rag[B])
  else if (P.skip_len) P.tile_start = tile_table(s, P.len, 1, 0, P.Tout, N_T);
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device: in-process multi-device replicas
// (MultiDeviceSynth) need it once per device, not once per process.  Returns true the first time per (flag word, device).
static bool big_lds_needed(std::atomic<unsigned long long>& done) {
  int dev = 0;
  hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev & 63);
  return !(done.fetch_or(bit) & bit);
}
// one launch of `kern`; a dynamic LDS size beyond 64 KB is allowed once per (kernel instantiation, DEVICE): `done` is the caller's flag word
template <typename Kern>
static void launch_big_lds(Kern kern, std::atomic<unsigned long long>& done, dim3 grid, int threads, size_t lds, int lds_attr, hipStream_t st, const ConvParams& P) {
  if (lds > 64 * 1024 && big_lds_needed(done)) hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_attr);
  hipLaunchKernelGGL(kern, grid, dim3(threads), lds, st, P);
}

// ---- the executors: one per kernel family.  Each sets ntiles_*, row_len, the tile table and the LDS size for the plan's tile, and launches.
static int plan_grid(vits_session* s, ConvParams& P, const ConvPlan& pl, bool table) {
  if (table) attach_tile_table(s, P, pl.N_T);
  else P.tile_start = nullptr;
  P.ntiles_m = cdiv(P.M, pl.M_T);
  P.ntiles_n = cdiv(P.Tout, pl.N_T);
  return P.ntiles_m * P.ntiles_n * P.B * P.n_groups;
}
template <int WM, int WN, int MI, int NI, int EPI>
static void launch_cfg(vits_session* s, ConvParams& P, const ConvPlan& pl, int halo) {
  const int nblk = plan_grid(s, P, pl, true);
  P.row_len = pl.N_T + halo;
  const size_t lds = (size_t)2 * CONV_CI_T * P.row_len * sizeof(float);
  hipLaunchKernelGGL((conv_mfma_kernel<WM, WN, MI, NI, EPI>), dim3(nblk), dim3(WM * WN * 64), lds, s->stream, P);
}
// Which K-split launches contract by input-channel chunk, the operand window staged once per chunk (ks_chunk_body, conv_mfma.hip.h), instead
// of by tap: one group on the 16-wave 32 x 32 STORE tile, at least 4 taps to share a window of at most KS_SLAB_PITCH columns, rows long
// enough for the vector loads, and a grid of about one workgroup per CU -- the single utterance's conv_pre, upsamplers and conv_post
// (measured: profiles/ks_chunk_bench.txt).  Not a planner leaf: the kernel instantiation, its name and the launch log do not change.
static bool ks_chunk_takes(const vits_session* s, const ConvParams& P, const ConvPlan& pl, long nblk) {
  const ConvGroup& G = P.g[0];
  if (!conv_select().env_ks_chunk || pl.NW != 16 || pl.MI != 1 || pl.NI != 1 || pl.epi != EPI_STORE || P.n_groups != 1) return false;
  const long cus = s->m->n_cu > 0 ? s->m->n_cu : 256;  // (vits_op_conv1d's scratch model carries no device description)
  return ks_chunk_rule(G.K, G.dil, P.Tin, nblk, cus);  // (the shape part: dec_end_rules.h, asserted by tests/test_dec_end_rules.py)
}
// Which chunk-split launches give a workgroup two adjacent column tiles (ks_chunk_body NT = 2, conv_mfma.hip.h): a compile-time tap count,
// 64 + halo columns inside the pair's slab pitch, no compact tile map (it counts single tiles), and a grid that is more than one round
// of the chip in single tiles and at most one in pairs -- of the single utterance's four launches, ups[1] (304 -> 160 workgroups;
// measured: profiles/dec_end_bench.txt).  VITS_KS_PAIR = 2 (tests): wherever there are two column tiles.  Not a planner leaf either.
static bool ks_pair_takes(const vits_session* s, const ConvParams& P, long nblk) {
  const ConvGroup& G = P.g[0];
  const long cus = s->m->n_cu > 0 ? s->m->n_cu : 256;
  return ks_pair_rule(conv_select().env_ks_pair, G.K, G.dil, P.ntiles_m, P.ntiles_n, P.B, P.tile_start != nullptr, nblk, cus);  // (dec_end_rules.h)
}
template <int MI, int NI, int EPI, int NIN>
static void launch_ks(vits_session* s, ConvParams& P, const ConvPlan& pl) {
  dim3 grid(plan_grid(s, P, pl, true));
  P.row_len = 0;  // no staging window: B fragments come straight from global memory
  P.ks_chunk = ks_chunk_takes(s, P, pl, (long)grid.x) ? 1 : 0;
  size_t lds = (size_t)pl.NW * MI * NI * 16 * 64 * sizeof(float);  // cross-wave reduction only
  if (P.ks_chunk && ks_pair_takes(s, P, (long)grid.x)) {  // column tiles in pairs: half the column tiles, two partial tiles per wave
    P.ks_chunk = 2;
    P.ntiles_n = cdiv(P.ntiles_n, 2);
    grid.x = P.ntiles_m * P.ntiles_n * P.B;
    lds *= 2;
  }
  static std::atomic<unsigned long long> done16{0};  // (beyond 64 KB: 16 waves of the 64 x 32 tile, and of the 32 x 32 tile in column pairs; 128 KB both)
  if (pl.NW == 16) launch_big_lds(conv_mfma_ks_kernel<MI, NI, EPI, NIN, 16>, done16, grid, 16 * 64, lds, (int)lds, s->stream, P);
  else if (pl.NW == 8) hipLaunchKernelGGL((conv_mfma_ks_kernel<MI, NI, EPI, NIN, 8>), grid, dim3(8 * 64), lds, s->stream, P);
  else hipLaunchKernelGGL((conv_mfma_ks_kernel<MI, NI, EPI, NIN, 4>), grid, dim3(4 * 64), lds, s->stream, P);
}
// small-tile kernel (conv_small.hip.h); PRO 2 / 3: LayerNorm-on-load, statistics redone per workgroup / from the producer (EPI_STORE only)
template <int EPI, int PRO>
static void launch_c16(vits_session* s, ConvParams& P, const ConvPlan& pl) {
  const int nw = pl.NW;
  P.tile_start = nullptr;
  P.ntiles_m = cdiv(EPI == EPI_GATE ? 2 * P.H : P.Cout, 16);
  P.ntiles_n = cdiv(P.Tout, 16);
  P.row_len = c16_row_pitch(16 + (P.g[0].K - 1) * P.g[0].dil);
  size_t lds = ((size_t)P.Cin * P.row_len + (PRO == 2 ? (size_t)nw * 2 * 32 : 0)) * sizeof(float);
  lds = std::max(lds, ((size_t)nw * 4 * 64 + (P.ln_stat_out ? 64 : 0)) * sizeof(float));
  const dim3 grid(8 * cdiv(P.ntiles_m, 8) * P.ntiles_n * P.B);
  static std::atomic<unsigned long long> done[4];
  const bool few = pl.MAXU == 8;
  if (nw == 8 && few) launch_big_lds(conv16_kernel<EPI, 8, 8, PRO>, done[0], grid, 512, lds, 160 * 1024, s->stream, P);
  else if (nw == 8) launch_big_lds(conv16_kernel<EPI, 8, C16_MAXU, PRO>, done[1], grid, 512, lds, 160 * 1024, s->stream, P);
  else if (few) launch_big_lds(conv16_kernel<EPI, 4, 8, PRO>, done[2], grid, 256, lds, 160 * 1024, s->stream, P);
  else launch_big_lds(conv16_kernel<EPI, 4, C16_MAXU, PRO>, done[3], grid, 256, lds, 160 * 1024, s->stream, P);
}
// wave-pipelined kernel (conv_small.hip.h conv_wp_kernel)
static void launch_conv_wp(vits_session* s, ConvParams& P, const ConvPlan& pl) {
  int nblk = plan_grid(s, P, pl, false);
  // a grouped launch whose workgroups are all resident at once (two per CU): choose the CU mates (conv_decode_block, mode 11).
  // Measured on the C = 256 stage of c2 (profiles/r3_blocktrace_c2.txt): makespan 26.9 -> 23.0 us.  Launches of several rounds keep
  // the heaviest-first order (the same mapping made the 900-workgroup C = 128 launch 14 % slower).
  // (Tried before that, measured in profiles/r3_xcd_map.txt, removed: giving every XCD one group's input and a range of its weight
  // rows or columns -- fabric traffic -35..44 %, launches 13-15 % slower.)
  const int per_xcd = cdiv(P.ntiles_m * P.ntiles_n, 8);
  if (P.B == 1 && P.n_groups == 3 && P.g[0].K >= P.g[1].K && P.g[1].K >= P.g[2].K && 3 * per_xcd <= 64 && per_xcd <= 32) {
    P.xcd_mode = 11;
    nblk = 8 * 3 * per_xcd;
  }
  const size_t lds = (size_t)pl.NW * CONV_CI_T * WP_PITCH * sizeof(float);
  hipLaunchKernelGGL(conv_wp_kernel<8>, dim3(nblk), dim3(pl.NW * 64), lds, s->stream, P);
}
// software-pipelined 64 x 64 kernel (conv_sp.hip.h)
template <int EPI>
static void launch_sp(vits_session* s, ConvParams& P, const ConvPlan& pl, int halo) {
  const dim3 grid(plan_grid(s, P, pl, true));
  P.row_len = 64 + halo;
  const size_t lds = (size_t)2 * 4 * P.row_len * SP_PITCH * sizeof(float);  // two stage buffers of four chunks [column][SP_PITCH]
  static std::atomic<unsigned long long> done1{0}, done2{0};
  if (pl.JT == 1) launch_big_lds(conv_sp_kernel<EPI, 1>, done1, grid, 256, lds, 160 * 1024, s->stream, P);
  else launch_big_lds(conv_sp_kernel<EPI, 2>, done2, grid, 256, lds, 160 * 1024, s->stream, P);
}
// split-bf16 variant (conv_bf3.hip.h)
template <int MI, int EPI>
static void launch_bf3(vits_session* s, ConvParams& P, const ConvPlan& pl, int halo) {
  const dim3 grid(plan_grid(s, P, pl, true));
  P.row_len = 128 + halo;
  const size_t lds = (size_t)2 * 2 * P.row_len * (BF3_PITCH * 2);
  hipLaunchKernelGGL((conv_bf3_kernel<MI, EPI>), grid, dim3(256), lds, s->stream, P);
}

// Runs the plan: the list of the instantiations that are built.  A plan outside it is a bug in plan_conv: say so, never launch something else.
static void exec_conv(vits_session* s, ConvParams& P, const ConvPlan& pl, int halo) {
  const int E = pl.epi;
  switch (pl.family) {
    case CONV_BIG:
#define BIG(WM_, WN_, MI_, NI_, EPI_) \
  if (pl.WM == WM_ && pl.WN == WN_ && pl.MI == MI_ && pl.NI == NI_ && E == EPI_) return launch_cfg<WM_, WN_, MI_, NI_, EPI_>(s, P, pl, halo)
      BIG(2, 2, 1, 1, EPI_STORE); BIG(2, 2, 1, 2, EPI_STORE); BIG(2, 2, 2, 2, EPI_STORE); BIG(1, 4, 1, 1, EPI_STORE);
      BIG(2, 2, 2, 1, EPI_GATE); BIG(2, 1, 2, 1, EPI_GATE); BIG(2, 2, 1, 1, EPI_RESSKIP); BIG(2, 2, 1, 1, EPI_COUPLE);
#undef BIG
      break;
    case CONV_KS:
#define KS(MI_, NI_, EPI_, NIN_) if (pl.MI == MI_ && pl.NI == NI_ && E == EPI_ && pl.NIN == NIN_) return launch_ks<MI_, NI_, EPI_, NIN_>(s, P, pl)
      KS(1, 1, EPI_STORE, 1); KS(1, 1, EPI_STORE, 2); KS(1, 1, EPI_STORE, 3); KS(1, 2, EPI_STORE, 1); KS(1, 2, EPI_STORE, 3);
      KS(2, 1, EPI_GATE, 1); KS(1, 1, EPI_RESSKIP, 1); KS(1, 1, EPI_COUPLE, 1);
#undef KS
      break;
    case CONV_C16:
#define C16(EPI_, PRO_) if (E == EPI_ && pl.PRO == PRO_) return launch_c16<EPI_, PRO_>(s, P, pl)
      C16(EPI_STORE, 0); C16(EPI_STORE, 2); C16(EPI_STORE, 3); C16(EPI_GATE, 0); C16(EPI_RESSKIP, 0); C16(EPI_COUPLE, 0);
#undef C16
      break;
    case CONV_WP: return launch_conv_wp(s, P, pl);
    case CONV_SP:
      if (E == EPI_STORE) return launch_sp<EPI_STORE>(s, P, pl, halo);
      if (E == EPI_RESSKIP) return launch_sp<EPI_RESSKIP>(s, P, pl, halo);
      if (E == EPI_COUPLE) return launch_sp<EPI_COUPLE>(s, P, pl, halo);
      break;
    case CONV_BF3:
      if (E == EPI_GATE && pl.MI == 2) return launch_bf3<2, EPI_GATE>(s, P, pl, halo);
      if (E == EPI_STORE && pl.MI == 2) return launch_bf3<2, EPI_STORE>(s, P, pl, halo);
      if (E == EPI_STORE && pl.MI == 1) return launch_bf3<1, EPI_STORE>(s, P, pl, halo);
      break;
  }
  fprintf(stderr, "[vits_mi355] conv plan %s is not a built kernel instantiation\n", conv_plan_name(pl).c_str());
  abort();
}
static void name_plan(ProfScope& ps, const ConvPlan& pl) {  // (formats only when somebody reads it)
  if (ps.on || ps.log) ps.set_kernel(conv_plan_name(pl).c_str());
}

// 1x1 conv whose B operand is produced by the DDSConv prologue (conv_small.hip.h PRO == 1, c16_dds_ok); P.dds_* set by the caller
static void launch_c16_dds(vits_session* s, ConvParams& P, const char* name, double flops) {
  ProfScope ps(s, name, flops);
  name_plan(ps, plan_c16_dds());
  P.tile_start = nullptr;
  P.ntiles_m = cdiv(P.Cout, 16);
  P.ntiles_n = cdiv(P.Tout, 16);
  P.row_len = 16;
  const size_t lds = ((size_t)P.Cin * (16 + DDS_XP + 8) + 16 * 32) * sizeof(float);  // B tile | x_in over the tap range | reductions | parameters
  const dim3 grid(8 * cdiv(P.ntiles_m, 8) * P.ntiles_n * P.B);
  DdsTimingScope timing(s, P, name);
  hipLaunchKernelGGL((conv16_kernel<EPI_STORE, 8, 8, 1>), grid, dim3(512), lds, s->stream, P);
}

// every convolution of both model families: plan (engine_convplan.hip.h), then execute
static void launch_conv(vits_session* s, ConvParams& P, int epi, const char* name, int halo_override = -1) {
  int halo = 0;
  double macs = 0;
  for (int g = 0; g < P.n_groups; ++g) {
    const int hg = halo_override >= 0 ? halo_override : (P.g[g].K - 1) * P.g[g].dil;
    if (hg > halo) halo = hg;
    // rows the conv actually computes: the gate kernel stores H channels but contracts 2H rows (tanh | sigmoid)
    macs += (double)(epi == EPI_GATE ? 2 * P.H : P.Cout) * P.Cin * P.g[g].K;
  }
  ProfScope ps(s, name, 2.0 * macs * (double)P.Tout * P.B);
  if (ps.on) {  // tools/profile_ops.py with VITS_PROF_SHAPES=1: one report line per distinct launch shape
    static const bool shapes = getenv("VITS_PROF_SHAPES") != nullptr;
    if (shapes) {
      char sh[96];
      snprintf(sh, sizeof sh, "/M%d.K%dx%d.N%dx%d.g%d", P.M, P.Cin, P.g[0].K, P.B, P.Tout, P.n_groups);
      s->prof.back().name += sh;
    }
  }
  ConvTimingScope timing(s, P, name);
  const ConvPlan pl = plan_conv(P, epi, halo, conv_select());
  name_plan(ps, pl);
  // heaviest group first (longest-processing-time order; see the big-tile kernel's block decode)
  for (int a = 0; a < P.n_groups; ++a)
    for (int c = a + 1; c < P.n_groups; ++c)
      if (P.g[c].K > P.g[a].K) { ConvGroup t = P.g[a]; P.g[a] = P.g[c]; P.g[c] = t; }
  exec_conv(s, P, pl, halo);
}

// common-case parameter block: one group, same-length 'same'-padded Conv1d over [B,C,T]
static ConvParams conv_params(const ConvW& W, const float* x, float* y, int B, int T, int dil, int pad_l) {
  ConvParams P;
  memset(&P, 0, sizeof P);
  P.n_groups = 1;
  P.g[0].x = x; P.g[0].w = W.w; P.g[0].w16 = W.w16; P.g[0].wb = W.wb; P.g[0].bias = W.bias; P.g[0].y = y;
  P.g[0].K = W.K; P.g[0].dil = dil; P.g[0].pad_l = pad_l; P.g[0].n_sg = W.n_sg;
  P.B = B; P.Cin = W.Cin; P.x_ch_off = 0; P.x_ch_sign = 1;
  P.x_bstride = (long long)W.Cin * T; P.Tin = T; P.Tin_stride = T;
  P.M = W.Mpad; P.Cout = W.M; P.Tout = T; P.Tout_stride = T; P.y_bstride = (long long)W.M * T;
  P.in_slope = 1.f; P.in_scale = 1.f;
  return P;
}

// masked-stage conv of a ragged batch: tiles beyond len[b] are skipped (conv_mfma.hip.h, skip_len)
static void mark_masked(vits_session* s, ConvParams& P, const int* len) {
  if (s->ragged) { P.skip_len = 1; P.len = len; }
}

static void launch_ln(vits_session* s, const float* a, const float* b, const float* base, float* y, const float* gamma,
                      const float* beta, const int* len, int B, int C, int T, int gelu, int mask) {
  ProfScope ps(s, "layernorm", 0, "layernorm_c_kernel");
  LNParams P{a, b, base, y, gamma, beta, len, C, T, gelu, mask, (s->ragged && len) ? 1 : 0, 0, 1e-5f, nullptr, nullptr};
  launch_layernorm(s->stream, P, B);
}

// ek / ev: relative-position tables [2W+1][dk] or null (plain scaled-dot-product attention: StableTTS DiT blocks, BERT).
// 16-query tiles (more, smaller workgroups) while the 32-query MFMA kernel's grid would not fill the chip: measured round 4
// (profiles/r4_c16_threshold.txt) single utterances of 200 - 600 tokens (T_y 600 - 1800) -15..-35 % attention time against the old rule
// (T <= 512), the 32-item batch c3 -6 % (its 200-token text side now runs the MFMA kernel).
static bool relpos_attention_use16(int B, int T, int nh) {
  const bool small_grid = (long)cdiv(T, 32) * nh * B < 256;
  return g_attn_impl == 3 || (g_attn_impl == 0 && (T <= 64 || (small_grid && T <= 4096)));
}
static const char* relpos_attention_kernel_name(int B, int T, int nh) {
  return relpos_attention_use16(B, T, nh) ? "relpos_attention16_kernel"
                                          : (g_attn_impl == 1 ? "relpos_attention_kernel" : "relpos_attention_mfma_kernel");
}
// the kernel choice and launch on stream st (head dim 32 / 64 / 96 and W <= 4: checked at load, or by vits_debug_relpos_attention)
static void launch_relpos_attention_on(hipStream_t st, const float* qkv, const float* ek, const float* ev, const int* len, float* out, int B,
                                       int H, int T, int nh, int W) {
  const int dk = H / nh;
  struct { const float* ek; const float* ev; } L{ek, ev};
  if (relpos_attention_use16(B, T, nh)) {  // short sequences: 16-query tiles, more and smaller workgroups
    dim3 grid(cdiv(T, 16), nh, B);
    const bool w8 = T > 64;
    const int nwv = w8 ? 8 : 4;
    const int wreg = 16 * (dk + 4) + 12 * 16 + 12 * 16, nv = (dk / 16) * 4 + 2;
    const size_t lds = (size_t)nwv * (wreg > nv * 64 ? wreg : nv * 64) * sizeof(float);
#define ATT16_GO(DK_)                                                                                                                  \
  do {                                                                                                                                 \
    if (w8) hipLaunchKernelGGL((relpos_attention16_kernel<DK_, 8>), grid, dim3(512), lds, st, qkv, L.ek, L.ev, len, out, H, T, W);        \
    else hipLaunchKernelGGL((relpos_attention16_kernel<DK_, 4>), grid, dim3(256), lds, st, qkv, L.ek, L.ev, len, out, H, T, W);          \
  } while (0)
    if (dk == 96) ATT16_GO(96);
    else if (dk == 64) ATT16_GO(64);
    else ATT16_GO(32);
#undef ATT16_GO
    return;
  }
  if (g_attn_impl != 1) {  // fp32-MFMA flash kernel (32-query tiles)
    dim3 grid(cdiv(T, 32), nh, B);
    const int wreg = dk * 33 + 10 * 32 + 9 * 32;
    const size_t lds = (size_t)4 * wreg * sizeof(float);
    if (dk == 96) hipLaunchKernelGGL((relpos_attention_mfma_kernel<96>), grid, dim3(256), lds, st, qkv, L.ek, L.ev, len, out, H, T, W);
    else if (dk == 64) hipLaunchKernelGGL((relpos_attention_mfma_kernel<64>), grid, dim3(256), lds, st, qkv, L.ek, L.ev, len, out, H, T, W);
    else hipLaunchKernelGGL((relpos_attention_mfma_kernel<32>), grid, dim3(256), lds, st, qkv, L.ek, L.ev, len, out, H, T, W);
    return;
  }
  dim3 grid(cdiv(T, ATT_TQ), nh, B);
  if (dk == 96) hipLaunchKernelGGL((relpos_attention_kernel<96>), grid, dim3(256), 0, st, qkv, L.ek, L.ev, len, out, H, T, W);
  else if (dk == 64) hipLaunchKernelGGL((relpos_attention_kernel<64>), grid, dim3(256), 0, st, qkv, L.ek, L.ev, len, out, H, T, W);
  else hipLaunchKernelGGL((relpos_attention_kernel<32>), grid, dim3(256), 0, st, qkv, L.ek, L.ev, len, out, H, T, W);
}
static void launch_attention_raw(vits_session* s, const float* qkv, const float* ek, const float* ev, const int* len, float* out, int B,
                                 int H, int T, int nh, int W) {
  ProfScope ps(s, "attention", 4.0 * (double)B * H * T * T, relpos_attention_kernel_name(B, T, nh));
  launch_relpos_attention_on(s->stream, qkv, ek, ev, len, out, B, H, T, nh, W);
}

// Attention with no relative-position terms (window_size=None: the pre-transformer of the `pre_conv` flow) on plain_attention*_kernel
// (kernels_misc.hip.h), the tile variant picked by the rule above; g_attn_impl 2 / 3 force the 32- / 16-query kernel (1, the VALU
// cross-check, has no plain form: the 32-query kernel runs).  Returns false for a head dim the kernels are not built for.
static bool plain_attention_use16(int B, int T, int nh) {
  const bool small_grid = (long)cdiv(T, 32) * nh * B < 256;
  return g_attn_impl == 3 || (g_attn_impl == 0 && (T <= 64 || (small_grid && T <= 4096)));
}
static bool launch_plain_attention_on(hipStream_t st, const float* qkv, const int* len, float* out, int B, int H, int T, int nh) {
  if (nh <= 0 || H % nh || !plain_attention_dk_ok(H / nh)) return false;
  const int dk = H / nh;
  if (plain_attention_use16(B, T, nh)) {
    dim3 grid(cdiv(T, 16), nh, B);
    const bool w8 = T > 64;
    const int wreg = 16 * (dk + 4), nv = (dk / 16) * 4 + 2;
    const size_t lds = (size_t)(w8 ? 8 : 4) * (wreg > nv * 64 ? wreg : nv * 64) * sizeof(float);
#define PATT16_GO(DK_)                                                                                                             \
  case DK_:                                                                                                                        \
    if (w8) hipLaunchKernelGGL((plain_attention16_kernel<DK_, 8>), grid, dim3(512), lds, st, qkv, len, out, H, T);               \
    else hipLaunchKernelGGL((plain_attention16_kernel<DK_, 4>), grid, dim3(256), lds, st, qkv, len, out, H, T);                  \
    break;
    switch (dk) { PATT16_GO(16) PATT16_GO(32) PATT16_GO(48) PATT16_GO(64) PATT16_GO(80) PATT16_GO(96) }
#undef PATT16_GO
    return true;
  }
  dim3 grid(cdiv(T, 32), nh, B);
  const int nd = (dk + 31) / 32, wreg = nd * 32 * 33, nv = nd * 16 + 2;
  const size_t lds = (size_t)4 * (wreg > nv * 64 ? wreg : nv * 64) * sizeof(float);
#define PATT_GO(DK_) \
  case DK_: hipLaunchKernelGGL((plain_attention_kernel<DK_>), grid, dim3(256), lds, st, qkv, len, out, H, T); break;
  switch (dk) { PATT_GO(16) PATT_GO(32) PATT_GO(48) PATT_GO(64) PATT_GO(80) PATT_GO(96) }
#undef PATT_GO
  return true;
}

// The tail of a MonoTransformerFlowLayer (mono_couple_kernel, kernels_misc.hip.h): z = cat(x0 * s, (x1 - (W h + b)) * s * mask) from
// h [B, C, T] and u [B, 2C, T]; mode 0: s = 1 (inter_residual), 1: s = 1/2 (post_residual).  Returns false for a width it is not built for.
static bool launch_mono_couple_on(hipStream_t st, const float* h, const float* u, const float* W, const float* bias, const int* len, float* z,
                                  int B, int C, int T, int mode) {
  if (!mono_couple_c_ok(C)) return false;
  dim3 grid(cdiv(T, 32), B);
#define MONO_GO(N_) \
  case N_: hipLaunchKernelGGL((mono_couple_kernel<N_>), grid, dim3(256), 0, st, h, u, W, bias, len, z, T, mode); break;
  switch (C / 32) { MONO_GO(1) MONO_GO(2) MONO_GO(3) MONO_GO(4) MONO_GO(5) MONO_GO(6) }
#undef MONO_GO
  return true;
}

// one attention layer of encoder E: its own head count, relative-position window (W < 0: none) and width
static void launch_attention(vits_session* s, const float* qkv, const EncoderW& E, const EncLayerW& L, const int* len, float* out, int B, int T) {
  if (E.W >= 0) {
    launch_attention_raw(s, qkv, L.ek, L.ev, len, out, B, E.H, T, E.nh, E.W);
    return;
  }
  ProfScope ps(s, "attention", 4.0 * (double)B * E.H * T * T,
               plain_attention_use16(B, T, E.nh) ? "plain_attention16_kernel" : "plain_attention_kernel");
  launch_plain_attention_on(s->stream, qkv, len, out, B, E.H, T, E.nh);  // (head dim checked at load)
}

