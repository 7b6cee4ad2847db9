// engine_convplan.hip.h -- conv KERNEL SELECTION as host arithmetic: which of the conv kernel instantiations a launch gets (plan_conv), under
// which switches (ConvSelect), and what the instantiation is called in profiles and in the launch log (conv_plan_name).  No HIP calls, no
// session.  Part of the ONE translation unit engine.hip (included there, in order; not a standalone header); launch_conv
// (engine_launch.hip.h) executes the plan.
#pragma once
// ---- every switch that steers the choice.  The hooks are per thread (a hook changes what the calling thread's engine calls launch, never
// what another server thread is running); the environment is read once per process.  A hook beats the environment where both exist.
struct ConvSelect {
  int force_tile = 0;  // vits_debug_force_tile: 0 = size heuristic, 1 = big-tile kernel, 2 = K-split kernel, 3 = small-tile kernel (tests only)
  int ks_waves = 0;    // vits_debug_ks_waves: waves per workgroup of the K-split kernel, 0 = heuristic (ks_pick_waves)
  int wp_mode = 0;     // vits_debug_conv_wp: 0 = heuristic, 1 = never, 2 = whenever eligible (tests)
  int sp_mode = -1;    // vits_debug_conv_sp: -1 = default (by grid size), 0 = never, 1 = by grid size, 2 = whenever eligible (tests)
  int no_bf3 = 0;      // vits_debug_no_bf16x3: 1 = a conv_precision == 1 model runs its fp32 kernels (A/B of the split-bf16 variant)
  long env_ks_threshold = 512;  // VITS_KS_THRESHOLD: 64 x 64 tiles below which a launch is "small" (K-split side of the tree)
  int env_ks_shape = 0;         // VITS_KS_SHAPE (tools/ks_shapes.py): 11 or 12 forces the K-split STORE tile
  long env_big_blocks = 512;    // VITS_BIG_BLOCKS: 128 x 128 tiles from which the 128 x 128 kernel runs
  int env_ks_waves = 0;         // VITS_KS_WAVES: as ks_waves
  int env_wp_mode = 0;          // VITS_CONV_WP: as wp_mode
  int env_ks_chunk = 1;         // VITS_KS_CHUNK: 0 = the 16-wave K-split kernel always splits by tap (A/B of ks_chunk_takes, engine_launch.hip.h)
  int env_ks_pair = 1;          // VITS_KS_PAIR: column-pair workgroups of the chunk split: 0 = never, 1 = ks_pair_takes, 2 = wherever there are two column tiles (tests)
  int ks_force() const { return ks_waves ? ks_waves : env_ks_waves; }
  int wp() const { return wp_mode ? wp_mode : env_wp_mode; }
  int sp() const { return sp_mode >= 0 ? sp_mode : 1; }
};
static ConvSelect conv_select_env() {
  ConvSelect e;
  if (const char* v = getenv("VITS_KS_THRESHOLD")) e.env_ks_threshold = atol(v);
  if (const char* v = getenv("VITS_KS_SHAPE")) e.env_ks_shape = atoi(v);
  if (const char* v = getenv("VITS_BIG_BLOCKS")) e.env_big_blocks = atol(v);
  if (const char* v = getenv("VITS_KS_WAVES")) e.env_ks_waves = atoi(v);
  if (const char* v = getenv("VITS_CONV_WP")) e.env_wp_mode = atoi(v);
  if (const char* v = getenv("VITS_KS_CHUNK")) e.env_ks_chunk = atoi(v);
  e.env_ks_pair = ks_pair_mode_env();  // VITS_KS_PAIR (dec_end_rules.h)
  return e;
}
static ConvSelect& conv_select() {  // the calling thread's copy (the vits_debug_* setters write it)
  static const ConvSelect env = conv_select_env();
  static thread_local ConvSelect sel = env;
  return sel;
}

// ---- the plan: one kernel instantiation and its tile
enum ConvFamily { CONV_BIG, CONV_KS, CONV_C16, CONV_WP, CONV_SP, CONV_BF3 };  // conv_mfma_kernel, conv_mfma_ks_kernel, conv16_kernel, conv_wp_kernel, conv_sp_kernel, conv_bf3_kernel
struct ConvPlan {
  ConvFamily family;
  int epi;
  int WM, WN, MI, NI;  // waves per workgroup in M x N, 32 x 32 blocks per wave in M x N (BIG; KS: MI, NI; BF3: MI)
  int NW;              // waves per workgroup (KS, C16, WP)
  int NIN;             // KS: 1 = one input, 2 = channel-split pair (x_split), 3 = summed inputs (x2)
  int MAXU, PRO;       // C16: tap units per wave; prologue 0 = none, 1 = DDSConv layer, 2 = LayerNorm, 3 = LayerNorm from the producer's statistics
  int JT;              // SP: 64-column blocks of the staging window
  int M_T, N_T;        // output tile
};
static ConvPlan plan_big(int WM, int WN, int MI, int NI, int epi) { return {CONV_BIG, epi, WM, WN, MI, NI, WM * WN, 1, 0, 0, 0, WM * MI * 32, WN * NI * 32}; }
static ConvPlan plan_bf3(int MI, int epi) { return {CONV_BF3, epi, 2, 2, MI, 2, 4, 1, 0, 0, 0, 64 * MI, 128}; }
static ConvPlan plan_sp(int epi, int halo) { return {CONV_SP, epi, 2, 2, 1, 1, 4, 1, 0, 0, halo ? 2 : 1, 64, 64}; }
static ConvPlan plan_wp() { return {CONV_WP, EPI_STORE, 1, 1, 1, 1, 8, 1, 0, 0, 0, 32, 32}; }
static ConvPlan plan_c16_dds() { return {CONV_C16, EPI_STORE, 1, 1, 1, 1, 8, 1, 8, 1, 0, 16, 16}; }

// "name<a,b,...>" exactly as committed profiles, bench.py's roofline line and the tests key on it.  Formats: call it only when the session
// profiles or the launch log is on.
static std::string conv_plan_name(const ConvPlan& p) {
  static const char* const epi[4] = {"STORE", "GATE", "RESSKIP", "COUPLE"};
  char b[64];
  switch (p.family) {
    case CONV_BIG: snprintf(b, sizeof b, "conv_mfma_kernel<%d,%d,%d,%d,%s>", p.WM, p.WN, p.MI, p.NI, epi[p.epi]); break;
    case CONV_KS: snprintf(b, sizeof b, "conv_mfma_ks_kernel<%d,%d,%s,%d,%d>", p.MI, p.NI, epi[p.epi], p.NIN, p.NW); break;
    case CONV_C16:
      if (p.PRO == 1) snprintf(b, sizeof b, "conv16_kernel<STORE,dds>");
      else if (p.PRO) snprintf(b, sizeof b, "conv16_kernel<STORE,ln,%d>", p.NW);
      else snprintf(b, sizeof b, "conv16_kernel<%s,%d>", epi[p.epi], p.NW);
      break;
    case CONV_WP: snprintf(b, sizeof b, "conv_wp_kernel<%d>", p.NW); break;
    case CONV_SP: snprintf(b, sizeof b, "conv_sp_kernel<%s>", epi[p.epi]); break;
    case CONV_BF3: snprintf(b, sizeof b, p.epi == EPI_GATE ? "conv_bf3_kernel<%d,GATE>" : "conv_bf3_kernel<%d>", p.MI); break;
  }
  return b;
}

// ---- eligibility of the special-purpose kernels
// waves per workgroup of the K-split kernel for a grid of nblk workgroups
static int ks_pick_waves(const ConvParams& P, long nblk, const ConvSelect& sel) {
  const int force = sel.ks_force();
  if (force == 4 || force == 8 || force == 16) return force;
  int taps = 0;
  for (int g = 0; g < P.n_groups; ++g) { const int t = P.Cin / CONV_CI_T * P.g[g].K; if (t > taps) taps = t; }
  // few workgroups (less than one per CU): 16 waves each, i.e. 4 per SIMD, as long as every wave still gets >= 2 taps;
  // up to two workgroups per CU: 8 waves (the register file holds 2 x 8 waves of <= 128 registers)
  // measured on the c2 forward (profiles/r2_c2_nw*_bench.json.txt): 16 waves win wherever a wave still gets >= 2 taps, also
  // for the grouped decoder launches of ~450 workgroups; 8 waves only pay for launches of a few rounds of the chip
  if (nblk <= 1024 && taps >= 32) return 16;
  if (nblk <= 2048 && taps >= 16) return 8;
  return 4;
}
// small-tile kernel (conv_small.hip.h): 0 when the launch cannot take it, else the wave count it would run with
static int c16_waves(const ConvParams& P, int epi) {
  const ConvGroup& G = P.g[0];
  if (P.n_groups != 1 || !G.w16 || P.ups_u || G.x3 || (G.x2 && !P.x_split) || P.reflect || P.rag || P.Cin % CONV_CI_T) return 0;
  if (epi == EPI_GATE && (P.H % 8)) return 0;
  const int halo = (G.K - 1) * G.dil;
  if (halo > 48) return 0;
  if (P.ln_g && P.Cin > 8 * C16_LN_MAXC) return 0;
  if (P.ln_g && (halo > 16 || P.in_slope != 1.f || P.in_scale != 1.f || P.x_split || P.x_ch_sign != 1 || P.x_ch_off || epi != EPI_STORE)) return 0;
  const size_t lds = ((size_t)P.Cin * c16_row_pitch(16 + halo) + 16 * 32) * sizeof(float);
  if (lds > 150 * 1024) return 0;
  const int units = P.Cin / CONV_CI_T * G.K;
  if (units <= 4 * C16_MAXU) return 4;
  if (units <= 8 * C16_MAXU) return 8;
  return 0;
}
// 1x1 conv whose B operand is produced by the DDSConv prologue (conv_small.hip.h PRO == 1); P.dds_* set by the caller, who asks for it
static constexpr long C16_COLS_DDS = 800;  // (the fused DDSConv layer wins to ~800 columns, profiles/r4_c16_threshold.txt)
static bool c16_dds_ok(const ConvParams& P, int dds_K, const ConvSelect& sel) {
  return (sel.force_tile == 0 || sel.force_tile == 3) && (long)P.B * P.Tout <= C16_COLS_DDS && P.g[0].w16 && P.g[0].K == 1 && P.Cin % 32 == 0 &&
         P.Cin <= 16 * DDS_MAXI && dds_K == 3 && P.Cin / CONV_CI_T <= 8 * 8 && P.len && (!P.dds_sw || P.dds_dil <= 9);
}
// wave-pipelined kernel for the single-utterance decoder's ResBlock convs (conv_small.hip.h conv_wp_kernel)
static bool conv_wp_ok(const ConvParams& P, int epi, int halo, bool small, const ConvSelect& sel) {
  const int mode = sel.wp();
  if (mode == 1 || epi != EPI_STORE) return false;
  if (P.x_ch_sign != 1 || P.x_ch_off || P.tile_start || P.ups_u || P.reflect || P.in_scale != 1.f || P.ln_g || P.dds_y2 || P.ln_stat_out) return false;
  if (P.Cin % CONV_CI_T || P.Tin < 4 || 32 + halo > WP_PITCH || P.in_slope < 0.f || P.in_slope > 1.f) return false;
  if (P.x_split && (P.n_groups != 1 || P.x_split % CONV_CI_T || !P.g[0].x2)) return false;
  for (int g = 0; g < P.n_groups; ++g)
    if (P.g[g].x3 || (P.g[g].x2 && !P.x_split)) return false;
  if (mode == 2) return true;
  // every wave gets at least one 16-channel chunk; enough columns that 32-column tiles pay (the few-column regime belongs to conv16)
  return small && P.Cin >= 8 * CONV_CI_T && (long)P.B * P.Tout >= 256;
}
// software-pipelined 64 x 64 kernel (conv_sp.hip.h): stands in for conv_mfma_kernel<2,2,1,1,*> on launches that leave a CU with few
// workgroups (grids of up to 2048 workgroups)
static bool conv_sp_ok(const ConvParams& P, int epi, int halo, const ConvSelect& sel) {
  if (sel.sp() == 0 || epi == EPI_GATE) return false;
  if (P.Cin % SP_STAGE_CH || P.ups_u || P.reflect || P.x_split || P.ln_g || P.dds_y2 || P.ln_stat_out || 64 + halo > 128 || P.Tin < 2) return false;
  for (int g = 0; g < P.n_groups; ++g)
    if (P.g[g].x2 || P.g[g].x3) return false;
  return true;
}
static bool sp_takes(const ConvParams& P, int epi, int halo, const ConvSelect& sel) {
  const long nblk = (long)cdiv(P.M, 64) * cdiv(P.Tout, 64) * P.B * P.n_groups;
  return sel.force_tile == 0 && conv_sp_ok(P, epi, halo, sel) && (sel.sp() == 2 || nblk <= 2048);
}
// split-bf16 variant (hparams.conv_precision == 1): same staging pattern as the big-tile kernel, 3 bf16 MFMAs per 16 channels x tap
static bool bf3_ok(const ConvParams& P, const ConvSelect& sel) {
  bool ok = !sel.no_bf3 && !P.reflect && !P.x_split && P.x_ch_sign == 1 && !P.x_ch_off && !P.ln_g;
  ok = ok && P.in_scale >= 0.f && P.in_slope >= 0.f && P.in_slope <= 1.f;  // the staging pass evaluates the leaky ReLU as a max
  if (P.ups_u && (P.ups_cout % 128 || P.n_groups != 1)) ok = false;  // a 128-row tile must lie inside one polyphase phase
  for (int g = 0; g < P.n_groups; ++g) ok = ok && P.g[g].wb && !P.g[g].x2 && !P.g[g].x3;
  return ok;
}

// ---- the decision tree: epilogue + problem size.  halo = max over groups of (K-1)*dil (or the polyphase spread).
// Large problems (>= 2 workgroups per CU with 64x64 tiles) use the big-tile kernel (more operand reuse); everything smaller uses the
// K-split kernel so that one utterance still fills the chip.  Does not write P: the executor moves the heaviest group to the front, so
// what the tree asks of "the first group" it asks of that one.
static ConvPlan plan_conv(const ConvParams& P, int epi, int halo, const ConvSelect& sel) {
  int h = 0;
  for (int g = 1; g < P.n_groups; ++g) if (P.g[g].K > P.g[h].K) h = g;
  const ConvGroup& G0 = P.g[h];
  const int ft = sel.force_tile;
  const long cols = (long)P.B * P.Tout, groups = (long)P.B * P.n_groups;
  const long blocks64 = (long)cdiv(P.M, 64) * cdiv(P.Tout, 64) * groups;
  bool small = ft == 2 || (ft == 0 && blocks64 < sel.env_ks_threshold);
  // (the polyphase upsamplers and the 32-row conv_post leave the K-split kernel earlier: 300-token utterance ups 0.20 -> 0.135 ms,
  //  conv_post 0.092 -> 0.046 ms -- profiles/r4_c16_threshold.txt)
  if (small && ft == 0 && epi == EPI_STORE && (P.ups_u || P.M % 64 == 32) && blocks64 >= 256) small = false;
  if (!G0.x2 && P.in_scale != 1.0f) small = false;  // the K-split kernel folds in_scale into the multi-input sum only
  // Few-column regime (a single utterance's encoder / duration predictor / flow): many small workgroups, LDS-staged B, up to this many
  // columns (B x T).  Round 4, measured on single utterances of 300 - 1000 tokens and on batches of 8 / 16 short requests
  // (profiles/r4_c16_threshold.txt): beyond ~256 columns the K-split / wave-pipelined kernels win the plain convolutions (although the
  // LayerNorm is then a launch of its own), the WaveNet gate conv -- 5 taps, 2H rows, tanh * sigmoid epilogue -- to ~512.
  const long c16_cols = epi == EPI_GATE ? 512 : 256;
  // between ~200 and ~1000 columns the 16-column tiles re-read every weight once per column tile (19 times at 304 columns: the
  // StableTTS estimator, 20 us per conv): the wave-pipelined 32x32 kernel takes those when it can (never a launch that carries a
  // prologue or writes LayerNorm statistics: only conv16 has those)
  const bool wp_first = ft == 0 && cols > 192 && P.Cin >= 256 && !P.ln_g && !P.dds_y2 && conv_wp_ok(P, epi, halo, small, sel);
  if (!wp_first && (ft == 3 || (ft == 0 && cols <= c16_cols))) {
    if (const int nw = c16_waves(P, epi)) {
      const bool few = cdiv(P.Cin / CONV_CI_T * G0.K, nw) <= 8;
      return {CONV_C16, epi, 1, 1, 1, 1, nw, 1, few ? 8 : C16_MAXU, P.ln_g ? (P.ln_stat_in ? 3 : 2) : 0, 0, 16, 16};
    }
  }
  if (sel.sp() == 2 && ft == 0 && conv_sp_ok(P, epi, halo, sel)) return plan_sp(epi, halo);  // A/B: the pipelined kernel wherever it is eligible
  auto ks = [&](int MI, int NI, int nin) {
    const long nblk = (long)cdiv(P.M, MI * 32) * cdiv(P.Tout, NI * 32) * groups;
    return ConvPlan{CONV_KS, epi, 1, 1, MI, NI, ks_pick_waves(P, nblk, sel), nin, 0, 0, 0, MI * 32, NI * 32};
  };
  if (epi == EPI_GATE) {
    if (small) return ks(2, 1, 1);
    if (!sel.no_bf3 && G0.wb && P.n_groups == 1 && P.M % 128 == 0 && P.x_ch_sign == 1 && !P.x_ch_off && !G0.x2 && !P.ln_g && P.in_scale >= 0.f &&
        P.in_slope >= 0.f && P.in_slope <= 1.f && (long)cdiv(P.M, 128) * cdiv(P.Tout, 128) * P.B >= 256)
      return plan_bf3(2, epi);  // split-bf16 WaveNet gate conv (conv_precision == 1)
    // (128 x 128 tiles for the gate conv: 2.30 against 1.77 ms per c3 forward, round 4, profiles/r4_c3_tile_ab.txt)
    // Round 6: a grid of 1 - 3 four-wave workgroups per CU (all resident at once) lasts as long as the CU with the most of them; the
    // same wave tiles in TWO-wave workgroups of 128 x 32 halve the quantum (c3: 580 tiles -> 1160)
    // (only where the four-wave grid is 2 - 6 workgroups per CU: a 6000-frame single utterance -- 282 four-wave workgroups, about one
    //  per CU -- is 3 % SLOWER on two-wave tiles, profiles/r6_gate2w_ab.txt)
    const long nblk64 = (long)cdiv(P.M, 128) * cdiv(P.Tout, 64) * P.B;
    return plan_big(2, ft == 0 && 32 + halo <= 64 && nblk64 >= 512 && nblk64 <= 1536 ? 1 : 2, 2, 1, epi);
  }
  if (epi == EPI_RESSKIP || epi == EPI_COUPLE) {
    if (small) return ks(1, 1, 1);
    return sp_takes(P, epi, halo, sel) ? plan_sp(epi, halo) : plan_big(2, 2, 1, 1, epi);
  }
  if (conv_wp_ok(P, epi, halo, small, sel)) return plan_wp();
  if (small) {
    if (P.x_split) return ks(1, 1, 2);
    const long blocks32 = (long)cdiv(P.M, 32) * cdiv(P.Tout, 32) * groups;
    const bool wide = sel.env_ks_shape == 12 || (sel.env_ks_shape == 0 && blocks32 > 2048);
    return ks(1, wide ? 2 : 1, G0.x2 ? 3 : 1);
  }
  // 32-row outputs (polyphase upsamplers with C_out % 64 != 0, the 32-channel last stage of HiFi-GAN V1): a 64-row tile
  // would spend half its MFMAs on padding rows -> 32 x 128 tiles
  if ((P.ups_u && (P.ups_cout % 64)) || (!P.ups_u && P.M % 64 == 32)) return plan_big(1, 4, 1, 1, epi);
  // 64-row outputs at batch size: 64 x 128 tiles (twice the columns per weight fragment of the 64 x 64 tile)
  if (!P.ups_u && P.M == 64 && (long)cdiv(P.Tout, 128) * groups >= 512) return bf3_ok(P, sel) ? plan_bf3(1, epi) : plan_big(2, 2, 1, 2, epi);
  const long big_blocks = (long)cdiv(P.M, 128) * cdiv(P.Tout, 128) * groups;
  const bool m_fits = (P.M % 128 == 0) && (!P.ups_u || P.ups_cout % 128 == 0);
  if (m_fits && big_blocks >= sel.env_big_blocks) return bf3_ok(P, sel) ? plan_bf3(2, epi) : plan_big(2, 2, 2, 2, epi);
  // 64-row multiples at batch size (encoder / flow STORE convs: 192, 576, 768 rows) of a conv_precision == 1 model
  if (P.M % 64 == 0 && (long)cdiv(P.M, 64) * cdiv(P.Tout, 128) * groups >= 256 && bf3_ok(P, sel)) return plan_bf3(1, epi);
  // (64 x 128 fp32 tiles for these convs were measured on the c3 batch in round 4: 2.21 - 2.42 ms against 2.17 ms per forward for the
  //  64 x 64 tiles -- profiles/r4_c3_tile_ab.txt; not a tile-shape problem)
  return sp_takes(P, epi, halo, sel) ? plan_sp(epi, halo) : plan_big(2, 2, 1, 1, epi);
}

// ---- what the stages ask before they fold a LayerNorm into a conv: only conv16_kernel has the prologue / the statistics epilogue, and a
// wrong answer would be a LayerNorm that is silently never applied.  P: the launch as it will be made, without the ln_* fields.
static int conv_halo(const ConvParams& P) {
  int halo = 0;
  for (int g = 0; g < P.n_groups; ++g) halo = std::max(halo, (P.g[g].K - 1) * P.g[g].dil);
  return halo;
}
static float g_ln_probe = 0.f;  // stands for "some gamma / some statistics buffer": the planner tests the pointers only
static bool conv_takes_ln_prologue(ConvParams P) {  // would this consumer conv normalise its input on load?
  P.ln_g = &g_ln_probe;
  return plan_conv(P, EPI_STORE, conv_halo(P), conv_select()).family == CONV_C16;
}
static bool conv_writes_ln_stats(ConvParams P) {  // would this producer conv write the LayerNorm statistics of its output?
  P.ln_stat_out = &g_ln_probe;
  return plan_conv(P, EPI_STORE, conv_halo(P), conv_select()).family == CONV_C16;
}
