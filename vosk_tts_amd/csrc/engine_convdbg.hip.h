// engine_convdbg.hip.h -- timing / phase-stamp instrumentation of the conv launches (tools/convdbg.py and friends), kept out of the
// dispatcher: the -DCONV_TIMING scopes of launch_conv and launch_c16_dds, and the VITS_CONV_DBG / VITS_CONV_BT report of vits_op_conv1d.
// Part of the ONE translation unit engine.hip (included there, in order; not a standalone header).
#pragma once
static constexpr size_t CONV_DBG_N = 128 + 4 * 4000;  // phase stamps + block trace (timing build)
// block trace: "blk <id> <start> <end> <hw_id> <xcc_id>" (wall clock, 10 ns units, relative to the earliest start)
static void conv_dbg_print_blocks(const long long* d_trace) {
  std::vector<long long> t(4 * 4000);
  hipMemcpy(t.data(), d_trace, t.size() * sizeof(long long), hipMemcpyDeviceToHost);
  long long t0 = 0;
  for (int i = 0; i < 4000; ++i) if (t[4 * i] && (!t0 || t[4 * i] < t0)) t0 = t[4 * i];
  for (int i = 0; i < 4000; ++i)
    if (t[4 * i]) fprintf(stderr, "blk %d %lld %lld %lld %lld\n", i, t[4 * i] - t0, t[4 * i + 1] ? t[4 * i + 1] - t0 : -1, t[4 * i + 2], t[4 * i + 3]);
}

#ifdef CONV_TIMING
// launch_conv: VITS_DBG_LAUNCH=<i> attaches the phase-stamp buffer to the i-th conv launch of the process and prints the stamps (cycles
// since kernel start, block 0) right after it; VITS_DBG_GROUPED=<n>: the n-th three-group launch of the process instead (the
// single-utterance decoder's ResBlock launches)
struct ConvTimingScope {
  bool on; hipStream_t st; const char* name; int M, Cin, K, T, B;
  static long long*& buf() { static long long* b = nullptr; return b; }
  ConvTimingScope(vits_session* s, ConvParams& P, const char* name_) : st(s->stream), name(name_), M(P.Cout), Cin(P.Cin), K(P.g[0].K), T(P.Tout), B(P.B) {
    static long dbg_counter = 0, grouped_counter = 0;
    static const long dbg_want = getenv("VITS_DBG_LAUNCH") ? atol(getenv("VITS_DBG_LAUNCH")) : -1;
    static const long grouped_want = getenv("VITS_DBG_GROUPED") ? atol(getenv("VITS_DBG_GROUPED")) : -1;
    on = (dbg_counter++ == dbg_want) || (P.n_groups == 3 && grouped_counter++ == grouped_want);
    if (!on) return;
    if (!buf()) hipMalloc((void**)&buf(), CONV_DBG_N * sizeof(long long));
    hipMemsetAsync(buf(), 0, CONV_DBG_N * sizeof(long long), st);
    P.dbg = buf();
  }
  ~ConvTimingScope() {
    if (!on) return;
    long long h[128];
    hipStreamSynchronize(st);
    hipMemcpy(h, buf(), sizeof h, hipMemcpyDeviceToHost);
    fprintf(stderr, "[in-forward conv dbg] %s M=%d Cin=%d K=%d T=%d B=%d\n", name, M, Cin, K, T, B);
    for (int w = 0; w < 4; ++w)
      fprintf(stderr, "   wave %d: +%lld first-loads-issued  +%lld loop_done  +%lld barrier  +%lld reduced  +%lld end\n", w, h[w * 8 + 1] - h[w * 8],
              h[w * 8 + 2] - h[w * 8], h[w * 8 + 3] - h[w * 8], h[w * 8 + 4] - h[w * 8], h[w * 8 + 5] - h[w * 8]);
    conv_dbg_print_blocks(buf() + 128);
  }
};
// launch_c16_dds: VITS_DBG_DDS=<i> prints the phase stamps (cycles since kernel start, block 0, wave 0) of the i-th DDS launch
struct DdsTimingScope {
  bool on; hipStream_t st; const char* name;
  static long long*& buf() { static long long* b = nullptr; return b; }
  DdsTimingScope(vits_session* s, ConvParams& P, const char* name_) : st(s->stream), name(name_) {
    static long dds_counter = 0;
    static const long dds_want = getenv("VITS_DBG_DDS") ? atol(getenv("VITS_DBG_DDS")) : -1;
    on = dds_counter++ == dds_want;
    if (!on) return;
    if (!buf()) hipMalloc((void**)&buf(), 128 * sizeof(long long));
    hipMemsetAsync(buf(), 0, 128 * sizeof(long long), st);
    P.dbg = buf();
  }
  ~DdsTimingScope() {
    if (!on) return;
    long long h[128];
    hipStreamSynchronize(st);
    hipMemcpy(h, buf(), sizeof h, hipMemcpyDeviceToHost);
    fprintf(stderr, "[dds dbg] %s: wave 0 cycles since start: prefetch-issued %lld | phaseA-done %lld | dw+sum1 %lld | staged %lld | mfma-done %lld | end %lld\n", name,
            h[1] - h[0], h[6] - h[0], h[7] - h[0], h[2] - h[0], h[3] - h[0], h[5] - h[0]);
  }
};
#else
struct ConvTimingScope { ConvTimingScope(vits_session*, ConvParams&, const char*) {} };
struct DdsTimingScope { DdsTimingScope(vits_session*, ConvParams&, const char*) {} };
#endif

// vits_op_conv1d: VITS_CONV_DBG=<reps> repeats the launch, times it with events and prints block 0's phase stamps (meaningful in the timing
// build); VITS_CONV_BT adds the block trace of the last launch
struct ConvOpDbg {
  const char* env = getenv("VITS_CONV_DBG");
  const int reps = env ? atoi(env) : 1;
  long long* d_dbg = nullptr;
  hipEvent_t e0, e1, ea;
  explicit ConvOpDbg(ConvParams& P) {
    if (env) { hipMalloc((void**)&d_dbg, CONV_DBG_N * sizeof(long long)); hipMemset(d_dbg, 0, CONV_DBG_N * sizeof(long long)); P.dbg = d_dbg; }
    hipEventCreate(&e0); hipEventCreate(&e1); hipEventCreate(&ea);
  }
  void before_launch(int r) {
    if (r == 1 || reps == 1) hipEventRecord(ea, 0);  // all launches after the first (steady state, operands cache-warm)
    if (r == reps - 1) hipEventRecord(e0, 0);
  }
  void after_launches() { hipEventRecord(e1, 0); }
  void report(int B, int Cin, int Cout, int Mpad, int T, int K, int dil) {
    if (!d_dbg) return;
    const int n = reps > 1 ? reps - 1 : 1;
    long long h[128]; float ms = 0, msa = 0;
    hipMemcpy(h, d_dbg, sizeof h, hipMemcpyDeviceToHost);
    hipEventElapsedTime(&ms, e0, e1);
    hipEventElapsedTime(&msa, ea, e1);
    fprintf(stderr, "[conv dbg] B=%d Cin=%d Cout=%d T=%d K=%d dil=%d: last launch %.2f us (event), %.2f us/launch over the last %d back-to-back launches = %.1f TFLOP/s; block 0 cycles since kernel start:\n",
            B, Cin, Cout, T, K, dil, ms * 1e3, msa * 1e3 / n, n, 2.0 * B * Cin * Cout * (double)T * K / (msa * 1e-3 / n) / 1e12);
    int nb = -1, nb2 = -1, nb3 = -1;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, conv_mfma_kernel<2, 2, 2, 2, EPI_STORE>, 256, 2 * CONV_CI_T * (128 + 64) * 4);
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb2, conv_mfma_kernel<2, 2, 1, 1, EPI_STORE>, 256, 2 * CONV_CI_T * (64 + 64) * 4);
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb3, conv_mfma_ks_kernel<1, 1, EPI_STORE, 1, 4>, 256, 16384);
    hipFuncAttributes fa; hipFuncGetAttributes(&fa, (const void*)conv_mfma_kernel<2, 2, 2, 2, EPI_STORE>);
    fprintf(stderr, "   occupancy API (blocks/CU): T128 %d  T64 %d  ks %d ; T128 numRegs %d sharedStatic %zu localMem %zu maxDynShared %d\n", nb, nb2, nb3, fa.numRegs,
            fa.sharedSizeBytes, fa.localSizeBytes, fa.maxDynamicSharedSizeBytes);
    if ((long)cdiv(Mpad, 64) * cdiv(T, 64) * B >= 512) {
      for (int w = 0; w < 4; ++w)
        fprintf(stderr, "   [big-tile] wave %d: prologue %lld  taps %lld  store+barrier %lld  mainloop_end %lld  end %lld  (MFMA floor %lld)\n", w, h[w * 8], h[w * 8 + 1],
                h[w * 8 + 2], h[w * 8 + 3], h[w * 8 + 4], (long long)(Cin / 2) * K * 4 * 64);
    } else {
      for (int w = 0; w < 16; ++w)  // stamps relative to wave 0's start; HW_ID: simd = bits 5:4, cu = bits 11:8, se = bits 15:13
        if (h[w * 8]) fprintf(stderr, "   wave %2d simd %lld cu %lld: start %+lld | +%lld  +%lld  +%lld  +%lld  +%lld  +%lld\n", w, (h[w * 8 + 7] >> 4) & 3, (h[w * 8 + 7] >> 8) & 15,
                h[w * 8] - h[0], h[w * 8 + 1] - h[w * 8], h[w * 8 + 2] - h[w * 8], h[w * 8 + 3] - h[w * 8], h[w * 8 + 4] - h[w * 8], h[w * 8 + 5] - h[w * 8], h[w * 8 + 6] - h[w * 8]);
    }
    if (getenv("VITS_CONV_BT")) conv_dbg_print_blocks(d_dbg + 128);  // block trace of the LAST launch (timing build)
  }
  ~ConvOpDbg() {
    if (d_dbg) hipFree(d_dbg);
    hipEventDestroy(e0); hipEventDestroy(e1); hipEventDestroy(ea);
  }
};
