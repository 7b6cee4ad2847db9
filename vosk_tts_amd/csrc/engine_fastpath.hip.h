// engine_fastpath.hip.h -- the graph-replayed host entry points (vits_synthesize / vits_synthesize_pcm16 fast path): front / back contexts, capture, replay.
// Part of the ONE translation unit engine.hip (included there, in order; not a standalone header): split out in round 6 so that the
// planner / launch selection / stages / host paths can be read on their own.
#pragma once
// ---- fast path of the host entry point --------------------------------------------------------------------------
// What Synth.synth_audio brackets (vosk_tts/synth.py:122-131) is ids on the host -> waveform on the host, one request at a
// time, each with its own scales and a fresh noise draw.  Replaying that as captured hipGraphs needs three things:
//   * per-call scalars (scales, seed, pcm scale) live in a device block the kernels read (SynthDev), inputs are copied
//     through ONE pinned staging buffer by a memcpy node of the graph -> a graph depends on shapes only;
//   * shapes are bucketed: T_x up to a multiple of 8, T_y up to a multiple of 32.  Every stage up to the flow masks per
//     item (exactly the ragged-batch machinery), and the decoder of a bucketed single utterance reads zeros beyond the
//     item's own end at every stage (rag halo 0) -- the arithmetic of the exact-size run on every valid sample;
//   * T_y is only known after the duration predictor: phase 1 (text encoder .. durations) is one graph of a FRONT
//     context (FastFront) keyed by (B, T_x bucket); phase 2 (prior sample, flow, decoder, optional int16 conversion, D2H) one
//     graph of a BACK context (FastBack) per frame bucket, which reads the front's stats / cum / cond vectors / lengths in place.
// Per call: take an idle front out of the model's cache (or build one), fill the pinned block, launch graph 1, wait (the one host
// round trip the path needs), find or build the back, launch graph 2, wait, copy out, put the front back.  No hipMalloc / hipFree /
// re-plan in steady state.  Who is kept and who goes is ctx_cache.hip.h (IdleCache of fronts per model, LruSlots of backs per front
// and of rates per back; the caps are named there); what a context owns and how it is freed is below.  Calls that inject noise
// tensors (parity tests) take the eager path below (synth_eager), which is also the A/B reference of the fast path in tests.
static thread_local int g_fast_path = 1;
// cap on the device memory idle fast-path contexts may pin per model: VITS_CACHE_MB, else a quarter of what was free on the device
// when the first call asked (at most 24 GiB).  Besides the cap, an allocation failure on the request path evicts every idle
// front and retries once (retry_nomem, fronts_evict_all).
static size_t fast_cache_cap() {
  static const size_t cap = [] {
    if (getenv("VITS_CACHE_MB")) return (size_t)atol(getenv("VITS_CACHE_MB")) << 20;
    size_t fr = 0, tot = 0;
    size_t c = (size_t)24 << 30;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr / 4 < c) c = fr / 4;
    return c;
  }();
  return cap;
}

// ---- the two contexts.  Each owns a session (`s`: workspace, error word, the fields the stages read) and, next to it, exactly what
// its phase of the call needs; front_free / back_free / rate_free release exactly that.
// BACK: phase 2 of one frame bucket.  Its session borrows the front's stream.
struct FastBack {
  vits_session* s = nullptr;
  float* out_d = nullptr;          // fp32 audio [B, T_y bucket * hop] on the device
  int16_t* pcm_d = nullptr;        // int16 PCM, same shape
  char* out_h = nullptr;           // pinned host copy of whichever output the call asked for
  size_t out_elems = 0;
  int* h_err = nullptr;            // pinned copy of s->d_err, written by the phase-2 graph
  hipGraphExec_t g2[16] = {};      // [item_scales*8 + persist*4 + solo*2 + pcm]; a call without per-item noise scales only ever touches 0..7
  // phase 2 at another output rate (include/vits_resample.h).  The rate changes a launch and the size of the output, so it is part of
  // the graph key: one entry per rate, with its own graphs and its own output buffers [B, ceil(T_y bucket * hop * L / M)].
  struct RateOut {
    hipGraphExec_t g2[16] = {};    // as g2 above
    void* y_d = nullptr;           // device: float or int16 (sized for float)
    char* y_h = nullptr;           // pinned host copy
    long long n_cap = 0;           // outputs per item
    LoudWs* lw = nullptr;          // as FastBack::lw below
  };
  LruSlots<int, RateOut> rates;    // by rate_out
  LoudWs* lw = nullptr;            // scratch and output buffers of the calls with VITS_FLAG_LOUDNESS, allocated by the first of them
};
// FRONT: phase 1 of one (B, T_x bucket), the call's stream, its input block and its backs.
struct FastFront {
  vits_session* s = nullptr;
  char *io_h = nullptr, *io_d = nullptr;  // per-call inputs: pinned host mirror and device copy (SynthDev | lengths | sid | ids | forced | seeds [| bert])
  size_t io_bytes = 0, io_len = 0, io_sid = 0, io_ids = 0, io_forced = 0, io_seeds = 0, io_bert = 0;  // io_bert: float [B, bert_dim, TxB] (BERT-conditioned voices), 0 = none
  int64_t* h_ylen = nullptr;       // pinned [B] + one int error word behind it
  hipGraphExec_t g1[32] = {};      // [ctl*16 + marks*8 + persist*4 + forced*2 + solo]; a call without marks only ever touches 0..7, one without controls 0..15
  // prosody controls (include/vits_prosody.h), behind everything an uncontrolled call copies (io_plain bytes): item scales float [B, 3],
  // token_length_scale float [B, TxB], token_pause int32 [B, TxB], fit_frames int32 [B], and the regulator's ratio block (float [B] +
  // int [B]), which the controlled variants of g1 copy back into the same place of the pinned mirror
  size_t io_plain = 0, io_iscales = 0, io_tls = 0, io_pause = 0, io_fit = 0, io_ratio = 0;
  // speech marks (include/vits_marks.h): token ends int64 [B, T_x bucket] on the device and their pinned copy, allocated by the first
  // request that asks for marks; the marks variants of g1 write and copy them in front of the h_ylen copy
  long long* marks_d = nullptr;
  int64_t* marks_h = nullptr;
  LruSlots<int, FastBack> backs;   // by frame bucket
};

// (every free of a rate or a back comes after a wait on the front's stream: their graphs and buffers may still be queued there)
static void rate_free(FastBack::RateOut* R) {
  for (hipGraphExec_t g : R->g2) if (g) hipGraphExecDestroy(g);
  if (R->y_d) hipFree(R->y_d);
  if (R->y_h) hipHostFree(R->y_h);
  loud_ws_delete(R->lw);
  delete R;
}
static void back_free(FastBack* Bk) {
  for (FastBack::RateOut* R : Bk->rates.drain()) rate_free(R);
  loud_ws_delete(Bk->lw);
  for (hipGraphExec_t g : Bk->g2) if (g) hipGraphExecDestroy(g);
  if (Bk->out_d) hipFree(Bk->out_d);
  if (Bk->pcm_d) hipFree(Bk->pcm_d);
  if (Bk->out_h) hipHostFree(Bk->out_h);
  if (Bk->h_err) hipHostFree(Bk->h_err);
  session_unborrow(Bk->s);
  delete Bk;
}
static void front_drop_backs(FastFront* F) {
  hipStreamSynchronize(F->s->stream);
  for (FastBack* Bk : F->backs.drain()) back_free(Bk);
}
static void front_free(FastFront* F) {
  if (!F) return;
  if (F->s) {
    hipSetDevice(F->s->m->device);
    front_drop_backs(F);
  }
  for (hipGraphExec_t g : F->g1) if (g) hipGraphExecDestroy(g);
  if (F->marks_d) hipFree(F->marks_d);
  if (F->marks_h) hipHostFree(F->marks_h);
  if (F->io_h) hipHostFree(F->io_h);
  if (F->io_d) hipFree(F->io_d);
  if (F->h_ylen) hipHostFree(F->h_ylen);
  session_free(F->s);
  delete F;
}

// device bytes a context pins while it is cached (a front: with its backs)
static size_t back_device_bytes(const FastBack* Bk) {
  size_t n = Bk->s->arena_bytes + Bk->out_elems * (sizeof(float) + sizeof(int16_t)) + loud_ws_bytes(Bk->lw);
  Bk->rates.for_each([&](const FastBack::RateOut& R) { n += (size_t)Bk->s->B * R.n_cap * sizeof(float) + loud_ws_bytes(R.lw); });
  return n;
}
static size_t front_device_bytes(const FastFront* F) {
  size_t n = F->s->arena_bytes + F->io_bytes;
  if (F->marks_d) n += sizeof(long long) * (size_t)F->s->B * F->s->Tx;
  F->backs.for_each([&](const FastBack& Bk) { n += back_device_bytes(&Bk); });
  return n;
}

static int front_acquire(vits_model* m, int B, int TxB, FastFront** out) {
  if ((*out = m->fronts.take(std::make_pair(B, TxB)))) return VITS_OK;
  FastFront* F = new FastFront();
  int rc = session_new(m, &F->s);
  if (rc != VITS_OK) { front_free(F); return rc; }
  vits_session* s = F->s;
  s->ps_roles = PERSIST_ENC | PERSIST_SDP;
  // per-call input block: [SynthDev | lengths int64 [B] | sid int64 [B] | ids int64 [B,TxB] | forced int32 [B,TxB]]
  // (allocated BEFORE the workspace is laid out: the text-encoder program of a BERT-conditioned voice is resolved against io_d + io_bert)
  F->io_len = align_up(sizeof(SynthDev), 64);
  F->io_sid = F->io_len + align_up(sizeof(int64_t) * B, 64);
  F->io_ids = F->io_sid + align_up(sizeof(int64_t) * B, 64);
  F->io_forced = F->io_ids + align_up(sizeof(int64_t) * (size_t)B * TxB, 64);
  F->io_seeds = F->io_forced + align_up(sizeof(int32_t) * (size_t)B * TxB, 64);
  F->io_bytes = F->io_seeds + align_up(sizeof(unsigned long long) * B, 64);
  if (m->hp.bert_dim > 0) {  // the `bert` feed of a BERT-conditioned voice (vosk_tts/synth.py:88-99) rides in the same block: [B, bert_dim, TxB]
    F->io_bert = F->io_bytes;
    F->io_bytes += align_up(sizeof(float) * (size_t)B * m->hp.bert_dim * TxB, 64) + 256;  // (+ slack: the program's operand window reads whole 16-column tiles)
  }
  F->io_plain = F->io_bytes;  // (what the uncontrolled graphs copy: the block as it was before the controls)
  F->io_iscales = F->io_bytes;
  F->io_tls = F->io_iscales + align_up(sizeof(float) * (size_t)B * 3, 64);
  F->io_pause = F->io_tls + align_up(sizeof(float) * (size_t)B * TxB, 64);
  F->io_fit = F->io_pause + align_up(sizeof(int32_t) * (size_t)B * TxB, 64);
  F->io_ratio = F->io_fit + align_up(sizeof(int32_t) * (size_t)B, 64);
  F->io_bytes = F->io_ratio + align_up(sizeof(float) * (size_t)2 * B, 64);
  if (hipHostMalloc((void**)&F->io_h, F->io_bytes) != hipSuccess || hipMalloc((void**)&F->io_d, F->io_bytes) != hipSuccess ||
      hipHostMalloc((void**)&F->h_ylen, sizeof(int64_t) * (B + 1)) != hipSuccess) {
    front_free(F);
    return fail(VITS_ERR_NOMEM, "fast-path staging buffers");
  }
  memset(F->io_h, 0, F->io_bytes);
  if (F->io_bert && B == 1) s->ps_bert = reinterpret_cast<const float*>(F->io_d + F->io_bert);
  rc = session_reserve(s, B, TxB, 1);
  if (rc != VITS_OK) { front_free(F); return rc; }
  *out = F;
  return VITS_OK;
}

static void front_release(vits_model* m, FastFront* F) {
  for (FastFront* e : m->fronts.put(std::make_pair(F->s->B, F->s->Tx), F, front_device_bytes(F))) front_free(e);
}

// frees every idle front (and its backs): the answer to a failed allocation on the request path
static void fronts_evict_all(vits_model* m) {
  for (FastFront* e : m->fronts.take_all()) front_free(e);
  (void)hipGetLastError();
}
extern "C++" {  // (two templates; this file is included inside engine.hip's extern "C")
// that answer itself: what failed for want of memory is tried once more after `relieve` has freed what the call can spare
template <typename Try, typename Relieve>
static int retry_nomem(Try attempt, Relieve relieve) {
  int rc = attempt();
  if (rc == VITS_ERR_NOMEM) { relieve(); rc = attempt(); }
  return rc;
}

// rows of Tx values -> rows of the bucket TxB, bucket columns zero
template <typename T>
static void pad_rows(T* dst, const T* src, size_t rows, int Tx, int TxB) {
  for (size_t r = 0; r < rows; ++r) {
    memcpy(dst + r * TxB, src + r * Tx, sizeof(T) * Tx);
    for (int t = Tx; t < TxB; ++t) dst[r * TxB + t] = 0;
  }
}
}  // extern "C++"

// back context of `F` for frame bucket TyB (created on first use; at most VITS_BACKS_PER_FRONT buckets stay cached per front)
static int back_get(FastFront* F, int TyB, FastBack** out) {
  if ((*out = F->backs.find(TyB))) return VITS_OK;
  if (FastBack* lru = F->backs.make_room(VITS_BACKS_PER_FRONT)) {
    hipStreamSynchronize(F->s->stream);
    back_free(lru);
  }
  vits_model* m = F->s->m;
  FastBack* Bk = new FastBack();
  int rc = session_borrow(m, F->s->stream, "back session", &Bk->s);
  if (rc != VITS_OK) { back_free(Bk); return rc; }
  vits_session* s = Bk->s;
  s->ps_roles = PERSIST_FLOW;
  s->ps_defer = true;  // planned below, once the shared tensors point into the front
  rc = session_reserve(s, F->s->B, F->s->Tx, TyB);
  Bk->out_elems = (size_t)F->s->B * TyB * m->hp.hop_length;
  if (rc == VITS_OK && (hipMalloc((void**)&Bk->out_d, Bk->out_elems * sizeof(float)) != hipSuccess ||
                        hipMalloc((void**)&Bk->pcm_d, Bk->out_elems * sizeof(int16_t)) != hipSuccess ||
                        hipHostMalloc((void**)&Bk->out_h, Bk->out_elems * sizeof(float)) != hipSuccess ||
                        hipHostMalloc((void**)&Bk->h_err, 64) != hipSuccess))
    rc = fail(VITS_ERR_NOMEM, "fast-path output buffers (%zu samples)", Bk->out_elems);
  if (Bk->h_err) *Bk->h_err = 0;
  if (rc != VITS_OK) { back_free(Bk); return rc; }
  // phase 2 reads the front's phase-1 results in place
  const vits_session* f = F->s;
  s->stats = f->stats; s->cum = f->cum; s->condv = f->condv; s->len_y = f->len_y; s->len_x = f->len_x; s->ylen64 = f->ylen64;
  s->dv = reinterpret_cast<const SynthDev*>(F->io_d);
  s->item_seeds = reinterpret_cast<const unsigned long long*>(F->io_d + F->io_seeds);
  // the persistent flow program was resolved against this session's own len_y / condv: resolve it again against the front's
  persist_plan(s);
  F->backs.insert(TyB, Bk);
  *out = Bk;
  return VITS_OK;
}

// output buffers and graphs of back Bk at the rate of `T` (created on first use; at most VITS_RATES_PER_BACK rates stay cached per back)
static int back_rate_get(FastFront* F, FastBack* Bk, const ResampleTab& T, FastBack::RateOut** out) {
  if ((*out = Bk->rates.find(T.P.rate_out))) return VITS_OK;
  if (FastBack::RateOut* lru = Bk->rates.make_room(VITS_RATES_PER_BACK)) {
    hipStreamSynchronize(F->s->stream);
    rate_free(lru);
  }
  FastBack::RateOut* R = new FastBack::RateOut();
  R->n_cap = T.P.n_out((long long)Bk->s->Ty * F->s->m->hp.hop_length);
  const size_t bytes = (size_t)F->s->B * R->n_cap * sizeof(float);
  if (hipMalloc(&R->y_d, bytes) != hipSuccess || hipHostMalloc((void**)&R->y_h, bytes) != hipSuccess) {
    rate_free(R);
    (void)hipGetLastError();
    return fail(VITS_ERR_NOMEM, "fast-path output buffers at %d Hz (%zu bytes)", T.P.rate_out, bytes);
  }
  Bk->rates.insert(T.P.rate_out, R);
  *out = R;
  return VITS_OK;
}

// A capture that does not reach capture_end (an early return between Begin and End) must not leave the stream in capture mode:
// every later call on the session would fail.  The guard ends and discards it.
struct CaptureGuard {
  hipStream_t st; bool done = false;
  explicit CaptureGuard(hipStream_t s) : st(s) {}
  ~CaptureGuard() {
    if (done) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
      hipGraph_t g = nullptr;
      hipStreamEndCapture(st, &g);
      if (g) hipGraphDestroy(g);
    }
    (void)hipGetLastError();
  }
};
static int capture_end(vits_session* s, hipGraphExec_t* out, CaptureGuard* guard = nullptr) {
  hipGraph_t g = nullptr;
  if (guard) guard->done = true;
  HIP_TRY(hipStreamEndCapture(s->stream, &g));
  hipError_t e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  if (e != hipSuccess) return fail(VITS_ERR_DEVICE, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
  return VITS_OK;
}

// marks: the variants that also turn cum into token ends (marks.hip.h) and copy them to F->marks_h, in front of the h_ylen copy -- the
// host reads them after the one synchronisation the call performs anyway.  L / M of the call ride in the per-call block.
// ctl (include/vits_prosody.h): the variants of a call whose controls reach past scalars -- they copy the whole input block, run the
// launch branch with regulate_ctl_kernel in place of durations_kernel (never the single-utterance program), let the noise-scale kernel read
// the item scales, and copy the regulator's ratio block back in front of the h_ylen copy.
static int phase1_launch(FastFront* F, bool forced, bool solo, bool marks = false, bool ctl = false) {
  vits_session* s = F->s;
  const int gi = (ctl ? 16 : 0) + (marks ? 8 : 0) + (persist_mask() ? 4 : 0) + (forced ? 2 : 0) + (solo ? 1 : 0);
  if (!F->g1[gi]) {
    const int B = s->B, TxB = s->Tx;
    HIP_TRY(hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal));
    CaptureGuard cg(s->stream);
    hipMemcpyAsync(F->io_d, F->io_h, ctl ? F->io_bytes : F->io_plain, hipMemcpyHostToDevice, s->stream);
    s->ragged = true; s->solo = solo; s->tile_keys.clear();
    if (ctl) {
      s->item_scales = reinterpret_cast<const float*>(F->io_d + F->io_iscales);
      s->ctl = RegCtl{s->item_scales, reinterpret_cast<const float*>(F->io_d + F->io_tls), reinterpret_cast<const int*>(F->io_d + F->io_pause),
                      reinterpret_cast<const int*>(F->io_d + F->io_fit), reinterpret_cast<float*>(F->io_d + F->io_ratio)};
      s->ctl_on = true;
    }
    struct CtlOff { vits_session* s; ~CtlOff() { s->item_scales = nullptr; s->ctl_on = false; s->ctl = RegCtl{}; } } ctl_off{s};
    s->dv = reinterpret_cast<const SynthDev*>(F->io_d);
    s->item_seeds = reinterpret_cast<const unsigned long long*>(F->io_d + F->io_seeds);
    const int64_t* d_len = reinterpret_cast<const int64_t*>(F->io_d + F->io_len);
    const int64_t* d_sid = reinterpret_cast<const int64_t*>(F->io_d + F->io_sid);
    const int64_t* d_ids = reinterpret_cast<const int64_t*>(F->io_d + F->io_ids);
    const int32_t* d_forced = reinterpret_cast<const int32_t*>(F->io_d + F->io_forced);
    run_cond(s, d_sid, B, d_len, s->len_x, TxB);
    if (!ctl && persist_mask() == (PERSIST_SDP | PERSIST_ENC | PERSIST_FLOW) && B == 1 && s->ps_front[forced ? 0 : 1].ok && (!F->io_bert || s->ps_bert)) {
      // text encoder [+ duration predictor] + durations as one persistent launch (a BERT-conditioned voice: the program reads the
      // `bert` tensor straight from the input block, two more steps)
      persist_launch(s, s->ps_front[forced ? 0 : 1], "front.persist", nullptr, 0.f, 0, d_ids, forced ? d_forced : nullptr, 1.f, 0.f);
      s->ea_pending = false;
    } else {
      run_text_encoder(s, d_ids, B, TxB, F->io_bert ? reinterpret_cast<const float*>(F->io_d + F->io_bert) : nullptr);
      if (!forced) run_duration(s, s->x, nullptr, 0.f, 0, B, TxB, true);
      run_durations(s, forced ? d_forced : nullptr, 1.f, B, TxB, 0);
    }
    if (marks) {
      token_ends_launch(s, s->cum, s->len_x, B, TxB, s->m->hp.hop_length, 1, 1, s->dv, F->marks_d);
      hipMemcpyAsync(F->marks_h, F->marks_d, sizeof(int64_t) * (size_t)B * TxB, hipMemcpyDeviceToHost, s->stream);
    }
    if (ctl) hipMemcpyAsync(F->io_h + F->io_ratio, F->io_d + F->io_ratio, sizeof(float) * (size_t)2 * B, hipMemcpyDeviceToHost, s->stream);
    hipMemcpyAsync(F->h_ylen, s->ylen64, sizeof(int64_t) * B, hipMemcpyDeviceToHost, s->stream);
    hipMemcpyAsync(F->h_ylen + B, s->d_err, sizeof(int), hipMemcpyDeviceToHost, s->stream);
    s->ragged = false; s->solo = false;
    TRY(capture_end(s, &F->g1[gi], &cg));
  }
  HIP_TRY(hipGraphLaunch(F->g1[gi], s->stream));
  return VITS_OK;
}

// R / T: the output rate's buffers and table (both null: the native rate)
// iscales (include/vits_prosody.h): the variants whose prior sample reads the item scales of the front's input block (B > 1 only)
static int phase2_launch(FastFront* F, FastBack* Bk, bool solo, bool pcm, FastBack::RateOut* R = nullptr, const ResampleTab* T = nullptr,
                         bool iscales = false) {
  vits_session* s = Bk->s;  // (its stream is the front's)
  const int gi = (iscales ? 8 : 0) + (persist_mask() ? 4 : 0) + (solo ? 2 : 0) + (pcm ? 1 : 0);
  hipGraphExec_t* g2 = R ? R->g2 : Bk->g2;
  if (!g2[gi]) {
    const int B = F->s->B, TxB = F->s->Tx, TyB = s->Ty;
    const long long stride = (long long)TyB * F->s->m->hp.hop_length;
    HIP_TRY(hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal));
    CaptureGuard cg(s->stream);
    s->ragged = true; s->solo = solo; s->rag_b1 = true; s->tile_keys.clear();
    s->item_scales = iscales ? reinterpret_cast<const float*>(F->io_d + F->io_iscales) : nullptr;
    struct ScalesOff { vits_session* s; ~ScalesOff() { s->item_scales = nullptr; } } scales_off{s};
    float* z;
    if (!iscales && persist_mask() == (PERSIST_SDP | PERSIST_ENC | PERSIST_FLOW) && B == 1 && s->ps_back.ok) {  // prior sample + flow as one persistent launch
      persist_launch(s, s->ps_back, "back.persist");
      z = s->zB;
    } else {
      run_expand(s, nullptr, TyB, 0.f, 0, s->zA, B, TxB, TyB);
      z = run_flow(s, B, TyB);
    }
    // a lone utterance decodes as the exact-size run does (zeros beyond its end); batches keep the reference's padded-batch
    // continuation over the halo unless the caller asked for independent items
    run_decoder(s, z, true, B, TyB, Bk->out_d, stride, true, !(solo || B == 1));
    if (R) {  // the resampler reads each item's own [0, len) of the decoder's output; at int16 it stands where pcm16_kernel stands
      ProfScope ps(s, "out.resample", 2.0 * B * R->n_cap * T->P.taps, pcm ? "resample_kernel<int16>" : "resample_kernel<float>");
      const int hop = F->s->m->hp.hop_length;
      if (pcm) resample_launch<int16_t>(s->stream, *T, Bk->out_d, stride, 0, stride, Items{s->len_y, hop}, B, static_cast<int16_t*>(R->y_d), R->n_cap, 0, R->n_cap, 1.f, s->dv);
      else resample_launch<float>(s->stream, *T, Bk->out_d, stride, 0, stride, Items{s->len_y, hop}, B, static_cast<float*>(R->y_d), R->n_cap, 0, R->n_cap, 1.f, nullptr);
      hipMemcpyAsync(R->y_h, R->y_d, (size_t)B * R->n_cap * (pcm ? sizeof(int16_t) : sizeof(float)), hipMemcpyDeviceToHost, s->stream);
    } else if (pcm) {
      {
        ProfScope ps(s, "out.pcm16", 0, "pcm16_kernel");
        hipLaunchKernelGGL(pcm16_kernel, dim3(cdiv((int)stride, 256), B), dim3(256), 0, s->stream, Bk->out_d, stride, Bk->pcm_d, stride, stride, 1.f, s->dv);
      }
      hipMemcpyAsync(Bk->out_h, Bk->pcm_d, Bk->out_elems * sizeof(int16_t), hipMemcpyDeviceToHost, s->stream);
    } else {
      hipMemcpyAsync(Bk->out_h, Bk->out_d, Bk->out_elems * sizeof(float), hipMemcpyDeviceToHost, s->stream);
    }
    hipMemcpyAsync(Bk->h_err, s->d_err, sizeof(int), hipMemcpyDeviceToHost, s->stream);  // (the flow program's error bits)
    s->ragged = false; s->solo = false;
    TRY(capture_end(s, &g2[gi], &cg));
  }
  HIP_TRY(hipGraphLaunch(g2[gi], s->stream));
  return VITS_OK;
}

static int device_error_word(int e) {
  if (e & PS_ERR_TIMEOUT) return persist_timed_out();  // first: a timeout invalidates every bit derived from computed data (check_err)
  if (e & 1) return fail(VITS_ERR_ARG, "token id out of range");
  if (e & 2) return fail(VITS_ERR_ARG, "speaker id out of range");
  if (e & 4) return fail(VITS_ERR_ARG, "T_y exceeds frame capacity");
  if (e & REG_ERR_FIT) return fail(VITS_ERR_UNSUPPORTED, "fit_frames: a fit was refused");
  return e ? fail(VITS_ERR_DEVICE, "device error word %d", e) : VITS_OK;
}

static int synth_fast(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t Tx, const float* scales,
                      const int64_t* sid, const vits_synth_opts* opts, const TailReq& req, void** out, int64_t* out_samples,
                      int64_t* out_lengths, int64_t* token_ends) {
  const vits_hparams& hp = m->hp;
  HIP_TRY(hipSetDevice(m->device));
  TailReq q = req;  // (its table: uploaded on the first call at this rate, before any capture)
  if (q.rate) TRY(resample_get(m->device, hp.sampling_rate, q.rate, &q.T));
  if (q.wm.on) TRY(stft_tab_get(m->device, WM_N, &q.wm.T));  // (include/vits_watermark.h: the frame transform's tables, as early)
  const ResampleTab* T = q.T;
  const Rate rt = rate_of(T);
  const NormReq& lq = q.norm;
  const bool pcm = q.pcm;
  const int TxB = (Tx + 7) / 8 * 8;
  const bool forced = opts && opts->forced_durations, solo = q.doc.on || (opts && (opts->flags & VITS_FLAG_SOLO_BATCH));
  ProsodyReq pr;  // (include/vits_prosody.h: checked before anything is launched; at B == 1 item_scales are the call's scalars)
  TRY(prosody_req(opts, lengths, B, Tx, scales, &pr));
  // (declared before the session guard: the call's last stream synchronisation happens before this scope ends)
  InFlight inflight(m->device);
  PersistScope pscope(B == 1 ? m->device : -1, inflight.before);  // a single utterance takes the persistent stages when the device is quiet enough as it starts
  FastFront* F = nullptr;
  TRY(retry_nomem([&] { return front_acquire(m, B, TxB, &F); }, [&] { fronts_evict_all(m); }));
  struct Rel { vits_model* m; FastFront* F; ~Rel() { front_release(m, F); } } rel{m, F};
  const hipStream_t st = F->s->stream;
  if (token_ends && !F->marks_d) {  // the first marks request of this bucket (before any capture)
    const size_t bytes = sizeof(int64_t) * (size_t)B * TxB;
    if (hipMalloc((void**)&F->marks_d, bytes) != hipSuccess || hipHostMalloc((void**)&F->marks_h, bytes) != hipSuccess) {
      if (F->marks_d) hipFree(F->marks_d);
      F->marks_d = nullptr; F->marks_h = nullptr;
      (void)hipGetLastError();
      return fail(VITS_ERR_NOMEM, "speech-mark buffers (%zu bytes)", bytes);
    }
  }
  // ---- inputs -> pinned block
  SynthDev* hv = reinterpret_cast<SynthDev*>(F->io_h);
  hv->rate_L = rt.L; hv->rate_M = rt.M;
  hv->scales[0] = pr.scales[0]; hv->scales[1] = pr.scales[1]; hv->scales[2] = pr.scales[2];
  hv->pcm_scale = q.pcm_scale;
  hv->seed = opts ? opts->seed : 0;
  int64_t* h_len = reinterpret_cast<int64_t*>(F->io_h + F->io_len);
  int64_t* h_sid = reinterpret_cast<int64_t*>(F->io_h + F->io_sid);
  int64_t* h_ids = reinterpret_cast<int64_t*>(F->io_h + F->io_ids);
  int32_t* h_forced = reinterpret_cast<int32_t*>(F->io_h + F->io_forced);
  unsigned long long* h_seeds = reinterpret_cast<unsigned long long*>(F->io_h + F->io_seeds);
  for (int b = 0; b < B; ++b) {
    h_seeds[b] = (opts && opts->item_seeds) ? opts->item_seeds[b] : hv->seed + (uint64_t)b;
    h_len[b] = lengths[b];
    h_sid[b] = sid ? sid[b] : 0;
  }
  pad_rows(h_ids, ids, B, Tx, TxB);
  if (forced) pad_rows(h_forced, opts->forced_durations, B, Tx, TxB);
  if (F->io_bert) pad_rows(reinterpret_cast<float*>(F->io_h + F->io_bert), opts->bert, (size_t)B * hp.bert_dim, Tx, TxB);  // [B, bert_dim, Tx] -> [B, bert_dim, TxB]
  if (pr.regulate) {  // the controls, an absent one as its neutral value: the call's scalars, ones, no pause, no fit
    const vits_prosody* p = pr.p;
    float* h_isc = reinterpret_cast<float*>(F->io_h + F->io_iscales);
    float* h_tls = reinterpret_cast<float*>(F->io_h + F->io_tls);
    int32_t* h_pause = reinterpret_cast<int32_t*>(F->io_h + F->io_pause);
    int32_t* h_fit = reinterpret_cast<int32_t*>(F->io_h + F->io_fit);
    for (int b = 0; b < B; ++b) {
      for (int k = 0; k < 3; ++k) h_isc[b * 3 + k] = pr.per_item_noise ? p->item_scales[(size_t)b * 3 + k] : pr.scales[k];
      h_fit[b] = p->fit_frames ? p->fit_frames[b] : 0;
    }
    if (p->token_length_scale) pad_rows(h_tls, p->token_length_scale, B, Tx, TxB);
    else std::fill(h_tls, h_tls + (size_t)B * TxB, 1.f);
    if (p->token_pause) pad_rows(h_pause, p->token_pause, B, Tx, TxB);
    else std::fill(h_pause, h_pause + (size_t)B * TxB, 0);
  }
  // ---- phase 1 and the one host round trip
  TRY(phase1_launch(F, forced, solo, token_ends != nullptr, pr.regulate));
  HIP_TRY(hipStreamSynchronize(st));
  {
    int e = 0;
    memcpy(&e, F->h_ylen + B, sizeof(int));
    if (e) {
      hipMemsetAsync(F->s->d_err, 0, sizeof(int), st);
      if ((e & REG_ERR_FIT) && !(e & (PS_ERR_TIMEOUT | 7)) && pr.regulate)  // the regulator refused a fit: its ratio block names the item
        return prosody_fit_refused(pr, reinterpret_cast<const float*>(F->io_h + F->io_ratio));
      return device_error_word(e);
    }
  }
  if (pr.p && pr.p->out_fit_ratio)
    for (int b = 0; b < B; ++b) pr.p->out_fit_ratio[b] = pr.regulate ? reinterpret_cast<const float*>(F->io_h + F->io_ratio)[b] : 1.f;
  int64_t Ty = 1;
  for (int b = 0; b < B; ++b) if (F->h_ylen[b] > Ty) Ty = F->h_ylen[b];
  if (opts && opts->max_frames > 0 && Ty > opts->max_frames) return fail(VITS_ERR_ARG, "T_y %lld exceeds max_frames %d", (long long)Ty, opts->max_frames);
  if (Ty > (1 << 24)) return fail(VITS_ERR_ARG, "T_y unreasonably large");
  // frame bucket: multiples of 32 for one utterance; batches round up in steps of 1/8 of the power of two below T_y (64 frames
  // at 512..1023): with free-running durations the longest item of a batch lands on a different multiple of 32 almost every
  // call, and every new bucket is a workspace + a graph capture on the request path.  The padding is not computed (ragged tile
  // maps skip dead tiles); it costs the D2H of the padded rows only.
  int ty_step = 32;
  if (B > 1) { int p2 = 32; while (p2 * 2 <= Ty) p2 *= 2; if (p2 / 8 > ty_step) ty_step = p2 / 8; }
  const int TyB = (int)((Ty + ty_step - 1) / ty_step * ty_step);
  // ---- phase 2
  FastBack* Bk = nullptr;
  // (idle fronts of other buckets and this front's other backs go first)
  TRY(retry_nomem([&] { return back_get(F, TyB, &Bk); }, [&] { fronts_evict_all(m); front_drop_backs(F); }));
  // (sizes in output samples)
  const int64_t S = T ? T->P.n_out(Ty * hp.hop_length) : Ty * hp.hop_length;
  const size_t esz = pcm ? sizeof(int16_t) : sizeof(float);
  // what either branch below ends with, once its work is queued: the buffer the caller gets ...
  auto host_out = [&](size_t n) -> char* {
    char* h = static_cast<char*>(malloc(n ? n : 1));
    if (!h) { hipStreamSynchronize(st); fail(VITS_ERR_NOMEM, "host alloc failed"); }
    return h;
  };
  // ... and the wait, the launch error (`queued`: of the branch's own copies), the flow program's error word, the lengths and the marks
  auto finish = [&](char* h_out, hipError_t queued) -> int {
    hipError_t e = hipStreamSynchronize(st);
    if (queued != hipSuccess) e = queued;
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { free(h_out); return fail(VITS_ERR_DEVICE, "kernel launch failed: %s", hipGetErrorString(e)); }
    if (*Bk->h_err) {
      const int e2 = *Bk->h_err;
      *Bk->h_err = 0;
      hipMemsetAsync(Bk->s->d_err, 0, sizeof(int), st);
      free(h_out);
      return device_error_word(e2);
    }
    *out = h_out;
    *out_samples = S;
    if (out_lengths) for (int b = 0; b < B; ++b) out_lengths[b] = T ? T->P.n_out(F->h_ylen[b] * hp.hop_length) : F->h_ylen[b] * hp.hop_length;
    if (token_ends) for (int b = 0; b < B; ++b) memcpy(token_ends + (size_t)b * Tx, F->marks_h + (size_t)b * TxB, sizeof(int64_t) * Tx);  // (bucket columns dropped)
    return VITS_OK;
  };
  if (q.pitch.on || q.contour.on || q.doc.on || q.wm.on) {
    // include/vits_pitch.h, vits_contour.h, vits_document.h, vits_watermark.h: the float, native-rate form of the graph as it is, then the tail (out_tail.hip.h) as launches
    // behind it on the same stream, in buffers of this call (the graph's own copy of the unshifted float audio to the host is not used)
    std::vector<long long> h_len(B);
    for (int b = 0; b < B; ++b) h_len[b] = F->h_ylen[b] * hp.hop_length;
    TailBufs bufs;
    if (q.doc.on) TRY(doc_prepare(bufs, st, q.doc, h_len.data(), hp.hop_length));  // (the bound is refused, the controls go up, in front of the decoder)
    TRY(phase2_launch(F, Bk, solo, false, nullptr, nullptr, pr.per_item_noise));
    const void* d_out = nullptr;
    const float* d_res = nullptr;
    long long So = 0;
    std::vector<float> res((size_t)B * 4);
    std::vector<int> doc_blk(q.doc.on ? q.doc.blk_ints() : 0), doc_cum(q.doc.token_ends ? (size_t)B * TxB : 0);
    const int rows = q.doc.on ? 1 : B;  // (a document goes on as one item)
    const int rc = tail_run(bufs, Bk->s, st, Bk->out_d, (long long)TyB * hp.hop_length, Bk->s->len_y, hp.hop_length, h_len.data(), B, F->s->cum, TxB, F->s->len_x, q, &d_out, &So, &d_res);
    if (rc != VITS_OK) { hipStreamSynchronize(st); return rc; }
    if (d_res) hipMemcpyAsync(res.data(), d_res, sizeof(float) * 4 * (size_t)rows, hipMemcpyDeviceToHost, st);
    if (q.doc.on) {  // the layout block (and the frame counts behind the marks) come back with the audio; F * hop of the row are the document
      hipMemcpyAsync(doc_blk.data(), q.doc.d_blk, sizeof(int) * doc_blk.size(), hipMemcpyDeviceToHost, st);
      if (q.doc.token_ends) hipMemcpyAsync(doc_cum.data(), F->s->cum, sizeof(int) * doc_cum.size(), hipMemcpyDeviceToHost, st);
      char* h_out = host_out(esz * (size_t)So);
      if (!h_out) return VITS_ERR_NOMEM;
      TRY(finish(h_out, hipMemcpyAsync(h_out, d_out, esz * (size_t)So, hipMemcpyDeviceToHost, st)));
      *out_samples = doc_results(q.doc, doc_blk.data(), doc_cum.data(), TxB, lengths, Tx, hp.hop_length, rt.L, rt.M);
      if (*out_samples < So) memset(h_out + esz * (size_t)*out_samples, 0, esz * (size_t)(So - *out_samples));  // (trim: the row was sized by the bound)
      if (d_res) norm_req_results(lq, res.data(), 1);
      return VITS_OK;
    }
    char* h_out = host_out(esz * (size_t)B * S);
    if (!h_out) return VITS_ERR_NOMEM;
    TRY(finish(h_out, hipMemcpy2DAsync(h_out, esz * (size_t)S, d_out, esz * (size_t)So, esz * (size_t)S, (size_t)B, hipMemcpyDeviceToHost, st)));
    if (d_res) norm_req_results(lq, res.data(), B);
    return VITS_OK;
  }
  // Without a shift a flagged request allocates nothing after the first call of its bucket: the resampler is part of the graph and the
  // last stage runs in buffers the bucket owns (RateOut, LoudWs), so this branch does not go through tail_run's allocator.
  FastBack::RateOut* R = nullptr;
  if (T) TRY(back_rate_get(F, Bk, *T, &R));
  const int64_t stride = R ? R->n_cap : (int64_t)TyB * hp.hop_length;
  const char* src_h = R ? R->y_h : Bk->out_h;
  if (lq.on()) {
    // include/vits_loudness.h: the float form of the graph as it is, then the measurement and the gain behind it on the same stream,
    // from the finished waveform on the device (the graph's own copy of the un-normalised float audio to the host is not used)
    LoudWs** pw = R ? &R->lw : &Bk->lw;
    TRY(loud_ws_ensure(pw, B, stride));  // (the first flagged request of this context allocates, before anything is launched)
    if (lq.lim.on) TRY(lim_ws_ensure(*pw, B, stride));  // (include/vits_limit.h: and its first limited one)
    const LoudWs& W = **pw;
    NormScratch NS;
    norm_ws_layout(lq, W, B, stride, &NS);
    TRY(phase2_launch(F, Bk, solo, false, R, T, pr.per_item_noise));
    const float* x_d = R ? static_cast<const float*>(R->y_d) : Bk->out_d;
    const Items it = items_at(T, Bk->s->len_y, hp.hop_length, stride);
    if (pcm) norm_launch<int16_t>(st, lq, NS, x_d, stride, it, B, static_cast<int16_t*>(W.y_d()), stride, stride, q.pcm_scale, Bk->s);
    else norm_launch<float>(st, lq, NS, x_d, stride, it, B, static_cast<float*>(W.y_d()), stride, stride, 1.f, Bk->s);
    hipMemcpyAsync(W.y_h(), W.y_d(), (size_t)B * stride * esz, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(W.res_h(), W.S.res, sizeof(float) * 4 * (size_t)B, hipMemcpyDeviceToHost, st);
    src_h = W.y_h();
  } else {
    TRY(phase2_launch(F, Bk, solo, pcm, R, T, pr.per_item_noise));
  }
  char* h_out = host_out(esz * (size_t)B * S);
  if (!h_out) return VITS_ERR_NOMEM;
  TRY(finish(h_out, hipSuccess));
  for (int b = 0; b < B; ++b) memcpy(h_out + esz * (size_t)b * S, src_h + esz * (size_t)b * stride, esz * (size_t)S);
  if (lq.on()) norm_req_results(lq, (R ? R->lw : Bk->lw)->res_h(), B);
  return VITS_OK;
}

static int synth_eager(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t Tx, const float* scales,
                       const int64_t* sid, const vits_synth_opts* opts, const TailReq& req, void** out, int64_t* out_samples,
                       int64_t* out_lengths, int64_t* token_ends) {
  const vits_hparams& hp = m->hp;
  TailReq q = req;
  if (q.rate) TRY(resample_get(m->device, hp.sampling_rate, q.rate, &q.T));
  if (q.wm.on) TRY(stft_tab_get(m->device, WM_N, &q.wm.T));  // (include/vits_watermark.h: the frame transform's tables, as early)
  const ResampleTab* T = q.T;
  const Rate rt = rate_of(T);
  std::vector<float> res((size_t)B * 4);  // (the last stage's result rows: declared before the stage, whose end waits for the stream)
  HostStage hs(m);
  std::vector<int64_t> ylen;
  std::vector<int> cum;  // (marks: copied out next to ylen, in acoustic_host's own round trip)
  int64_t Ty = 0;
  float* z = nullptr;
  TRY(acoustic_host(hs, ids, lengths, B, Tx, scales, sid, opts, ylen, Ty, z, (token_ends || q.doc.token_ends) ? &cum : nullptr, q.doc.on));
  if (token_ends)
    for (int b = 0; b < B; ++b) marks_fill_host(cum.data() + (size_t)b * Tx, lengths[b], Tx, hp.hop_length, rt.L, rt.M, token_ends + (size_t)b * Tx);
  vits_session* s = hs.s;
  s->ragged = B > 1;
  s->solo = q.doc.on || (opts && (opts->flags & VITS_FLAG_SOLO_BATCH));
  struct RaggedOff { vits_session* s; ~RaggedOff() { s->ragged = false; s->solo = false; } } ragged_off{s};
  const int64_t S = Ty * hp.hop_length;
  float* d_audio = hs.dev_alloc<float>((size_t)B * S);
  if (!d_audio) return fail(VITS_ERR_NOMEM, "device alloc failed");
  std::vector<long long> h_len(B);
  for (int b = 0; b < B; ++b) h_len[b] = ylen[b] * hp.hop_length;
  std::vector<int> doc_blk(q.doc.on ? q.doc.blk_ints() : 0);
  if (q.doc.on)  // (the bound is refused, the controls go up, in front of the decoder)
    TRY(doc_prepare([&](size_t bytes) { return hs.raw_alloc(bytes); }, s->stream, q.doc, h_len.data(), hp.hop_length));
  run_decoder(s, z, true, B, (int)Ty, d_audio, S, true, !s->solo);
  // the tail (out_tail.hip.h) behind the decoder, in the staging area of this call
  const void* d_src = nullptr;
  const float* d_res = nullptr;
  long long So = 0;  // samples per item as returned
  TRY(tail_run([&](size_t bytes) { return hs.raw_alloc(bytes); }, s, s->stream, d_audio, S, s->len_y, hp.hop_length, h_len.data(), B, s->cum, Tx, s->len_x, q, &d_src, &So, &d_res));
  const int rows = q.doc.on ? 1 : B;  // (a document goes on as one item)
  if (d_res) hipMemcpyAsync(res.data(), d_res, sizeof(float) * 4 * (size_t)rows, hipMemcpyDeviceToHost, s->stream);
  if (q.doc.on) hipMemcpyAsync(doc_blk.data(), q.doc.d_blk, sizeof(int) * doc_blk.size(), hipMemcpyDeviceToHost, s->stream);
  const size_t esz = q.pcm ? sizeof(int16_t) : sizeof(float);
  const size_t out_bytes = esz * (size_t)rows * So;
  void* h_out = malloc(out_bytes ? out_bytes : 1);
  if (!h_out) return fail(VITS_ERR_NOMEM, "host alloc failed");
  hipError_t e = hipMemcpyAsync(h_out, d_src, out_bytes, hipMemcpyDeviceToHost, s->stream);
  int rc = e == hipSuccess ? check_err(s) : fail(VITS_ERR_DEVICE, "D2H failed: %s", hipGetErrorString(e));
  if (rc != VITS_OK) { free(h_out); return rc; }
  if (d_res) norm_req_results(q.norm, res.data(), rows);
  *out = h_out;
  *out_samples = So;
  if (q.doc.on) {
    *out_samples = doc_results(q.doc, doc_blk.data(), cum.data(), Tx, lengths, Tx, hp.hop_length, rt.L, rt.M);
    if (*out_samples < So)  // (trim: the row was sized by the bound)
      memset(static_cast<char*>(h_out) + esz * (size_t)*out_samples, 0, esz * (size_t)(So - *out_samples));
  }
  if (out_lengths) for (int b = 0; b < B; ++b) out_lengths[b] = T ? T->P.n_out(ylen[b] * hp.hop_length) : ylen[b] * hp.hop_length;
  return VITS_OK;
}

static int synth_dispatch(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t Tx, const float* scales,
                          const int64_t* sid, const vits_synth_opts* opts, bool pcm, float pcm_scale, int32_t sample_rate, void** out,
                          int64_t* out_samples, int64_t* out_lengths, int64_t* token_ends = nullptr, const DocReq* doc = nullptr) {
  if (!m || !ids || !lengths || !scales || !out || !out_samples || B <= 0 || Tx <= 0) return fail(VITS_ERR_ARG, "bad argument");
  if (!m->acoustic) return fail(VITS_ERR_UNSUPPORTED, "vocoder-only model: only the decoder stage is available");
  for (int b = 0; b < B; ++b) if (lengths[b] < 0 || lengths[b] > Tx) return fail(VITS_ERR_ARG, "length out of range");
  TailReq q;  // (out_tail.hip.h: the rate, the loudness target, the limiter and the shift, checked before anything is queued)
  const TailFields tf = tail_fields_vits(opts);
  TRY(tail_req(m, tf, sample_rate, pcm, pcm_scale, B, &q));
  TRY(tail_contour_req(m, tf, lengths, B, Tx, &q));
  if (doc) q.doc = *doc;
  static const bool env_off = getenv("VITS_NO_FASTPATH") != nullptr;
  if (m->hp.bert_dim > 0 && (!opts || !opts->bert)) return fail(VITS_ERR_ARG, "this voice is BERT-conditioned: the bert feed [B,%d,T_x] is required", m->hp.bert_dim);
  if (m->hp.bert_dim == 0 && opts && opts->bert) return fail(VITS_ERR_ARG, "the bert feed was given but this voice has no BERT projection (hparams.bert_dim == 0)");
  // (round 5: the `bert` feed of a BERT-conditioned voice is an INPUT like the ids and goes through the graph-replayed path; only
  //  injected noise tensors -- parity tests -- take the eager path)
  bool injected = opts && (opts->noise_dp || opts->noise_prior);
  // a large padded batch of a BERT-conditioned voice: its bert feed ([B, 768, T_x], tens of MB) would be pinned once per shape bucket --
  // such calls keep the exact-size eager path (hipMemcpy from the caller's buffer)
  if (m->hp.bert_dim > 0 && (size_t)B * m->hp.bert_dim * ((Tx + 7) / 8 * 8) * sizeof(float) > ((size_t)8 << 20)) injected = true;
  for (int attempt = 0;; ++attempt) {
    tl_ps_timed_out = false;
    const int rc = (g_fast_path && !env_off && !injected)
                       ? synth_fast(m, ids, lengths, B, Tx, scales, sid, opts, q, out, out_samples, out_lengths, token_ends)
                       : synth_eager(m, ids, lengths, B, Tx, scales, sid, opts, q, out, out_samples, out_lengths, token_ends);
    if (rc == VITS_OK || !tl_ps_timed_out || attempt) return rc;  // a persistent program timed out: once more, on launches
  }
}

int vits_synthesize(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t Tx, const float* scales,
                    const int64_t* sid, const vits_synth_opts* opts, float** out_audio, int64_t* out_samples, int64_t* out_lengths) {
  return synth_dispatch(m, ids, lengths, B, Tx, scales, sid, opts, false, 1.f, 0, reinterpret_cast<void**>(out_audio), out_samples, out_lengths);
}

int vits_synthesize_rate(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t Tx, const float* scales,
                         const int64_t* sid, const vits_synth_opts* opts, int32_t sample_rate, float** out_audio, int64_t* out_samples,
                         int64_t* out_lengths) {
  if (sample_rate < 0) return fail(VITS_ERR_UNSUPPORTED, "sample_rate %d: must be positive, or 0 for the voice's own rate", sample_rate);
  return synth_dispatch(m, ids, lengths, B, Tx, scales, sid, opts, false, 1.f, sample_rate, reinterpret_cast<void**>(out_audio), out_samples, out_lengths);
}

int vits_synthesize_pcm16(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t Tx, const float* scales,
                          const int64_t* sid, const vits_synth_opts* opts, float pcm_scale, int16_t** out_pcm, int64_t* out_samples,
                          int64_t* out_lengths) {
  return synth_dispatch(m, ids, lengths, B, Tx, scales, sid, opts, true, pcm_scale, 0, reinterpret_cast<void**>(out_pcm), out_samples, out_lengths);
}

int vits_synthesize_pcm16_rate(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t Tx, const float* scales,
                               const int64_t* sid, const vits_synth_opts* opts, float pcm_scale, int32_t sample_rate, int16_t** out_pcm,
                               int64_t* out_samples, int64_t* out_lengths) {
  if (sample_rate < 0) return fail(VITS_ERR_UNSUPPORTED, "sample_rate %d: must be positive, or 0 for the voice's own rate", sample_rate);
  return synth_dispatch(m, ids, lengths, B, Tx, scales, sid, opts, true, pcm_scale, sample_rate, reinterpret_cast<void**>(out_pcm), out_samples, out_lengths);
}

// ---- include/vits_marks.h
int vits_synthesize_marks(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t Tx, const float* scales,
                          const int64_t* sid, const vits_synth_opts* opts, int32_t sample_rate, float** out_audio, int64_t* out_samples,
                          int64_t* out_lengths, int64_t* token_ends) {
  if (!token_ends) return fail(VITS_ERR_ARG, "token_ends must not be NULL (vits_synthesize_rate is the call without marks)");
  if (sample_rate < 0) return fail(VITS_ERR_UNSUPPORTED, "sample_rate %d: must be positive, or 0 for the voice's own rate", sample_rate);
  return synth_dispatch(m, ids, lengths, B, Tx, scales, sid, opts, false, 1.f, sample_rate, reinterpret_cast<void**>(out_audio), out_samples, out_lengths,
                        token_ends);
}

int vits_synthesize_pcm16_marks(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t Tx, const float* scales,
                                const int64_t* sid, const vits_synth_opts* opts, float pcm_scale, int32_t sample_rate, int16_t** out_pcm,
                                int64_t* out_samples, int64_t* out_lengths, int64_t* token_ends) {
  if (!token_ends) return fail(VITS_ERR_ARG, "token_ends must not be NULL (vits_synthesize_pcm16_rate is the call without marks)");
  if (sample_rate < 0) return fail(VITS_ERR_UNSUPPORTED, "sample_rate %d: must be positive, or 0 for the voice's own rate", sample_rate);
  return synth_dispatch(m, ids, lengths, B, Tx, scales, sid, opts, true, pcm_scale, sample_rate, reinterpret_cast<void**>(out_pcm), out_samples, out_lengths,
                        token_ends);
}

// ---- include/vits_document.h
static int synth_document(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t Tx, const float* scales, const int64_t* sid,
                          const vits_synth_opts* opts, const vits_document* doc, bool pcm, float pcm_scale, int32_t sample_rate, void** out,
                          int64_t* out_samples, int64_t* token_ends) {
  if (!m) return fail(VITS_ERR_ARG, "bad argument");
  if (sample_rate < 0) return fail(VITS_ERR_UNSUPPORTED, "sample_rate %d: must be positive, or 0 for the voice's own rate", sample_rate);
  DocReq dq;  // (refused before anything is launched)
  TRY(doc_req(doc, B, m->hp.hop_length, &dq));
  dq.token_ends = token_ends;
  return synth_dispatch(m, ids, lengths, B, Tx, scales, sid, opts, pcm, pcm_scale, sample_rate, out, out_samples, nullptr, nullptr, &dq);
}

int vits_synthesize_document(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t Tx, const float* scales,
                             const int64_t* sid, const vits_synth_opts* opts, const vits_document* doc, int32_t sample_rate, float** out_audio,
                             int64_t* out_samples, int64_t* token_ends) {
  return synth_document(m, ids, lengths, B, Tx, scales, sid, opts, doc, false, 1.f, sample_rate, reinterpret_cast<void**>(out_audio), out_samples,
                        token_ends);
}

int vits_synthesize_document_pcm16(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t Tx, const float* scales,
                                   const int64_t* sid, const vits_synth_opts* opts, const vits_document* doc, float pcm_scale, int32_t sample_rate,
                                   int16_t** out_pcm, int64_t* out_samples, int64_t* token_ends) {
  return synth_document(m, ids, lengths, B, Tx, scales, sid, opts, doc, true, pcm_scale, sample_rate, reinterpret_cast<void**>(out_pcm), out_samples,
                        token_ends);
}

void vits_free_pcm16(int16_t* p) { free(p); }
void vits_debug_fast_path(int on) { g_fast_path = on; }

void vits_free_output(float* p) { free(p); }

