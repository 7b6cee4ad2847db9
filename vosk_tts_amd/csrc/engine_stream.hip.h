// engine_stream.hip.h -- streaming synthesis (vits_stream_*): first chunk alone, then double-buffered eight-chunk windows.
// Part of the ONE translation unit engine.hip (included there, in order; not a standalone header): split out in round 6 so that the
// planner / launch selection / stages / host paths can be read on their own.
#pragma once
// ---- streaming synthesis (BASELINE configs[4]; the server's `stream AudioChunk`, tts_service.proto:46-54)
// The flow has global attention, so the acoustic half runs once over the whole utterance; the decoder is purely
// convolutional with a receptive field < 25 frames, so it is run on fixed-width frame windows
// [lo - halo, hi + halo) and only the samples of [lo, hi) are emitted -- identical to the one-shot decode.  Every
// window has the same width W = chunk + 2*halo (clamped to the utterance at both ends, where the true zero padding
// applies), so ONE captured hipGraph of the decoder is replayed per chunk; the next chunk is decoded while the
// caller consumes the current one.
struct vits_stream {
  vits_model* m = nullptr;
  HostStage* hs = nullptr;          // acoustic session + temporaries; z lives in its workspace
  const float* z = nullptr;
  int Ty = 0, chunk = 0, W = 0, halo = VITS_RAGGED_HALO;  // halo is set from the model's receptive field at open
  int pos = 0;                      // first frame not yet handed to the caller
  // The first chunk gets its own narrow window (time to first audio); after it ONE wide window of kmax chunks + halo is decoded
  // per slot: a single 192-frame decode is latency-bound (0.6 ms per chunk) and pays the 2 x 32-frame halo per 128 frames, a
  // wide window pays it once per kmax chunks and runs the one-shot's kernels.  Two audio slots: while the chunks of one window
  // are copied out on the session's copy stream, the next window is decoded into the other slot on the compute stream.
  struct Win { int lo = -1, hi = -1, start = -1, width = 0; float* aud = nullptr; hipEvent_t done = nullptr; };
  Win win[2];
  int kmax = 8, WK = 0;
  bool clamp = false;               // audio clamped to [-1, 1] (the StableTTS export, onnx/export.py:28-31)
  float *d_win = nullptr, *h_pin = nullptr;
  // another output rate (include/vits_resample.h): every emitted chunk is resampled from its window's audio slot into d_rs on the copy
  // stream, then copied out.  The windows carry ceil(half_width_in / hop) more halo frames, so the filter reads exactly decoded samples.
  const ResampleTab* rs = nullptr;
  float* d_rs = nullptr;
  long long rs_cap = 0;             // outputs one chunk can have: ceil(chunk * hop * L / M) + 1
  // the vocoder-bias denoiser (include/vits_denoise.h): every emitted chunk is denoised from its window's audio slot into d_dn on the
  // copy stream (two launches), then copied out.  The windows carry ceil(filter_length / hop) more halo frames.
  const StftTab* dn = nullptr;
  const float* dn_bias = nullptr;
  float dn_strength = 0.f;
  float *d_dn = nullptr, *d_dn_scr = nullptr;
  size_t dn_scr_elems = 0;
  hipEvent_t ev = nullptr;
  std::vector<int64_t> marks;       // token ends in output samples (include/vits_marks.h); empty: a latent stream, which has no tokens
  int find(int lo) const { for (int i = 0; i < 2; ++i) if (lo >= win[i].lo && lo < win[i].hi) return i; return -1; }
};

// enqueues the decode of the window that starts with chunk `lo` into slot `slot`
static int stream_launch(vits_stream* st, int lo, int slot) {
  vits_session* s = st->hs->s;
  const int I = st->m->hp.inter_channels;
  const bool wide = lo > 0 && st->WK > st->W;
  const int width = wide ? st->WK : st->W;
  int start = lo - st->halo;
  if (start > st->Ty - width) start = st->Ty - width;  // at the end the window is shifted inward: the true zero padding applies
  if (start < 0) start = 0;
  vits_stream::Win& w = st->win[slot];
  w.lo = lo;
  w.hi = wide ? lo + st->kmax * st->chunk : lo + st->chunk;
  w.start = start;
  w.width = width;
  hipLaunchKernelGGL(window_copy_kernel, dim3(cdiv(width, 256), I), dim3(256), 0, s->stream, st->z, (long long)st->Ty, start, width, st->d_win);
  const long long S = (long long)width * st->m->hp.hop_length;
  run_decoder(s, st->d_win, false, 1, width, w.aud, S);
  if (st->clamp) hipLaunchKernelGGL(clamp_kernel, dim3(cdiv((int)S, 256)), dim3(256), 0, s->stream, w.aud, S);
  HIP_TRY(hipEventRecord(w.done, s->stream));
  return VITS_OK;
}

void vits_stream_close(vits_stream* st) {
  if (!st) return;
  hipSetDevice(st->m->device);
  if (st->hs && st->hs->s) hipStreamSynchronize(st->hs->s->stream);
  if (st->hs && st->hs->s && st->hs->s->copy_stream) hipStreamSynchronize(st->hs->s->copy_stream);
  for (auto& w : st->win) if (w.done) hipEventDestroy(w.done);
  if (st->ev) hipEventDestroy(st->ev);
  if (st->h_pin) hipHostFree(st->h_pin);
  delete st->hs;  // frees d_win/d_aud and returns the session to the pool
  delete st;
}

// second half of every stream open: window geometry, buffers, first chunk in flight.  Closes the stream on failure.
static int stream_start(vits_stream* st, const float* z, int Ty, int chunk_frames, vits_stream** out, int64_t* total_samples) {
  vits_model* m = st->m;
  int rc = VITS_OK;
  const vits_hparams& hp = m->hp;
  st->z = z;
  st->Ty = (int)Ty;
  st->halo = m->rag_halo;
  size_t pin_elems = (size_t)chunk_frames * hp.hop_length;
  if (st->rs) {
    st->halo += cdiv(st->rs->P.half, hp.hop_length);
    st->rs_cap = st->rs->P.n_out((long long)chunk_frames * hp.hop_length) + 1;
    pin_elems = (size_t)st->rs_cap;
    st->d_rs = st->hs->dev_alloc<float>((size_t)st->rs_cap);
    if (!st->d_rs) { vits_stream_close(st); return fail(VITS_ERR_NOMEM, "stream buffers"); }
  }
  if (st->dn && (long long)Ty * hp.hop_length < st->dn->n / 2 + 1) st->dn = nullptr;  // too short for the reflection: streamed undenoised
  if (st->dn) {
    st->halo += cdiv(st->dn->n, hp.hop_length);
    st->dn_scr_elems = denoise_scratch_elems(st->dn->n, (long long)chunk_frames * hp.hop_length);
    st->d_dn = st->hs->dev_alloc<float>(pin_elems);
    st->d_dn_scr = st->hs->dev_alloc<float>(st->dn_scr_elems);
    if (!st->d_dn || !st->d_dn_scr) { vits_stream_close(st); return fail(VITS_ERR_NOMEM, "stream buffers"); }
  }
  st->chunk = chunk_frames;
  st->W = chunk_frames + 2 * st->halo;
  if (st->W > st->Ty) st->W = st->Ty;
  st->WK = st->kmax * chunk_frames + 2 * st->halo;  // the wide window of the chunks after the first
  if (st->WK > st->Ty) st->WK = st->Ty;
  st->d_win = st->hs->dev_alloc<float>((size_t)hp.inter_channels * st->WK);
  for (auto& w : st->win) w.aud = st->hs->dev_alloc<float>((size_t)st->WK * hp.hop_length);
  if (!st->hs->s->copy_stream && hipStreamCreateWithFlags(&st->hs->s->copy_stream, hipStreamNonBlocking) != hipSuccess) {
    vits_stream_close(st);
    return fail(VITS_ERR_DEVICE, "stream: hipStreamCreate failed");
  }
  if (!st->d_win || !st->win[0].aud || !st->win[1].aud ||
      hipEventCreateWithFlags(&st->win[0].done, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&st->win[1].done, hipEventDisableTiming) != hipSuccess || hipHostMalloc((void**)&st->h_pin, sizeof(float) * pin_elems) != hipSuccess ||
      hipEventCreateWithFlags(&st->ev, hipEventDisableTiming) != hipSuccess) {
    vits_stream_close(st);
    return fail(VITS_ERR_NOMEM, "stream buffers");
  }
  // the acoustic half is done with the persistent stages: wait for them and hand the token back (the stream object lives on)
  hipStreamSynchronize(st->hs->s->stream);
  st->hs->pscope.release();
  rc = stream_launch(st, 0, 0);  // first chunk is already decoding when the caller asks for it
  if (rc != VITS_OK) { vits_stream_close(st); return rc; }
  if (total_samples) *total_samples = st->rs ? st->rs->P.n_out((long long)Ty * hp.hop_length) : (int64_t)Ty * hp.hop_length;
  *out = st;
  return VITS_OK;
}


// the table of a stream at `sample_rate` (null: the native rate)
static int stream_rate(vits_model* m, int32_t sample_rate, const ResampleTab** T) {
  *T = nullptr;
  if (sample_rate < 0) return fail(VITS_ERR_UNSUPPORTED, "sample_rate %d: must be positive, or 0 for the voice's own rate", sample_rate);
  int rate = 0;
  TRY(resample_rate_arg(m, sample_rate, &rate));
  if (!rate) return VITS_OK;
  HIP_TRY(hipSetDevice(m->device));
  return resample_get(m->device, m->hp.sampling_rate, rate, T);
}

int vits_stream_open(vits_model* m, const int64_t* ids, int32_t Tx, const float* scales, int64_t sid, const vits_synth_opts* opts,
                     int32_t chunk_frames, vits_stream** out, int64_t* total_samples) {
  return vits_stream_open_rate(m, ids, Tx, scales, sid, opts, chunk_frames, 0, out, total_samples);
}

int vits_stream_open_rate(vits_model* m, const int64_t* ids, int32_t Tx, const float* scales, int64_t sid, const vits_synth_opts* opts,
                          int32_t chunk_frames, int32_t sample_rate, vits_stream** out, int64_t* total_samples) {
  if (!m || !ids || !scales || !out || Tx <= 0 || chunk_frames <= 0) return fail(VITS_ERR_ARG, "bad argument");
  if (opts) TRY(tail_refuse_stream(opts->flags, TAIL_VITS));
  const ResampleTab* T = nullptr;
  TRY(stream_rate(m, sample_rate, &T));
  for (int attempt = 0;; ++attempt) {
    vits_stream* st = new vits_stream();
    st->m = m;
    st->rs = T;
    st->hs = new HostStage(m);
    std::vector<int64_t> ylen;
    std::vector<int> cum;
    int64_t Ty = 0, len = Tx;
    float* z = nullptr;
    tl_ps_timed_out = false;
    const int rc = acoustic_host(*st->hs, ids, &len, 1, Tx, scales, &sid, opts, ylen, Ty, z, &cum);
    if (rc == VITS_OK) {
      st->marks.resize(Tx);
      const Rate rt = rate_of(T);
      marks_fill_host(cum.data(), Tx, Tx, m->hp.hop_length, rt.L, rt.M, st->marks.data());
      return stream_start(st, z, (int)Ty, chunk_frames, out, total_samples);
    }
    vits_stream_close(st);
    if (!tl_ps_timed_out || attempt) return rc;  // a persistent program timed out: once more, on launches
  }
}

// Streams the decoder over a latent the caller already holds (host, [inter_channels, T_y] row-major): the vocoder half of a
// two-model voice (StableTTS mel -> vocoder, vosk_tts/synth.py:113-126) or a z produced elsewhere.  flags bit 0: clamp to [-1, 1].
int vits_stream_open_latent(vits_model* m, const float* z, int32_t Ty, int32_t chunk_frames, uint32_t flags, vits_stream** out,
                            int64_t* total_samples) {
  return vits_stream_open_latent_rate(m, z, Ty, chunk_frames, flags, 0, out, total_samples);
}

// the latent opens' common body: a stream over the device copy of z, with the resampler's table (null: native rate) or the denoiser's
// tables and bias (dn null: none) behind every chunk
static int stream_open_latent(vits_model* m, const float* z, int32_t Ty, int32_t chunk_frames, uint32_t flags, const ResampleTab* rs,
                              const StftTab* dn, const float* dn_bias, float dn_strength, vits_stream** out, int64_t* total_samples) {
  vits_stream* st = new vits_stream();
  st->m = m;
  st->rs = rs;
  st->dn = dn;
  st->dn_bias = dn_bias;
  st->dn_strength = dn_strength;
  st->hs = new HostStage(m);
  st->clamp = (flags & 1u) != 0;
  int rc = begin_stage(*st->hs, 1, 1, Ty, 0);
  if (rc != VITS_OK) { vits_stream_close(st); return rc; }
  const float* d_z = st->hs->to_dev(z, (size_t)m->hp.inter_channels * Ty);
  if (!d_z) { vits_stream_close(st); return fail(VITS_ERR_NOMEM, "device alloc failed"); }
  return stream_start(st, d_z, Ty, chunk_frames, out, total_samples);
}

int vits_stream_open_latent_rate(vits_model* m, const float* z, int32_t Ty, int32_t chunk_frames, uint32_t flags, int32_t sample_rate,
                                 vits_stream** out, int64_t* total_samples) {
  if (!m || !z || !out || Ty <= 0 || chunk_frames <= 0) return fail(VITS_ERR_ARG, "bad argument");
  if (Ty > (1 << 18)) return fail(VITS_ERR_ARG, "T_y unreasonably large");
  const ResampleTab* T = nullptr;
  TRY(stream_rate(m, sample_rate, &T));
  return stream_open_latent(m, z, Ty, chunk_frames, flags, T, nullptr, nullptr, 0.f, out, total_samples);
}

int vits_stream_open_latent_denoise(vits_model* m, const float* z, int32_t Ty, int32_t chunk_frames, uint32_t flags, float strength,
                                    int32_t filter_length, vits_stream** out, int64_t* total_samples) {
  if (!m || !z || !out || Ty <= 0 || chunk_frames <= 0) return fail(VITS_ERR_ARG, "bad argument");
  if (Ty > (1 << 18)) return fail(VITS_ERR_ARG, "T_y unreasonably large");
  const StftTab* T = nullptr;
  const float* d_bias = nullptr;
  TRY(denoise_prepare(m, strength, filter_length, &T, &d_bias));
  return stream_open_latent(m, z, Ty, chunk_frames, flags, nullptr, T, d_bias, strength, out, total_samples);
}

int vits_stream_marks(vits_stream* st, int64_t* token_ends, int32_t cap, int32_t* n_tokens) {
  if (!st || !n_tokens || cap < 0 || (!token_ends && cap > 0)) return fail(VITS_ERR_ARG, "bad argument");
  *n_tokens = (int32_t)st->marks.size();
  if (st->marks.empty() || (!token_ends && cap == 0)) return VITS_OK;  // (NULL with capacity 0 asks for the count only)
  if (cap < *n_tokens) return fail(VITS_ERR_ARG, "token_ends capacity %d < %d tokens", cap, *n_tokens);
  memcpy(token_ends, st->marks.data(), sizeof(int64_t) * st->marks.size());
  return VITS_OK;
}

int vits_stream_next(vits_stream* st, float* audio, int64_t capacity, int64_t* n_samples) {
  if (!st || !audio || !n_samples) return fail(VITS_ERR_ARG, "bad argument");
  *n_samples = 0;
  if (st->pos >= st->Ty) return VITS_OK;  // end of stream
  HIP_TRY(hipSetDevice(st->m->device));
  vits_session* s = st->hs->s;
  const int hop = st->m->hp.hop_length;
  const int lo = st->pos, hi = lo + st->chunk < st->Ty ? lo + st->chunk : st->Ty;
  // at another rate the chunk that covers input samples [a, b) is the outputs ceil(a L / M) <= n < ceil(b L / M)
  const int64_t n_first = st->rs ? st->rs->P.n_out((long long)lo * hop) : 0;
  const int64_t n = st->rs ? st->rs->P.n_out((long long)hi * hop) - n_first : (int64_t)(hi - lo) * hop;
  if (capacity < n) return fail(VITS_ERR_ARG, "chunk capacity %lld < %lld samples", (long long)capacity, (long long)n);
  int slot = st->find(lo);
  if (slot < 0) { slot = 0; TRY(stream_launch(st, lo, slot)); }  // only the first call: later windows are decoded ahead
  const vits_stream::Win& w = st->win[slot];
  HIP_TRY(hipStreamWaitEvent(s->copy_stream, w.done, 0));
  if (st->rs) {
    // the window's slot holds input samples [w.start * hop, (w.start + width) * hop); beyond the utterance's end the filter sees zeros
    resample_launch<float>(s->copy_stream, *st->rs, w.aud, 0, (long long)w.start * hop, (long long)w.width * hop, Items{nullptr, (long long)st->Ty * hop}, 1, st->d_rs, 0,
                           n_first, n, 1.f, nullptr);
    HIP_TRY(hipMemcpyAsync(st->h_pin, st->d_rs, sizeof(float) * n, hipMemcpyDeviceToHost, s->copy_stream));
  } else if (st->dn) {
    // outputs [lo * hop, hi * hop) of the utterance's transform: its frames read the slot, which holds samples [w.start * hop, ...)
    denoise_launch(s->copy_stream, *st->dn, w.aud, 0, (long long)w.start * hop, (long long)w.width * hop, Items{nullptr, (long long)st->Ty * hop}, 1, st->dn_bias,
                   st->dn_strength, st->d_dn_scr, (long long)st->dn_scr_elems, st->d_dn, 0, (long long)lo * hop, n);
    HIP_TRY(hipMemcpyAsync(st->h_pin, st->d_dn, sizeof(float) * n, hipMemcpyDeviceToHost, s->copy_stream));
  } else {
    HIP_TRY(hipMemcpyAsync(st->h_pin, w.aud + (size_t)(lo - w.start) * hop, sizeof(float) * n, hipMemcpyDeviceToHost, s->copy_stream));
  }
  HIP_TRY(hipEventRecord(st->ev, s->copy_stream));
  st->pos = hi;
  // decode ahead into the other slot: every chunk of the window it held was handed over (and waited for) before this call
  if (w.hi < st->Ty && st->find(w.hi) < 0) TRY(stream_launch(st, w.hi, slot ^ 1));
  HIP_TRY(hipEventSynchronize(st->ev));
  memcpy(audio, st->h_pin, sizeof(float) * n);
  *n_samples = n;
  return VITS_OK;
}

