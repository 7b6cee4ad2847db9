// out_tail.hip.h -- the output tail: what a synthesize call asks of the stages behind the decoder (TailReq, built by tail_req from the
// plain fields behind the option flags), and the one runner of the chain  pitch / contour / intonation -> resample -> watermark -> normalise / limit -> int16
// on the device (tail_run).  The kernels and their launches are those of resample / loudness / limit / pitch / contour / watermark.hip.h; this file
// only orders them.
// Part of the ONE translation unit engine.hip (included there, behind limit.hip.h, pitch.hip.h, contour.hip.h and watermark.hip.h; not a standalone header).
#pragma once

// ---- the request ----------------------------------------------------------------------------------------------------------
// The flag bits and the name of an API family: the two families number the same four flags differently.
struct TailFamily { const char* name; uint32_t loudness, limit, pitch, formant, contour, intonation, watermark, watermark_payload; };
static const TailFamily TAIL_VITS = {"VITS", VITS_FLAG_LOUDNESS, VITS_FLAG_LIMIT, VITS_FLAG_PITCH, VITS_FLAG_PITCH_FORMANT, VITS_FLAG_CONTOUR,
                                     VITS_FLAG_INTONATION, VITS_FLAG_WATERMARK, VITS_FLAG_WATERMARK_PAYLOAD};
static const TailFamily TAIL_STTS = {"STTS", STTS_FLAG_LOUDNESS, STTS_FLAG_LIMIT, STTS_FLAG_PITCH, STTS_FLAG_PITCH_FORMANT, STTS_FLAG_CONTOUR,
                                     STTS_FLAG_INTONATION, STTS_FLAG_WATERMARK, STTS_FLAG_WATERMARK_PAYLOAD};

// The values behind the flags of a call, flat.  A group is meaningful only where its `on` is set (`formant` is the bare flag bit).
struct TailFields {
  const char* family = "VITS";
  bool loud_on = false;
  int loud_mode = 0;
  float loud_target = 0.f, loud_ceiling = 0.f;
  float *out_loudness = nullptr, *out_gain = nullptr;
  bool lim_on = false;
  int lim_mode = 0;
  float lim_ceiling = 0.f, lim_lookahead_ms = 0.f, lim_release_ms = 0.f, lim_gain = 0.f;
  float* out_reduction = nullptr;
  bool pitch_on = false, formant = false;
  float semitones = 0.f;
  bool contour_on = false;
  const vits_contour* contour = nullptr;
  bool inton_on = false;
  float pitch_range = 1.f;
  bool wm_on = false;
  uint32_t wm_key = 0;
  float wm_depth_db = 0.f;
  bool wm_payload_on = false;  // (include/vits_watermark_payload.h; the bare flag bit: without wm_on it is refused by tail_req)
  uint32_t wm_payload = 0;
  const uint32_t* wm_payloads = nullptr;  // null or one per item of the call
};

// The only two places that cast down the `base` chain of the extended option structs: a struct's own fields are read under its flag
// alone, so a caller who sets no flag may pass the plain struct (include/vits_loudness.h, vits_pitch.h, vits_limit.h).
template <typename Pitch, typename Limit, typename Contour, typename Inton, typename Wm, typename WmP, typename Loud, typename Opts>
static TailFields tail_fields(const TailFamily& fam, const Opts* opts, const Loud* lo) {
  TailFields f;
  f.family = fam.name;
  if (!opts) return f;
  const uint32_t fl = opts->flags;
  f.loud_on = (fl & fam.loudness) != 0; f.lim_on = (fl & fam.limit) != 0; f.pitch_on = (fl & fam.pitch) != 0; f.formant = (fl & fam.formant) != 0;
  if (f.loud_on) {
    f.loud_mode = lo->loudness_mode; f.loud_target = lo->loudness_target; f.loud_ceiling = lo->loudness_ceiling;
    f.out_loudness = lo->out_loudness; f.out_gain = lo->out_gain;
  }
  if (f.lim_on) {
    const Limit* mo = reinterpret_cast<const Limit*>(opts);
    f.lim_mode = mo->limit_mode; f.lim_ceiling = mo->limit_ceiling; f.lim_lookahead_ms = mo->limit_lookahead_ms;
    f.lim_release_ms = mo->limit_release_ms; f.lim_gain = mo->limit_gain; f.out_reduction = mo->out_reduction;
  }
  if (f.pitch_on) f.semitones = reinterpret_cast<const Pitch*>(opts)->pitch_semitones;
  f.contour_on = (fl & fam.contour) != 0;
  if (f.contour_on) f.contour = reinterpret_cast<const Contour*>(opts)->contour;
  f.inton_on = (fl & fam.intonation) != 0;
  if (f.inton_on) f.pitch_range = reinterpret_cast<const Inton*>(opts)->pitch_range;
  f.wm_on = (fl & fam.watermark) != 0;
  if (f.wm_on) {
    const Wm* wo = reinterpret_cast<const Wm*>(opts);
    f.wm_key = wo->watermark_key; f.wm_depth_db = wo->watermark_depth_db;
  }
  f.wm_payload_on = (fl & fam.watermark_payload) != 0;
  if (f.wm_payload_on) {
    const WmP* po = reinterpret_cast<const WmP*>(opts);
    f.wm_payload = po->watermark_payload; f.wm_payloads = po->watermark_payloads;
  }
  return f;
}
static TailFields tail_fields_vits(const vits_synth_opts* opts) {  // (the loudness fields are the plain struct's own)
  static_assert(offsetof(vits_synth_opts_limit, base) == 0 && offsetof(vits_synth_opts_pitch, base) == 0 && offsetof(vits_synth_opts_prosody, base) == 0 &&
                    offsetof(vits_synth_opts_contour, base) == 0 && offsetof(vits_synth_opts_intonation, base) == 0 &&
                    offsetof(vits_synth_opts_watermark, base) == 0 && offsetof(vits_synth_opts_watermark_payload, base) == 0,
                "the extended options begin with the plain ones");
  return tail_fields<vits_synth_opts_pitch, vits_synth_opts_limit, vits_synth_opts_contour, vits_synth_opts_intonation, vits_synth_opts_watermark,
                     vits_synth_opts_watermark_payload>(
      TAIL_VITS, opts, opts);
}
static TailFields tail_fields_stts(const stts_synth_opts* opts) {
  static_assert(offsetof(stts_synth_opts_limit, base) == 0 && offsetof(stts_synth_opts_pitch, base) == 0 && offsetof(stts_synth_opts_loudness, base) == 0 &&
                    offsetof(stts_synth_opts_contour, base) == 0 && offsetof(stts_synth_opts_intonation, base) == 0 &&
                    offsetof(stts_synth_opts_watermark, base) == 0 && offsetof(stts_synth_opts_watermark_payload, base) == 0,
                "the extended options begin with the plain ones");
  return tail_fields<stts_synth_opts_pitch, stts_synth_opts_limit, stts_synth_opts_contour, stts_synth_opts_intonation, stts_synth_opts_watermark,
                     stts_synth_opts_watermark_payload>(
      TAIL_STTS, opts, reinterpret_cast<const stts_synth_opts_loudness*>(opts));
}

// the formant bit modifies a pitch request: alone it is refused, before any work is queued
static int tail_formant_check(bool formant, bool pitch, const char* family) {
  if (formant && !pitch)
    return fail(VITS_ERR_ARG, "%s_FLAG_PITCH_FORMANT without %s_FLAG_PITCH: the flag modifies a pitch request (include/vits_pitch.h)", family, family);
  return VITS_OK;
}

// a stream has no tail: each of its stages needs the whole utterance
static int tail_refuse_stream(uint32_t flags, const TailFamily& fam) {
  if (flags & fam.loudness)
    return fail(VITS_ERR_UNSUPPORTED, "%s_FLAG_LOUDNESS on a stream: an integrated-loudness or peak target needs the whole utterance before the first chunk", fam.name);
  if (flags & fam.limit)
    return fail(VITS_ERR_UNSUPPORTED, "%s_FLAG_LIMIT on a stream: the limiter's look-ahead and its loudness passes need the whole utterance before the first chunk", fam.name);
  TRY(tail_formant_check((flags & fam.formant) != 0, (flags & fam.pitch) != 0, fam.name));
  if (flags & fam.pitch)
    return fail(VITS_ERR_UNSUPPORTED, "%s_FLAG_PITCH on a stream: the phase recursion needs the frames before a chunk, and its state is not carried across chunks", fam.name);
  if (flags & fam.contour)
    return fail(VITS_ERR_UNSUPPORTED, "%s_FLAG_CONTOUR on a stream: the position recurrence and the phase recursion need the whole utterance before the first chunk", fam.name);
  if (flags & fam.intonation)
    return fail(VITS_ERR_UNSUPPORTED, "%s_FLAG_INTONATION on a stream: the median of the F0 track needs the whole utterance before the first chunk", fam.name);
  if (flags & fam.watermark_payload)
    return fail(VITS_ERR_UNSUPPORTED, "%s_FLAG_WATERMARK_PAYLOAD on a stream: the mark is a stage of the output tail, and a stream has none (include/vits_watermark_payload.h)", fam.name);
  if (flags & fam.watermark)
    return fail(VITS_ERR_UNSUPPORTED, "%s_FLAG_WATERMARK on a stream: the mark is a stage of the output tail, and a stream has none (include/vits_watermark.h)", fam.name);
  return VITS_OK;
}

// Everything a call asks of the stages behind the decoder.  T: the table of `rate` on the device, set by the callers that resample there
// (resample_get: uploaded on first use, before any capture); rate 0: the vocoder's own.
struct TailReq {
  PitchReq pitch;
  ContourReq contour;  // (include/vits_contour.h; where it is on, the call's own shift is part of its tokens and `pitch` is off)
  IntonReq inton;      // (include/vits_intonation.h; where it is on, `contour` is on too and carries the tokens, neutral without a contour)
  const IntonReq* inton_arg() const { return inton.on ? &inton : nullptr; }  // what contour_run takes
  const ResampleTab* T = nullptr;
  int rate = 0;
  WmReq wm;  // (include/vits_watermark.h: behind the rate and the join, in front of `norm`)
  NormReq norm;
  bool pcm = false;
  float pcm_scale = 1.f;
  DocReq doc;  // (include/vits_document.h; empty: the call is not a document)
};

// Checked before anything is synthesised, so a refusal costs nothing: the rate, the loudness target, the limiter, the shift.  `vocoder`
// is null for a multistream model without one: its entry point has resolved the rate (stts_marks_arg) and any stage asked for is refused.
// B: the items of the call (what a per-item payload array is read with).
static int tail_req(const vits_model* vocoder, const TailFields& f, int32_t sample_rate, bool pcm, float pcm_scale, int B, TailReq* out) {
  *out = TailReq();
  out->pcm = pcm; out->pcm_scale = pcm_scale;
  if (vocoder) TRY(resample_rate_arg(vocoder, sample_rate, &out->rate));
  else out->rate = sample_rate;
  if ((f.loud_on || f.lim_on) && !vocoder) return fail(VITS_ERR_ARG, "no vocoder attached");
  const int rate = out->rate ? out->rate : vocoder ? vocoder->hp.sampling_rate : 0;  // (what the last stage measures is the audio as returned)
  TRY(loud_req(f.loud_on, f.loud_mode, f.loud_target, f.loud_ceiling, f.out_loudness, f.out_gain, rate, &out->norm.loud));
  TRY(lim_req(f.lim_on, f.lim_mode, f.lim_ceiling, f.lim_lookahead_ms, f.lim_release_ms, f.lim_gain, f.out_reduction, rate,
              out->norm.loud.on ? f.loud_ceiling : 0.f, &out->norm));
  TRY(tail_formant_check(f.formant, f.pitch_on, f.family));
  if (f.wm_on && !vocoder) return fail(VITS_ERR_ARG, "no vocoder attached");
  if (f.wm_payload_on && !f.wm_on)
    return fail(VITS_ERR_ARG, "%s_FLAG_WATERMARK_PAYLOAD without %s_FLAG_WATERMARK: the flag modifies a watermark request (include/vits_watermark_payload.h)",
                f.family, f.family);
  TRY(wm_req(f.wm_on, f.wm_key, f.wm_depth_db, &out->wm, f.wm_payload_on, f.wm_payload, f.wm_payloads, B));
  if (!f.pitch_on) return VITS_OK;
  if (!vocoder) return fail(VITS_ERR_ARG, "no vocoder attached");
  return pitch_req(vocoder, f.semitones, f.formant, &out->pitch);
}

// The contour of a call (include/vits_contour.h), behind tail_req, which knows nothing of the tokens: refused or planned before anything is
// synthesised.  A contour whose every token is neutral leaves the request as tail_req made it (case (a): the call as it was, the
// pitch stage included); otherwise VITS_FLAG_PITCH's semitones are added to every token and the pitch stage itself does not run.
static int tail_contour_req(const vits_model* vocoder, const TailFields& f, const int64_t* tok_lengths, int B, int Tx, TailReq* out) {
  // include/vits_intonation.h: refused or planned here too, as its frame table is the contour's; r_m == 1000 is the call without the flag
  int r_m = 1000;
  if (f.inton_on) {
    TRY(inton_range_arg(f.pitch_range, &r_m));
    if (f.formant)
      return fail(VITS_ERR_UNSUPPORTED, "%s_FLAG_INTONATION with %s_FLAG_PITCH_FORMANT: the envelope pre-warp assumes one ratio per call (include/vits_intonation.h)",
                  f.family, f.family);
  }
  const bool inton = r_m != 1000;
  if (!f.contour_on && !inton) return VITS_OK;
  if (f.contour_on && !f.contour) return fail(VITS_ERR_ARG, "%s_FLAG_CONTOUR with a NULL contour pointer (include/vits_contour.h)", f.family);
  if (f.contour_on && f.formant)
    return fail(VITS_ERR_UNSUPPORTED, "%s_FLAG_CONTOUR with %s_FLAG_PITCH_FORMANT: the envelope pre-warp assumes one ratio per call (include/vits_contour.h)",
                f.family, f.family);
  if (!vocoder) return fail(VITS_ERR_ARG, "no vocoder attached");
  const float* ts = f.contour_on ? f.contour->token_semitones : nullptr;
  const float* tg = f.contour_on ? f.contour->token_gain_db : nullptr;
  TRY(contour_plan(ts, tg, 0.f, tok_lengths, B, Tx, &out->contour));
  if (!out->contour.on && !inton) return VITS_OK;
  if (f.pitch_on) TRY(contour_plan(ts, tg, f.semitones, tok_lengths, B, Tx, &out->contour));
  out->contour.on = true;
  out->pitch = PitchReq();
  if (vocoder->hp.hop_length % PT_H)
    return fail(VITS_ERR_UNSUPPORTED, "%s: the vocoder's hop_length %d is not a multiple of the pitch stage's hop %d", f.contour_on ? "contour" : "intonation",
                vocoder->hp.hop_length, PT_H);
  if (inton) {
    TRY(inton_rate_arg(vocoder->hp.sampling_rate));
    out->inton.on = true;
    out->inton.r_m = r_m;
    out->inton.rate = vocoder->hp.sampling_rate;
  }
  return VITS_OK;
}

// ---- the runner -----------------------------------------------------------------------------------------------------------
// device buffers owned by one call (the allocator of a tail_run that has no arena to draw from), freed with it
using TailBufs = DevBufs;  // op_door.hip.h

// The tail of a vits_synthesize* call, as launches on `stream` from the float native-rate waveform x [B, S] on the device (item b is
// len_y[b] * hop samples, h_len[b] on the host; its tokens' inclusive frame counts cum [B][cum_bstride] and their number tok_len [B] on the
// device, read by a contoured call only): pitch or contour, resample, watermark, normalise and / or limit; the last stage that runs converts to int16
// where q.pcm.  *d_out is [B, *So] of float or int16 (x itself where nothing is asked), *d_res the [B, 4] result rows of the last
// stage on the device (null without one), for the caller's own copies to the host.  A document (q.doc, prepared by doc_prepare) is joined
// behind the contour stage and goes on as ONE item: *d_out is then [1, *So], the joined length F in frames is q.doc.d_blk[0] on the device
// and *d_res has one row.  alloc(bytes) -> void* is the caller's: buffers
// that outlive the launches queued here.  s: the session the launches are counted under (ProfScope).
template <typename Alloc>
static int tail_run(Alloc&& alloc, vits_session* s, hipStream_t stream, const float* x, long long S, const int* len_y, int hop, const long long* h_len,
                    int B, const int* d_cum, long long cum_bstride, const int* d_toklen, const TailReq& q, const void** d_out, long long* So_out,
                    const float** d_res) {
  const ResampleTab* T = q.T;
  const size_t esz = q.pcm ? sizeof(int16_t) : sizeof(float);
  *So_out = T ? T->P.n_out(S) : S;
  *d_res = nullptr;
  Items in{len_y, hop};  // the items at the vocoder's rate
  if (q.pitch.on) {
    float* d_p = static_cast<float*>(alloc(sizeof(float) * (size_t)B * S));
    if (!d_p) return fail(VITS_ERR_NOMEM, "device alloc failed");
    TRY(pitch_run(s->m->device, stream, x, S, S, in, h_len, B, q.pitch.P, q.pitch.Q, q.pitch.formant, d_p, S, S, nullptr, 0));
    x = d_p;
  }
  if (q.contour.on) {  // in the pitch stage's place; the last stage of a call that neither resamples nor normalises
    const bool cp = q.pcm && !T && !q.norm.on() && !q.doc.on && !q.wm.on;
    void* d_c = alloc((cp ? sizeof(int16_t) : sizeof(float)) * (size_t)B * S);
    if (!d_c) return fail(VITS_ERR_NOMEM, "device alloc failed");
    TRY(contour_run(s->m->device, stream, x, S, h_len, B, q.contour, d_cum, cum_bstride, d_toklen, hop, d_c, cp, q.pcm_scale, S, S, nullptr, 0, nullptr, 0,
                    q.inton_arg()));
    if (cp) { *d_out = d_c; return VITS_OK; }
    x = static_cast<const float*>(d_c);
  }
  if (q.doc.on) {  // the items become one: the last stage of a call that neither resamples nor normalises
    const bool jp = q.pcm && !T && !q.norm.on() && !q.wm.on;
    const long long Sd = q.doc.bound * hop;
    void* d_j = alloc((jp ? sizeof(int16_t) : sizeof(float)) * (size_t)Sd);
    if (!d_j) return fail(VITS_ERR_NOMEM, "device alloc failed");
    doc_join_launch(s, stream, x, S, len_y, hop, q.doc, d_j, jp, q.pcm_scale);
    B = 1; S = Sd; len_y = q.doc.d_blk;
    in = Items{len_y, hop};
    *So_out = T ? T->P.n_out(S) : S;
    if (jp) { *d_out = d_j; return VITS_OK; }
    x = static_cast<const float*>(d_j);
  }
  const long long So = *So_out;
  const Items ret = items_at(T, len_y, hop, So);  // the items as they are returned
  *d_out = x;
  bool at_rate = !T;  // x is at the rate it is returned at
  if (q.wm.on) {  // marked at the rate it is returned at (the resampler in front writes float); the last stage of a call that does not normalise
    if (T) {
      float* d_y = static_cast<float*>(alloc(sizeof(float) * (size_t)B * So));
      if (!d_y) return fail(VITS_ERR_NOMEM, "device alloc failed");
      ProfScope ps(s, "out.resample", 2.0 * B * So * T->P.taps, "resample_kernel<float>");
      resample_launch<float>(stream, *T, x, S, 0, S, in, B, d_y, So, 0, So, 1.f, nullptr);
      x = d_y;
      at_rate = true;
    }
    const bool wp = q.pcm && !q.norm.on();
    const size_t sc = wm_scratch_elems(So);
    float* d_scr = static_cast<float*>(alloc(sizeof(float) * (size_t)B * sc));
    void* d_w = alloc((wp ? sizeof(int16_t) : sizeof(float)) * (size_t)B * So);
    if (!d_scr || !d_w) return fail(VITS_ERR_NOMEM, "device alloc failed");
    uint32_t* d_words = nullptr;
    if (q.wm.payload) {  // (include/vits_watermark_payload.h: the words of THIS call go up in front of its launch; B is 1 behind a join)
      d_words = static_cast<uint32_t*>(alloc(sizeof(uint32_t) * (size_t)B));
      if (!d_words) return fail(VITS_ERR_NOMEM, "device alloc failed");
      HIP_TRY(hipMemcpyAsync(d_words, q.wm.host_words(q.doc.on), sizeof(uint32_t) * (size_t)B, hipMemcpyHostToDevice, stream));
    }
    {
      ProfScope ps(s, "out.watermark", 0, wp ? "wm_frames_kernel + wm_ola_kernel<int16>" : "wm_frames_kernel + wm_ola_kernel<float>");
      if (wp) wm_launch<int16_t>(stream, q.wm, x, So, ret, B, d_scr, (long long)sc, static_cast<int16_t*>(d_w), So, So, q.pcm_scale, d_words);
      else wm_launch<float>(stream, q.wm, x, So, ret, B, d_scr, (long long)sc, static_cast<float*>(d_w), So, So, 1.f, d_words);
    }
    *d_out = d_w;
    if (!q.norm.on()) return VITS_OK;
    x = static_cast<const float*>(d_w);
  }
  if (q.norm.on()) {  // the float waveform at the rate it is returned at, measured, then the gain (and the conversion)
    if (!at_rate) {
      float* d_y = static_cast<float*>(alloc(sizeof(float) * (size_t)B * So));
      if (!d_y) return fail(VITS_ERR_NOMEM, "device alloc failed");
      ProfScope ps(s, "out.resample", 2.0 * B * So * T->P.taps, "resample_kernel<float>");
      resample_launch<float>(stream, *T, x, S, 0, S, in, B, d_y, So, 0, So, 1.f, nullptr);
      x = d_y;
    }
    char* d_scr = static_cast<char*>(alloc(norm_scratch_bytes(q.norm, B, So)));
    void* d_n = alloc(esz * (size_t)B * So);
    if (!d_scr || !d_n) return fail(VITS_ERR_NOMEM, "device alloc failed");
    NormScratch NS;
    norm_scratch_layout(q.norm, B, So, d_scr, &NS);
    if (q.pcm) norm_launch<int16_t>(stream, q.norm, NS, x, So, ret, B, static_cast<int16_t*>(d_n), So, So, q.pcm_scale, s);
    else norm_launch<float>(stream, q.norm, NS, x, So, ret, B, static_cast<float*>(d_n), So, So, 1.f, s);
    *d_res = NS.LS.res;
    *d_out = d_n;
  } else if (T) {  // item b from its own [0, len) of x; at int16 in place of pcm16_kernel
    void* d_y = alloc(esz * (size_t)B * So);
    if (!d_y) return fail(VITS_ERR_NOMEM, "device alloc failed");
    ProfScope ps(s, "out.resample", 2.0 * B * So * T->P.taps, q.pcm ? "resample_kernel<int16>" : "resample_kernel<float>");
    if (q.pcm) resample_launch<int16_t>(stream, *T, x, S, 0, S, in, B, static_cast<int16_t*>(d_y), So, 0, So, q.pcm_scale, nullptr);
    else resample_launch<float>(stream, *T, x, S, 0, S, in, B, static_cast<float*>(d_y), So, 0, So, 1.f, nullptr);
    *d_out = d_y;
  } else if (q.pcm) {
    int16_t* d_pcm = static_cast<int16_t*>(alloc(sizeof(int16_t) * (size_t)B * S));
    if (!d_pcm) return fail(VITS_ERR_NOMEM, "device alloc failed");
    ProfScope ps(s, "out.pcm16", 0, "pcm16_kernel");
    hipLaunchKernelGGL(pcm16_kernel, dim3(cdiv((int)S, 256), B), dim3(256), 0, stream, x, S, d_pcm, S, S, q.pcm_scale, (const SynthDev*)nullptr);
    *d_out = d_pcm;
  }
  return VITS_OK;
}
