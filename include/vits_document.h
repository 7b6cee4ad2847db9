/*
 * vits_document.h — documents: the B items of one batch call joined into ONE piece of audio on the device, in front of the
 * resampler, the loudness stage, the limiter and the int16 conversion.  What a caller with a paragraph, a page or a dialogue needs:
 * sentences are synthesised as the sentences the voice was trained on (a batch: per-item speakers, scales, prosody and contours), and
 * the whole-output stages see the whole output.
 *
 * An extension of the product library like include/vits_marks.h and vits_prosody.h: the CPU oracle has no counterpart and the entry
 * points are checked against a NumPy restatement of the definition below (tests/document_ref.py).  Same status codes and
 * vits_last_error as include/vits_mi355.h; all are re-entrant.  These entry points live in this header only.
 *
 * Inputs.  A document is B >= 1 segments, the items of one VITS_FLAG_SOLO_BATCH call (item b is what a lone call with seed + b gives;
 * the flag is implied).  hop = hparams.hop_length.  Item b behind the per-item stages (decode, clamp, denoise, pitch / contour /
 * intonation: they run as they do for a batch) has len_b >= 1 frames, x_b[0 .. len_b*hop).
 *
 * Controls (vits_document).  lead_frames >= 0; gap_frames[b] >= 0 frames of silence behind segment b (the last entry is the trailing
 * silence; NULL = no gaps); fade_samples in [0, hop/2]; trim_db: 0 = off, otherwise a negative finite dBFS value; trim_keep_frames >= 0.
 * Anything else is VITS_ERR_ARG naming segment and value, before anything is launched.
 *
 * Trim (only when on).  thr = (float)pow(10, trim_db / 20), computed in double on the host.  peak_b[f] = max |x_b[f*hop .. (f+1)*hop)|.
 * The maximum starts from 0 and leaves a NaN sample out (fmaxf), so a frame of NaNs has peak 0 and is never loud; the join itself copies
 * NaN like any other sample.  A frame is loud iff peak_b[f] > thr: strict, exact in fp32.  With f0 / f1 the first / last loud frame:
 *     lo_b = max(f0 - keep, 0)        hi_b = min(f1 + 1 + keep, len_b)
 * No loud frame: lo_b = hi_b = 0 (the segment is empty and its gap stays).  Off: lo_b = 0, hi_b = len_b.  n_b = hi_b - lo_b.
 *
 * Layout (integers, in frames).
 *     start_0 = lead_frames      start_{b+1} = start_b + n_b + gap_frames[b]      F = start_{B-1} + n_{B-1} + gap_frames[B-1]
 * Refused (VITS_ERR_ARG) before the decoder runs when the untrimmed bound (lead + sum(len_b + gap_b)) * hop reaches 2^31.
 *
 * Join.  d[start_b*hop + i] = x_b[lo_b*hop + i] * h(i) * t(i) for i < n_b*hop; everything else in d[0 .. F*hop) is exactly 0.
 *     w[j] = (float)(0.5 - 0.5*cos(pi*(j + 0.5)/fade))    a host-made table, j < fade (double arithmetic, rounded once)
 *     h(i) = w[i] for i < fade;  t(i) = w[n_b*hop - 1 - i] for the last `fade` samples;  both 1 elsewhere.
 * fade <= hop/2, so h and t never meet; each is one fp32 multiply, and where the factor is 1 nothing is multiplied: fade = 0 is a copy,
 * bit for bit.
 *
 * Behind the join the joined signal is ONE item of F frames: it goes through the rest of the chain as a B = 1 item does (resample L / M,
 * normalise and / or limit, int16).  Where the join is the last stage of an int16 call it converts itself, with the arithmetic of the
 * plain int16 call (v*scale, *32767, clamp to +-32767, truncate).  F = 0 is VITS_OK with *out_samples = 0.
 *
 * Marks, with n_out of include/vits_marks.h (cum: the inclusive cumulative frame counts of the batch):
 *     seg_start[b] = n_out(start_b*hop)      seg_end[b] = n_out((start_b + n_b)*hop)
 *     token_end[b, t] = n_out((start_b + clamp(cum[b, t] - lo_b, 0, n_b)) * hop)
 * with the padding rule beyond lengths[b] of vits_marks.h (the last valid entry repeats; 0 for an item without tokens).
 *
 * Cost.  The layout is made on the device (doc_edges_kernel with trim, doc_layout_kernel, doc_join_kernel): there is no host
 * synchronisation between the decoder and the call's final copies, the buffers are sized by the untrimmed bound, and the layout block
 * comes back with the final copies.  A call that is not a document launches exactly what it launched before.
 */
#ifndef VITS_DOCUMENT_H
#define VITS_DOCUMENT_H

#include "vits_marks.h"
#include "vits_prosody.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vits_document {
  int32_t        lead_frames;
  const int32_t* gap_frames;        /* [B] or NULL (no gaps) */
  int32_t        fade_samples;
  float          trim_db;           /* 0 = off */
  int32_t        trim_keep_frames;
  int64_t*       out_seg_start;     /* [B] or NULL, output samples */
  int64_t*       out_seg_end;       /* [B] or NULL */
  int32_t*       out_trim;          /* [B,2] or NULL: lo_b, hi_b in frames */
} vits_document;

/* One SOLO batch call, joined.  *out_audio is one row of *out_samples samples (vits_free_output); token_ends int64 [B, T_x] or NULL.
 * Every option of vits_synth_opts is honoured (a prosody fit_frames fits a segment); a loudness / limiter result is ONE value
 * (out_loudness[0], ...), of the whole document.  sample_rate 0 = the voice's own. */
int vits_synthesize_document(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t T_x, const float* scales,
                             const int64_t* sid, const vits_synth_opts* opts, const vits_document* doc, int32_t sample_rate,
                             float** out_audio, int64_t* out_samples, int64_t* token_ends);
int vits_synthesize_document_pcm16(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t T_x, const float* scales,
                                   const int64_t* sid, const vits_synth_opts* opts, const vits_document* doc, float pcm_scale,
                                   int32_t sample_rate, int16_t** out_pcm, int64_t* out_samples, int64_t* token_ends);

/* stts_synthesize_batch_marks's parameters plus doc, for the multistream family: the items of the batch call, joined.  That family's
 * tail crosses the host through the doors' kernels, so the document does too, in the same place: behind pitch, in front of the rate.
 * token_ends may be NULL.  Needs an attached vocoder. */
int stts_synthesize_document(stts_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t T_x, const float* scales,
                             const int64_t* sid, const float* bert, const float* phone_duration_extra, const stts_synth_opts* opts,
                             const vits_document* doc, int32_t sample_rate, float** out_audio, int64_t* out_samples, int64_t* token_ends);

/* The parity door, on host buffers, float: x [B, N], len_frames int64 [B] (1 <= len_frames[b], len_frames[b]*hop <= N); y has room for
 * y_cap samples, of which [0, *out_frames * hop) are written and the rest is left as it was (VITS_ERR_ARG when the untrimmed bound
 * exceeds y_cap); start int32 [B] and trim int32 [B,2] (lo, hi) may be NULL.  doc->out_* are not used. */
int vits_op_document_join(int device, const float* x, const int64_t* len_frames, int32_t B, int64_t N, int32_t hop, const vits_document* doc,
                          float* y, int64_t y_cap, int64_t* out_frames, int32_t* start, int32_t* trim);

#ifdef __cplusplus
}
#endif
#endif /* VITS_DOCUMENT_H */
