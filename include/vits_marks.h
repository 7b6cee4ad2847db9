/*
 * vits_marks.h — speech marks: when every input token is spoken, on the time axis of the audio the call returns.  What subtitles,
 * lip-sync, highlighting and barge-in positions are built from (a serving engine is expected to say when each word is spoken; the
 * reference's modules compute the alignment -- SynthesizerTrn.infer's `attn`, training/vits2/models.py:1694,1704; MatchaTTS.synthesise's
 * "attn", matcha_tts.py:167,206 -- and its exported graphs drop it).
 *
 * An extension of the product library like include/vits_resample.h: the CPU oracle has no counterpart and these entry points are
 * checked against an integer restatement of the definition below (tests/marks_ref.py).  Same status codes and vits_last_error as
 * include/vits_mi355.h; all are re-entrant.
 *
 * Definition.  hop = hparams.hop_length; cum[b, t] = the inclusive cumulative FRAME count of item b over its own tokens 0..t, of the
 * frame counts the engine actually used: w_ceil or the forced durations for the VITS family (models.py:1689-1694), w_round for the
 * multistream family (matcha_tts.py:152).  n_out(x) = ceil(x * L / M) is the resampler's length rule (vits_resample.h; L = M = 1 at
 * the voice's own rate), in exact 64-bit integer arithmetic: (x*L + M - 1) / M.
 *     token_end[b, t] = n_out(cum[b, t] * hop)            0 <= t < lengths[b]
 *     token_end[b, t] = token_end[b, lengths[b] - 1]      lengths[b] <= t < T_x      (0 when lengths[b] == 0)
 * Token t occupies the output samples [token_end[b, t-1], token_end[b, t]), token_end[b, -1] = 0.  A token of zero frames has an empty
 * span; token_end is non-decreasing; token_end[b, lengths[b] - 1] == out_lengths[b] whenever the item has at least one frame.
 *
 * The one exception is the reference's clamp_min(y_lengths, 1) (models.py:1691): an item whose durations are all zero still yields ONE
 * frame of audio (out_lengths[b] = n_out(hop)) while every token_end of it is 0 -- that frame belongs to no token.
 *
 * The denoiser, the [-1, 1] clamp and the int16 conversion move no samples: marks are identical with and without them.
 *
 * Cost.  On the graph-replayed path a marks request replays its own phase-1 graph variants: today's graph plus one launch of
 * token_ends_kernel (one thread per token) and one copy of the [B, T_x] block to pinned memory, both in front of the copy of the frame
 * counts -- the host reads the marks after the one synchronisation the call performs anyway.  A call without marks replays exactly
 * the graphs it replayed before.  Every other path (eager, streams, multistream) has the frame counts on the host and fills the marks
 * there.
 */
#ifndef VITS_MARKS_H
#define VITS_MARKS_H

#include "vits_resample.h"
#include "stts_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vits_synthesize_rate / vits_synthesize_pcm16_rate plus token_ends: caller-owned int64 [B, T_x], must not be NULL (VITS_ERR_ARG).
 * sample_rate 0 = the voice's own rate.  Every option of vits_synth_opts is accepted.  Audio, *out_samples and out_lengths are exactly
 * what the call without marks returns. */
int vits_synthesize_marks(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t T_x, const float* scales,
                          const int64_t* sid, const vits_synth_opts* opts, int32_t sample_rate,
                          float** out_audio, int64_t* out_samples, int64_t* out_lengths, int64_t* token_ends);
int vits_synthesize_pcm16_marks(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t T_x, const float* scales,
                                const int64_t* sid, const vits_synth_opts* opts, float pcm_scale, int32_t sample_rate,
                                int16_t** out_pcm, int64_t* out_samples, int64_t* out_lengths, int64_t* token_ends);

/* The marks of a stream, valid from the open to the close, in the stream's own output samples (vits_stream_open_rate: at that rate).
 * *n_tokens = the utterance's T_x; token_ends (capacity `cap` entries) receives them, VITS_ERR_ARG when cap is too small; NULL with
 * cap 0 asks for the count only.  A latent stream (vits_stream_open_latent*) has no tokens: *n_tokens = 0 and token_ends is not
 * touched.  A stream opened by stts_stream_open returns the marks that call recorded. */
int vits_stream_marks(vits_stream* s, int64_t* token_ends, int32_t cap, int32_t* n_tokens);

/* stts_synthesize / stts_synthesize_batch plus token_ends (int64 [T_x] / [B, T_x], must not be NULL) and sample_rate (0 = the voice's
 * own): marks, audio, *out_samples and out_lengths are at that rate (the finished waveform goes through vits_op_resample; the mel is
 * untouched).  The multistream durations are on the host in every path, so the marks are filled there. */
int stts_synthesize_marks(stts_model* m, const int64_t* ids, int32_t T_x, const float* scales, int64_t sid, const float* bert,
                          const float* phone_duration_extra, const stts_synth_opts* opts, int32_t sample_rate, float** out_audio,
                          int64_t* out_samples, float** out_mel, int64_t* out_frames, int64_t* token_ends);
int stts_synthesize_batch_marks(stts_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t T_x, const float* scales,
                                const int64_t* sid, const float* bert, const float* phone_duration_extra, const stts_synth_opts* opts,
                                int32_t sample_rate, float** out_audio, int64_t* out_samples, int64_t* out_lengths, int64_t* token_ends);

#ifdef __cplusplus
}
#endif
#endif /* VITS_MARKS_H */
