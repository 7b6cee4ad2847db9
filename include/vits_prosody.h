/*
 * vits_prosody.h — prosody controls of the VITS family: per-item scales, per-token rates, pauses and "speak this in N frames".
 *
 * The reference feeds three scalars per call, scales = [noise_scale, length_scale, noise_scale_w] (training/vits2/onnx_export.py:62-64):
 * length_scale is one multiply in the length regulator (models.py:1689), noise_scale one in the prior sample (models.py:1700) and
 * noise_scale_w one in the stochastic duration predictor's z (models.py:96).  None of the three needs to be per call, and the regulator
 * has every number it needs to land an utterance on a frame count in one pass.  The multistream family keeps its own pause markup
 * (phone_duration_extra, vosk_tts/synth.py:361-454, matcha_tts.py:147-152); this header is the VITS family's counterpart.
 *
 * An extension of the product library like include/vits_marks.h: the CPU oracle has no counterpart and the entry points are checked
 * against a NumPy restatement of the definition below (tests/prosody_ref.py).  Same status codes and vits_last_error as
 * include/vits_mi355.h.
 *
 * Definition.  Item b, token t < lengths[b].  `scales` is the call's float[3].  Every control array is optional.
 *   scales per item   ns_b, ls_b, nsw_b = item_scales[b, 0..2] when item_scales is given, else scales[0..2].  ls_b replaces length_scale
 *                     (models.py:1689), ns_b noise_scale (:1700), nsw_b noise_scale_w (models.py:96; ignored by the deterministic
 *                     predictor, as scales[2] is).  The Philox streams are untouched.
 *   base duration     free-running: w_t = expf(logw_t) * ls_b, then w_t = w_t * token_length_scale[b, t] when that array is given (fp32,
 *                     in this order: an array of ones gives the uncontrolled bits); d0_t = max((int)ceilf(w_t), 0).
 *                     With forced_durations: d0_t = max(forced[b, t], 0).  token_length_scale with forced durations is VITS_ERR_ARG.
 *   pauses            token_pause[b, t] >= 0 frames are appended to token t's own span: they carry that token's m_p / logs_p exactly as
 *                     if its duration had been longer.
 *   without a fit     d_t = d0_t + pause_t.
 *   with a fit        F_b = fit_frames[b] > 0 (0: the item is not fitted).  u_t = (double)w_t free-running (before the ceil),
 *                     u_t = (double)d0_t with forced durations; U = sum u_t, P = sum pause_t, s = (F_b - P) / U;
 *                     c_t = rint(s * sum_{j<=t} u_j) in double precision, round-half-even, c_{-1} = 0; d_t = c_t - c_{t-1} + pause_t.
 *                     The item then has exactly F_b frames.  fit_ratio[b] = s (1 for an item that is not fitted).
 *                     VITS_ERR_UNSUPPORTED when F_b <= P, U == 0 or s outside [0.25, 4]; the message names the item, F_b, P and s.
 *                     A target above max_frames or the frame capacity is the VITS_ERR_ARG it is without a fit.
 * Everything behind d_t is unchanged: the cumulative sums, y_length = max(sum d, 1), the expansion as a gather, the speech marks.
 *
 * Refused before anything is launched (VITS_ERR_ARG, naming item, token and value): a token_length_scale that is not finite or outside
 * [0, 16], a negative pause, a negative fit_frames, an item scale that is not finite or is negative.
 *
 * Cost.  A call without VITS_FLAG_PROSODY launches and replays exactly what it did before.  A controlled call runs regulate_ctl_kernel
 * where the uncontrolled one runs durations_kernel, and replays graph variants of its own.  A single utterance whose controls reach past
 * scalars (token_length_scale, token_pause, fit_frames) runs the text side as launches, not as the single-utterance program;
 * item_scales alone at B == 1 is folded into the call's scalars and takes the uncontrolled path.
 */
#ifndef VITS_PROSODY_H
#define VITS_PROSODY_H

#include "vits_limit.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vits_prosody {
  const float*   item_scales;         /* [B,3] or NULL */
  const float*   token_length_scale;  /* [B,T_x] or NULL */
  const int32_t* token_pause;         /* [B,T_x] frames or NULL */
  const int32_t* fit_frames;          /* [B] or NULL */
  float*         out_fit_ratio;       /* [B] or NULL */
} vits_prosody;

/* vits_synth_opts.flags: the call is controlled as defined above.  vits_synth_opts and the structs that extend it keep their layouts
 * (their mirrors are pinned to them, as include/vits_pitch.h and vits_limit.h found); a caller that sets the flag passes the extended
 * struct below through the same `const vits_synth_opts*` parameter (&o.base.base.base), and `prosody` is read only when the flag is set.
 * The loudness, pitch and limiter fields inside are still read only under their own flags.  The flag with a NULL `prosody` is
 * VITS_ERR_ARG.  Honoured by vits_synthesize*, their *_rate and *_marks forms and vits_stream_open* (total_samples and
 * vits_stream_marks reflect the controls). */
#define VITS_FLAG_PROSODY 32

typedef struct vits_synth_opts_prosody {
  vits_synth_opts_limit base;
  const vits_prosody* prosody;
} vits_synth_opts_prosody;

#define VITS_PROSODY_MAX_TOKEN_SCALE 16.0f
#define VITS_PROSODY_MIN_FIT_RATIO 0.25
#define VITS_PROSODY_MAX_FIT_RATIO 4.0

/* The controlled length regulator alone, on host buffers, without a model: logw float [B,T_x] (or NULL with `forced` int32 [B,T_x]),
 * lengths int64 [B], p NULL or the controls (p->out_fit_ratio is not used: fit_ratio is).  Outputs: durations and cum int32 [B,T_x]
 * (cum inclusive; both 0 / constant beyond lengths[b]), y_lengths int64 [B], fit_ratio float [B] or NULL. */
int vits_op_regulate(int device, const float* logw, const int32_t* forced, const int64_t* lengths, int32_t B, int32_t T_x,
                     float length_scale, const vits_prosody* p, int32_t* durations, int32_t* cum, int64_t* y_lengths, float* fit_ratio);

#ifdef __cplusplus
}
#endif
#endif /* VITS_PROSODY_H */
