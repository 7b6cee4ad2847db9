/*
 * vits_contour.h — per-token pitch and volume contours: every token of an utterance raised or lowered by its own number of semitones
 * and decibels, at unchanged duration, on the device behind the decoder.  include/vits_pitch.h shifts a whole utterance by one ratio;
 * here the ratio follows the tokens, so the vocoder's time map is a position recurrence and the resampler that undoes it warps.
 *
 * An extension of the product library: the reference has no counterpart, so these entry points are checked against a float64
 * restatement of the definition below (tests/contour_ref.py, the authority).  Same status codes and vits_last_error as
 * include/vits_mi355.h; all are re-entrant.
 *
 * Inputs.  Item b, token t < tok_lengths[b]: s_t = token_semitones[b, t] (NULL: zeros; under VITS_FLAG_PITCH pitch_semitones is added
 * to every token), v_t = token_gain_db[b, t] (NULL: zeros), the inclusive cumulative frame counts cum[b, t] of include/vits_marks.h
 * (frames of `hop` samples), and the native-rate waveform x[0 .. len).
 *   Host, per token, in double:  P_t = lround(1000 * 2^(s_t / 12)) (the rule of vits_pitch_plan), g_t = (float) 10^(v_t / 20).  The
 *   device is handed P_t and g_t and never evaluates exp2 or pow for them.
 *   Accepted: |s_t| <= VITS_PITCH_MAX_SEMITONES (the sum, under VITS_FLAG_PITCH), VITS_CONTOUR_MIN_DB <= v_t <= VITS_CONTOUR_MAX_DB;
 *   anything else, NaN included, is VITS_ERR_ARG naming item, token and value, before anything is launched.
 *
 * Frame tracks.  n = VITS_PITCH_FRAME = 1024, H = n / 4 = 256, F = 1 + floor(len / H) rows f (for len >= n/2 + 1 this is F_a of
 * include/vits_pitch.h).  tok(f) is the first token t < tok_lengths[b] with cum[t] * hop > min(f H, len - 1), i.e. the token whose span
 * [cum[t-1] hop, cum[t] hop) contains that sample; where there is none (all durations zero, or a waveform longer than its tokens
 * cover) the row has P = 1000, g = 1.  R = VITS_CONTOUR_RAMP = 4, K = 2 R + 1:
 *     Sigma_f = sum_{j = -R .. R} P_tok(clamp(f + j, 0, F - 1))                          (an integer in [500 K, 2000 K])
 *     gbar_f  = fp32( (sum_{j = -R .. R} (double) g_tok(clamp(f + j, 0, F - 1))) / K )   (summed in double in ascending j, one rounding)
 *     gbar_F  = gbar_{F-1}
 * so a token boundary is a ramp of K frames (about 100 ms at 22.05 kHz), never a step.
 *
 * Positions.  Signed 64-bit integers in units of 2^-24 analysis frames; the same on the host, in NumPy and on the device.
 *     inc_f = (2^24 * 1000 * K) / Sigma_f   (integer division; 2^23 <= inc_f <= 2^25)
 *     a_0 = 0, i_t = a_t >> 24, a_{t+1} = a_t + inc_{min(i_t, F_a - 1)}
 *     F_s = the number of t with a_t < (F_a + 1) << 24; F_s <= 2 (F_a + 1) because every step is at least half a frame.  The table of an
 *     item is a_0 .. a_{F_s}.
 *     alpha_t = (float)(a_t & (2^24 - 1)) * 2^-24   (exact in fp32)
 *
 * Vocoder.  Steps 1 to 4 of include/vits_pitch.h word for word, with this i_t, alpha_t and F_s in place of floor(t Q / P),
 * (t Q mod P) / P and ceil((F_a + 1) P / Q): u[0 .. N_u), N_u = H (F_s - 1).  Arithmetic as there, with one exception: the device forms
 * the transform of step 1 in double and rounds mag_f[k] to fp32 and theta_f[k] to its 32 bits once.  The recursion of step 3 adds
 * the phase error of a bin twice a step, a contour takes up to two steps per analysis frame and its alpha_t carries no rounding, so
 * the fp32 transform's error was what set the distance of u from the float64 restatement.
 *
 * Warp.  For output sample n < len: A = n << 16; t = the largest index with a_t <= A (t <= F_s - 1, as a_{F_s} >= (F_a + 1) << 24 > A);
 *     d = a_{t+1} - a_t; tau_n = H * (t + (double)(A - a_t) / (double) d); s_n = min(1, d * 2^-24) (= min(1, 1 / rho_n), rho_n = 2^24 / d);
 *     v[n] = sum_k u[k] h_{s_n}(tau_n - k) over 0 <= k < N_u, ceil(tau_n - Z / s_n) <= k <= floor(tau_n + Z / s_n), the bounds formed
 *     in double, in ascending k with fp32 accumulation; v[n] = 0 where tau_n >= N_u.
 *   That last case never happens for a length that is a multiple of H: then F_a = len / H + 1, a_{F_s} >= (F_a + 1) << 24 and the last
 *   step is at most 2 frames (P >= 500), so a_{F_s - 1} >= (len / H) << 24 > A for every n < len: t <= F_s - 2 and tau_n < N_u.
 *   Synthesis lengths are multiples of the vocoder's hop, which must be a multiple of H (else VITS_ERR_UNSUPPORTED naming both).
 *   h is the Kaiser-windowed sinc of include/vits_resample.h, c = 0.9 s, Hw = Z / s, Z = 16, beta = 10, which is h_s(x) = s h_1(s x).
 *   It is evaluated from ONE table, part of this definition: T[j] = (float) h_1(j / VITS_CONTOUR_TABLE_RES), j = 0 .. Z RES, formed on the
 *   host in double (h_1(y) = 0.9 sinc(0.9 y) I0(beta sqrt(1 - (y / Z)^2)) / I0(beta)), and T[Z RES + 1] = 0.  For a tap:
 *     p = |tau_n - k| * (s_n * RES) in double, j = min((int) p, Z RES), fr = (float)(p - j),
 *     h = (float) s_n * (T[j] + fr * (T[j + 1] - T[j]))                                   (fp32; the restatement keeps fr in double)
 *   Linear interpolation at RES = 256 sits within 1.5e-5 of h_1 (its second derivative is below 8).
 *
 * Output.  f = n >> 8, fr = (n & 255) / 256: G[n] = fp32(fp32((1 - fr) * gbar_f) + fp32(fr * gbar_{f+1})), y[n] = fp32(G[n] * v[n]);
 * y is exactly 0 from len on.
 *
 * Three exact cases, decided per item (an item's result does not depend on its batch):
 *   (a) every P_t == 1000 and every g_t == 1 in every item of the call: the call is not contoured at all; it runs the launches and
 *       graphs of the call without the flag and returns its bits.
 *   (b) every P_t == 1000 in the item: no vocoder and no warp, y[n] = fp32(G[n] * x[n]) from one elementwise kernel.
 *   (c) len < n/2 + 1: no pitch (the short-item rule of include/vits_pitch.h); the gain of (b) still applies.
 * A contour never changes out_samples, out_lengths or the marks.  Determinism as in the pitch stage: no atomics, fixed summation
 * orders, the same call twice gives the same bits.
 */
#ifndef VITS_CONTOUR_H
#define VITS_CONTOUR_H

#include "vits_prosody.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITS_CONTOUR_RAMP 4          /* R: the tracks are box means over 2 R + 1 analysis frames */
#define VITS_CONTOUR_MIN_DB (-40.0f)
#define VITS_CONTOUR_MAX_DB 12.0f
#define VITS_CONTOUR_TABLE_RES 256   /* entries of the filter table per unit of its argument */

typedef struct vits_contour {
  const float* token_semitones;  /* [B,T_x] or NULL */
  const float* token_gain_db;    /* [B,T_x] or NULL */
} vits_contour;

/* vits_synth_opts.flags / stts_synth_opts.flags: contour the returned audio as defined above, in the order decode, clamp, denoise,
 * contour (in the pitch stage's place), resample, normalise / limit.  The older structs keep their layouts; a caller that sets the flag
 * passes the extended struct below through the same `const vits_synth_opts*` / `const stts_synth_opts*` parameter, and `contour` is read
 * only when the flag is set.  The flag with a NULL `contour` is VITS_ERR_ARG.  Honoured by every entry point that honours the pitch flag.
 * With *_FLAG_PITCH_FORMANT: VITS_ERR_UNSUPPORTED naming both flags (the envelope pre-warp assumes one ratio per call).  The vocoder
 * needs the whole utterance: vits_stream_open* and stts_stream_open with the flag return VITS_ERR_UNSUPPORTED. */
#define VITS_FLAG_CONTOUR 64
#define STTS_FLAG_CONTOUR 64

typedef struct vits_synth_opts_contour {
  vits_synth_opts_prosody base;
  const vits_contour* contour;
} vits_synth_opts_contour;

typedef struct stts_synth_opts_contour {
  stts_synth_opts_limit base;
  const vits_contour* contour;
} stts_synth_opts_contour;

/* Kernel-level parity doors, host buffers, the conventions of vits_op_pitch_*: x float [B, N], lengths int64 [B] with
 * 0 <= lengths[b] <= N, cum int32 [B, T_x] (inclusive, non-decreasing over t < tok_lengths[b]), tok_lengths int64 [B] with
 * 0 <= tok_lengths[b] <= T_x, hop > 0, token_semitones / token_gain_db float [B, T_x] or NULL.  y float [B, N], exactly 0 at and beyond
 * lengths[b]; samples of x at and beyond lengths[b] are never read. */
int vits_op_contour(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, const int32_t* cum, const int64_t* tok_lengths,
                    int32_t T_x, int32_t hop, const float* token_semitones, const float* token_gain_db, float* y);
/* ... and the stages before the warp: u float [B, H * (2 * (N / H + 2) - 1)], exactly 0 at and beyond N_u[b]; steps int64
 * [B, 2 * (N / H + 2) + 2]: row b is F_s, a_0 .. a_{F_s}, then zeros.  An item of case (b) or (c) gives rows of zeros.  With it a
 * difference can be placed in the positions, the vocoder or the warp. */
int vits_op_contour_stretch(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, const int32_t* cum,
                            const int64_t* tok_lengths, int32_t T_x, int32_t hop, const float* token_semitones, const float* token_gain_db,
                            float* u, int64_t* steps);

#ifdef __cplusplus
}
#endif
#endif /* VITS_CONTOUR_H */
