/*
 * vits_intonation.h — intonation range: how far the voice moves about its own median pitch, scaled by r at unchanged duration, on the
 * device behind the decoder.  include/vits_pitch.h moves a whole utterance by one ratio and include/vits_contour.h a token by its own;
 * here the ratio follows the signal: an F0 track of the finished waveform at the pitch stage's frame geometry, integer offsets that
 * scale its deviation from the median, and the contour stage run on the per-frame ratios that come of it.  r = 0 is a monotone,
 * r < 1 a calmer reading, r > 1 a livelier one (W3C SSML: the `range` attribute of `prosody`).
 *
 * An extension of the product library: the reference has no counterpart, so these entry points are checked against a float64
 * restatement of the definition below (tests/intonation_ref.py, the authority).  Same status codes and vits_last_error as
 * include/vits_mi355.h; all are re-entrant.
 *
 * Geometry.  That of include/vits_pitch.h: n = VITS_PITCH_FRAME = 1024, H = 256, reflect-pad n/2, F = 1 + floor(len / H) rows, row f is
 * fr = xp[f H .. f H + n), always at the voice's native rate sr.  An item below n/2 + 1 samples has no track (every cents_f = 0).
 *
 * F0 track (YIN: de Cheveigne & Kawahara, "YIN, a fundamental frequency estimator for speech and music", 2002), per row.
 *   W = VITS_INTONATION_WINDOW = 512, tau_min = max(2, floor(sr / 550)), tau_max = min(ceil(sr / 55), W - 1);
 *   VITS_INTONATION_MIN_RATE <= sr <= VITS_INTONATION_MAX_RATE, anything else is VITS_ERR_UNSUPPORTED naming the rate.
 *     d(tau)  = sum_{j < W} (fr[j] - fr[j + tau])^2, tau = 1 .. tau_max + 1, in fp32 in ascending j: the direct form (the
 *               autocorrelation form r(0) + r_tau(0) - 2 r(tau) cancels in fp32 where the frame is periodic, which is where it matters)
 *     d'(tau) = d(tau) tau / sum_{i <= tau} d(i), and 1 where that sum is 0 (fp32; the running sum in ascending tau)
 *   Decision: the first tau in [tau_min, tau_max] with d'(tau) < VITS_INTONATION_THRESHOLD (fp32), walked forward while
 *   d'(tau + 1) < d'(tau) and tau + 1 <= tau_max.  In double from there: y0, y1, y2 = d'(tau - 1), d'(tau), d'(tau + 1),
 *   c = y0 - 2 y1 + y2, off = c > 0 ? clamp((y0 - y2) / (2 c), -0.5, 0.5) : 0, f0 = sr / (tau + off),
 *     cents_f = lround(1200 log2(f0 / 27.5))           (always > 0: f0 > 54 Hz)
 *   No tau under the threshold: the row is unvoiced, cents_f = 0.
 *
 * Offsets.  Integers, the same on the host, in NumPy and on the device.  rha(a / b), b > 0, is sign(a) ((2 |a| + b) div (2 b)): round
 * half away from zero.
 *     r_m   = lround(1000 r), 0 <= r <= VITS_INTONATION_MAX_RANGE; NaN or out of range is VITS_ERR_ARG naming the value
 *     c_med = the lower median of the item's voiced cents_f (the element (V - 1) div 2 of the V voiced values in ascending order)
 *     voiced row:    o_f = rha((r_m - 1000) (cents_f - c_med) / 1000)
 *     unvoiced row between the nearest voiced rows l < f < g:  o_f = o_l + rha((o_g - o_l) (f - l) / (g - l));
 *     before the first voiced row and behind the last: that row's o; no voiced row: every o_f = 0
 *     then o_f = clamp(o_f, -1200, 1200), R_f = TAB[o_f + 1200], TAB[j] = lround(1000 * 2^((j - 1200) / 1200)): 2401 entries formed on
 *     the host in double.
 *
 * Ratios.  P_f = clamp((P_tok(f) R_rho(f) + 500) div 1000, 500, 2000): P_tok(f) is the contour stage's token ratio of the row (1000
 * without a contour; under VITS_FLAG_PITCH it carries the call's own shift, as the contour does), and rho(f) = min(f H, len - 1) div H
 * is the row that holds the sample by which the contour stage finds tok(f): f itself, except the last row of a length that is a
 * multiple of H.  So a call without a token contour is the contour of include/vits_contour.h with one token per analysis row
 * (cum = 1 .. F, hop = H, o_f / 100 semitones), integer for integer.
 *
 * From here include/vits_contour.h word for word with P_f in place of P_tok(f): Sigma_f, inc_f, the position table, the vocoder with
 * its analysis transform in double, the warp, the gain track (token gains apply as there where a contour is given) and the output.
 *
 * Exact cases.
 *   r_m == 1000: the call without the flag, on the graphs and launches of before, bit for bit.
 *   An item whose every P_f is 1000 (no voiced row, a constant track, or len < n/2 + 1) is case (b) of include/vits_contour.h: without
 *   token gains it is x bit for bit.  That is decided from the device's own track: one word per item is read back per call.
 * Intonation never changes out_samples, out_lengths or the marks.  Determinism: no float atomics (the median's histogram counts with
 * integer atomics, which commute), fixed summation orders, an item's result does not depend on its batch.
 */
#ifndef VITS_INTONATION_H
#define VITS_INTONATION_H

#include "vits_contour.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITS_INTONATION_WINDOW 512
#define VITS_INTONATION_THRESHOLD 0.15f
#define VITS_INTONATION_MIN_RATE 8000
#define VITS_INTONATION_MAX_RATE 32000
#define VITS_INTONATION_MAX_RANGE 4.0f
#define VITS_INTONATION_MAX_CENTS 1200   /* |o_f| is clamped to an octave */

/* vits_synth_opts.flags / stts_synth_opts.flags: scale the intonation range of the returned audio as defined above, in the contour
 * stage's place (decode, clamp, denoise, contour / intonation, resample, normalise / limit).  The older structs keep their layouts; a
 * caller that sets the flag passes the extended struct below through the same `const vits_synth_opts*` / `const stts_synth_opts*`
 * parameter, and pitch_range is read only when the flag is set.  With or without *_FLAG_CONTOUR (its pointer is read under its own flag
 * alone) and *_FLAG_PITCH.  Honoured by every entry point that honours the contour flag.  With *_FLAG_PITCH_FORMANT:
 * VITS_ERR_UNSUPPORTED naming both flags.  The median needs the whole utterance: vits_stream_open* and stts_stream_open with the flag
 * return VITS_ERR_UNSUPPORTED.  The vocoder's hop must be a multiple of H, as for a contour. */
#define VITS_FLAG_INTONATION 128
#define STTS_FLAG_INTONATION 128

typedef struct vits_synth_opts_intonation {
  vits_synth_opts_contour base;
  float pitch_range;
} vits_synth_opts_intonation;

typedef struct stts_synth_opts_intonation {
  stts_synth_opts_contour base;
  float pitch_range;
} stts_synth_opts_intonation;

/* Kernel-level parity doors, host buffers, the conventions of vits_op_contour*: x float [B, N], lengths int64 [B] with
 * 0 <= lengths[b] <= N; samples of x at and beyond lengths[b] are never read.
 * The track alone: cents int32 [B, 1 + N / H]; row b holds cents_f for f < 1 + lengths[b] / H and zeros behind, all zeros for an item
 * below n/2 + 1 samples. */
int vits_op_f0_track(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, int32_t* cents);
/* The stage: cum / tok_lengths / token_semitones / token_gain_db as in vits_op_contour, or cum == NULL with T_x == 0 for no tokens
 * (then tok_lengths and both token arrays are not read).  y float [B, N], exactly 0 at and beyond lengths[b]. */
int vits_op_intonation(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, const int32_t* cum,
                       const int64_t* tok_lengths, int32_t T_x, int32_t hop, const float* token_semitones, const float* token_gain_db,
                       float pitch_range, float* y);
/* ... and the stages before the warp, u and steps with the shapes of vits_op_contour_stretch, and the track the ratios came from:
 * cents int32 [B, 1 + N / H] as above. */
int vits_op_intonation_stretch(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, const int32_t* cum,
                               const int64_t* tok_lengths, int32_t T_x, int32_t hop, const float* token_semitones,
                               const float* token_gain_db, float pitch_range, float* u, int64_t* steps, int32_t* cents);

#ifdef __cplusplus
}
#endif
#endif /* VITS_INTONATION_H */
