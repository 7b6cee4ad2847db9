/*
 * vits_limit.h — a look-ahead peak limiter for the finished waveform, on the device: a sample-peak mode and a true-peak mode (4x
 * oversampled), run with a fixed pre-gain or with the BS.1770 loudness gain of include/vits_loudness.h.  The loudness feature meets a
 * LUFS target only while gain * peak <= ceiling and otherwise falls back to ceiling / peak, which leaves peaky speech too quiet; a limiter
 * takes the gain down around the peaks only.
 *
 * An extension of the product library: the reference has no counterpart, so these entry points are checked against a float64
 * restatement of the definition below (tests/limit_ref.py).  Same status codes and vits_last_error as include/vits_mi355.h; all
 * are re-entrant.
 *
 * Definition.  `rate` is the rate of the audio, x[0 .. len) an item as include/vits_loudness.h defines it, c the ceiling in (0, 1],
 * g >= 0 the pre-gain (fp32), W = round(lookahead_ms * rate / 1000) with 1 <= W <= VITS_LIMIT_MAX_LOOKAHEAD,
 * a = exp(-1 / (release_ms * rate / 1000)), both formed on the host in double from the fp32 arguments.  r[j] = 1 for j < 0 and j >= len.
 *   1 envelope p[n]
 *       VITS_LIMIT_SAMPLE: p[n] = |x[n]|
 *       VITS_LIMIT_TRUE:   u = the item resampled by the definition of include/vits_resample.h with rate_in = rate, rate_out = 4 rate
 *                          (L = 4, M = 1, the fp32 table of vits_resample_table(rate, 4 rate): 4 rows of 33 taps, half width 16; fp32
 *                          accumulation in ascending tap order, as resample_kernel does it);
 *                          p[n] = max(|x[n]|, |u[4n]|, |u[4n+1]|, |u[4n+2]|, |u[4n+3]|).  u is never written to memory.
 *       The true peak of an item is max_n p[n] in VITS_LIMIT_TRUE mode, 0 for len = 0.
 *   2 required gain    r[n] = min(1, c / (g p[n])), r[n] = 1 where g p[n] = 0
 *   3 look-ahead min   m[k] = min r[k .. k+W]                              k in [-W, len)
 *   4 release          e[-W-1] = 1, e[k] = min(m[k], a e[k-1] + (1 - a))   k in [-W, len)
 *   5 attack (box)     s[n] = (e[n-W] + ... + e[n]) / (W + 1)              n in [0, len)
 *   6 output           y[n] = fp32(fp32(g s[n]) x[n]); y is exactly 0 at and beyond len.
 * Every e[k] that s[n] averages has n inside its own look-ahead window, so s[n] <= r[n] and g s[n] p[n] <= c: the pre-roll [-W, 0) is
 * what makes that hold for a peak at sample 0.
 *
 * Arithmetic: p is fp32; steps 2-5 are formed in double from the fp32 values p, c and g, and g s[n] is rounded once.  r is a
 * non-increasing function of p, so m[k] = r(max p[k .. k+W]) exactly and the device slides a maximum over fp32 p.  The device carries the
 * deficit d = 1 - e, d[k] = max(1 - m[k], a d[k-1]), d[-W-1] = 0, and s[n] = 1 - (d[n-W] + ... + d[n]) / (W + 1): the same recurrence,
 * whose maps v -> max(C, A v) compose without an additive term.  An item that never reaches the ceiling therefore has d = 0, s = 1 and
 * y = fp32(g x) exactly.  The maps compose associatively: a tile's composite is folded over the tiles by one wave per item, in a fixed
 * order; no atomics, the same call twice gives the same bits.
 *
 * With a LUFS target T (vits_op_loudness_limit), VITS_LIMIT_PASSES = 2 passes:
 *     g_0 = 10^((T - L) / 20) with no cap (1 when L = -inf), as include/vits_loudness.h forms it, rounded to fp32
 *     y_0 = limit(x, g_0), L_0 = the integrated loudness of y_0 by the same kernels
 *     g_1 = fp32(g_0 * fp32(10^((T - L_0) / 20))), g_1 = g_0 when L_0 = -inf; the output is limit(x, g_1)
 * An item whose first pass did not limit (g_0 max p <= c) is at its target already and keeps g_1 = g_0: its output is the un-capped
 * normalisation fp32(g_0 x) bit for bit.
 *
 * Accepted values: ceiling in (0, 1], lookahead_ms in (0, 10], release_ms in [1, 1000], gain in [0, 64], mode VITS_LIMIT_SAMPLE or
 * VITS_LIMIT_TRUE; anything else (NaN included) is VITS_ERR_ARG naming the value.  W outside [1, VITS_LIMIT_MAX_LOOKAHEAD] is
 * VITS_ERR_UNSUPPORTED naming W.  rate in [1, 2^24]; the LUFS form also needs rate >= VITS_LOUDNESS_MIN_RATE.
 */
#ifndef VITS_LIMIT_H
#define VITS_LIMIT_H

#include "vits_pitch.h"
#include "vits_resample.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITS_LIMIT_TILE 2048          /* consecutive samples of one item that one workgroup of the limiter kernels owns */
#define VITS_LIMIT_MAX_LOOKAHEAD 1024 /* W, samples */
#define VITS_LIMIT_OVERSAMPLE 4       /* VITS_LIMIT_TRUE */
#define VITS_LIMIT_PASSES 2           /* of the LUFS form */
#define VITS_LIMIT_SAMPLE 1           /* mode */
#define VITS_LIMIT_TRUE 2

/* vits_synth_opts.flags / stts_synth_opts.flags: limit the returned audio as defined above, in the order decode, clamp, denoise, pitch,
 * resample, normalise + limit (pcm_scale / `scale` multiplies afterwards, as before).  The older structs keep their layouts (their mirrors
 * are pinned to them); a caller that sets the flag passes the extended struct below through the same `const vits_synth_opts*` /
 * `const stts_synth_opts*` parameter (&o.base.base, or &o.base.base.base), and the six fields are read only when the flag is set.  The
 * loudness and pitch fields inside are still read only under their own flags.
 *     int32_t limit_mode;          VITS_LIMIT_SAMPLE or VITS_LIMIT_TRUE
 *     float   limit_ceiling;       c in (0, 1]
 *     float   limit_lookahead_ms;  (0, 10]
 *     float   limit_release_ms;    [1, 1000]
 *     float   limit_gain;          g in [0, 64]; read only without the loudness flag
 *     float*  out_reduction;       [B] or NULL: min_n s[n] of the last pass (1: the item was not limited)
 * With the loudness flag in VITS_LOUDNESS_LUFS mode: the two-pass form above at loudness_target, out_gain receives g_1, and
 * loudness_ceiling must be 0 -- anything else is VITS_ERR_ARG naming loudness_ceiling and limit_ceiling, so that two ceilings never compete.
 * With it in VITS_LOUDNESS_PEAK mode: VITS_ERR_ARG.  Without it: one pass at g = limit_gain, a plain limiter.
 * Honoured by every entry point that honours VITS_FLAG_LOUDNESS / STTS_FLAG_LOUDNESS, padded and solo batches alike; in a limited call
 * limit_apply_kernel takes the place of loud_apply_kernel, so at int16 output still only int16 crosses to the host.  The look-ahead and the
 * loudness passes need the whole utterance: vits_stream_open* and stts_stream_open with the flag return VITS_ERR_UNSUPPORTED.
 * A call without the flag replays exactly the graphs and launches it did before this header existed. */
#define VITS_FLAG_LIMIT 16
#define STTS_FLAG_LIMIT 32

typedef struct vits_synth_opts_limit {
  vits_synth_opts_pitch base;
  int32_t limit_mode;
  float limit_ceiling;
  float limit_lookahead_ms;
  float limit_release_ms;
  float limit_gain;
  float* out_reduction;
} vits_synth_opts_limit;

typedef struct stts_synth_opts_limit {
  stts_synth_opts_pitch base;
  int32_t limit_mode;
  float limit_ceiling;
  float limit_lookahead_ms;
  float limit_release_ms;
  float limit_gain;
  float* out_reduction;
} stts_synth_opts_limit;

/* Host only: W and a of a setting at `rate`.  Either out pointer may be NULL. */
int vits_limit_plan(int32_t rate, float lookahead_ms, float release_ms, int32_t* W, double* a);

/* Kernel-level parity doors, host buffers, the conventions of vits_op_loudness: x float [B, N], lengths int64 [B] with
 * 0 <= lengths[b] <= N; item b is taken from x[b, 0 : lengths[b]) only -- samples at and beyond lengths[b] are never read. */
/* tp float [B]: the true peak of every item (step 1, VITS_LIMIT_TRUE). */
int vits_op_true_peak(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, float* tp);
/* s float [B, N]: the gain curve of step 5 rounded to fp32, exactly 1 at and beyond lengths[b]: with it a difference can be placed in the
 * curve or in its application. */
int vits_op_limit_gain(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, int32_t mode, float ceiling,
                       float lookahead_ms, float release_ms, float gain, float* s);
/* y float [B, N] (step 6, exactly 0 at and beyond lengths[b]); reduction float [B] or NULL: min_n fp32(s[n]), 1 for an empty item. */
int vits_op_limit(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, int32_t mode, float ceiling,
                  float lookahead_ms, float release_ms, float gain, float* y, float* reduction);
/* The two-pass LUFS form.  loudness float [B]: L of the item as given (-INFINITY for silence); gain float [B]: g_1; reduction float [B]:
 * min s of the last pass; any of the three may be NULL. */
int vits_op_loudness_limit(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, float target, int32_t mode,
                           float ceiling, float lookahead_ms, float release_ms, float* y, float* loudness, float* gain, float* reduction);

#ifdef __cplusplus
}
#endif
#endif /* VITS_LIMIT_H */
