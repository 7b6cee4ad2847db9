/*
 * vits_loudness.h — loudness-normalised output: an ITU-R BS.1770 integrated-loudness (LUFS) target or a max-peak target per request,
 * measured and applied on the device behind the decoder (server/tts_service.proto is modelled on an API family that takes exactly
 * these two; the reference's only volume control is the per-voice `inference.scale` multiplier, vosk_tts/synth.py:127-130).
 *
 * An extension of the product library: the reference has no counterpart, so these entry points are checked against a float64
 * restatement of the definition below (tests/loudness_ref.py).  Same status codes and vits_last_error as include/vits_mi355.h; all
 * are re-entrant.
 *
 * Definition.  `rate` is the rate of the audio the call returns (the voice's own, or the requested sample_rate).  x[0 .. len) is an
 * item's finished waveform: after the decoder and, where requested, the clamp, the denoiser and the resampler; before pcm_scale /
 * `scale` and before the int16 conversion.
 *
 * K-weighting: two biquads in cascade, zero initial state, x = 0 before sample 0; coefficients computed on the host in double and
 * rounded once to fp32.
 *   stage 1 (shelf):     f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196
 *                        K = tan(pi f0 / rate), Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2
 *                        b = [Vh + Vb K/Q + K^2, 2 (K^2 - Vh), Vh - Vb K/Q + K^2] / a0
 *                        a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0]
 *   stage 2 (high-pass): f0 = 38.13547087602444, Q = 0.5003270373238773, K and a0 formed as in stage 1
 *                        b = [1, -2, 1],  a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0]
 * (at 48000 Hz these are the BS.1770-4 table values to all printed digits).  rate >= VITS_LOUDNESS_MIN_RATE; anything below is
 * VITS_ERR_UNSUPPORTED naming the value.
 *
 * Blocks: hop = (rate + 5) / 10 (integer division, 100 ms), a block is 4 hop samples, y the filtered signal,
 *   E_i = sum y[n]^2 over n in [i hop, (i+1) hop), i < nh = floor(len / hop)
 *   nh >= 4:           z_j = (E_j + E_j+1 + E_j+2 + E_j+3) / (4 hop), j = 0 .. nh - 4 (the incomplete tail is dropped)
 *   1 <= len < 4 hop:  one block over the whole item, z_0 = sum_{n < len} y[n]^2 / len
 *   len = 0:           no block
 * Gating: l_j = -0.691 + 10 log10 z_j;  J_a = { j : l_j > -70 };  Gamma = -0.691 + 10 log10(mean_{J_a} z) - 10;
 *   J = { j in J_a : l_j > Gamma };  L = -0.691 + 10 log10(mean_J z);  L = -inf when J_a is empty (silence, or no block).
 * Peak: max |x[n]| over n < len on the unfiltered signal, 0 for len = 0.
 * Gain:
 *   VITS_LOUDNESS_LUFS, target T in [-70, 0]: g = 10^((T - L) / 20), g = 1 when L = -inf; with ceiling > 0 and g peak > ceiling,
 *                                             g = ceiling / peak (ceiling 0 = no cap)
 *   VITS_LOUDNESS_PEAK, target P in (0, 1]:   g = P / peak, g = 1 when peak = 0
 *   a value out of range is VITS_ERR_ARG naming the value.
 * Output: the float output is fp32(g x[n]); the int16 output is the conversion of vits_synthesize_pcm16 (scale, * 32767, clip,
 * truncating cast) of that float value.  Samples at and beyond an item's length stay zero and are never read; lengths, marks and sample
 * counts do not change.
 *
 * Arithmetic: the samples and the coefficients are fp32 values; the recurrence, the squares, the per-hop sums, both gates and the gain
 * are formed in double and L and the gain rounded once.  The cascade is a 4-state linear system, so the recurrence is cut into runs
 * that start from zero state and are joined by an affine scan whose matrices (powers of the state matrix) come from the host in
 * double.  Partial sums go to fixed slots and are added in a fixed order: no atomics, the same call twice gives the same bits.
 */
#ifndef VITS_LOUDNESS_H
#define VITS_LOUDNESS_H

#include "vits_marks.h"
#include "vits_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITS_LOUDNESS_TILE 2048     /* consecutive samples of one item that one workgroup of the loudness kernels owns */
#define VITS_LOUDNESS_MIN_RATE 4000 /* Hz */
#define VITS_LOUDNESS_LUFS 1        /* loudness_mode */
#define VITS_LOUDNESS_PEAK 2

/* vits_synth_opts.flags / stts_synth_opts.flags: normalise the returned audio as defined above.  The flag says that the five fields
 * below follow the older fields of the options struct the caller passes, and they are read only when it is set (the rule item_seeds and
 * denoiser_strength follow): a caller built against the shorter struct never sets the flag.  vits_synth_opts (include/vits_mi355.h)
 * declares them itself, behind `bert`.  stts_synth_opts (include/stts_mi355.h) keeps its size and its last fields as they were -- its
 * mirrors are pinned to that layout -- so a multistream caller that sets STTS_FLAG_LOUDNESS passes a stts_synth_opts_loudness (below)
 * through the same `const stts_synth_opts*` parameter: the same bytes an appended field list would give.
 *     int32_t loudness_mode;      VITS_LOUDNESS_LUFS or VITS_LOUDNESS_PEAK
 *     float   loudness_target;    LUFS in [-70, 0], or peak in (0, 1]
 *     float   loudness_ceiling;   LUFS mode: cap on g * peak, 0 = none (>= 0); ignored in PEAK mode
 *     float*  out_loudness;       [B] or NULL: the measured L of the un-normalised item (-INFINITY for silence)
 *     float*  out_gain;           [B] or NULL: the gain applied
 * Honoured by vits_synthesize, vits_synthesize_pcm16, their _rate and _marks forms (padded and VITS_FLAG_SOLO_BATCH batches, a gain per
 * item) and by stts_synthesize, stts_synthesize_batch and their _marks forms, in the order decode, clamp, denoise, resample,
 * normalise.  An integrated-loudness target needs the whole utterance: vits_stream_open* and stts_stream_open with the flag return
 * VITS_ERR_UNSUPPORTED.  vits_session_synthesize_device takes no options and so has no normalised form.
 * A call without the flag replays exactly the graphs and launches it did before this header existed; a call with it runs the float
 * form of its phase-2 graph and the loudness launches behind it on the same stream. */
#define VITS_FLAG_LOUDNESS 2
#define STTS_FLAG_LOUDNESS 4

/* What `opts` points to in a multistream call with STTS_FLAG_LOUDNESS in base.flags: pass &o.base. */
typedef struct stts_synth_opts_loudness {
  stts_synth_opts base;
  int32_t loudness_mode;
  float loudness_target;
  float loudness_ceiling;
  float* out_loudness;
  float* out_gain;
} stts_synth_opts_loudness;

/* Host only: the K-weighting coefficients at `rate` in double, sos[stage] = {b0, b1, b2, 1, a1, a2}, and the hop.  Either out pointer
 * may be NULL. */
int vits_loudness_plan(int32_t rate, double sos[2][6], int32_t* hop);

/* Kernel-level parity doors (as vits_op_resample is for the resampler), host buffers: x float [B, N], lengths int64 [B] with
 * 0 <= lengths[b] <= N.  Item b is measured from x[b, 0 : lengths[b]) only -- samples at and beyond lengths[b] are never read.
 * loudness float [B] (L, -INFINITY for silence or length 0), peak float [B]; either may be NULL. */
int vits_op_loudness(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, float* loudness,
                     float* peak);
/* ... and normalised: y float [B, N] = fp32(gain[b] * x[b, n]) for n < lengths[b], exactly 0 beyond; loudness / gain float [B], either
 * may be NULL. */
int vits_op_loudness_normalize(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, int32_t mode,
                               float target, float ceiling, float* y, float* loudness, float* gain);

#ifdef __cplusplus
}
#endif
#endif /* VITS_LOUDNESS_H */
