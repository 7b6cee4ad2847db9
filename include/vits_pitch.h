/*
 * vits_pitch.h — pitch-shifted output: the finished waveform raised or lowered by a number of semitones at unchanged duration, on the
 * device behind the decoder.  VITS and Matcha have no F0 input, so pitch is signal processing on the waveform: an identity-phase-locked
 * vocoder (Laroche & Dolson, "Improved phase vocoder time-scale modification of audio", 1999) stretches the item by P/Q and the
 * resampler of include/vits_resample.h (P -> Q) brings it back to its length.  (The plain phase vocoder returns a 440 Hz sine at a tenth
 * of its amplitude: DESIGN.md "Pitch shift".)  Formants move with the pitch, as with every resampling shifter, unless the caller sets
 * VITS_FLAG_PITCH_FORMANT: then steps 3a-3d below pre-warp the magnitudes the synthesis uses, so that the spectral envelope is back
 * where it was behind the resampler.
 *
 * An extension of the product library: the reference has no counterpart, so these entry points are checked against a float64
 * restatement of the definition below (tests/pitch_ref.py, the authority).  Same status codes and vits_last_error as
 * include/vits_mi355.h; all are re-entrant.
 *
 * Ratio.  s in semitones, |s| <= VITS_PITCH_MAX_SEMITONES; P0 = lround(1000 * 2^(s/12)) in double, Q0 = 1000, g = gcd(P0, Q0),
 * P = P0 / g, Q = Q0 / g (steps of 0.1 %, about 1.7 cents).  P == Q is the identity.  Out of range or NaN is VITS_ERR_ARG naming the value.
 *
 * Geometry.  n = VITS_PITCH_FRAME = 1024, H = n / 4, w[i] = sin^2(pi i / n), NB = n / 2 + 1 bins; always at the voice's native rate.
 * For an item x[0 .. len), len >= n/2 + 1:
 *   1 analysis   reflect-pad n/2; F_a = 1 + floor(len / H) frames, X_f = rFFT(xp[f H .. f H + n) * w); mag_f[k] = |X_f[k]|;
 *                theta_f[k] = low 32 bits of (int64) rint(atan2(im, re) / 2 pi * 2^32), atan2(0, 0) = 0: the phase in 32-bit fixed-point
 *                turns.  Rows f >= F_a are zero.  All phase arithmetic from here on is unsigned 32-bit addition that wraps: exact,
 *                associative, the same in the restatement and on the device.
 *   2 steps      F_s = ceil((F_a + 1) P / Q); for t = 0 .. F_s - 1: i_t = floor(t Q / P), alpha_t = (t Q mod P) / P (integers; one
 *                division in fp32); m_t[k] = (1 - alpha_t) mag_{i_t}[k] + alpha_t mag_{i_t + 1}[k]
 *   3 phase      Phi_0 = theta_0.  For t >= 1, j = i_{t-1}, i = i_t:
 *                  adv[k] = Phi_{t-1}[k] + theta_{j+1}[k] - theta_j[k]
 *                  k is a peak of m_t iff m[k] > m[k-1], m[k] > m[k-2], m[k] >= m[k+1], m[k] >= m[k+2] (outside [0, NB): -1)
 *                  own(k) = the peak nearest to k, the lower one on a tie
 *                  Phi_t[k] = adv[own(k)] + theta_i[k] - theta_i[own(k)]          (no peak: Phi_t = adv)
 *   Under VITS_FLAG_PITCH_FORMANT, for every analysis row f < F_a (C = VITS_PITCH_LIFTER, floor = VITS_PITCH_LOG_FLOOR,
 *   g_max = VITS_PITCH_FORMANT_MAX_DB * ln(10) / 20 nepers):
 *   3a log spectrum  L[k] = ln(max(mag_f[k], floor)), k = 0 .. n/2
 *   3b cepstrum      the low quefrencies of the real, even log spectrum, q = 0 .. C:
 *                      c[q] = (D[0] + (-1)^q D[n/2] + 2 sum_{k=1}^{n/2-1} D[k] cos(2 pi k q / n)) / n,   D[k] = L[k] - L[0]
 *                    (the sums run over L less its first value: the constant adds exactly 0 to c[q], q >= 1, and c[0] cancels in 3d,
 *                    so a row of one value -- a frame of exact zeros -- has c = 0 and g = 1 exactly, in every precision); the cosine is
 *                    the n-entry table cos(2 pi j / n) at j = (k q) mod n
 *   3c envelope      at a real bin position kappa in [0, n/2]: e(kappa) = c[0] + 2 sum_{q=1}^{C} c[q] cos(2 pi kappa q / n).  The
 *                    shifted position of bin k is kappa_k = min(k P / Q, n/2); its angle is formed from integers:
 *                    r = (k P q) mod (Q n), angle = 2 pi r / (Q n) (r advances by (k P) mod (Q n) per q with one conditional
 *                    subtraction; every value stays below 2^31; one division in fp32), and where k P >= (n/2) Q the cosine is (-1)^q
 *   3d gain          g_f[k] = exp(clamp(e(kappa_k) - e(k), -g_max, +g_max)); mag'_f[k] = mag_f[k] g_f[k]; rows f >= F_a are zero,
 *                    like mag.  After the resampler bin k of u sits at k P / Q: the envelope wanted there is E(k P / Q), what bin k
 *                    carries is E(k).
 *   Steps 2 and 3 (m_t, the peak test, the owners, Phi_t) use the unscaled mag: the phases of a corrected call are those of the plain
 *   call, bit for bit.  Step 4 then takes m'_t[k] = (1 - alpha_t) mag'_{i_t}[k] + alpha_t mag'_{i_t + 1}[k] in place of m_t.
 *   4 synthesis  turn = (int32) Phi_t[k] * 2^-32; Y_t[k] = m_t[k] (cos 2 pi turn, sin 2 pi turn), the imaginary parts of bins 0 and n/2
 *                dropped; y_t = irFFT(Y_t) * w, overlap-added at hop H, times 1 / (overlap-added w^2), n/2 dropped from both ends:
 *                u[0 .. N_u), N_u = H (F_s - 1)
 *   5 resample   v = the resampler of include/vits_resample.h with rate_in = P, rate_out = Q on u; N_v = ceil(N_u Q / P)
 *   6 output     y[n] = v[n] for n < min(len, N_v), exactly 0 up to len.  N_v >= H floor(len / H) for every P, and synthesis lengths are
 *                multiples of the vocoder's hop, which must be a multiple of H (else VITS_ERR_UNSUPPORTED naming both): nothing is lost.
 * An item shorter than n/2 + 1 samples is returned unshifted (the denoiser's rule for short utterances).
 *
 * Arithmetic: fp32 apart from the integer phases and the magnitude under the logarithm of 3a, which the device takes from a transform of
 * the frame in double and rounds to fp32 once (the logarithm magnifies the fp32 transform's error at bins near zero); twiddles, window, 1 / sum w^2 and resampler coefficients are host-computed tables;
 * every sum has a fixed order, no atomics: the same call twice gives the same bits, and an item's result does not depend on its batch.
 */
#ifndef VITS_PITCH_H
#define VITS_PITCH_H

#include "vits_loudness.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITS_PITCH_FRAME 1024
#define VITS_PITCH_MAX_SEMITONES 12
#define VITS_PITCH_LIFTER 40          /* C: the quefrencies 0 .. C make the envelope */
#define VITS_PITCH_LOG_FLOOR 1e-4f    /* floor of the magnitude under the logarithm */
#define VITS_PITCH_FORMANT_MAX_DB 30  /* G: the envelope gain of a bin is clamped to +- G dB */
/* Device scratch one group of items may take, in bytes.  An item needs about 4 KiB per analysis frame (magnitudes and phases) and 7 KiB
 * per step (phases, the frame, its share of u): 16 bytes per sample plus 28 bytes per sample times P / Q; under VITS_FLAG_PITCH_FORMANT
 * another 2 KiB per analysis frame (the corrected magnitudes): 24 bytes per sample plus the same.  The items of a batch run in
 * groups of consecutive items that fit, and a single item that does not (about 7 M samples at +12 semitones) is VITS_ERR_UNSUPPORTED
 * naming its length. */
#define VITS_PITCH_MAX_SCRATCH (512LL << 20)

/* vits_synth_opts.flags / stts_synth_opts.flags: shift the returned audio as defined above, in the order decode, clamp, denoise,
 * pitch, resample, normalise.  vits_synth_opts and stts_synth_opts_loudness keep their layouts (their mirrors are pinned to them); a
 * caller that sets the flag passes the extended struct below through the same `const vits_synth_opts*` / `const stts_synth_opts*`
 * parameter (pass &o.base, or &o.base.base), and pitch_semitones is read only when the flag is set.  The loudness fields inside are
 * still read only under their own flag. */
#define VITS_FLAG_PITCH 4
#define STTS_FLAG_PITCH 8
/* ... and keep the spectral envelope (the formants) where it was: steps 3a-3d.  These bits modify a pitch request and add no field.  Set
 * without the pitch flag: VITS_ERR_ARG naming both flags.  Set with a shift that reduces to P = Q: the call as it was. */
#define VITS_FLAG_PITCH_FORMANT 8
#define STTS_FLAG_PITCH_FORMANT 16

typedef struct vits_synth_opts_pitch {
  vits_synth_opts base;
  float pitch_semitones;
} vits_synth_opts_pitch;

typedef struct stts_synth_opts_pitch {
  stts_synth_opts_loudness base;
  float pitch_semitones;
} stts_synth_opts_pitch;

/* Host only: the ratio of a shift.  Either out pointer may be NULL. */
int vits_pitch_plan(float semitones, int32_t* P, int32_t* Q);

/* Kernel-level parity door, host buffers: x float [B, N], lengths int64 [B] with 0 <= lengths[b] <= N, y float [B, N].  Item b is shifted
 * from x[b, 0 : lengths[b]) only -- samples at and beyond lengths[b] are never read -- and y is exactly 0 there.  A length below
 * n/2 + 1 copies the item; P == Q copies every item. */
int vits_op_pitch_shift(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, float semitones, float* y);
/* ... and u, the vocoder's output before the resampler: y float [B, H * (ceil((floor(N / H) + 2) * P / Q) - 1)], exactly 0 at and beyond
 * N_u[b]; an item below n/2 + 1 samples gives a row of zeros.  With it a difference can be placed in the vocoder or in the resampler.
 * P == Q is VITS_ERR_ARG (there is no stretch to return). */
int vits_op_pitch_stretch(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, float semitones, float* y);

#ifdef __cplusplus
}
#endif

/* the parity doors of steps 3a-3d: vits_op_pitch_shift_formant, vits_op_pitch_stretch_formant, vits_op_pitch_formant_gain */
#include "vits_pitch_formant.h"

#endif /* VITS_PITCH_H */
