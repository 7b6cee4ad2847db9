/*
 * vits_watermark.h — a keyed audio watermark: a magnitude ripple written into the returned audio by a stage of the output tail, and a
 * detector that recognises it, both on the device.  A service that hands out synthetic speech marks it with its key and later
 * recognises its own output, cropped or requantised.
 *
 * An extension of the product library: the reference has no counterpart, so these entry points are checked against a float64
 * restatement of the definition below (tests/watermark_ref.py, the authority).  Same status codes and vits_last_error as
 * include/vits_mi355.h; all are re-entrant.
 *
 * The key is a 32-bit SELECTOR, not a cryptographic secret: the chips are a public integer hash of it, anyone who holds marked and
 * unmarked copies of one utterance can read the pattern off their ratio, and 2^32 keys can be tried.  It tells one service's output
 * from another's; it proves nothing to an adversary.
 *
 * Geometry.  The transform is the denoiser's (include/vits_denoise.h, steps 1, 2 and 4): n = VITS_WATERMARK_FRAME = 1024, H = 256,
 * w[i] = sin^2(pi i / n), reflect padding n/2.  It always runs at the rate the audio is returned at.  Band: the bins
 * k in [VITS_WATERMARK_BIN_LO, VITS_WATERMARK_BIN_HI) = [16, 400), in 96 groups of 4 bins, group j = (k - 16) >> 2.  Tile rows of
 * 4 frames; the pattern repeats every 16 rows = 64 frames = 16384 samples.
 *
 * Chips.  mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16, all in uint32.
 *   c(key, q, j) = +1 if mix(mix(key) ^ (96 q + j + 1)) & 1, else -1, for q in [0, 16), j in [0, 96).
 * Integer arithmetic only: the device and the restatement agree bit for bit.
 *
 * Embed.  For an item x[0 .. len) with len >= n/2 + 1 and a = 10^(depth_dB / 20) - 1 (formed on the host in double, rounded to fp32):
 *   F = 1 + floor(len / H) frames, X_f = rFFT(frame f)
 *   X'_f[k] = X_f[k] (1 + a c(key, (f >> 2) & 15, (k - 16) >> 2)) inside the band, X_f[k] outside
 *   y = iSTFT(X') by the denoiser's step 4 on [0, H floor(len / H)); the samples from there up to len are copied from x;
 *   everything at and beyond len is exactly 0.
 * An item shorter than n/2 + 1 samples is returned unmarked (the denoiser's rule: a one-phoneme request must not fail).
 * depth_dB: 0 < depth_dB <= VITS_WATERMARK_MAX_DEPTH_DB; 0 = VITS_WATERMARK_DEFAULT_DEPTH_DB; anything else, NaN included, is
 * VITS_ERR_ARG naming the value.  The default is a design choice -- a +-1 dB magnitude ripple in 86 Hz x 46 ms tiles (at 22050 Hz) --
 * and nobody has run a listening test on it.
 *
 * Detect.  For an item x[0 .. len) (an item below n/2 + 1 samples has no frames: z = 0, offset = 0, rows = 0):
 *   1. hop-128 transform: F' = 1 + floor(len / 128) frames, frame g centred on sample 128 g, same window and padding
 *   2. A[g, k] = |X_g[k]| on the band, m_g = max_k A[g, k]
 *   3. Lb[g, j] = 1/4 sum_{i < 4} ln(max(A[g, 16 + 4 j + i], 1e-4 m_g)); a frame with m_g = 0 has Lb = 0.  The floor is relative to
 *      the frame, so the score does not move with gain, and bins that are only fp32 transform noise (below -80 dB of the frame's
 *      peak) carry nothing.
 *   4. offset index o in [0, 128) (the audio starts 128 o samples into the pattern): frames g = (o & 1) + 2 f, f = 0, 1, ..;
 *      pattern frame p = f + (o + (o & 1)) / 2; row rho = p >> 2; only rows with all four frames present count
 *   5. T[rho, j] = the mean of the row's four Lb; D[rho, j] = T[rho, j] - (T[rho, j - 1] + T[rho, j + 1]) / 2 for j = 1 .. 94;
 *      G[q, j] = sum_{rho = q (mod 16)} D[rho, j]
 *   6. z_o = sum_{q, j} c(key, q, j) G[q, j] / sqrt(sum G^2); z_o = 0 where sum G^2 = 0 or no complete row exists
 *   7. z = max_o z_o, the lowest o on a tie; offset = 128 o; rows = the complete rows at that o
 *   8. detected iff z >= VITS_WATERMARK_THRESHOLD.
 * The threshold is derived, not tuned.  For a key independent of the audio the chips c(key, q, j) are independent fair signs, and z_o is
 * their sum weighted by G[q, j] / sqrt(sum G^2), weights whose squares sum to 1.  Hoeffding: P(z_o >= t) <= exp(-t^2 / 2).  Over the 128
 * offsets, at t = 6: 128 e^(-18) = 1.9e-6 per item.  This is why the normaliser is sum G^2 over the 16 x 94 DISTINCT chips and not
 * sum D^2 over all rows: rows that share a chip are not independent terms.
 *
 * Arithmetic.  The transforms are fp32 with the host-made tables of the denoiser; the gains 1 + a and 1 - a are fp32; ln and the
 * four-term sum of Lb are fp32 (ascending i).  T, D, G, the two sums of z_o and the division are double: a few thousand terms per
 * offset.  Every sum has a fixed order and there are no atomics: the same call twice gives the same bits, and an item does not depend
 * on its batch.
 */
#ifndef VITS_WATERMARK_H
#define VITS_WATERMARK_H

#include "vits_intonation.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITS_WATERMARK_FRAME 1024
#define VITS_WATERMARK_BIN_LO 16
#define VITS_WATERMARK_BIN_HI 400
#define VITS_WATERMARK_GROUPS 96
#define VITS_WATERMARK_ROWS 16           /* tile rows per pattern period */
#define VITS_WATERMARK_OFFSETS 128
#define VITS_WATERMARK_DETECT_HOP 128
#define VITS_WATERMARK_DEFAULT_DEPTH_DB 1.0f
#define VITS_WATERMARK_MAX_DEPTH_DB 2.0f
#define VITS_WATERMARK_THRESHOLD 6.0

/* vits_synth_opts.flags / stts_synth_opts.flags: mark the returned audio as defined above.  The stage sits behind the resampler and
 * the document join and in front of normalise / limit / int16: decode, clamp, denoise, pitch / contour, join, resample, watermark,
 * normalise, limit, convert -- so the loudness gain and the limiter's ceiling still see and bound the final audio (the score is
 * gain-invariant), and a document is marked as the one item it has become.  The older structs keep their layouts; a caller that sets
 * the flag passes the extended struct below through the same `const vits_synth_opts*` / `const stts_synth_opts*` parameter, and the two
 * fields are read only when the flag is set.  Honoured by the one-shot, batch, marks and document entry points of both families.  A
 * stream has no tail: vits_stream_open* and stts_stream_open with the flag return VITS_ERR_UNSUPPORTED naming it.  Lengths and marks do
 * not change. */
#define VITS_FLAG_WATERMARK 256
#define STTS_FLAG_WATERMARK 256

typedef struct vits_synth_opts_watermark {
  vits_synth_opts_intonation base;
  uint32_t watermark_key;
  float watermark_depth_db; /* 0 = VITS_WATERMARK_DEFAULT_DEPTH_DB */
} vits_synth_opts_watermark;

typedef struct stts_synth_opts_watermark {
  stts_synth_opts_intonation base;
  uint32_t watermark_key;
  float watermark_depth_db;
} stts_synth_opts_watermark;

/* Kernel-level parity doors, host buffers, the conventions of vits_op_denoise: x float [B, N], lengths int64 [B] with
 * 0 <= lengths[b] <= N; samples of x at and beyond lengths[b] are never read.
 * The embed stage: y float [B, N]; item b is marked on [0, H floor(lengths[b] / H)), equals x from there up to lengths[b] and is
 * exactly 0 beyond; an item below n/2 + 1 samples comes back as it went in. */
int vits_op_watermark(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, float depth_db, float* y);
/* The detector: z double [B], offset int32 [B] (in samples, 128 o), rows int32 [B], and, unless NULL, z_all double [B, 128], the
 * score of every offset index. */
int vits_op_watermark_detect(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, double* z,
                             int32_t* offset, int32_t* rows, double* z_all);

#ifdef __cplusplus
}
#endif
#endif /* VITS_WATERMARK_H */
