/*
 * vits_watermark_scan.h — where in a recording the keyed audio watermark of include/vits_watermark.h sits: a device scan that scores
 * every window of `span` pattern periods at every offset, and the threshold that goes with it.  The detector and the reader answer one
 * question about a whole item; on a recording in which a few seconds of marked audio sit between other speech their score dilutes, and
 * it cannot say where the mark is.  The scan sums the same per-row differences over windows instead of over the whole item.
 *
 * An extension of the product library: the reference has no counterpart, so this entry point is checked against a float64
 * restatement of the definition below (tests/watermark_scan_ref.py, the authority, on top of tests/watermark_ref.py).  Same status
 * codes and vits_last_error as include/vits_mi355.h; re-entrant.
 *
 * Definition.  Steps 1 to 4 of Detect (vits_watermark.h) unchanged: Lb, and g0, pbase and the complete rows r0 .. r1 of offset index o.
 *   S1. Row differences.  For every complete row rho, T[rho, j] and D[rho, j] are those of Detect step 5, in double.
 *   S2. Complete periods.  Period p is the rows 16 p .. 16 p + 15.  The complete periods of offset o are
 *       p0 = ceil(r0 / 16) .. p1 = floor((r1 + 1) / 16) - 1.  Gp[p][q, j] = D[16 p + q, j].
 *   S3. Windows.  Window w >= 0 of span S covers periods p0 + w .. p0 + w + S - 1; W_o = max(0, p1 - p0 + 2 - S) windows exist at
 *       offset o.  G = ((Gp[p0 + w] + Gp[p0 + w + 1]) + ...), ascending, in double: the written sum, not a running add and subtract,
 *       so a window does not depend on the windows before it.
 *   S4. Score.  z[o, w] = sum_{q, j} c G / sqrt(sum G^2) over j = 1 .. 94, and 0 where sum G^2 = 0.  With
 *       VITS_WATERMARK_SCAN_PILOTS both sums run over the pilot positions (q + j) & 1 only: the payload reader's rule
 *       (vits_watermark_payload.h, step 6'), so audio marked with a payload is localised with that flag.
 *   S5. Nominal range.  Window (o, w) covers the audio samples [16384 (p0 + w) - 128 o, 16384 (p0 + w + S) - 128 o), clipped to
 *       [0, len): hop-256 pattern frame p is centred on audio sample 256 p - 128 o.
 *   S6. Threshold.  t(Wmax) = sqrt(36 + 2 ln(max(1, Wmax))), Wmax = max_o W_o.  Hoeffding gives exp(-t^2 / 2) per (offset, window),
 *       as it does for the detector; the union bound over at most 128 Wmax of them gives 128 Wmax e^(-t^2 / 2) = 128 e^(-18) = 1.9e-6
 *       per item, the detector's own figure, and t(1) = 6.  Overlapping windows are dependent, and the union bound does not care.
 *       Derived, like the detector's; not tuned.
 * span: 1 .. VITS_WATERMARK_SCAN_MAX_SPAN; 0 = VITS_WATERMARK_SCAN_DEFAULT_SPAN; anything else is VITS_ERR_ARG naming the value.  An
 * item below n/2 + 1 = 513 samples, or one with fewer than S complete periods at an offset, has W_o = 0 there.
 *
 * Arithmetic.  As in Detect: the transform, ln and Lb are fp32 (the detector's own kernel produces Lb); T, D, the window sums, the two
 * sums of S4 and the division are double.  Every sum has a fixed order and there are no atomics: the same call twice gives the same
 * bits, and an item depends neither on its batch nor on how the windows are shared out over workgroups.
 */
#ifndef VITS_WATERMARK_SCAN_H
#define VITS_WATERMARK_SCAN_H

#include "vits_watermark_payload.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITS_WATERMARK_SCAN_MAX_SPAN 8
#define VITS_WATERMARK_SCAN_DEFAULT_SPAN 4
#define VITS_WATERMARK_PERIOD_SAMPLES 16384 /* 16 tile rows of 4 frames at hop 256 */

/* vits_op_watermark_scan flags */
#define VITS_WATERMARK_SCAN_PILOTS 1u

/* max_o W_o of an item of n_samples at this span: what sizes z_scan.  -1 (and vits_last_error) for a negative n_samples or a span
 * outside [0, VITS_WATERMARK_SCAN_MAX_SPAN]. */
int64_t vits_watermark_scan_windows(int64_t n_samples, int32_t span);

/* The scan, host buffers, the conventions of vits_op_watermark_detect: x float [B, N], lengths int64 [B] with 0 <= lengths[b] <= N;
 * samples of x at and beyond lengths[b] are never read.  z_scan double [B, 128, w_cap]: z[o, w] of item b, exactly 0 at and beyond
 * W_o; first_period int32 [B, 128]: p0; windows int32 [B, 128]: W_o.  w_cap below what the longest item needs
 * (vits_watermark_scan_windows) is VITS_ERR_ARG naming both numbers; flags with an unknown bit are VITS_ERR_ARG naming them. */
int vits_op_watermark_scan(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, int32_t span,
                           uint32_t flags, int64_t w_cap, double* z_scan, int32_t* first_period, int32_t* windows);

#ifdef __cplusplus
}
#endif
#endif /* VITS_WATERMARK_SCAN_H */
