/*
 * vits_pitch_formant.h -- the kernel-level parity doors of the formant-preserving pitch shift (VITS_FLAG_PITCH_FORMANT, steps 3a-3d of
 * include/vits_pitch.h, which includes this file: a caller includes that one).  Checked against the float64 restatement
 * tests/pitch_formant_ref.py.  Buffers, lengths and status codes as for vits_op_pitch_shift / vits_op_pitch_stretch.
 */
#ifndef VITS_PITCH_FORMANT_H
#define VITS_PITCH_FORMANT_H

#include "vits_pitch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vits_op_pitch_shift and vits_op_pitch_stretch with steps 3a-3d: the same signatures, the same shapes, the same rules for short items
 * and for P == Q. */
int vits_op_pitch_shift_formant(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, float semitones, float* y);
int vits_op_pitch_stretch_formant(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, float semitones, float* y);
/* The gains of step 3d themselves: gain float [B, N / H + 3, NB]; row f of item b is g_f for f < F_a[b], and every other row is exactly
 * 0, the rows of an item below n/2 + 1 samples included.  P == Q is VITS_ERR_ARG (there is no gain to return). */
int vits_op_pitch_formant_gain(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, float semitones, float* gain);

#ifdef __cplusplus
}
#endif
#endif /* VITS_PITCH_FORMANT_H */
