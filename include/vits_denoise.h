/*
 * vits_denoise.h — the vocoder-bias denoiser of the StableTTS / Matcha ("multistream") voices
 * (training/stabletts/matcha/hifigan/denoiser.py; built for every HiFi-GAN vocoder at matcha/cli.py:105-108, --denoiser_strength
 * at cli.py:253-256), as a device STFT / per-bin gain / iSTFT behind the decoder.
 *
 * An extension of the product library: the exported graph the CPU oracle mirrors has no denoiser, so these entry points are checked
 * against a float64 restatement of the definition below (tests/denoise_ref.py).  Same status codes and vits_last_error as
 * include/vits_mi355.h; all are re-entrant.
 *
 * Definition.  n = filter_length, a power of two in [VITS_DENOISE_MIN_FILTER, VITS_DENOISE_MAX_FILTER] (0 where an entry point says
 * so = 1024); n_overlap = 4, hop = n / 4; window w[i] = sin^2(pi i / n) (the periodic Hann), win_length = n.  For an item
 * x[0 .. len) (denoiser.py:62-68):
 *   1. pad n/2 on both sides by reflection (torch.stft, center = True); needs len >= n/2 + 1
 *   2. F = 1 + floor(len / hop) frames, frame f = xp[f hop .. f hop + n) * w, X_f = rFFT(frame f)             (n/2 + 1 bins)
 *   3. X'_f[k] = X_f[k] * max(|X_f[k]| - strength * bias[k], 0) / |X_f[k]|, and 0 where |X_f[k]| = 0
 *      (the reference's magnitude / atan2 / cos / sin round trip without the trigonometry; continuous in X)
 *   4. y_f = irFFT(X'_f) * w; the frames are overlap-added, divided by the overlap-added w^2, and n/2 is dropped from both ends
 *      (torch.istft): hop * (F - 1) = hop * floor(len / hop) output samples
 * bias[k] (denoiser.py:22-23,56-60, mode "zeros") = |X_0[k]| of the vocoder's own output for an all-zero mel [channels, 88]: frame 0
 * only, the reflect-padded frame centred on sample 0.
 *
 * Arithmetic: fp32; twiddles, window and 1 / sum w^2 come from tables computed on the host in double and rounded once.  Every output
 * sample sums its (at most four) frames in ascending frame order: no atomics, the same call twice gives the same bits.
 */
#ifndef VITS_DENOISE_H
#define VITS_DENOISE_H

#include "stts_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITS_DENOISE_MIN_FILTER 64
#define VITS_DENOISE_MAX_FILTER 1024
#define VITS_DENOISE_BIAS_FRAMES 88 /* frames of the all-zero mel the bias is taken from (denoiser.py:23) */

/* stts_synth_opts.flags (include/stts_mi355.h): denoise the audio with opts->denoiser_strength and opts->denoiser_filter_length
 * (0 = 1024).  The two fields were appended to the struct with this flag and are read only when it is set, the rule item_seeds
 * follows.  Honoured by stts_synthesize, stts_synthesize_batch (each item from its own length, as if alone) and stts_stream_open,
 * in the reference's order: decode, clamp to [-1, 1], denoise.  The vocoder's hop_length must be a multiple of hop
 * (VITS_ERR_UNSUPPORTED with both values otherwise), so output lengths are unchanged.  An utterance shorter than n/2 + 1 samples
 * is returned undenoised: the reference would raise in the reflection padding, and a server must not fail a one-phoneme request.
 * Strength < 0 is VITS_ERR_ARG. */
#define STTS_FLAG_DENOISE 2

/* bias float [n/2 + 1] of a vocoder-only model: decodes the all-zero input [decoder input channels, VITS_DENOISE_BIAS_FRAMES] and
 * takes the magnitudes of frame 0.  Computed once per filter_length and cached in the model (under a lock of the model's own).
 * cap = floats `bias` can hold (VITS_ERR_ARG when too small).  A decoder that takes speaker conditioning is refused
 * (VITS_ERR_UNSUPPORTED naming gin_channels): its bias would depend on the speaker. */
int vits_denoise_bias(vits_model* vocoder, int32_t filter_length, float* bias, int64_t cap);

/* Kernel-level parity door (as vits_op_resample is for the resampler), host buffers: x float [B, N], lengths int64 [B] with
 * n/2 + 1 <= lengths[b] <= N, bias float [n/2 + 1] (any values), y float [B, hop * floor(N / hop)].  Item b is denoised from
 * x[b, 0 : lengths[b]) only -- samples at and beyond lengths[b] are never read -- and y[b, j] is exactly 0 for
 * j >= hop * floor(lengths[b] / hop).  VITS_ERR_ARG for a length out of range or strength < 0 (the value is named);
 * VITS_ERR_UNSUPPORTED, naming the value, for a filter_length that is not a power of two in [64, 1024]. */
int vits_op_denoise(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, const float* bias, int32_t filter_length,
                    float strength, float* y);

/* vits_stream_open_latent with the denoiser behind every chunk (stts_stream_open uses it when STTS_FLAG_DENOISE is set; strength 0
 * still runs the transform).  filter_length 0 = 1024.  The decode windows carry ceil(n / hop_length) more halo frames on each side,
 * so every frame of the transform reads exactly decoded samples, and reflection happens only at the true ends of the utterance,
 * which the windows reach.  Chunk sizes and *total_samples are those of vits_stream_open_latent; the concatenated chunks equal the
 * one-shot result.  An utterance shorter than n/2 + 1 samples streams undenoised.  No entry point takes both a denoiser and another
 * sample rate, so there is nothing to refuse at this level: the Python wrappers (VitsModel.stream_latent, SttsSession.run_stream)
 * refuse the combination themselves, as VitsError with the code of VITS_ERR_UNSUPPORTED. */
int vits_stream_open_latent_denoise(vits_model* m, const float* z, int32_t T_y, int32_t chunk_frames, uint32_t flags, float strength,
                                    int32_t filter_length, vits_stream** out, int64_t* total_samples);

#ifdef __cplusplus
}
#endif
#endif /* VITS_DENOISE_H */
