/*
 * vits_resample.h — synthesis at the sample rate the caller asks for (server/tts_service.proto:15-28,87-88:
 * output_audio_spec.raw_audio.sample_rate_hertz), by a polyphase windowed-sinc resampler fused behind the decoder.
 *
 * An extension of the product library: the reference always sends the voice's native rate (server/tts_server.py:42-54), so the CPU
 * oracle has no counterpart and these entry points are checked against a float64 restatement of the definition below
 * (tests/resample_ref.py).  Same status codes and vits_last_error as include/vits_mi355.h; all are re-entrant.
 *
 * Definition.  rate_in = hparams.sampling_rate, g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g, s = min(1, L / M).
 * For an item of `len` input samples x[0 .. len), taken as zero outside that range:
 *     N_out = ceil(len * L / M)
 *     y[n]  = sum_k x[k] * h(n*M/L - k)                                   0 <= n < N_out
 *     h(t)  = c * sinc(c*t) * I0(beta * sqrt(1 - (t/Hw)^2)) / I0(beta)    for |t| <= Hw, else 0
 *     sinc(v) = sin(pi v)/(pi v),  c = rho * s,  Hw = Z / s,  Z = 16,  rho = 0.9,  beta = 10
 * Coefficients are computed on the host in double and rounded once to fp32; the accumulation is fp32.
 *
 * Phase table.  Output n has phase p = (n*M) mod L and position q = floor(n*M / L); with W = Z * max(L, M) (so Hw = W / L),
 * lo(p) = floor((W - p) / L) and hi(p) = floor((W + p) / L) it reads x[q - lo(p) .. q + hi(p)].  Row p of the table holds
 *     table[p][i] = h(lo(p) - i + p/L)          0 <= i < taps,   taps = max_p (lo(p) + hi(p) + 1)
 * (entries with |t| > Hw are 0), so y[n] = sum_i table[p][i] * x[q - lo(p) + i].  half_width_in = ceil(Hw) bounds both reaches.
 *
 * Accepted rates: rate_in / 4 <= rate_out <= 4 * rate_in and L * taps <= VITS_RESAMPLE_MAX_TABLE floats; anything else is
 * VITS_ERR_UNSUPPORTED with the values in the message.  rate_out == rate_in (or 0 where an entry point says so) is the identity and takes
 * the path of the entry point without a rate, untouched.
 */
#ifndef VITS_RESAMPLE_H
#define VITS_RESAMPLE_H

#include "vits_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITS_RESAMPLE_MAX_TABLE 65536 /* floats in a phase table */
#define VITS_RESAMPLE_TILE 256        /* consecutive outputs of one item that one workgroup of resample_kernel owns */

/* Host only (no device is touched): the geometry of rate_in -> rate_out.  Any out pointer may be NULL. */
int vits_resample_plan(int32_t rate_in, int32_t rate_out, int32_t* L, int32_t* M, int32_t* taps, int32_t* half_width_in);
/* Host only: the fp32 phase table [L][taps] as defined above; cap = floats `table` can hold (VITS_ERR_ARG when too small). */
int vits_resample_table(int32_t rate_in, int32_t rate_out, float* table, int64_t cap);

/* Kernel-level parity door (as vits_op_conv1d is for convs), host buffers: x float [B, N], lengths int64 [B] with
 * 0 <= lengths[b] <= N, y float [B, ceil(N*L/M)].  Item b is resampled from x[b, 0 : lengths[b]) only -- samples at and beyond
 * lengths[b] are never read and count as zero -- and y[b, n] is exactly 0 for n >= ceil(lengths[b]*L/M).  rate_out == rate_in copies. */
int vits_op_resample(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate_in, int32_t rate_out,
                     float* y);

/* vits_synthesize / vits_synthesize_pcm16 at `sample_rate` Hz (0 or hparams.sampling_rate: exactly those calls).  *out_samples and
 * out_lengths are in OUTPUT samples: out_lengths[b] = ceil(frames[b] * hop_length * L / M).  Item b equals vits_op_resample of the
 * native-rate output of the same call cut at its own length, in padded and in solo batches.  At int16 output the resampler takes the
 * place of the conversion kernel (same scale, clip and truncating cast), so a request at another rate costs no extra launch; the float
 * output costs one. */
int vits_synthesize_rate(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t T_x, const float* scales,
                         const int64_t* sid, const vits_synth_opts* opts, int32_t sample_rate,
                         float** out_audio, int64_t* out_samples, int64_t* out_lengths);
int vits_synthesize_pcm16_rate(vits_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t T_x, const float* scales,
                               const int64_t* sid, const vits_synth_opts* opts, float pcm_scale, int32_t sample_rate,
                               int16_t** out_pcm, int64_t* out_samples, int64_t* out_lengths);

/* vits_stream_open / vits_stream_open_latent at `sample_rate` Hz (0 = native; the plain opens call these with 0).
 * *total_samples = ceil(T_y * hop_length * L / M).  A chunk that covers input samples [a, b) returns the outputs
 * ceil(a*L/M) <= n < ceil(b*L/M): chunk sizes vary by one sample, at most ceil(chunk_frames * hop_length * L / M) + 1, and the last
 * chunk ends at total_samples; vits_stream_next checks `capacity` against the chunk's own count.  The concatenated chunks equal
 * vits_synthesize_rate: the stream's decode windows carry ceil(half_width_in / hop_length) more halo frames each side, so the filter
 * reads exactly decoded samples only, and zeros beyond the end of the utterance. */
int vits_stream_open_rate(vits_model* m, const int64_t* ids, int32_t T_x, const float* scales, int64_t sid, const vits_synth_opts* opts,
                          int32_t chunk_frames, int32_t sample_rate, vits_stream** out, int64_t* total_samples);
int vits_stream_open_latent_rate(vits_model* m, const float* z, int32_t T_y, int32_t chunk_frames, uint32_t flags, int32_t sample_rate,
                                 vits_stream** out, int64_t* total_samples);

#ifdef __cplusplus
}
#endif
#endif /* VITS_RESAMPLE_H */
