// denoise.hip.h -- the vocoder-bias denoiser (include/vits_denoise.h): STFT, per-bin gain and iSTFT behind the decoder.
// Part of the ONE translation unit engine.hip (included there, after stft.hip.h, whose frame transform, LDS layout and tables it uses).
//
// Two launches per request:
//   denoise_frames_kernel  one wave per frame: load, transform and unpack (stft.hip.h), the gain of each bin from the bias, pack,
//                          invert, the windowed frame to a scratch [frames, n]; mag_only: the magnitudes instead (the bias itself)
//   denoise_ola_kernel     the gather of stft.hip.h over a span of outputs; an item too short to have frames is copied from x
#pragma once
#include "../../include/vits_denoise.h"

__device__ __forceinline__ float dn_gain(float re, float im, float sb) {
  const float mag = sqrtf(re * re + im * im);
  return mag > 0.f ? fmaxf(mag - sb, 0.f) / mag : 0.f;
}

// Frames [f_begin, f_begin + f_count) of every item; wave w of workgroup blockIdx.x owns frame f_begin + blockIdx.x * SF_FPB + w.
//   x        item b's input at x + b * x_bstride; x[j] is sample x_off + j, and only 0 <= j < x_n is ever read
//   len      valid samples of item b: it.len_in(b) (ragged.hip.h); an item shorter than n/2 + 1 has
//            no frames (denoise_ola_kernel passes it through)
//   out      mag_only 0: the windowed inverse frames, out[b * out_bstride + (f - f_begin) * n + i]
//            mag_only 1: |X_f[k]|, out[b * out_bstride + (f - f_begin) * (n/2 + 1) + k]  (the bias; no gain, no inverse)
__global__ __launch_bounds__(64 * SF_FPB) void denoise_frames_kernel(const float* __restrict__ x, long long x_bstride, long long x_off, long long x_n,
                                                                     const Items it, const float* __restrict__ win, const float2* __restrict__ tw,
                                                                     const float* __restrict__ bias, float strength, int n, int log2m,
                                                                     long long f_begin, int f_count, float* __restrict__ out, long long out_bstride,
                                                                     int mag_only) {
  __shared__ float lds[SF_FPB][4][SF_PLANE];
  const int M = n >> 1, hop = n >> 2;
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  const int b = blockIdx.y;
  const long long len = it.len_in(b);
  const long long F = len >= M + 1 ? 1 + len / hop : 0;
  const long long fi = (long long)blockIdx.x * SF_FPB + wv;  // index in the scratch
  const long long f = f_begin + fi;
  if (f_begin + (long long)blockIdx.x * SF_FPB >= F) return;  // the whole workgroup is beyond the item: uniform exit
  const bool valid = fi < f_count && f < F;
  float *ar = lds[wv][0], *ai = lds[wv][1], *br = lds[wv][2], *bi = lds[wv][3];
  const float* xb = x + (long long)b * x_bstride;
  sf_frame_load(xb, f * hop, M, len, x_off, x_n, win, valid, t, ar, ai);
  __syncthreads();
  sf_fft(ar, ai, br, bi, M, log2m, tw, t);
  float* ob = out + (long long)b * out_bstride;
  for (int k = t; k <= (M >> 1); k += 64) {
    const int kp = M - k;
    SfBins X = sf_unpack(ar, ai, tw, M, k);
    if (mag_only) {
      if (valid) {
        ob[fi * (M + 1) + k] = sqrtf(X.kr * X.kr + X.ki * X.ki);
        ob[fi * (M + 1) + kp] = sqrtf(X.pr * X.pr + X.pi * X.pi);
      }
      continue;
    }
    const float gk = dn_gain(X.kr, X.ki, strength * bias[k]), gp = dn_gain(X.pr, X.pi, strength * bias[kp]);
    X.kr *= gk; X.ki *= gk; X.pr *= gp; X.pi *= gp;
    sf_pack(br, bi, tw, M, k, X.kr, X.ki, X.pr, X.pi);
  }
  if (mag_only) return;
  __syncthreads();
  { float* s = ar; ar = br; br = s; s = ai; ai = bi; bi = s; }
  sf_fft(ar, ai, br, bi, M, log2m, tw, t);
  if (!valid) return;
  sf_frame_store(ar, ai, M, win, t, ob + fi * n);
}

// Outputs [n_begin, n_begin + n_count) of every item from the frames scratch (fr[b * fr_bstride + (f - f_begin) * n + i]).
// y[b * y_bstride + j] is output n_begin + j: exactly 0 at and beyond hop * floor(len / hop); an item shorter than n/2 + 1 samples
// is copied from x (same addressing as denoise_frames_kernel) and is 0 beyond its length.
__global__ __launch_bounds__(256) void denoise_ola_kernel(const float* __restrict__ fr, long long fr_bstride, long long f_begin,
                                                          const float* __restrict__ x, long long x_bstride, long long x_off, long long x_n,
                                                          const Items it, const float* __restrict__ inv_env, int n, float* __restrict__ y,
                                                          long long y_bstride, long long n_begin, long long n_count) {
  const int b = blockIdx.y;
  const long long jo = (long long)blockIdx.x * 256 + threadIdx.x;
  if (jo >= n_count) return;
  const long long j = n_begin + jo;
  const int M = n >> 1, hop = n >> 2;
  const long long len = it.len_in(b);
  float v = 0.f;
  if (len >= M + 1) {
    const long long F = 1 + len / hop;
    if (j < hop * (F - 1)) {
      const long long p = j + M, fl = p / hop;
      const int r = (int)(p - fl * hop);
      int region;
      const float acc = sf_ola_sum(fr + (long long)b * fr_bstride, fl, r, n, hop, F, f_begin, &region);
      v = acc * inv_env[region * hop + r];
    }
  } else if (j < len) {
    const long long kk = j - x_off;
    if (kk >= 0 && kk < x_n) v = x[(long long)b * x_bstride + kk];
  }
  y[(long long)b * y_bstride + jo] = v;
}

// 0 -> 1024; anything but a power of two in [64, 1024] is refused by name
static int denoise_filter_arg(int32_t filter_length, int* n) {
  const int v = filter_length == 0 ? VITS_DENOISE_MAX_FILTER : filter_length;
  if (v < VITS_DENOISE_MIN_FILTER || v > VITS_DENOISE_MAX_FILTER || (v & (v - 1)))
    return fail(VITS_ERR_UNSUPPORTED, "denoise: filter_length %d is not a power of two in [%d, %d]", filter_length, VITS_DENOISE_MIN_FILTER, VITS_DENOISE_MAX_FILTER);
  *n = v;
  return VITS_OK;
}

// frames that outputs [n_begin, n_begin + n_count) read: first frame and how many (an upper bound; frames beyond an item's own
// count are skipped by the kernels)
static void denoise_frame_span(int n, long long n_begin, long long n_count, long long* f_begin, long long* f_count) {
  const int M = n / 2, hop = n / 4;
  long long f0 = (n_begin + M) / hop - 3;
  if (f0 < 0) f0 = 0;
  const long long f1 = (n_begin + n_count - 1 + M) / hop;
  *f_begin = f0;
  *f_count = f1 - f0 + 1;
}
// floats of scratch one item needs for n_count outputs
static size_t denoise_scratch_elems(int n, long long n_count) { return (size_t)(n_count / (n / 4) + 5) * n; }

// Outputs [n_begin, n_begin + n_count) of B items on `stream` (capturable: no allocation, no synchronisation).  scratch holds
// B * scratch_bstride floats, scratch_bstride >= denoise_scratch_elems(n, n_count).  Arguments as for the two kernels.
static void denoise_launch(hipStream_t stream, const StftTab& T, const float* x, long long x_bstride, long long x_off, long long x_n, const Items& it,
                           int B, const float* d_bias, float strength, float* scratch, long long scratch_bstride, float* y, long long y_bstride,
                           long long n_begin, long long n_count) {
  if (n_count <= 0 || B <= 0) return;
  long long f_begin = 0, f_count = 0;
  denoise_frame_span(T.n, n_begin, n_count, &f_begin, &f_count);
  hipLaunchKernelGGL(denoise_frames_kernel, dim3((unsigned)cdiv((int)f_count, SF_FPB), B), dim3(64 * SF_FPB), 0, stream, x, x_bstride, x_off, x_n, it,
                     T.d_win, T.d_tw, d_bias, strength, T.n, T.log2m, f_begin, (int)f_count, scratch, scratch_bstride, 0);
  hipLaunchKernelGGL(denoise_ola_kernel, dim3((unsigned)((n_count + 255) / 256), B), dim3(256), 0, stream, scratch, scratch_bstride, f_begin, x,
                     x_bstride, x_off, x_n, it, T.d_env, T.n, y, y_bstride, n_begin, n_count);
}

// ---- the bias of a vocoder, cached in the model per filter_length -----------------------------------------------------------
// -> the device copy [n/2 + 1] (lives as long as the model) and, when asked, the host copy
static int denoise_bias_get(vits_model* m, int n, const float** d_bias, const std::vector<float>** h_bias) {
  std::lock_guard<std::mutex> g(m->dn_mu);
  auto it = m->dn_bias.find(n);
  if (it == m->dn_bias.end()) {
    const vits_hparams& hp = m->hp;
    if (m->cond_dec_off >= 0)
      return fail(VITS_ERR_UNSUPPORTED, "denoise: the decoder takes speaker conditioning (gin_channels %d): its bias would depend on the speaker", hp.gin_channels);
    const int Tb = VITS_DENOISE_BIAS_FRAMES, M = n / 2;
    const long long S = (long long)Tb * hp.hop_length;
    if (S < M + 1) return fail(VITS_ERR_UNSUPPORTED, "denoise: %d frames of hop_length %d are shorter than filter_length %d / 2 + 1", Tb, hp.hop_length, n);
    const StftTab* T = nullptr;
    TRY(stft_tab_get(m->device, n, &T));
    std::vector<float> z((size_t)hp.inter_channels * Tb, 0.f), audio((size_t)S), mag((size_t)M + 1);
    TRY(vits_stage_decoder(m, z.data(), 1, Tb, nullptr, audio.data(), nullptr));
    OpDoor d("denoise: bias", m->device);
    float* dx = d.up(audio.data(), (size_t)(M + 1));  // frame 0 reads samples 0 .. n/2 only
    float* db = d.dev<float>((size_t)(M + 1));
    if (d.ok()) hipLaunchKernelGGL(denoise_frames_kernel, dim3(1, 1), dim3(64 * SF_FPB), 0, nullptr, dx, 0, 0, (long long)(M + 1), Items{nullptr, S},
                                   T->d_win, T->d_tw, nullptr, 0.f, n, T->log2m, 0, 1, db, 0, 1);
    d.finish();
    d.down(mag.data(), db, (size_t)(M + 1));
    if (!d.ok()) return d.rc();
    d.bufs.release(db);  // the model's from here
    m->allocs.push_back(db);
    it = m->dn_bias.emplace(n, std::make_pair(std::move(mag), db)).first;
  }
  if (d_bias) *d_bias = it->second.second;
  if (h_bias) *h_bias = &it->second.first;
  return VITS_OK;
}

// what a denoising entry point of a vocoder needs: the filter length, hop_length a multiple of hop, the tables and the bias
static int denoise_prepare(vits_model* v, float strength, int32_t filter_length, const StftTab** T, const float** d_bias) {
  int n = 0;
  TRY(denoise_filter_arg(filter_length, &n));
  if (!(strength >= 0.f)) return fail(VITS_ERR_ARG, "denoise: strength %g is negative", (double)strength);
  if (v->hp.hop_length % (n / 4)) return fail(VITS_ERR_UNSUPPORTED, "denoise: the vocoder's hop_length %d is not a multiple of the denoiser's hop %d (filter_length %d)", v->hp.hop_length, n / 4, n);
  TRY(stft_tab_get(v->device, n, T));
  return denoise_bias_get(v, n, d_bias, nullptr);
}

// ---- entry points ----------------------------------------------------------------------------------------------------
int vits_denoise_bias(vits_model* m, int32_t filter_length, float* bias, int64_t cap) {
  if (!m || !bias) return fail(VITS_ERR_ARG, "denoise: bad argument");
  int n = 0;
  TRY(denoise_filter_arg(filter_length, &n));
  if (cap < n / 2 + 1) return fail(VITS_ERR_ARG, "denoise: bias capacity %lld < %d floats", (long long)cap, n / 2 + 1);
  const std::vector<float>* h = nullptr;
  TRY(denoise_bias_get(m, n, nullptr, &h));
  memcpy(bias, h->data(), sizeof(float) * h->size());
  return VITS_OK;
}

int vits_op_denoise(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, const float* bias, int32_t filter_length,
                    float strength, float* y) {
  if (!x || !lengths || !bias || !y || B <= 0 || B > 65535 || N <= 0 || N >= (1LL << 31)) return fail(VITS_ERR_ARG, "denoise: bad argument");
  int n = 0;
  TRY(denoise_filter_arg(filter_length, &n));
  if (!(strength >= 0.f)) return fail(VITS_ERR_ARG, "denoise: strength %g is negative", (double)strength);
  const int M = n / 2, hop = n / 4;
  std::vector<int> len32(B);
  for (int b = 0; b < B; ++b) {
    if (lengths[b] < M + 1) return fail(VITS_ERR_ARG, "denoise: length %lld of item %d is below filter_length / 2 + 1 = %d", (long long)lengths[b], b, M + 1);
    if (lengths[b] > N) return fail(VITS_ERR_ARG, "denoise: length %lld of item %d exceeds N = %lld", (long long)lengths[b], b, (long long)N);
    len32[b] = (int)lengths[b];
  }
  const StftTab* T = nullptr;
  TRY(stft_tab_get(device, n, &T));
  OpDoor d("denoise", device);
  const long long Ny = (long long)hop * (N / hop);
  const size_t sc = denoise_scratch_elems(n, Ny);
  float* dx = d.up(x, (size_t)B * N);
  float* db = d.up(bias, (size_t)(M + 1));
  int* dl = d.up(len32.data(), B);
  float* ds = d.dev<float>(B * sc);
  float* dy = d.out<float>((size_t)B * Ny);
  if (d.ok()) denoise_launch(nullptr, *T, dx, N, 0, N, Items{dl, 1}, B, db, strength, ds, (long long)sc, dy, Ny, 0, Ny);
  d.finish();
  d.down(y, dy, (size_t)B * Ny);
  return d.rc();
}
