// denoise.hip.h -- the vocoder-bias denoiser (include/vits_denoise.h): STFT, per-bin gain and iSTFT behind the decoder.
// Part of the ONE translation unit engine.hip (included there, after the resampler).
//
// Two launches per request:
//   denoise_frames_kernel  one wave per frame, DN_FPB frames per workgroup: the frame is read with reflect indexing, the item's own
//                          length and the window; the real n-point transform runs as an M = n/2 point complex FFT in LDS (Stockham
//                          autosort, radix-4 passes and one radix-2 pass when log2 M is odd); the half-size spectrum is unpacked to
//                          the bins k and M - k in registers, the gain is applied, the pair is packed back (conjugated, so the
//                          SAME forward passes invert it) and the windowed frame goes to a scratch [frames, n]
//   denoise_ola_kernel     a gather: every output sample sums its four or fewer frames in ascending frame order and multiplies by a
//                          host-computed 1 / sum w^2 (three rows: the first hop samples miss frame -1, the last hop miss frame F)
// LDS: re and im planes apart (4-byte accesses), ping and pong, index i stored at i + (i >> 4).  Reads of a pass are contiguous
// across the lanes; its writes go to 4 (j - k) + k + r Ns, a power-of-two stride that unpadded puts 4 lanes of a 32-lane group on
// one bank in the Ns = 1 and Ns = 4 passes; with the padding no pass has more than 2 (worked out from the bank rule for every
// pass of M = 32 .. 512, not measured).  4 x 544 floats = 8.5 KiB per 1024-sample frame, 34 KiB per workgroup.
#pragma once
#include "../../include/vits_denoise.h"

#define DN_FPB 4                        // frames (= waves) per workgroup
#define DN_MAXM (VITS_DENOISE_MAX_FILTER / 2)
#define DN_PAD(i) ((i) + ((i) >> 4))
#define DN_PLANE (DN_MAXM + DN_MAXM / 16)

// sample p of the reflect-padded item (p counts from the start of the padding): x[b] holds samples x_off .. x_off + x_n of it
__device__ __forceinline__ float dn_load(const float* __restrict__ xb, long long p, int M, long long len, long long x_off, long long x_n) {
  long long k = p - M;
  if (k < 0) k = -k;
  if (k >= len) k = 2 * (len - 1) - k;
  const long long kk = k - x_off;
  return (k >= 0 && k < len && kk >= 0 && kk < x_n) ? xb[kk] : 0.f;
}

// forward M-point FFT of the wave's planes (a -> result left in a; b is the other buffer).  tw is the n-point table
// tw[t] = exp(-2 pi i t / n), n = 2 M.  Every thread of the workgroup calls it (the barriers are the workgroup's).
__device__ __forceinline__ void dn_fft(float*& ar, float*& ai, float*& br, float*& bi, int M, int log2m, const float2* __restrict__ tw, int t) {
  int Ns = 1, rem = log2m;
  while (rem >= 2) {
    const int Q = M >> 2;
    for (int j = t; j < Q; j += 64) {
      const int k = j & (Ns - 1);
      const int ts = (M / (4 * Ns)) * 2 * k;  // 3 ts < 3 n / 4
      const float2 w1 = tw[ts], w2 = tw[2 * ts], w3 = tw[3 * ts];
      const float x0r = ar[DN_PAD(j)], x0i = ai[DN_PAD(j)];
      const float x1r = ar[DN_PAD(j + Q)], x1i = ai[DN_PAD(j + Q)];
      const float x2r = ar[DN_PAD(j + 2 * Q)], x2i = ai[DN_PAD(j + 2 * Q)];
      const float x3r = ar[DN_PAD(j + 3 * Q)], x3i = ai[DN_PAD(j + 3 * Q)];
      const float v1r = x1r * w1.x - x1i * w1.y, v1i = x1r * w1.y + x1i * w1.x;
      const float v2r = x2r * w2.x - x2i * w2.y, v2i = x2r * w2.y + x2i * w2.x;
      const float v3r = x3r * w3.x - x3i * w3.y, v3i = x3r * w3.y + x3i * w3.x;
      const float a0r = x0r + v2r, a0i = x0i + v2i, a1r = x0r - v2r, a1i = x0i - v2i;
      const float a2r = v1r + v3r, a2i = v1i + v3i;
      const float a3r = v1i - v3i, a3i = -(v1r - v3r);  // -i (v1 - v3)
      const int j0 = ((j - k) << 2) + k;
      br[DN_PAD(j0)] = a0r + a2r;          bi[DN_PAD(j0)] = a0i + a2i;
      br[DN_PAD(j0 + Ns)] = a1r + a3r;     bi[DN_PAD(j0 + Ns)] = a1i + a3i;
      br[DN_PAD(j0 + 2 * Ns)] = a0r - a2r; bi[DN_PAD(j0 + 2 * Ns)] = a0i - a2i;
      br[DN_PAD(j0 + 3 * Ns)] = a1r - a3r; bi[DN_PAD(j0 + 3 * Ns)] = a1i - a3i;
    }
    __syncthreads();
    float* s = ar; ar = br; br = s;
    s = ai; ai = bi; bi = s;
    Ns <<= 2;
    rem -= 2;
  }
  if (rem) {
    const int H = M >> 1;
    for (int j = t; j < H; j += 64) {
      const int k = j & (Ns - 1);
      const float2 w1 = tw[k * (M / Ns)];
      const float x0r = ar[DN_PAD(j)], x0i = ai[DN_PAD(j)];
      const float x1r = ar[DN_PAD(j + H)], x1i = ai[DN_PAD(j + H)];
      const float v1r = x1r * w1.x - x1i * w1.y, v1i = x1r * w1.y + x1i * w1.x;
      const int j0 = ((j - k) << 1) + k;
      br[DN_PAD(j0)] = x0r + v1r;      bi[DN_PAD(j0)] = x0i + v1i;
      br[DN_PAD(j0 + Ns)] = x0r - v1r; bi[DN_PAD(j0 + Ns)] = x0i - v1i;
    }
    __syncthreads();
    float* s = ar; ar = br; br = s;
    s = ai; ai = bi; bi = s;
  }
}

__device__ __forceinline__ float dn_gain(float re, float im, float sb) {
  const float mag = sqrtf(re * re + im * im);
  return mag > 0.f ? fmaxf(mag - sb, 0.f) / mag : 0.f;
}

// Frames [f_begin, f_begin + f_count) of every item; wave w of workgroup blockIdx.x owns frame f_begin + blockIdx.x * DN_FPB + w.
//   x        item b's input at x + b * x_bstride; x[j] is sample x_off + j, and only 0 <= j < x_n is ever read
//   len      valid samples of item b: len_frames[b] * len_mul (len_frames null: len_mul itself); an item shorter than n/2 + 1 has
//            no frames (denoise_ola_kernel passes it through)
//   out      mag_only 0: the windowed inverse frames, out[b * out_bstride + (f - f_begin) * n + i]
//            mag_only 1: |X_f[k]|, out[b * out_bstride + (f - f_begin) * (n/2 + 1) + k]  (the bias; no gain, no inverse)
__global__ __launch_bounds__(64 * DN_FPB) void denoise_frames_kernel(const float* __restrict__ x, long long x_bstride, long long x_off,
                                                                     long long x_n, const int* __restrict__ len_frames, long long len_mul,
                                                                     const float* __restrict__ win, const float2* __restrict__ tw,
                                                                     const float* __restrict__ bias, float strength, int n, int log2m,
                                                                     long long f_begin, int f_count, float* __restrict__ out,
                                                                     long long out_bstride, int mag_only) {
  __shared__ float lds[DN_FPB][4][DN_PLANE];
  const int M = n >> 1, hop = n >> 2;
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  const int b = blockIdx.y;
  const long long len = len_frames ? len_frames[b] * len_mul : len_mul;
  const long long F = len >= M + 1 ? 1 + len / hop : 0;
  const long long fi = (long long)blockIdx.x * DN_FPB + wv;  // index in the scratch
  const long long f = f_begin + fi;
  if (f_begin + (long long)blockIdx.x * DN_FPB >= F) return;  // the whole workgroup is beyond the item: uniform exit
  const bool valid = fi < f_count && f < F;
  float *ar = lds[wv][0], *ai = lds[wv][1], *br = lds[wv][2], *bi = lds[wv][3];
  const float* xb = x + (long long)b * x_bstride;
  for (int m = t; m < M; m += 64) {
    float v0 = 0.f, v1 = 0.f;
    if (valid) {
      const long long p = f * hop + 2 * m;
      v0 = dn_load(xb, p, M, len, x_off, x_n) * win[2 * m];
      v1 = dn_load(xb, p + 1, M, len, x_off, x_n) * win[2 * m + 1];
    }
    ar[DN_PAD(m)] = v0;
    ai[DN_PAD(m)] = v1;
  }
  __syncthreads();
  dn_fft(ar, ai, br, bi, M, log2m, tw, t);
  // Z (in a) -> the bins k and kp = M - k of the real transform: X[k] = E + W^k O, X[kp] = conj(E - W^k O), with
  // E = (Z[k] + conj Z[kp]) / 2, O = -i (Z[k] - conj Z[kp]) / 2, W = exp(-2 pi i / n), Z[M] = Z[0]
  float* ob = out + (long long)b * out_bstride;
  for (int k = t; k <= (M >> 1); k += 64) {
    const int kp = M - k, kq = kp & (M - 1);
    const float zkr = ar[DN_PAD(k)], zki = ai[DN_PAD(k)], zpr = ar[DN_PAD(kq)], zpi = ai[DN_PAD(kq)];
    const float2 w = tw[k];
    const float er = 0.5f * (zkr + zpr), ei = 0.5f * (zki - zpi);
    const float o_r = 0.5f * (zki + zpi), o_i = -0.5f * (zkr - zpr);
    const float tr = w.x * o_r - w.y * o_i, ti = w.x * o_i + w.y * o_r;
    float xkr = er + tr, xki = ei + ti, xpr = er - tr, xpi = -(ei - ti);
    if (mag_only) {
      if (valid) {
        ob[fi * (M + 1) + k] = sqrtf(xkr * xkr + xki * xki);
        ob[fi * (M + 1) + kp] = sqrtf(xpr * xpr + xpi * xpi);
      }
      continue;
    }
    const float gk = dn_gain(xkr, xki, strength * bias[k]), gp = dn_gain(xpr, xpi, strength * bias[kp]);
    xkr *= gk; xki *= gk; xpr *= gp; xpi *= gp;
    // back: Z'[k] = E2 + i O2, Z'[kp] = conj(E2) + i conj(O2), E2 = (X'[k] + conj X'[kp]) / 2, O2 = (X'[k] - conj X'[kp]) / 2 * conj(W^k);
    // stored conjugated: the inverse transform is conj(FFT(conj Z')) / M
    const float e2r = 0.5f * (xkr + xpr), e2i = 0.5f * (xki - xpi);
    const float dr = 0.5f * (xkr - xpr), di = 0.5f * (xki + xpi);
    const float o2r = dr * w.x + di * w.y, o2i = di * w.x - dr * w.y;
    br[DN_PAD(k)] = e2r - o2i;
    bi[DN_PAD(k)] = -(e2i + o2r);
    if (k > 0 && kp != k) {
      br[DN_PAD(kp)] = e2r + o2i;
      bi[DN_PAD(kp)] = -(o2r - e2i);
    }
  }
  if (mag_only) return;
  __syncthreads();
  { float* s = ar; ar = br; br = s; s = ai; ai = bi; bi = s; }
  dn_fft(ar, ai, br, bi, M, log2m, tw, t);
  if (!valid) return;
  const float inv_m = 1.0f / (float)M;
  float2* of = reinterpret_cast<float2*>(ob + fi * n);  // (n and every stride are even: 8-byte aligned)
  for (int m = t; m < M; m += 64)
    of[m] = make_float2(ar[DN_PAD(m)] * inv_m * win[2 * m], -ai[DN_PAD(m)] * inv_m * win[2 * m + 1]);
}

// Outputs [n_begin, n_begin + n_count) of every item from the frames scratch (fr[b * fr_bstride + (f - f_begin) * n + i]).
// y[b * y_bstride + j] is output n_begin + j: exactly 0 at and beyond hop * floor(len / hop); an item shorter than n/2 + 1 samples
// is copied from x (same addressing as denoise_frames_kernel) and is 0 beyond its length.
__global__ __launch_bounds__(256) void denoise_ola_kernel(const float* __restrict__ fr, long long fr_bstride, long long f_begin,
                                                          const float* __restrict__ x, long long x_bstride, long long x_off, long long x_n,
                                                          const int* __restrict__ len_frames, long long len_mul,
                                                          const float* __restrict__ inv_env, int n, float* __restrict__ y,
                                                          long long y_bstride, long long n_begin, long long n_count) {
  const int b = blockIdx.y;
  const long long jo = (long long)blockIdx.x * 256 + threadIdx.x;
  if (jo >= n_count) return;
  const long long j = n_begin + jo;
  const int M = n >> 1, hop = n >> 2;
  const long long len = len_frames ? len_frames[b] * len_mul : len_mul;
  float v = 0.f;
  if (len >= M + 1) {
    const long long F = 1 + len / hop;
    if (j < hop * (F - 1)) {
      const long long p = j + M, fl = p / hop;
      const int r = (int)(p - fl * hop);
      const int region = fl < 3 ? 0 : (fl >= F ? 2 : 1);
      const float* fb = fr + (long long)b * fr_bstride;
      float acc = 0.f;
      for (int d = 3; d >= 0; --d) {
        const long long f = fl - d;
        if (f >= 0 && f < F && f >= f_begin) acc += fb[(f - f_begin) * n + r + d * hop];
      }
      v = acc * inv_env[region * hop + r];
    }
  } else if (j < len) {
    const long long kk = j - x_off;
    if (kk >= 0 && kk < x_n) v = x[(long long)b * x_bstride + kk];
  }
  y[(long long)b * y_bstride + jo] = v;
}

// ---- host tables, cached per (device, filter_length) ----------------------------------------------------------------------
struct DenoiseTab {
  int n = 0, log2m = 0;
  float* d_win = nullptr;    // [n]
  float2* d_tw = nullptr;    // [n]  exp(-2 pi i t / n)
  float* d_env = nullptr;    // [3][hop]  1 / sum w^2: head (frame -1 missing), interior, tail (frame F missing)
};
static std::mutex g_dn_mu;
static std::map<std::pair<int, int>, DenoiseTab> g_dn_tabs;  // never evicted: at most five filter lengths per device

// 0 -> 1024; anything but a power of two in [64, 1024] is refused by name
static int denoise_filter_arg(int32_t filter_length, int* n) {
  const int v = filter_length == 0 ? VITS_DENOISE_MAX_FILTER : filter_length;
  if (v < VITS_DENOISE_MIN_FILTER || v > VITS_DENOISE_MAX_FILTER || (v & (v - 1)))
    return fail(VITS_ERR_UNSUPPORTED, "denoise: filter_length %d is not a power of two in [%d, %d]", filter_length, VITS_DENOISE_MIN_FILTER, VITS_DENOISE_MAX_FILTER);
  *n = v;
  return VITS_OK;
}

// Uploads on first use (hipMalloc + synchronous copies: call it outside stream capture).
static int denoise_get(int device, int n, const DenoiseTab** out) {
  std::lock_guard<std::mutex> g(g_dn_mu);
  const auto key = std::make_pair(device, n);
  auto it = g_dn_tabs.find(key);
  if (it != g_dn_tabs.end()) { *out = &it->second; return VITS_OK; }
  DenoiseTab T;
  T.n = n;
  for (int m = n >> 1; m > 1; m >>= 1) ++T.log2m;
  const int hop = n / 4;
  std::vector<float> win(n), env((size_t)3 * hop);
  std::vector<float2> tw(n);
  std::vector<double> w2(n);
  for (int i = 0; i < n; ++i) {
    const double s = sin(M_PI * (double)i / (double)n), a = 2.0 * M_PI * (double)i / (double)n;
    win[i] = (float)(s * s);
    w2[i] = (s * s) * (s * s);
    tw[i] = make_float2((float)cos(a), (float)-sin(a));
  }
  for (int r = 0; r < hop; ++r) {
    env[r] = (float)(1.0 / (w2[r] + w2[r + hop] + w2[r + 2 * hop]));
    env[hop + r] = (float)(1.0 / (w2[r] + w2[r + hop] + w2[r + 2 * hop] + w2[r + 3 * hop]));
    env[2 * hop + r] = (float)(1.0 / (w2[r + hop] + w2[r + 2 * hop] + w2[r + 3 * hop]));
  }
  HIP_TRY(hipSetDevice(device));
  char* d = nullptr;
  const size_t b_win = sizeof(float) * n, b_tw = sizeof(float2) * n, b_env = sizeof(float) * 3 * hop;
  if (hipMalloc((void**)&d, b_win + b_tw + b_env) != hipSuccess) return fail(VITS_ERR_NOMEM, "denoise: table alloc failed");
  T.d_tw = reinterpret_cast<float2*>(d);
  T.d_win = reinterpret_cast<float*>(d + b_tw);
  T.d_env = reinterpret_cast<float*>(d + b_tw + b_win);
  if (hipMemcpy(T.d_tw, tw.data(), b_tw, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(T.d_win, win.data(), b_win, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(T.d_env, env.data(), b_env, hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(d);
    return fail(VITS_ERR_DEVICE, "denoise: table upload failed");
  }
  *out = &g_dn_tabs.emplace(key, T).first->second;
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
static void denoise_launch(hipStream_t stream, const DenoiseTab& T, const float* x, long long x_bstride, long long x_off, long long x_n,
                           const int* len_frames, long long len_mul, int B, const float* d_bias, float strength, float* scratch,
                           long long scratch_bstride, float* y, long long y_bstride, long long n_begin, long long n_count) {
  if (n_count <= 0 || B <= 0) return;
  long long f_begin = 0, f_count = 0;
  denoise_frame_span(T.n, n_begin, n_count, &f_begin, &f_count);
  hipLaunchKernelGGL(denoise_frames_kernel, dim3((unsigned)cdiv((int)f_count, DN_FPB), B), dim3(64 * DN_FPB), 0, stream, x, x_bstride, x_off, x_n,
                     len_frames, len_mul, T.d_win, T.d_tw, d_bias, strength, T.n, T.log2m, f_begin, (int)f_count, scratch, scratch_bstride, 0);
  hipLaunchKernelGGL(denoise_ola_kernel, dim3((unsigned)((n_count + 255) / 256), B), dim3(256), 0, stream, scratch, scratch_bstride, f_begin, x,
                     x_bstride, x_off, x_n, len_frames, len_mul, T.d_env, T.n, y, y_bstride, n_begin, n_count);
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
    const DenoiseTab* T = nullptr;
    TRY(denoise_get(m->device, n, &T));
    std::vector<float> z((size_t)hp.inter_channels * Tb, 0.f), audio((size_t)S), mag((size_t)M + 1);
    TRY(vits_stage_decoder(m, z.data(), 1, Tb, nullptr, audio.data(), nullptr));
    OpDoor d("denoise: bias", m->device);
    float* dx = d.up(audio.data(), (size_t)(M + 1));  // frame 0 reads samples 0 .. n/2 only
    float* db = d.dev<float>((size_t)(M + 1));
    if (d.ok())
      hipLaunchKernelGGL(denoise_frames_kernel, dim3(1, 1), dim3(64 * DN_FPB), 0, nullptr, dx, 0, 0, (long long)(M + 1), nullptr, S, T->d_win, T->d_tw,
                         nullptr, 0.f, n, T->log2m, 0, 1, db, 0, 1);
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
static int denoise_prepare(vits_model* v, float strength, int32_t filter_length, const DenoiseTab** T, const float** d_bias) {
  int n = 0;
  TRY(denoise_filter_arg(filter_length, &n));
  if (!(strength >= 0.f)) return fail(VITS_ERR_ARG, "denoise: strength %g is negative", (double)strength);
  if (v->hp.hop_length % (n / 4)) return fail(VITS_ERR_UNSUPPORTED, "denoise: the vocoder's hop_length %d is not a multiple of the denoiser's hop %d (filter_length %d)", v->hp.hop_length, n / 4, n);
  TRY(denoise_get(v->device, n, T));
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
  const DenoiseTab* T = nullptr;
  TRY(denoise_get(device, n, &T));
  OpDoor d("denoise", device);
  const long long Ny = (long long)hop * (N / hop);
  const size_t sc = denoise_scratch_elems(n, Ny);
  float* dx = d.up(x, (size_t)B * N);
  float* db = d.up(bias, (size_t)(M + 1));
  int* dl = d.up(len32.data(), B);
  float* ds = d.dev<float>(B * sc);
  float* dy = d.out<float>((size_t)B * Ny);
  if (d.ok()) denoise_launch(nullptr, *T, dx, N, 0, N, dl, 1, B, db, strength, ds, (long long)sc, dy, Ny, 0, Ny);
  d.finish();
  d.down(y, dy, (size_t)B * Ny);
  return d.rc();
}
