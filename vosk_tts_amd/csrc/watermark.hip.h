// watermark.hip.h -- the keyed audio watermark (include/vits_watermark.h): the embed stage of the output tail and the detector.
// Part of the ONE translation unit engine.hip (included there, behind stft.hip.h and loudness.hip.h, in front of out_tail.hip.h).
//
// Embed, two launches (the frame transform of stft.hip.h at n = 1024: its device functions, LDS layout and StftTab):
//   wm_frames_kernel   one wave per frame: load, transform and unpack, the chip of each bin computed in registers from f and k, pack,
//                      inverse, the windowed frame to a scratch [frames, n]
//   wm_ola_kernel      the gather of stft.hip.h; behind H floor(len / H) it copies x, beyond len it writes 0; OUT = int16_t: pcm16_of
// Detect, three launches:
//   wm_lb_kernel       the same load, transform and unpack at hop 128: band magnitudes to the wave's free LDS plane, their maximum
//                      by a wave reduction, the four-bin log mean before the store: Lb [F', 96] floats
//   wm_score_kernel    one workgroup per (item, offset index): 16 tile rows at a time, T of a row of every q in LDS as doubles
//                      [16][96], D and the running G of the thread's six (q, j) in registers, then the two sums in a fixed tree
//   wm_argmax_kernel   one thread per item over its 128 scores
// LDS of wm_score_kernel: thread id -> (q, j) = (id / 96, id % 96) and T is stored at q * 96 + j = id, so the lanes of a wave read
// consecutive doubles for T[id], T[id - 1] and T[id + 1] alike: the 32 lanes of a half-wave cover 256 contiguous bytes, the 64 banks
// of an 8-byte read once each, and the 96-wide rows need no padding BECAUSE the mapping is linear in id (lanes walking down a column
// of [16][96] doubles would all meet on one bank pair).  The band magnitudes of wm_lb_kernel are read four in a row per lane (stride 4
// dwords, 4 lanes to a bank): 384 reads per frame next to the FFT's 9 passes, left as it is.
// Nothing waits between workgroups; there are no atomics.
#pragma once
#include "../../include/vits_watermark.h"

#define WM_N VITS_WATERMARK_FRAME
#define WM_M (WM_N / 2)
#define WM_H (WM_N / 4)
#define WM_LOG2M 9
#define WM_LO VITS_WATERMARK_BIN_LO
#define WM_HI VITS_WATERMARK_BIN_HI
#define WM_G VITS_WATERMARK_GROUPS
#define WM_Q VITS_WATERMARK_ROWS
#define WM_DH VITS_WATERMARK_DETECT_HOP
#define WM_SCORE_THREADS 256
static_assert(WM_N <= SF_N && (1 << WM_LOG2M) == WM_M, "the watermark runs on the frame transform of stft.hip.h");
static_assert((WM_HI - WM_LO) == 4 * WM_G && (WM_Q * WM_G) % WM_SCORE_THREADS == 0, "96 groups of 4 bins; whole (q, j) per thread");

__host__ __device__ __forceinline__ uint32_t wm_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
// the chip of tile row q, group j under mk = wm_mix(key): true = +1
__host__ __device__ __forceinline__ bool wm_chip(uint32_t mk, int q, int j) { return (wm_mix(mk ^ (uint32_t)(WM_G * q + j + 1)) & 1u) != 0; }
// the gain of bin k in a frame of tile row q: gp = fp32(1 + a), gm = fp32(1 - a)
__device__ __forceinline__ float wm_bin_gain(uint32_t mk, int q, int k, float gp, float gm) {
  if (k < WM_LO || k >= WM_HI) return 1.f;
  return wm_chip(mk, q, (k - WM_LO) >> 2) ? gp : gm;
}

// The marked, windowed frames of every item: wave w of workgroup blockIdx.x owns frame f = blockIdx.x * SF_FPB + w.
//   x      item b at x + b * x_bstride, samples [0, len), len = ld_len(..) (loudness.hip.h: the item as returned, at most N)
//   out    out[b * out_bstride + f * n + i]; an item shorter than n/2 + 1 has no frames (wm_ola_kernel passes it through)
__global__ __launch_bounds__(64 * SF_FPB) void wm_frames_kernel(const float* __restrict__ x, long long x_bstride, long long N,
                                                                const int* __restrict__ len_frames, long long len_mul, int L, int Mr,
                                                                const float* __restrict__ win, const float2* __restrict__ tw, uint32_t mk,
                                                                float gp, float gm, float* __restrict__ out, long long out_bstride) {
  __shared__ float lds[SF_FPB][4][SF_PLANE];
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  const int b = blockIdx.y;
  const long long len = ld_len(len_frames, len_mul, L, Mr, N, b);
  const long long F = len >= WM_M + 1 ? 1 + len / WM_H : 0;
  const long long f = (long long)blockIdx.x * SF_FPB + wv;
  if ((long long)blockIdx.x * SF_FPB >= F) return;  // the whole workgroup is beyond the item: uniform exit
  const bool valid = f < F;
  float *ar = lds[wv][0], *ai = lds[wv][1], *br = lds[wv][2], *bi = lds[wv][3];
  const float* xb = x + (long long)b * x_bstride;
  sf_frame_load(xb, f * WM_H, WM_M, len, 0, len, win, valid, t, ar, ai);
  __syncthreads();
  sf_fft(ar, ai, br, bi, WM_M, WM_LOG2M, tw, t);
  const int q = (int)((f >> 2) & (WM_Q - 1));
  for (int k = t; k <= (WM_M >> 1); k += 64) {  // unpack, the chip's gain, pack
    SfBins X = sf_unpack(ar, ai, tw, WM_M, k);
    const float gk = wm_bin_gain(mk, q, k, gp, gm), gq = wm_bin_gain(mk, q, WM_M - k, gp, gm);
    X.kr *= gk; X.ki *= gk; X.pr *= gq; X.pi *= gq;
    sf_pack(br, bi, tw, WM_M, k, X.kr, X.ki, X.pr, X.pi);
  }
  __syncthreads();
  { float* s = ar; ar = br; br = s; s = ai; ai = bi; bi = s; }
  sf_fft(ar, ai, br, bi, WM_M, WM_LOG2M, tw, t);
  if (!valid) return;
  sf_frame_store(ar, ai, WM_M, win, t, out + (long long)b * out_bstride + f * WM_N);
}

// y[b * y_bstride + j], 0 <= j < n_count: the overlap-added frames on [0, H floor(len / H)), x from there up to len, exactly 0 at and
// beyond len; an item shorter than n/2 + 1 samples is x.  OUT = int16_t: pcm16_of.
template <typename OUT>
__global__ __launch_bounds__(256) void wm_ola_kernel(const float* __restrict__ fr, long long fr_bstride, const float* __restrict__ x,
                                                     long long x_bstride, long long N, const int* __restrict__ len_frames, long long len_mul,
                                                     int L, int Mr, const float* __restrict__ inv_env, OUT* __restrict__ y, long long y_bstride,
                                                     long long n_count, float scale) {
  const int b = blockIdx.y;
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_count) return;
  const long long len = ld_len(len_frames, len_mul, L, Mr, N, b);
  float v = 0.f;
  if (j < len) {
    const long long F = 1 + len / WM_H;
    if (len >= WM_M + 1 && j < WM_H * (F - 1)) {
      const long long p = j + WM_M, fl = p / WM_H;
      const int r = (int)(p - fl * WM_H);
      int region;
      const float acc = sf_ola_sum(fr + (long long)b * fr_bstride, fl, r, WM_N, WM_H, F, 0, &region);
      v = acc * inv_env[region * WM_H + r];
    } else {
      v = x[(long long)b * x_bstride + j];
    }
  }
  if constexpr (sizeof(OUT) == sizeof(int16_t)) y[(long long)b * y_bstride + j] = pcm16_of(v, scale);
  else y[(long long)b * y_bstride + j] = v;
}

// Lb[b * lb_bstride + g * 96 + j] of the hop-128 frames g < F' = 1 + len / 128 of every item (none below n/2 + 1 samples).
__global__ __launch_bounds__(64 * SF_FPB) void wm_lb_kernel(const float* __restrict__ x, long long x_bstride, const int* __restrict__ lens,
                                                            const float* __restrict__ win, const float2* __restrict__ tw,
                                                            float* __restrict__ Lb, long long lb_bstride) {
  __shared__ float lds[SF_FPB][4][SF_PLANE];
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  const int b = blockIdx.y;
  const long long len = lens[b];
  const long long F = len >= WM_M + 1 ? 1 + len / WM_DH : 0;
  const long long g = (long long)blockIdx.x * SF_FPB + wv;
  if ((long long)blockIdx.x * SF_FPB >= F) return;  // uniform exit
  const bool valid = g < F;
  float *ar = lds[wv][0], *ai = lds[wv][1], *br = lds[wv][2], *bi = lds[wv][3];
  const float* xb = x + (long long)b * x_bstride;
  sf_frame_load(xb, g * WM_DH, WM_M, len, 0, len, win, valid, t, ar, ai);  // (the padded signal from 128 g on: centred on sample 128 g)
  __syncthreads();
  sf_fft(ar, ai, br, bi, WM_M, WM_LOG2M, tw, t);
  // |X[k]| and |X[M - k]| of the band into the free plane br, at k - 16 (unpadded: 384 floats, read four in a row per lane below)
  float mx = 0.f;
  for (int k = t; k <= (WM_M >> 1); k += 64) {
    const int kp = WM_M - k;
    const SfBins X = sf_unpack(ar, ai, tw, WM_M, k);
    if (k >= WM_LO && k < WM_HI) {
      const float a = sqrtf(X.kr * X.kr + X.ki * X.ki);
      br[k - WM_LO] = a;
      mx = fmaxf(mx, a);
    }
    if (kp != k && kp >= WM_LO && kp < WM_HI) {
      const float a = sqrtf(X.pr * X.pr + X.pi * X.pi);
      br[kp - WM_LO] = a;
      mx = fmaxf(mx, a);
    }
  }
  for (int off = 32; off; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));  // m_g: the whole wave holds it
  __syncthreads();
  if (!valid) return;
  const float fl = 1e-4f * mx;
  float* lb = Lb + (long long)b * lb_bstride + g * WM_G;
  for (int j = t; j < WM_G; j += 64) {
    float s = 0.f;
    if (mx > 0.f) {
      s = logf(fmaxf(br[4 * j], fl));
      s += logf(fmaxf(br[4 * j + 1], fl));
      s += logf(fmaxf(br[4 * j + 2], fl));
      s += logf(fmaxf(br[4 * j + 3], fl));
      s *= 0.25f;
    }
    lb[j] = s;
  }
}

// z_all[b * 128 + o] and rows_all[b * 128 + o] of offset index o = blockIdx.x of item b = blockIdx.y, from Lb.
__global__ __launch_bounds__(WM_SCORE_THREADS) void wm_score_kernel(const float* __restrict__ Lb, long long lb_bstride,
                                                                   const int* __restrict__ lens, uint32_t mk, double* __restrict__ z_all,
                                                                   int* __restrict__ rows_all) {
  constexpr int PER = WM_Q * WM_G / WM_SCORE_THREADS;  // (q, j) pairs per thread: 6
  __shared__ double T[WM_Q * WM_G];
  __shared__ double red[2][WM_SCORE_THREADS];
  const int o = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const long long len = lens[b];
  const long long F = len >= WM_M + 1 ? 1 + len / WM_DH : 0;
  const int g0 = o & 1;
  const long long pbase = (o + g0) >> 1;
  const long long nf = F > g0 ? (F - g0 + 1) / 2 : 0;             // frames g = g0 + 2 f < F
  const long long r0 = (pbase + 3) >> 2, r1 = ((pbase + nf) >> 2) - 1;  // the complete rows, inclusive
  const long long rows = r1 >= r0 ? r1 - r0 + 1 : 0;
  const float* lb = Lb + (long long)b * lb_bstride;
  double G[PER];
  for (int i = 0; i < PER; ++i) G[i] = 0.0;
  for (long long c = r0; c <= r1; c += WM_Q) {  // rows c .. c + 15: every q once (uniform trip count)
    bool live[PER];
    for (int i = 0; i < PER; ++i) {
      const int id = tid + i * WM_SCORE_THREADS, q = id / WM_G, j = id - q * WM_G;
      const long long rho = c + ((q - (int)(c & (WM_Q - 1))) & (WM_Q - 1));
      live[i] = rho <= r1;
      double v = 0.0;
      if (live[i]) {
        const long long gf = g0 + 2 * (4 * rho - pbase);  // the row's first frame; its four are 2 apart
        const float* p = lb + gf * WM_G + j;
        v = (((double)p[0] + (double)p[2 * WM_G]) + (double)p[4 * WM_G] + (double)p[6 * WM_G]) * 0.25;
      }
      T[id] = v;
    }
    __syncthreads();
    for (int i = 0; i < PER; ++i) {
      const int id = tid + i * WM_SCORE_THREADS, j = id % WM_G;
      if (live[i] && j >= 1 && j <= WM_G - 2) G[i] += T[id] - 0.5 * (T[id - 1] + T[id + 1]);
    }
    __syncthreads();
  }
  double num = 0.0, den = 0.0;
  for (int i = 0; i < PER; ++i) {
    const int id = tid + i * WM_SCORE_THREADS, q = id / WM_G, j = id - q * WM_G;
    num += wm_chip(mk, q, j) ? G[i] : -G[i];
    den += G[i] * G[i];
  }
  red[0][tid] = num;
  red[1][tid] = den;
  __syncthreads();
  for (int s = WM_SCORE_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    const double d = red[1][0];
    z_all[(long long)b * VITS_WATERMARK_OFFSETS + o] = (rows > 0 && d > 0.0) ? red[0][0] / sqrt(d) : 0.0;
    rows_all[(long long)b * VITS_WATERMARK_OFFSETS + o] = (int)rows;
  }
}

// z[b] = max_o z_all[b, o], the lowest o on a tie; offset[b] = 128 o; rows[b] = rows_all[b, o]
__global__ void wm_argmax_kernel(const double* __restrict__ z_all, const int* __restrict__ rows_all, int B, double* __restrict__ z,
                                 int* __restrict__ offset, int* __restrict__ rows) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* zb = z_all + (long long)b * VITS_WATERMARK_OFFSETS;
  int best = 0;
  for (int o = 1; o < VITS_WATERMARK_OFFSETS; ++o) if (zb[o] > zb[best]) best = o;
  z[b] = zb[best];
  offset[b] = best * WM_DH;
  rows[b] = rows_all[(long long)b * VITS_WATERMARK_OFFSETS + best];
}

// ---- the request and the launches --------------------------------------------------------------------------------------------
struct WmReq {
  bool on = false;
  uint32_t key = 0;
  float gp = 1.f, gm = 1.f;  // fp32(1 + a), fp32(1 - a)
  const StftTab* T = nullptr;  // set by the callers that launch on the device (stft_tab_get: uploaded on first use, before any capture)
};

// 0 -> the default; a depth outside (0, 2] dB, NaN included, is refused by name
static int wm_req(bool on, uint32_t key, float depth_db, WmReq* out) {
  *out = WmReq();
  if (!on) return VITS_OK;
  const float d = depth_db == 0.f ? VITS_WATERMARK_DEFAULT_DEPTH_DB : depth_db;
  if (!(d > 0.f && d <= VITS_WATERMARK_MAX_DEPTH_DB))
    return fail(VITS_ERR_ARG, "watermark: depth %g dB outside (0, %g] (0 = the default, %g dB)", (double)depth_db, (double)VITS_WATERMARK_MAX_DEPTH_DB,
                (double)VITS_WATERMARK_DEFAULT_DEPTH_DB);
  const float a = (float)(pow(10.0, (double)d / 20.0) - 1.0);
  out->on = true;
  out->key = key;
  out->gp = 1.0f + a;
  out->gm = 1.0f - a;
  return VITS_OK;
}
// floats of scratch one item of N samples needs
static size_t wm_scratch_elems(long long N) { return (size_t)(N / WM_H + 1) * WM_N; }

// B items x [B, N] (item b: ld_len(len_frames, len_mul, L, Mr, N, b) samples) -> y [B, n_count columns] on `stream` (capturable: no
// allocation, no synchronisation).  scratch holds B * scratch_bstride floats, scratch_bstride >= wm_scratch_elems(N).
template <typename OUT>
static void wm_launch(hipStream_t stream, const WmReq& q, const float* x, long long x_bstride, long long N, const int* len_frames,
                      long long len_mul, int L, int Mr, int B, float* scratch, long long scratch_bstride, OUT* y, long long y_bstride,
                      long long n_count, float scale) {
  if (n_count <= 0 || B <= 0) return;
  const StftTab& T = *q.T;
  const long long Fmax = N >= WM_M + 1 ? 1 + N / WM_H : 0;
  const uint32_t mk = wm_mix(q.key);
  if (Fmax > 0)
    hipLaunchKernelGGL(wm_frames_kernel, dim3((unsigned)cdiv((int)Fmax, SF_FPB), B), dim3(64 * SF_FPB), 0, stream, x, x_bstride, N, len_frames, len_mul, L,
                       Mr, T.d_win, T.d_tw, mk, q.gp, q.gm, scratch, scratch_bstride);
  hipLaunchKernelGGL(wm_ola_kernel<OUT>, dim3((unsigned)((n_count + 255) / 256), B), dim3(256), 0, stream, scratch, scratch_bstride, x, x_bstride, N,
                     len_frames, len_mul, L, Mr, T.d_env, y, y_bstride, n_count, scale);
}

// ---- entry points ----------------------------------------------------------------------------------------------------------
// the door behind a request (stts_tail_host runs the stage through it, as it runs the others through theirs)
static int wm_op(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, WmReq q, float* y) {
  std::vector<int> len32;
  TRY(op_items_check("watermark", x, lengths, B, N, &len32));
  if (!y) return fail(VITS_ERR_ARG, "watermark: bad argument");
  TRY(stft_tab_get(device, WM_N, &q.T));
  OpDoor d("watermark", device);
  const size_t sc = wm_scratch_elems(N);
  float* dx = d.up(x, (size_t)B * N);
  int* dl = d.up(len32.data(), B);
  float* ds = d.dev<float>((size_t)B * sc);
  float* dy = d.out<float>((size_t)B * N);
  if (d.ok()) wm_launch<float>(nullptr, q, dx, N, N, dl, 1, 1, 1, B, ds, (long long)sc, dy, N, N, 1.f);
  d.finish();
  d.down(y, dy, (size_t)B * N);
  return d.rc();
}

int vits_op_watermark(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, float depth_db, float* y) {
  WmReq q;
  TRY(wm_req(true, key, depth_db, &q));
  return wm_op(device, x, lengths, B, N, q, y);
}

int vits_op_watermark_detect(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, double* z,
                             int32_t* offset, int32_t* rows, double* z_all) {
  std::vector<int> len32;
  TRY(op_items_check("watermark detect", x, lengths, B, N, &len32));
  if (!z || !offset || !rows) return fail(VITS_ERR_ARG, "watermark detect: bad argument");
  const StftTab* T = nullptr;
  TRY(stft_tab_get(device, WM_N, &T));
  OpDoor d("watermark detect", device);
  const long long Fmax = N >= WM_M + 1 ? 1 + N / WM_DH : 0;
  const long long lbs = (Fmax ? Fmax : 1) * WM_G;
  const size_t nz = (size_t)B * VITS_WATERMARK_OFFSETS;
  float* dx = d.up(x, (size_t)B * N);
  int* dl = d.up(len32.data(), B);
  float* dlb = d.dev<float>((size_t)B * lbs);
  double* dza = d.out<double>(nz);
  int* dra = d.out<int>(nz);
  double* dz = d.out<double>(B);
  int* dof = d.out<int>(B);
  int* dro = d.out<int>(B);
  if (d.ok()) {
    const uint32_t mk = wm_mix(key);
    if (Fmax > 0)
      hipLaunchKernelGGL(wm_lb_kernel, dim3((unsigned)cdiv((int)Fmax, SF_FPB), B), dim3(64 * SF_FPB), 0, nullptr, dx, N, dl, T->d_win, T->d_tw, dlb, lbs);
    hipLaunchKernelGGL(wm_score_kernel, dim3(VITS_WATERMARK_OFFSETS, B), dim3(WM_SCORE_THREADS), 0, nullptr, dlb, lbs, dl, mk, dza, dra);
    hipLaunchKernelGGL(wm_argmax_kernel, dim3(cdiv(B, 64)), dim3(64), 0, nullptr, dza, dra, B, dz, dof, dro);
  }
  d.finish();
  d.down(z, dz, (size_t)B);
  d.down(offset, dof, (size_t)B);
  d.down(rows, dro, (size_t)B);
  if (z_all) d.down(z_all, dza, nz);
  return d.rc();
}
