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
// The payload (include/vits_watermark_payload.h) is a template parameter of two of these kernels and one kernel more:
//   wm_frames_kernel<true>   the chip of a payload position flipped by its coded bit of the item's word (words[blockIdx.y])
//   wm_score_kernel<true>    the two sums over the pilot positions only
//   wm_bits_kernel           one workgroup per item at the offset wm_argmax_kernel chose (read on the device): G again by the shared row
//                            loop (wm_rows_G), c G and G^2 of every position to LDS at the thread's linear id 96 q + j -- the layout argued
//                            above, T's own plane and one more, 2 x 1536 doubles = 24 KiB -- then 24 threads sum their bit's positions in
//                            ascending id (all 24 lanes read the same address: a broadcast), one thread packs the word and checks the CRC
// The <false> forms are the kernels as they were.
// The scan (include/vits_watermark_scan.h), two launches: wm_lb_kernel as it is, then
//   wm_scan_kernel<PILOT>    one workgroup per (item, offset index, chunk of WM_SCAN_CHUNK consecutive windows), the ownership of
//                            wm_score_kernel: thread id owns the six (q, j) at id + 256 i.  It walks the chunk's periods in order: T of the
//                            period's 16 rows to LDS (the plane and the argument above), D of its six pairs into the newest slot of a
//                            ring of the last 8 periods, the window's ascending sum over the last S slots, the two sums of the score
//                            through the fixed LDS tree of wm_score_kernel.  The ring is registers, 8 x 6 doubles = 96 VGPRs: it is
//                            shifted by one slot per period with every index a compile-time constant (42 register moves next to 6 LDS
//                            rounds), because a slot index that rotates at run time would send the array to scratch, and an LDS ring
//                            would cost 8 x 12 KiB per workgroup and an LDS read per term where the value is already in the thread
//                            that owns it.  Chunks overlap by S - 1 periods (the first S - 1 periods of a chunk fill the ring and
//                            score nothing), so 60 s of audio are 128 x 10 workgroups and not 128 serial ones; a window is the written
//                            sum of its own S periods, so its bits do not depend on the chunking.  Gp is never stored.
// Nothing waits between workgroups; there are no atomics.
#pragma once
#include "../../include/vits_watermark_scan.h"

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
#define WM_SCAN_SPAN VITS_WATERMARK_SCAN_MAX_SPAN
#define WM_SCAN_CHUNK 8  // windows per workgroup of wm_scan_kernel
static_assert(WM_N <= SF_N && (1 << WM_LOG2M) == WM_M, "the watermark runs on the frame transform of stft.hip.h");
static_assert((WM_HI - WM_LO) == 4 * WM_G && (WM_Q * WM_G) % WM_SCORE_THREADS == 0, "96 groups of 4 bins; whole (q, j) per thread");

__host__ __device__ __forceinline__ uint32_t wm_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
// the chip of tile row q, group j under mk = wm_mix(key): true = +1
__host__ __device__ __forceinline__ bool wm_chip(uint32_t mk, int q, int j) { return (wm_mix(mk ^ (uint32_t)(WM_G * q + j + 1)) & 1u) != 0; }
// include/vits_watermark_payload.h: crc8 over the 16 payload bits MSB first (polynomial 0x07, initial value 0xFF, no final xor) ...
__host__ __device__ __forceinline__ uint32_t wm_crc8(uint32_t p) {
  uint32_t c = 0xFFu;
  for (int i = 15; i >= 0; --i) {
    const uint32_t fb = ((c >> 7) ^ (p >> i)) & 1u;
    c = (c << 1) & 0xFFu;
    if (fb) c ^= 0x07u;
  }
  return c;
}
// ... the coded word of a payload ...
__host__ __device__ __forceinline__ uint32_t wm_word(uint32_t p) { return (p << 8) | wm_crc8(p); }
// ... a pilot position, and the coded bit a payload position carries
__host__ __device__ __forceinline__ bool wm_pilot(int q, int j) { return ((q + j) & 1) != 0; }
__host__ __device__ __forceinline__ int wm_bit_index(uint32_t mk, int q, int j) {
  return (int)(wm_mix(mk ^ (0x80000000u | (uint32_t)(WM_G * q + j + 1))) % VITS_WATERMARK_CODED_BITS);
}
// c'(q, j) under the coded word: the chip, flipped on a payload position whose bit is set
__host__ __device__ __forceinline__ bool wm_chip_word(uint32_t mk, int q, int j, uint32_t word) {
  bool c = wm_chip(mk, q, j);
  if (!wm_pilot(q, j) && ((word >> (VITS_WATERMARK_CODED_BITS - 1 - wm_bit_index(mk, q, j))) & 1u)) c = !c;
  return c;
}
// the gain of bin k in a frame of tile row q: gp = fp32(1 + a), gm = fp32(1 - a); PAYLOAD: under the item's coded word
template <bool PAYLOAD>
__device__ __forceinline__ float wm_bin_gain(uint32_t mk, int q, int k, float gp, float gm, uint32_t word) {
  if (k < WM_LO || k >= WM_HI) return 1.f;
  if constexpr (PAYLOAD) return wm_chip_word(mk, q, (k - WM_LO) >> 2, word) ? gp : gm;
  else return wm_chip(mk, q, (k - WM_LO) >> 2) ? gp : gm;
}

// The marked, windowed frames of every item: wave w of workgroup blockIdx.x owns frame f = blockIdx.x * SF_FPB + w.
//   x      item b at x + b * x_bstride, samples [0, len), len = it.len_out(b) (ragged.hip.h: the item as returned, at most it.cap)
//   out    out[b * out_bstride + f * n + i]; an item shorter than n/2 + 1 has no frames (wm_ola_kernel passes it through)
//   words  PAYLOAD: the coded word of item b at words[b]; not read otherwise
template <bool PAYLOAD>
__global__ __launch_bounds__(64 * SF_FPB) void wm_frames_kernel(const float* __restrict__ x, long long x_bstride, const Items it,
                                                                const float* __restrict__ win, const float2* __restrict__ tw, uint32_t mk, float gp,
                                                                float gm, float* __restrict__ out, long long out_bstride,
                                                                const uint32_t* __restrict__ words) {
  __shared__ float lds[SF_FPB][4][SF_PLANE];
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  const int b = blockIdx.y;
  const long long len = it.len_out(b);
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
  uint32_t word = 0;
  if constexpr (PAYLOAD) word = words[b];
  for (int k = t; k <= (WM_M >> 1); k += 64) {  // unpack, the chip's gain, pack
    SfBins X = sf_unpack(ar, ai, tw, WM_M, k);
    const float gk = wm_bin_gain<PAYLOAD>(mk, q, k, gp, gm, word), gq = wm_bin_gain<PAYLOAD>(mk, q, WM_M - k, gp, gm, word);
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
                                                     long long x_bstride, const Items it, const float* __restrict__ inv_env, OUT* __restrict__ y,
                                                     long long y_bstride, long long n_count, float scale) {
  const int b = blockIdx.y;
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_count) return;
  const long long len = it.len_out(b);
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

constexpr int WM_PER = WM_Q * WM_G / WM_SCORE_THREADS;  // (q, j) pairs per thread: 6, at the linear ids tid + i * WM_SCORE_THREADS
// the complete rows [r0, r1] of offset index o of an item of F hop-128 frames, and where its pattern starts
struct WmRows { int g0; long long pbase, r0, r1, rows; };
__host__ __device__ __forceinline__ WmRows wm_rows_of(long long len, int o) {
  WmRows R;
  const long long F = len >= WM_M + 1 ? 1 + len / WM_DH : 0;
  R.g0 = o & 1;
  R.pbase = (o + R.g0) >> 1;
  const long long nf = F > R.g0 ? (F - R.g0 + 1) / 2 : 0;  // frames g = g0 + 2 f < F
  R.r0 = (R.pbase + 3) >> 2; R.r1 = ((R.pbase + nf) >> 2) - 1;  // inclusive
  R.rows = R.r1 >= R.r0 ? R.r1 - R.r0 + 1 : 0;
  return R;
}
// G of the thread's six (q, j) over the complete rows, 16 tile rows at a time: T of a row of every q in LDS as doubles [16][96], D and
// the running G in registers.  The whole workgroup calls it (uniform trip count, two barriers per round); T is free again on return.
__device__ __forceinline__ void wm_rows_G(const float* __restrict__ lb, const WmRows& R, int tid, double* __restrict__ T, double (&G)[WM_PER]) {
  for (int i = 0; i < WM_PER; ++i) G[i] = 0.0;
  for (long long c = R.r0; c <= R.r1; c += WM_Q) {  // rows c .. c + 15: every q once
    bool live[WM_PER];
    for (int i = 0; i < WM_PER; ++i) {
      const int id = tid + i * WM_SCORE_THREADS, q = id / WM_G, j = id - q * WM_G;
      const long long rho = c + ((q - (int)(c & (WM_Q - 1))) & (WM_Q - 1));
      live[i] = rho <= R.r1;
      double v = 0.0;
      if (live[i]) {
        const long long gf = R.g0 + 2 * (4 * rho - R.pbase);  // the row's first frame; its four are 2 apart
        const float* p = lb + gf * WM_G + j;
        v = (((double)p[0] + (double)p[2 * WM_G]) + (double)p[4 * WM_G] + (double)p[6 * WM_G]) * 0.25;
      }
      T[id] = v;
    }
    __syncthreads();
    for (int i = 0; i < WM_PER; ++i) {
      const int id = tid + i * WM_SCORE_THREADS, j = id % WM_G;
      if (live[i] && j >= 1 && j <= WM_G - 2) G[i] += T[id] - 0.5 * (T[id - 1] + T[id + 1]);
    }
    __syncthreads();
  }
}

// z_all[b * 128 + o] and rows_all[b * 128 + o] of offset index o = blockIdx.x of item b = blockIdx.y, from Lb.  PILOT: the two sums
// over the pilot positions only (include/vits_watermark_payload.h, step 6').
template <bool PILOT>
__global__ __launch_bounds__(WM_SCORE_THREADS) void wm_score_kernel(const float* __restrict__ Lb, long long lb_bstride,
                                                                   const int* __restrict__ lens, uint32_t mk, double* __restrict__ z_all,
                                                                   int* __restrict__ rows_all) {
  __shared__ double T[WM_Q * WM_G];
  __shared__ double red[2][WM_SCORE_THREADS];
  const int o = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const WmRows R = wm_rows_of(lens[b], o);
  double G[WM_PER];
  wm_rows_G(Lb + (long long)b * lb_bstride, R, tid, T, G);
  double num = 0.0, den = 0.0;
  for (int i = 0; i < WM_PER; ++i) {
    const int id = tid + i * WM_SCORE_THREADS, q = id / WM_G, j = id - q * WM_G;
    if (PILOT && !wm_pilot(q, j)) continue;
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
    z_all[(long long)b * VITS_WATERMARK_OFFSETS + o] = (R.rows > 0 && d > 0.0) ? red[0][0] / sqrt(d) : 0.0;
    rows_all[(long long)b * VITS_WATERMARK_OFFSETS + o] = (int)R.rows;
  }
}

// include/vits_watermark_scan.h, S2 and S3: the first complete period of the rows R and the windows of span S they hold
struct WmPeriods { long long p0, W; };
__host__ __device__ __forceinline__ WmPeriods wm_periods_of(const WmRows& R, int S) {
  WmPeriods P;
  P.p0 = (R.r0 + WM_Q - 1) / WM_Q;                // (r0 >= 0, r1 >= -1: the divisions round as the definition's ceil and floor)
  const long long p1 = (R.r1 + 1) / WM_Q - 1;
  const long long n = p1 - P.p0 + 2 - S;
  P.W = n > 0 ? n : 0;
  return P;
}

// z_scan[(b * 128 + o) * w_cap + w] of the windows w in [blockIdx.y * WM_SCAN_CHUNK, +WM_SCAN_CHUNK) below W_o, of offset index
// o = blockIdx.x of item b = blockIdx.z, from Lb; first_period and windows [b * 128 + o] by the workgroup of chunk 0.  S in [1, 8].
// z_scan arrives zeroed: what lies at and beyond W_o is not written.  PILOT: the two sums over the pilot positions only.
template <bool PILOT>
__global__ __launch_bounds__(WM_SCORE_THREADS) void wm_scan_kernel(const float* __restrict__ Lb, long long lb_bstride, const int* __restrict__ lens,
                                                                  uint32_t mk, int S, long long w_cap, double* __restrict__ z_scan,
                                                                  int* __restrict__ first_period, int* __restrict__ windows) {
  __shared__ double T[WM_Q * WM_G];
  __shared__ double red[2][WM_SCORE_THREADS];
  const int o = blockIdx.x, b = blockIdx.z, tid = threadIdx.x;
  const WmRows R = wm_rows_of(lens[b], o);
  const WmPeriods P = wm_periods_of(R, S);
  const long long bo = (long long)b * VITS_WATERMARK_OFFSETS + o;
  if (blockIdx.y == 0 && tid == 0) { first_period[bo] = (int)P.p0; windows[bo] = (int)P.W; }
  const long long w0 = (long long)blockIdx.y * WM_SCAN_CHUNK;
  const long long w1 = P.W < w0 + WM_SCAN_CHUNK ? P.W : w0 + WM_SCAN_CHUNK;  // this workgroup's windows: [w0, w1)
  if (w1 <= w0) return;                                                       // uniform
  const float* lb = Lb + (long long)b * lb_bstride;
  double ring[WM_SCAN_SPAN][WM_PER];  // D of the thread's pairs in the last 8 periods, the newest in slot 7; static indices only
#pragma unroll
  for (int k = 0; k < WM_SCAN_SPAN; ++k)
#pragma unroll
    for (int i = 0; i < WM_PER; ++i) ring[k][i] = 0.0;
  for (long long p = P.p0 + w0; p < P.p0 + w1 + S - 1; ++p) {  // every one a complete period: its 16 rows lie in [r0, r1]
#pragma unroll
    for (int i = 0; i < WM_PER; ++i) {
      const int id = tid + i * WM_SCORE_THREADS, q = id / WM_G, j = id - q * WM_G;
      const long long gf = R.g0 + 2 * (4 * (WM_Q * p + q) - R.pbase);  // the row's first frame; its four are 2 apart
      const float* f = lb + gf * WM_G + j;
      T[id] = (((double)f[0] + (double)f[2 * WM_G]) + (double)f[4 * WM_G] + (double)f[6 * WM_G]) * 0.25;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < WM_PER; ++i) {
      const int id = tid + i * WM_SCORE_THREADS, j = id % WM_G;
#pragma unroll
      for (int k = 0; k + 1 < WM_SCAN_SPAN; ++k) ring[k][i] = ring[k + 1][i];
      ring[WM_SCAN_SPAN - 1][i] = (j >= 1 && j <= WM_G - 2) ? T[id] - 0.5 * (T[id - 1] + T[id + 1]) : 0.0;
    }
    const long long w = p - (S - 1) - P.p0;  // the window this period completes
    if (w >= w0) {                           // uniform
      double num = 0.0, den = 0.0;
#pragma unroll
      for (int i = 0; i < WM_PER; ++i) {
        const int id = tid + i * WM_SCORE_THREADS, q = id / WM_G, j = id - q * WM_G;
        if (PILOT && !wm_pilot(q, j)) continue;
        double G = 0.0;  // ((Gp[p0 + w] + Gp[p0 + w + 1]) + ...): slots 8 - S .. 7, ascending
#pragma unroll
        for (int k = 0; k < WM_SCAN_SPAN; ++k)
          if (k >= WM_SCAN_SPAN - S) G = k == WM_SCAN_SPAN - S ? ring[k][i] : G + ring[k][i];
        num += wm_chip(mk, q, j) ? G : -G;
        den += G * G;
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
        z_scan[bo * w_cap + w] = d > 0.0 ? red[0][0] / sqrt(d) : 0.0;
      }
    }
    __syncthreads();  // T and red are free for the next period
  }
}

// The coded word of item b = blockIdx.x at the offset wm_argmax_kernel chose for it (offset[b], z[b]: read here, on the device):
// payload[b] = W' >> 8, valid[b] = z[b] >= 6 and the CRC holds, bit_z[b * 24 + i] = z_i (steps 8' and 9').
__global__ __launch_bounds__(WM_SCORE_THREADS) void wm_bits_kernel(const float* __restrict__ Lb, long long lb_bstride, const int* __restrict__ lens,
                                                                  uint32_t mk, const double* __restrict__ z, const int* __restrict__ offset,
                                                                  uint32_t* __restrict__ payload, int* __restrict__ valid, double* __restrict__ bit_z) {
  __shared__ double T[WM_Q * WM_G];   // the row loop's plane, then c G at 96 q + j
  __shared__ double G2[WM_Q * WM_G];  // G^2 at 96 q + j
  __shared__ unsigned char bix[WM_Q * WM_G];  // the coded bit of a scored payload position, 255 elsewhere
  __shared__ double bz[VITS_WATERMARK_CODED_BITS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int o = (offset[b] / WM_DH) & (VITS_WATERMARK_OFFSETS - 1);
  const WmRows R = wm_rows_of(lens[b], o);
  double G[WM_PER];
  wm_rows_G(Lb + (long long)b * lb_bstride, R, tid, T, G);  // (ends behind a barrier: T is free)
  for (int i = 0; i < WM_PER; ++i) {
    const int id = tid + i * WM_SCORE_THREADS, q = id / WM_G, j = id - q * WM_G;
    T[id] = wm_chip(mk, q, j) ? G[i] : -G[i];
    G2[id] = G[i] * G[i];
    bix[id] = (!wm_pilot(q, j) && j >= 1 && j <= WM_G - 2) ? (unsigned char)wm_bit_index(mk, q, j) : (unsigned char)255;
  }
  __syncthreads();
  if (tid < VITS_WATERMARK_CODED_BITS) {
    double s = 0.0, n = 0.0;
    for (int id = 0; id < WM_Q * WM_G; ++id)  // ascending 96 q + j
      if (bix[id] == tid) { s += T[id]; n += G2[id]; }
    const double zi = n > 0.0 ? s / sqrt(n) : 0.0;
    bz[tid] = zi;
    bit_z[(long long)b * VITS_WATERMARK_CODED_BITS + tid] = zi;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t W = 0;
    for (int i = 0; i < VITS_WATERMARK_CODED_BITS; ++i) W = (W << 1) | (bz[i] < 0.0 ? 1u : 0u);
    payload[b] = W >> 8;
    valid[b] = (z[b] >= VITS_WATERMARK_THRESHOLD && wm_crc8(W >> 8) == (W & 0xFFu)) ? 1 : 0;
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
  // include/vits_watermark_payload.h: the coded words, on the host; they go up with each call that launches
  bool payload = false;
  uint32_t word = 0;            // of the scalar: what a document, the one item it has become, is marked with
  std::vector<uint32_t> words;  // of each item of the call, [B]
  const uint32_t* host_words(bool doc) const { return !payload ? nullptr : doc ? &word : words.data(); }
};

static int wm_payload_arg(uint32_t p, int item, uint32_t* word) {
  if (p > VITS_WATERMARK_PAYLOAD_MAX) {
    if (item < 0) return fail(VITS_ERR_ARG, "watermark: payload %u outside [0, %u]", p, VITS_WATERMARK_PAYLOAD_MAX);
    return fail(VITS_ERR_ARG, "watermark: payload %u of item %d outside [0, %u]", p, item, VITS_WATERMARK_PAYLOAD_MAX);
  }
  *word = wm_word(p);
  return VITS_OK;
}

// 0 -> the default (1 dB, 2 dB with a payload); a depth outside (0, 2] dB, NaN included, is refused by name.  payload_on: the scalar
// `payload`, or payloads[0 .. B) where that is not null; a value above 65535 is refused by name.
static int wm_req(bool on, uint32_t key, float depth_db, WmReq* out, bool payload_on = false, uint32_t payload = 0,
                  const uint32_t* payloads = nullptr, int B = 0) {
  *out = WmReq();
  if (!on) return VITS_OK;
  const float dflt = payload_on ? VITS_WATERMARK_PAYLOAD_DEFAULT_DEPTH_DB : VITS_WATERMARK_DEFAULT_DEPTH_DB;
  const float d = depth_db == 0.f ? dflt : depth_db;
  if (!(d > 0.f && d <= VITS_WATERMARK_MAX_DEPTH_DB))
    return fail(VITS_ERR_ARG, "watermark: depth %g dB outside (0, %g] (0 = the default, %g dB)", (double)depth_db, (double)VITS_WATERMARK_MAX_DEPTH_DB,
                (double)dflt);
  const float a = (float)(pow(10.0, (double)d / 20.0) - 1.0);
  out->on = true;
  out->key = key;
  out->gp = 1.0f + a;
  out->gm = 1.0f - a;
  if (payload_on) {
    out->payload = true;
    out->words.resize(B > 0 ? B : 0);
    if (payloads) {
      for (int b = 0; b < B; ++b) TRY(wm_payload_arg(payloads[b], b, &out->words[b]));
      if (payload <= VITS_WATERMARK_PAYLOAD_MAX) out->word = wm_word(payload);  // (overridden; a document reads it)
      else out->word = out->words.empty() ? 0 : out->words[0];
    } else {
      TRY(wm_payload_arg(payload, -1, &out->word));
      std::fill(out->words.begin(), out->words.end(), out->word);
    }
  }
  return VITS_OK;
}
// floats of scratch one item of N samples needs
static size_t wm_scratch_elems(long long N) { return (size_t)(N / WM_H + 1) * WM_N; }

// B items x [B, N] (item b: it.len_out(b) samples) -> y [B, n_count columns] on `stream` (capturable: no
// allocation, no synchronisation).  scratch holds B * scratch_bstride floats, scratch_bstride >= wm_scratch_elems(it.cap).  d_words: the
// coded words [B] on the device where q.payload (an argument of the launch), not read otherwise.
template <typename OUT>
static void wm_launch(hipStream_t stream, const WmReq& q, const float* x, long long x_bstride, const Items& it, int B, float* scratch,
                      long long scratch_bstride, OUT* y, long long y_bstride, long long n_count, float scale, const uint32_t* d_words = nullptr) {
  if (n_count <= 0 || B <= 0) return;
  const StftTab& T = *q.T;
  const long long Fmax = it.cap >= WM_M + 1 ? 1 + it.cap / WM_H : 0;
  const uint32_t mk = wm_mix(q.key);
  if (Fmax > 0) {
    const dim3 grid((unsigned)cdiv((int)Fmax, SF_FPB), B), block(64 * SF_FPB);
    if (q.payload) hipLaunchKernelGGL(wm_frames_kernel<true>, grid, block, 0, stream, x, x_bstride, it, T.d_win, T.d_tw, mk, q.gp, q.gm, scratch,
                                      scratch_bstride, d_words);
    else hipLaunchKernelGGL(wm_frames_kernel<false>, grid, block, 0, stream, x, x_bstride, it, T.d_win, T.d_tw, mk, q.gp, q.gm, scratch,
                            scratch_bstride, (const uint32_t*)nullptr);
  }
  hipLaunchKernelGGL(wm_ola_kernel<OUT>, dim3((unsigned)((n_count + 255) / 256), B), dim3(256), 0, stream, scratch, scratch_bstride, x, x_bstride, it, T.d_env, y, y_bstride, n_count, scale);
}

// ---- entry points ----------------------------------------------------------------------------------------------------------
// the door behind a request (stts_tail_host runs the stage through it, as it runs the others through theirs); words: the coded words
// [B] on the host where q.payload
static int wm_op(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, WmReq q, float* y, const uint32_t* words = nullptr) {
  std::vector<int> len32;
  TRY(op_items_check("watermark", x, lengths, B, N, &len32));
  if (!y || (q.payload && !words)) return fail(VITS_ERR_ARG, "watermark: bad argument");
  TRY(stft_tab_get(device, WM_N, &q.T));
  OpDoor d("watermark", device);
  const size_t sc = wm_scratch_elems(N);
  float* dx = d.up(x, (size_t)B * N);
  int* dl = d.up(len32.data(), B);
  uint32_t* dw = q.payload ? d.up(words, (size_t)B) : nullptr;
  float* ds = d.dev<float>((size_t)B * sc);
  float* dy = d.out<float>((size_t)B * N);
  if (d.ok()) wm_launch<float>(nullptr, q, dx, N, Items{dl, 1, 1, 1, N}, B, ds, (long long)sc, dy, N, N, 1.f, dw);
  d.finish();
  d.down(y, dy, (size_t)B * N);
  return d.rc();
}

int vits_op_watermark(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, float depth_db, float* y) {
  WmReq q;
  TRY(wm_req(true, key, depth_db, &q));
  return wm_op(device, x, lengths, B, N, q, y);
}

int vits_op_watermark_payload(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, float depth_db,
                              const uint32_t* payloads, float* y) {
  if (!payloads || B <= 0) return fail(VITS_ERR_ARG, "watermark: bad argument");
  WmReq q;
  TRY(wm_req(true, key, depth_db, &q, true, 0, payloads, B));
  return wm_op(device, x, lengths, B, N, q, y, q.words.data());
}

// the detector, and the reader where `payload` is not null (the pilot scores, then the word at the best offset)
static int wm_detect_op(const char* what, int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, double* z,
                        int32_t* offset, int32_t* rows, double* z_all, uint32_t* payload, int32_t* valid, double* bit_z) {
  std::vector<int> len32;
  TRY(op_items_check(what, x, lengths, B, N, &len32));
  if (!z || !offset || !rows || (payload && !valid)) return fail(VITS_ERR_ARG, "%s: bad argument", what);
  const StftTab* T = nullptr;
  TRY(stft_tab_get(device, WM_N, &T));
  OpDoor d(what, device);
  const long long Fmax = N >= WM_M + 1 ? 1 + N / WM_DH : 0;
  const long long lbs = (Fmax ? Fmax : 1) * WM_G;
  const size_t nz = (size_t)B * VITS_WATERMARK_OFFSETS, nb = (size_t)B * VITS_WATERMARK_CODED_BITS;
  float* dx = d.up(x, (size_t)B * N);
  int* dl = d.up(len32.data(), B);
  float* dlb = d.dev<float>((size_t)B * lbs);
  double* dza = d.out<double>(nz);
  int* dra = d.out<int>(nz);
  double* dz = d.out<double>(B);
  int* dof = d.out<int>(B);
  int* dro = d.out<int>(B);
  uint32_t* dpl = payload ? d.out<uint32_t>(B) : nullptr;
  int* dva = payload ? d.out<int>(B) : nullptr;
  double* dbz = payload ? d.out<double>(nb) : nullptr;
  if (d.ok()) {
    const uint32_t mk = wm_mix(key);
    if (Fmax > 0)
      hipLaunchKernelGGL(wm_lb_kernel, dim3((unsigned)cdiv((int)Fmax, SF_FPB), B), dim3(64 * SF_FPB), 0, nullptr, dx, N, dl, T->d_win, T->d_tw, dlb, lbs);
    if (payload) hipLaunchKernelGGL(wm_score_kernel<true>, dim3(VITS_WATERMARK_OFFSETS, B), dim3(WM_SCORE_THREADS), 0, nullptr, dlb, lbs, dl, mk, dza, dra);
    else hipLaunchKernelGGL(wm_score_kernel<false>, dim3(VITS_WATERMARK_OFFSETS, B), dim3(WM_SCORE_THREADS), 0, nullptr, dlb, lbs, dl, mk, dza, dra);
    hipLaunchKernelGGL(wm_argmax_kernel, dim3(cdiv(B, 64)), dim3(64), 0, nullptr, dza, dra, B, dz, dof, dro);
    if (payload) hipLaunchKernelGGL(wm_bits_kernel, dim3(B), dim3(WM_SCORE_THREADS), 0, nullptr, dlb, lbs, dl, mk, dz, dof, dpl, dva, dbz);
  }
  d.finish();
  d.down(z, dz, (size_t)B);
  d.down(offset, dof, (size_t)B);
  d.down(rows, dro, (size_t)B);
  if (z_all) d.down(z_all, dza, nz);
  if (payload) {
    d.down(payload, dpl, (size_t)B);
    d.down(valid, dva, (size_t)B);
    if (bit_z) d.down(bit_z, dbz, nb);
  }
  return d.rc();
}

int vits_op_watermark_detect(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, double* z,
                             int32_t* offset, int32_t* rows, double* z_all) {
  return wm_detect_op("watermark detect", device, x, lengths, B, N, key, z, offset, rows, z_all, nullptr, nullptr, nullptr);
}

int vits_op_watermark_read(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, double* z,
                           int32_t* offset, int32_t* rows, uint32_t* payload, int32_t* valid, double* z_all, double* bit_z) {
  if (!payload || !valid) return fail(VITS_ERR_ARG, "watermark read: bad argument");
  return wm_detect_op("watermark read", device, x, lengths, B, N, key, z, offset, rows, z_all, payload, valid, bit_z);
}

// ---- the scan (include/vits_watermark_scan.h) ---------------------------------------------------------------------------------
static int wm_span_arg(int32_t span, int* S) {
  if (span < 0 || span > VITS_WATERMARK_SCAN_MAX_SPAN)
    return fail(VITS_ERR_ARG, "watermark scan: span %d outside [1, %d] (0 = the default, %d)", (int)span, VITS_WATERMARK_SCAN_MAX_SPAN,
                VITS_WATERMARK_SCAN_DEFAULT_SPAN);
  *S = span ? span : VITS_WATERMARK_SCAN_DEFAULT_SPAN;
  return VITS_OK;
}
// max_o W_o of an item of len samples
static long long wm_scan_windows(long long len, int S) {
  long long W = 0;
  for (int o = 0; o < VITS_WATERMARK_OFFSETS; ++o) W = std::max(W, wm_periods_of(wm_rows_of(len, o), S).W);
  return W;
}

int64_t vits_watermark_scan_windows(int64_t n_samples, int32_t span) {
  int S = 0;
  if (wm_span_arg(span, &S) != VITS_OK) return -1;
  if (n_samples < 0) {
    fail(VITS_ERR_ARG, "watermark scan: %lld samples", (long long)n_samples);
    return -1;
  }
  return wm_scan_windows(n_samples, S);
}

int vits_op_watermark_scan(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, int32_t span,
                           uint32_t flags, int64_t w_cap, double* z_scan, int32_t* first_period, int32_t* windows) {
  const char* what = "watermark scan";
  int S = 0;
  TRY(wm_span_arg(span, &S));
  if (flags & ~VITS_WATERMARK_SCAN_PILOTS) return fail(VITS_ERR_ARG, "%s: unknown flags 0x%x", what, flags & ~VITS_WATERMARK_SCAN_PILOTS);
  std::vector<int> len32;
  TRY(op_items_check(what, x, lengths, B, N, &len32));
  if (!z_scan || !first_period || !windows || w_cap < 0) return fail(VITS_ERR_ARG, "%s: bad argument", what);
  long long need = 0;
  for (int b = 0; b < B; ++b) need = std::max(need, wm_scan_windows(len32[b], S));
  if (w_cap < need) return fail(VITS_ERR_ARG, "%s: w_cap %lld below the %lld windows of the longest item", what, (long long)w_cap, need);
  const StftTab* T = nullptr;
  TRY(stft_tab_get(device, WM_N, &T));
  OpDoor d(what, device);
  const long long Fmax = N >= WM_M + 1 ? 1 + N / WM_DH : 0;
  const long long lbs = (Fmax ? Fmax : 1) * WM_G;
  const size_t no = (size_t)B * VITS_WATERMARK_OFFSETS, nz = no * (size_t)w_cap;
  float* dx = d.up(x, (size_t)B * N);
  int* dl = d.up(len32.data(), B);
  float* dlb = d.dev<float>((size_t)B * lbs);
  double* dz = d.out<double>(nz ? nz : 1, 0);  // exactly 0 at and beyond W_o
  int* dp0 = d.out<int>(no);
  int* dw = d.out<int>(no);
  if (d.ok()) {
    const uint32_t mk = wm_mix(key);
    if (Fmax > 0)
      hipLaunchKernelGGL(wm_lb_kernel, dim3((unsigned)cdiv((int)Fmax, SF_FPB), B), dim3(64 * SF_FPB), 0, nullptr, dx, N, dl, T->d_win, T->d_tw, dlb, lbs);
    const dim3 grid(VITS_WATERMARK_OFFSETS, (unsigned)std::max(1LL, (need + WM_SCAN_CHUNK - 1) / WM_SCAN_CHUNK), B);
    if (flags & VITS_WATERMARK_SCAN_PILOTS)
      hipLaunchKernelGGL(wm_scan_kernel<true>, grid, dim3(WM_SCORE_THREADS), 0, nullptr, dlb, lbs, dl, mk, S, (long long)w_cap, dz, dp0, dw);
    else
      hipLaunchKernelGGL(wm_scan_kernel<false>, grid, dim3(WM_SCORE_THREADS), 0, nullptr, dlb, lbs, dl, mk, S, (long long)w_cap, dz, dp0, dw);
  }
  d.finish();
  if (nz) d.down(z_scan, dz, nz);
  d.down(first_period, dp0, no);
  d.down(windows, dw, no);
  return d.rc();
}
