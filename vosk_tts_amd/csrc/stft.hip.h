// stft.hip.h -- the frame transform of the output tail and what goes round it: the denoiser (denoise.hip.h), the pitch vocoder
// (pitch.hip.h), the contours (contour.hip.h) and the watermark (watermark.hip.h) all frame, transform, pack, invert and overlap-add
// with the device functions of this file and the tables of stft_tab_get.  Part of the ONE translation unit engine.hip (included there,
// in front of denoise.hip.h).
//
// A stage's frames kernel runs one wave per frame, SF_FPB frames per workgroup, on __shared__ float lds[SF_FPB][4][SF_PLANE]:
//   sf_frame_load   the frame, read with reflect indexing, the item's own length and the window, two samples to a complex point
//   sf_fft          the real n-point transform as an M = n/2 point complex FFT in LDS (Stockham autosort, radix-4 passes and one
//                   radix-2 pass when log2 M is odd)
//   sf_unpack       the half-size spectrum to the bins k and M - k of the real transform, in registers
//   sf_pack         a pair of bins back to the half-size spectrum, conjugated, so that the SAME forward passes invert it
//   sf_frame_store  1 / M, the window, the frame to a scratch [frames, n]
// and its overlap-add kernel is a gather:
//   sf_ola_sum      an output sample sums its four or fewer frames in ascending frame order; the caller multiplies by the row of
//                   the host-computed 1 / sum w^2 that the function names (three rows: the first hop samples miss frame -1, the
//                   last hop miss frame F)
// Where fp32 bins are not enough (pitch_formant_kernel, contour_analysis_kernel: the reasons stand there) a wave transforms its
// 1024-sample frame in double: sf_frame_spectrum_f64 and sf_bin_f64, on double2 LDS that the kernel declares.
//
// LDS: re and im planes apart (4-byte accesses), ping and pong, index i stored at i + (i >> 4).  Reads of a pass are contiguous
// across the lanes; its writes go to 4 (j - k) + k + r Ns, a power-of-two stride that unpadded puts 4 lanes of a 32-lane group on
// one bank in the Ns = 1 and Ns = 4 passes; with the padding no pass has more than 2 (worked out from the bank rule for every
// pass of M = 32 .. 512, not measured).  4 x 544 floats = 8.5 KiB per 1024-sample frame, 34 KiB per workgroup.
#pragma once
#include "../../include/vits_denoise.h"

#define SF_FPB 4                        // frames (= waves) per workgroup
#define SF_N VITS_DENOISE_MAX_FILTER    // the longest frame, and the frame of the double-precision transform
#define SF_MAXM (SF_N / 2)
#define SF_LOG2MAXM 9
#define SF_PAD(i) ((i) + ((i) >> 4))
#define SF_PLANE (SF_MAXM + SF_MAXM / 16)
static_assert((1 << SF_LOG2MAXM) == SF_MAXM, "log2 of the half-size transform");

// sample p of the reflect-padded item (p counts from the start of the padding): x[b] holds samples x_off .. x_off + x_n of it
__device__ __forceinline__ float sf_load(const float* __restrict__ xb, long long p, int M, long long len, long long x_off, long long x_n) {
  long long k = p - M;
  if (k < 0) k = -k;
  if (k >= len) k = 2 * (len - 1) - k;
  const long long kk = k - x_off;
  return (k >= 0 && k < len && kk >= 0 && kk < x_n) ? xb[kk] : 0.f;
}

// The windowed frame that starts at padded position p0 into the wave's planes, samples 2 m and 2 m + 1 to point m (lane t of the
// wave; a wave that is not valid transforms zeros).  p0 is frame index times the caller's hop.
__device__ __forceinline__ void sf_frame_load(const float* __restrict__ xb, long long p0, int M, long long len, long long x_off, long long x_n,
                                              const float* __restrict__ win, bool valid, int t, float* ar, float* ai) {
  for (int m = t; m < M; m += 64) {
    float v0 = 0.f, v1 = 0.f;
    if (valid) {
      const long long p = p0 + 2 * m;
      v0 = sf_load(xb, p, M, len, x_off, x_n) * win[2 * m];
      v1 = sf_load(xb, p + 1, M, len, x_off, x_n) * win[2 * m + 1];
    }
    ar[SF_PAD(m)] = v0;
    ai[SF_PAD(m)] = v1;
  }
}

// forward M-point FFT of the wave's planes (a -> result left in a; b is the other buffer).  tw is the n-point table
// tw[t] = exp(-2 pi i t / n), n = 2 M.  Every thread of the workgroup calls it (the barriers are the workgroup's).
__device__ __forceinline__ void sf_fft(float*& ar, float*& ai, float*& br, float*& bi, int M, int log2m, const float2* __restrict__ tw, int t) {
  int Ns = 1, rem = log2m;
  while (rem >= 2) {
    const int Q = M >> 2;
    for (int j = t; j < Q; j += 64) {
      const int k = j & (Ns - 1);
      const int ts = (M / (4 * Ns)) * 2 * k;  // 3 ts < 3 n / 4
      const float2 w1 = tw[ts], w2 = tw[2 * ts], w3 = tw[3 * ts];
      const float x0r = ar[SF_PAD(j)], x0i = ai[SF_PAD(j)];
      const float x1r = ar[SF_PAD(j + Q)], x1i = ai[SF_PAD(j + Q)];
      const float x2r = ar[SF_PAD(j + 2 * Q)], x2i = ai[SF_PAD(j + 2 * Q)];
      const float x3r = ar[SF_PAD(j + 3 * Q)], x3i = ai[SF_PAD(j + 3 * Q)];
      const float v1r = x1r * w1.x - x1i * w1.y, v1i = x1r * w1.y + x1i * w1.x;
      const float v2r = x2r * w2.x - x2i * w2.y, v2i = x2r * w2.y + x2i * w2.x;
      const float v3r = x3r * w3.x - x3i * w3.y, v3i = x3r * w3.y + x3i * w3.x;
      const float a0r = x0r + v2r, a0i = x0i + v2i, a1r = x0r - v2r, a1i = x0i - v2i;
      const float a2r = v1r + v3r, a2i = v1i + v3i;
      const float a3r = v1i - v3i, a3i = -(v1r - v3r);  // -i (v1 - v3)
      const int j0 = ((j - k) << 2) + k;
      br[SF_PAD(j0)] = a0r + a2r;          bi[SF_PAD(j0)] = a0i + a2i;
      br[SF_PAD(j0 + Ns)] = a1r + a3r;     bi[SF_PAD(j0 + Ns)] = a1i + a3i;
      br[SF_PAD(j0 + 2 * Ns)] = a0r - a2r; bi[SF_PAD(j0 + 2 * Ns)] = a0i - a2i;
      br[SF_PAD(j0 + 3 * Ns)] = a1r - a3r; bi[SF_PAD(j0 + 3 * Ns)] = a1i - a3i;
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
      const float x0r = ar[SF_PAD(j)], x0i = ai[SF_PAD(j)];
      const float x1r = ar[SF_PAD(j + H)], x1i = ai[SF_PAD(j + H)];
      const float v1r = x1r * w1.x - x1i * w1.y, v1i = x1r * w1.y + x1i * w1.x;
      const int j0 = ((j - k) << 1) + k;
      br[SF_PAD(j0)] = x0r + v1r;      bi[SF_PAD(j0)] = x0i + v1i;
      br[SF_PAD(j0 + Ns)] = x0r - v1r; bi[SF_PAD(j0 + Ns)] = x0i - v1i;
    }
    __syncthreads();
    float* s = ar; ar = br; br = s;
    s = ai; ai = bi; bi = s;
  }
}

// the bins k and kp = M - k of the real transform
struct SfBins { float kr, ki, pr, pi; };

// Z (in a) -> X[k] = E + W^k O, X[kp] = conj(E - W^k O), with E = (Z[k] + conj Z[kp]) / 2, O = -i (Z[k] - conj Z[kp]) / 2,
// W = exp(-2 pi i / n), Z[M] = Z[0]; 0 <= k <= M / 2
__device__ __forceinline__ SfBins sf_unpack(const float* ar, const float* ai, const float2* __restrict__ tw, int M, int k) {
  const int kp = M - k, kq = kp & (M - 1);
  const float zkr = ar[SF_PAD(k)], zki = ai[SF_PAD(k)], zpr = ar[SF_PAD(kq)], zpi = ai[SF_PAD(kq)];
  const float2 w = tw[k];
  const float er = 0.5f * (zkr + zpr), ei = 0.5f * (zki - zpi);
  const float o_r = 0.5f * (zki + zpi), o_i = -0.5f * (zkr - zpr);
  const float tr = w.x * o_r - w.y * o_i, ti = w.x * o_i + w.y * o_r;
  SfBins X;
  X.kr = er + tr; X.ki = ei + ti; X.pr = er - tr; X.pi = -(ei - ti);
  return X;
}

// back, into b: Z'[k] = E2 + i O2, Z'[kp] = conj(E2) + i conj(O2), E2 = (X[k] + conj X[kp]) / 2, O2 = (X[k] - conj X[kp]) / 2 * conj(W^k);
// stored conjugated: the inverse transform is conj(FFT(conj Z')) / M
__device__ __forceinline__ void sf_pack(float* br, float* bi, const float2* __restrict__ tw, int M, int k, float xkr, float xki, float xpr,
                                        float xpi) {
  const int kp = M - k;
  const float2 w = tw[k];
  const float e2r = 0.5f * (xkr + xpr), e2i = 0.5f * (xki - xpi);
  const float dr = 0.5f * (xkr - xpr), di = 0.5f * (xki + xpi);
  const float o2r = dr * w.x + di * w.y, o2i = di * w.x - dr * w.y;
  br[SF_PAD(k)] = e2r - o2i;
  bi[SF_PAD(k)] = -(e2i + o2r);
  if (k > 0 && kp != k) {
    br[SF_PAD(kp)] = e2r + o2i;
    bi[SF_PAD(kp)] = -(o2r - e2i);
  }
}

// the inverted frame (in a, still conjugated) times 1 / M and the window to frame[0 .. n)  (n and every stride are even: 8-byte aligned)
__device__ __forceinline__ void sf_frame_store(const float* ar, const float* ai, int M, const float* __restrict__ win, int t,
                                               float* __restrict__ frame) {
  const float inv_m = 1.0f / (float)M;
  float2* of = reinterpret_cast<float2*>(frame);
  for (int m = t; m < M; m += 64)
    of[m] = make_float2(ar[SF_PAD(m)] * inv_m * win[2 * m], -ai[SF_PAD(m)] * inv_m * win[2 * m + 1]);
}

// The overlap-add of one output sample: padded position p = fl hop + r, the frames f = fl - 3 .. fl of an item's F that the scratch
// fb holds from f_begin on (frame f at (f - f_begin) * n), in ascending order.  *region: the row of the 1 / sum w^2 table that holds
// for it (0 head, 1 interior, 2 tail).  0 <= f < F is written as the one unsigned comparison the compiler makes of it in a kernel of
// its own (F is a frame count, never negative): as two signed comparisons in this shared function wm_ola_kernel takes 14 VGPRs, not 12.
__device__ __forceinline__ float sf_ola_sum(const float* __restrict__ fb, long long fl, int r, int n, int hop, long long F, long long f_begin,
                                            int* region) {
  *region = fl < 3 ? 0 : (fl >= F ? 2 : 1);
  float acc = 0.f;
  for (int d = 3; d >= 0; --d) {
    const long long f = fl - d;
    if ((unsigned long long)f < (unsigned long long)F && f >= f_begin) acc += fb[(f - f_begin) * n + r + d * hop];  // 0 <= f < F
  }
  return acc;
}

// The SF_N-sample frame at padded position p0 transformed in double, by the SF_FPB waves of a workgroup at once: the twiddles
// exp(-2 pi i t / n), t < n/2, to s_tw (the workgroup's), the window as sinpi^2, the packed frame in bit-reversed order to the wave's
// Z [SF_MAXM] and the radix-2 passes in place.  Every thread of the workgroup calls it (the barriers are the workgroup's).
__device__ __forceinline__ void sf_frame_spectrum_f64(const float* __restrict__ xb, long long p0, long long len, long long x_n, bool valid, int t,
                                                      double2* s_tw, double2* Z) {
  for (int i = threadIdx.x; i < SF_MAXM; i += 64 * SF_FPB) {
    double sn, cs;
    sincospi((double)i * (2.0 / SF_N), &sn, &cs);
    s_tw[i] = make_double2(cs, -sn);
  }
  // the windowed frame, two samples to a complex point, in bit-reversed order (a wave that is not valid transforms zeros)
  for (int m = t; m < SF_MAXM; m += 64) {
    double v0 = 0.0, v1 = 0.0;
    if (valid) {
      const long long p = p0 + 2 * m;
      const double w0 = sinpi((double)(2 * m) * (1.0 / SF_N)), w1 = sinpi((double)(2 * m + 1) * (1.0 / SF_N));
      v0 = (double)sf_load(xb, p, SF_MAXM, len, 0, x_n) * (w0 * w0);
      v1 = (double)sf_load(xb, p + 1, SF_MAXM, len, 0, x_n) * (w1 * w1);
    }
    Z[__brev((unsigned)m) >> (32 - SF_LOG2MAXM)] = make_double2(v0, v1);
  }
  __syncthreads();
  for (int h = 1; h < SF_MAXM; h <<= 1) {  // groups of 2 h points, twiddle exp(-2 pi i pos / (2 h))
    for (int j = t; j < SF_MAXM / 2; j += 64) {
      const int pos = j & (h - 1), i0 = ((j - pos) << 1) + pos, i1 = i0 + h;
      const double2 w = s_tw[pos * (SF_MAXM / h)], u = Z[i0], v = Z[i1];
      const double tr = w.x * v.x - w.y * v.y, ti = w.x * v.y + w.y * v.x;
      Z[i0] = make_double2(u.x + tr, u.y + ti);
      Z[i1] = make_double2(u.x - tr, u.y - ti);
    }
    __syncthreads();
  }
}

// X[k] = E[k] + exp(-2 pi i k / n) O[k] of that packed transform, 0 <= k <= n/2
__device__ __forceinline__ double2 sf_bin_f64(const double2* Z, const double2* s_tw, int k) {
  const double2 zk = Z[k & (SF_MAXM - 1)], zp = Z[(SF_MAXM - k) & (SF_MAXM - 1)];
  const double2 w = k < SF_MAXM ? s_tw[k] : make_double2(-1.0, 0.0);
  const double er = 0.5 * (zk.x + zp.x), ei = 0.5 * (zk.y - zp.y), o_r = 0.5 * (zk.y + zp.y), o_i = -0.5 * (zk.x - zp.x);
  const double xr = er + (w.x * o_r - w.y * o_i), xi = ei + (w.x * o_i + w.y * o_r);
  return make_double2(xr, xi);
}

// ---- host tables, cached per (device, frame length) -------------------------------------------------------------------------
struct StftTab {
  int n = 0, log2m = 0;
  float* d_win = nullptr;    // [n]
  float2* d_tw = nullptr;    // [n]  exp(-2 pi i t / n)
  float* d_env = nullptr;    // [3][hop]  1 / sum w^2: head (frame -1 missing), interior, tail (frame F missing)
};
static DevTabs<std::pair<int, int>, StftTab> g_sf_tabs;  // at most five frame lengths per device

// Uploads on first use (hipMalloc + a synchronous copy: call it outside stream capture).  n: a power of two in
// [VITS_DENOISE_MIN_FILTER, VITS_DENOISE_MAX_FILTER] (denoise_filter_arg).
static int stft_tab_get(int device, int n, const StftTab** out) {
  return g_sf_tabs.get(std::make_pair(device, n), out, [&](StftTab& T) {
    T.n = n;
    for (int m = n >> 1; m > 1; m >>= 1) ++T.log2m;
    const int hop = n / 4;
    std::vector<float> host((size_t)3 * n + 3 * hop);  // tw | win | env, as on the device
    float *tw = host.data(), *win = tw + 2 * n, *env = win + n;
    std::vector<double> w2(n);
    for (int i = 0; i < n; ++i) {
      const double s = sin(M_PI * (double)i / (double)n), a = 2.0 * M_PI * (double)i / (double)n;
      win[i] = (float)(s * s);
      w2[i] = (s * s) * (s * s);
      tw[2 * i] = (float)cos(a);
      tw[2 * i + 1] = (float)-sin(a);
    }
    for (int r = 0; r < hop; ++r) {
      env[r] = (float)(1.0 / (w2[r] + w2[r + hop] + w2[r + 2 * hop]));
      env[hop + r] = (float)(1.0 / (w2[r] + w2[r + hop] + w2[r + 2 * hop] + w2[r + 3 * hop]));
      env[2 * hop + r] = (float)(1.0 / (w2[r + hop] + w2[r + 2 * hop] + w2[r + 3 * hop]));
    }
    float* d = nullptr;
    TRY(dev_table_upload(device, "denoise", host.data(), host.size() * sizeof(float), (void**)&d));
    T.d_tw = reinterpret_cast<float2*>(d);
    T.d_win = d + 2 * n;
    T.d_env = d + 3 * n;
    return VITS_OK;
  });
}
