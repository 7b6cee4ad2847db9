// pitch.hip.h -- pitch-shifted output (include/vits_pitch.h): an identity-phase-locked vocoder that stretches the finished waveform by
// P/Q, then the resampler (P -> Q).  Part of the ONE translation unit engine.hip (included there, after stft.hip.h, whose frame
// transform it runs at n = 1024: the device functions, the LDS layout and the StftTab).
//
// Launches per group of items (every kernel derives an item's F_a, F_s and N_u from its length: no per-item host tables):
//   pitch_analysis_kernel  one wave per frame, load, transform and unpack of stft.hip.h: |X| and the phase as a 32-bit
//                          fixed-point turn, [B][F_a + 2][NB]; the two rows behind an item's last frame are written as zeros
//   pitch_formant_kernel   (VITS_FLAG_PITCH_FORMANT only) one wave per analysis row: the cepstral envelope of the row and the gain that
//                          pre-warps it, mag' = mag g, [B][F_a + 2][NB]; pitch_synth_kernel then reads mag' where it read mag, and
//                          pitch_phase_kernel still reads mag: the phases are those of the plain call
//   pitch_phase_kernel     one workgroup per item, one thread per bin, a loop over the steps t.  Phi_{t-1}[k] stays in thread k's
//                          register; a step stages m_t, adv and theta_i in LDS, tests the peak against the four neighbours, publishes
//                          the peaks as one 64-bit ballot per wave and finds the nearest set bit either side of k in those nine words;
//                          two barriers per step (the LDS is double-buffered by the parity of t).  The five global rows of the next
//                          PT_AHEAD steps are in flight while one step computes: their addresses depend on t alone.
//   pitch_synth_kernel     one wave per step: the interpolated magnitude times sincospif of the phase, then pack, inverse and
//                          windowed store of stft.hip.h: [B][F_s][n]
//   pitch_ola_kernel       the gather of stft.hip.h with the frame count F_s of the item (an F_s of 2 or 3, which a 513-sample item
//                          has at -12, is below what the denoiser takes); 1 / sum w^2 from the StftTab rows, and for the one case
//                          they do not hold (F_s = 2: both neighbours missing) formed in double in the kernel
//   pitch_geom_kernel      N_u / H and min(len, N_v) per item, for the resampler
//   resample_kernel<float, true>   u -> y, cropped; pitch_short_kernel copies the items below n/2 + 1 samples
#pragma once
#include <memory>
#include "../../include/vits_pitch.h"

#define PT_N VITS_PITCH_FRAME
#define PT_M (PT_N / 2)
#define PT_H (PT_N / 4)
#define PT_NB (PT_M + 1)
#define PT_LOG2M 9
#define PT_WAVES 9                       // of pitch_phase_kernel: 576 threads, bin k = threadIdx.x < PT_NB
#define PT_AHEAD 4                       // steps whose rows pitch_phase_kernel has in flight
static_assert(PT_N == SF_N && PT_LOG2M == SF_LOG2MAXM, "the pitch stage runs on the 1024-point frame transform of stft.hip.h");
static_assert(PT_WAVES * 64 >= PT_NB, "a thread per bin");

__host__ __device__ __forceinline__ long long pt_frames_a(long long len) { return len >= PT_M + 1 ? 1 + len / PT_H : 0; }
__host__ __device__ __forceinline__ long long pt_frames_s(long long len, int P, int Q) {
  const long long fa = pt_frames_a(len);
  return fa ? ((fa + 1) * P + Q - 1) / Q : 0;
}

__device__ __forceinline__ unsigned pt_theta(float re, float im) {
  if (re == 0.f && im == 0.f) return 0u;
  const float t = __fdiv_rn(atan2f(im, re), 6.28318530717958647692f);
  return (unsigned)(long long)rintf(t * 4294967296.f);  // |t| <= 0.5: the product is exact, the cast keeps the low 32 bits
}

// m_t[k] of step 2: one rounding per operation, as the restatement has them
__device__ __forceinline__ float pt_interp(float a, float b, float alpha) {
  return __fadd_rn(__fmul_rn(__fsub_rn(1.f, alpha), a), __fmul_rn(alpha, b));
}

// Rows [0, F_a + 2) of every item: wave w of workgroup blockIdx.x owns row blockIdx.x * SF_FPB + w.  x, x_n and len as
// sf_frame_load takes them (x_off = 0); mag / th: [B][a_bstride], row f at f * PT_NB.
__global__ __launch_bounds__(64 * SF_FPB) void pitch_analysis_kernel(const float* __restrict__ x, long long x_bstride, long long x_n, const Items it,
                                                                     const float* __restrict__ win, const float2* __restrict__ tw,
                                                                     float* __restrict__ mag, unsigned* __restrict__ th, long long a_bstride) {
  __shared__ float lds[SF_FPB][4][SF_PLANE];
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  const int b = blockIdx.y;
  const long long len = it.len_in(b);
  const long long Fa = pt_frames_a(len);
  if (Fa == 0 || (long long)blockIdx.x * SF_FPB >= Fa + 2) return;  // uniform over the workgroup
  const long long f = (long long)blockIdx.x * SF_FPB + wv;
  const bool valid = f < Fa;
  float *ar = lds[wv][0], *ai = lds[wv][1], *br = lds[wv][2], *bi = lds[wv][3];
  const float* xb = x + (long long)b * x_bstride;
  sf_frame_load(xb, f * PT_H, PT_M, len, 0, x_n, win, valid, t, ar, ai);
  __syncthreads();
  sf_fft(ar, ai, br, bi, PT_M, PT_LOG2M, tw, t);
  if (f >= Fa + 2) return;
  float* mo = mag + (long long)b * a_bstride + f * PT_NB;
  unsigned* to = th + (long long)b * a_bstride + f * PT_NB;
  for (int k = t; k <= (PT_M >> 1); k += 64) {
    const int kp = PT_M - k;
    const SfBins X = sf_unpack(ar, ai, tw, PT_M, k);
    mo[k] = valid ? sqrtf(X.kr * X.kr + X.ki * X.ki) : 0.f;
    mo[kp] = valid ? sqrtf(X.pr * X.pr + X.pi * X.pi) : 0.f;
    to[k] = valid ? pt_theta(X.kr, X.ki) : 0u;
    to[kp] = valid ? pt_theta(X.pr, X.pi) : 0u;
  }
}

// Steps 3a-3d of include/vits_pitch.h (VITS_FLAG_PITCH_FORMANT) on rows [0, F_a + 2) of every item, the grid and the row ownership of
// pitch_analysis_kernel: out_f[k] = mag_f[k] g_f[k] (GAIN: g_f[k] itself, and mag is not read), zeros in the two rows behind the last
// frame.
//   The magnitudes under the logarithm are not the fp32 rows of pitch_analysis_kernel: those sit a few 1e-7 of the frame's level from
// the exact spectrum, which the logarithm turns into a relative error of 1e-4 and more at a bin near zero (the reflect-symmetric first
// frame has many: its spectrum is real up to a linear phase and crosses zero), and every such bin moves the whole envelope of its row
// (measured through vits_op_pitch_formant_gain: 3.2 to 4.5 times the fp32 restatement's distance from float64, where the rest of this
// kernel adds nothing that shows).  So a wave transforms its frame again in double (sf_frame_spectrum_f64 and sf_bin_f64
// of stft.hip.h), the magnitude rounded to fp32 once.  From there on fp32.
//   A wave keeps L of its row in LDS; lane t sums D[k] cos(2 pi k q / n), D = L - L[0], over its bins k = t + 64 j into C + 1 registers
// (k = 0 carries D = 0 and adds nothing; the cosine comes from the n-entry table in LDS, padded by one word per 32 so that the stride
// 32 k of q = 32 spreads over the banks), a butterfly adds the lanes (the same order in every lane, so every lane holds the same
// c[q]), and each lane then forms the two series of 3c for its bins: e(k) from the table, e(kappa_k) with cospif of 2 r / (Q n).  No
// transform for the cepstrum: at C = 40 the direct sums are about 42 k multiply-adds a row.
#define PT_C VITS_PITCH_LIFTER
#define PT_COS(i) ((i) + ((i) >> 5))
static_assert(PT_M * 1999 < (1 << 30) && 1000 * PT_N < (1 << 30), "k P, Q n and r + (k P mod Q n) stay below 2^31");

template <bool GAIN>
__global__ __launch_bounds__(64 * SF_FPB) void pitch_formant_kernel(const float* __restrict__ x, long long x_bstride, long long x_n,
                                                                    const float* __restrict__ mag, long long a_bstride, const Items it, int P, int Q,
                                                                    float* __restrict__ out) {
  __shared__ double2 s_tw[PT_M];  // exp(-2 pi i t / n), t < n/2
  __shared__ double2 s_z[SF_FPB][PT_M];
  __shared__ float s_cos[PT_N + PT_N / 32];
  __shared__ float s_l[SF_FPB][PT_NB];
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  const int b = blockIdx.y;
  const long long len = it.len_in(b);
  const long long Fa = pt_frames_a(len);
  if (Fa == 0 || (long long)blockIdx.x * SF_FPB >= Fa + 2) return;  // uniform over the workgroup
  const long long f = (long long)blockIdx.x * SF_FPB + wv;
  const bool valid = f < Fa;
  for (int i = threadIdx.x; i < PT_N; i += 64 * SF_FPB) s_cos[PT_COS(i)] = cospif((float)i * (2.f / PT_N));
  double2* Z = s_z[wv];
  sf_frame_spectrum_f64(x + (long long)b * x_bstride, f * PT_H, len, x_n, valid, t, s_tw, Z);
  float* L = s_l[wv];
  if (valid)
    for (int k = t; k < PT_NB; k += 64) {
      const double2 X = sf_bin_f64(Z, s_tw, k);
      L[k] = logf(fmaxf((float)sqrt(X.x * X.x + X.y * X.y), VITS_PITCH_LOG_FLOOR));
    }
  __syncthreads();
  if (f >= Fa + 2) return;
  float* o = out + (long long)b * a_bstride + f * PT_NB;
  if (!valid) {
    for (int k = t; k < PT_NB; k += 64) o[k] = 0.f;
    return;
  }
  float c[PT_C + 1];
#pragma unroll
  for (int q = 0; q <= PT_C; ++q) c[q] = 0.f;
  const float* mi = mag + (long long)b * a_bstride + f * PT_NB;  // (a row of this item: f < F_a)
  const float l0 = L[0];
  for (int k = t; k < PT_M; k += 64) {
    const float d = L[k] - l0;
    int idx = 0;
#pragma unroll
    for (int q = 0; q <= PT_C; ++q) {
      c[q] = fmaf(d, s_cos[PT_COS(idx)], c[q]);
      idx = (idx + k) & (PT_N - 1);
    }
  }
  const float d0 = 0.f, dm = L[PT_M] - l0;  // D[0], D[n/2]
#pragma unroll
  for (int q = 0; q <= PT_C; ++q) {
    float s = c[q];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    c[q] = (d0 + ((q & 1) ? -dm : dm) + 2.f * s) * (1.f / PT_N);
  }
  const int QN = Q * PT_N;
  const float g_max = (float)(VITS_PITCH_FORMANT_MAX_DB * 2.30258509299404568402 / 20.0), qn_f = (float)QN;
  for (int k = t; k < PT_NB; k += 64) {
    const int kP = k * P, step = kP % QN;
    const bool top = kP >= PT_M * Q;  // kappa_k = n/2
    int idx = 0, r = 0;
    float sk = 0.f, sx = 0.f;
#pragma unroll
    for (int q = 1; q <= PT_C; ++q) {
      idx = (idx + k) & (PT_N - 1);
      r += step;
      if (r >= QN) r -= QN;
      const float cx = top ? ((q & 1) ? -1.f : 1.f) : cospif(__fdiv_rn((float)(2 * r), qn_f));
      sk = fmaf(c[q], s_cos[PT_COS(idx)], sk);
      sx = fmaf(c[q], cx, sx);
    }
    const float ek = c[0] + 2.f * sk, ex = c[0] + 2.f * sx;
    const float g = expf(fminf(fmaxf(ex - ek, -g_max), g_max));
    if constexpr (GAIN) o[k] = g;
    else o[k] = mi[k] * g;
  }
}

// The step table of include/vits_contour.h (TAB instantiations of the three kernels below): row b of `steps` is F_s, a_0 .. a_{F_s} at
// stride s_bstride.  What a kernel takes from it is clamped to what the item's length allows -- F_s <= 2 (F_a + 1), i_t <= F_a -- so no
// loop bound and no row address rests on the table's contents alone.  The plain instantiations do not read it.
#define PT_ONE (1LL << 24)
__device__ __forceinline__ long long pt_tab_fs(const long long* __restrict__ row, long long Fa) {
  const long long fs = row[0], cap = 2 * (Fa + 1);
  return Fa ? (fs < 0 ? 0 : (fs > cap ? cap : fs)) : 0;
}
__device__ __forceinline__ int pt_tab_i(long long a, long long Fa) {
  const long long i = a >> 24;
  return (int)(i < 0 ? 0 : (i > Fa ? Fa : i));
}

// One workgroup per item (blockIdx.x), thread k = bin k.  phi: [B][p_bstride], row t at t * PT_NB.
template <bool TAB>
__global__ __launch_bounds__(64 * PT_WAVES) void pitch_phase_kernel(const float* __restrict__ mag, const unsigned* __restrict__ th,
                                                                    long long a_bstride, const Items it, int P, int Q, const long long* __restrict__ steps,
                                                                    long long s_bstride, unsigned* __restrict__ phi, long long p_bstride) {
  __shared__ float s_m[2][PT_NB + 4];  // m[k] at k + 2; -1 either side
  __shared__ unsigned s_adv[2][PT_NB], s_th[2][PT_NB];
  __shared__ unsigned long long s_pk[2][PT_WAVES];
  const int b = blockIdx.x, k = threadIdx.x, wv = k >> 6, lane = k & 63;
  const long long len = it.len_in(b);
  const long long Fa = pt_frames_a(len);
  const long long* ab = TAB ? steps + (long long)b * s_bstride + 1 : nullptr;  // a_0 ..
  long long Fs;
  if constexpr (TAB) Fs = pt_tab_fs(ab - 1, Fa);
  else Fs = pt_frames_s(len, P, Q);
  if (Fs == 0) return;
  const bool act = k < PT_NB;
  const int kc = act ? k : 0;  // (the idle lanes of the last wave form valid addresses and touch nothing)
  const float* mb = mag + (long long)b * a_bstride + kc;
  const unsigned* tb = th + (long long)b * a_bstride + kc;
  unsigned* pb = phi + (long long)b * p_bstride + kc;
  if (k < 2) {
    s_m[0][k] = s_m[1][k] = -1.f;
    s_m[0][PT_NB + 2 + k] = s_m[1][PT_NB + 2 + k] = -1.f;
  }
  unsigned ph = act ? tb[0] : 0u;  // Phi_0 = theta_0
  if (act) pb[0] = ph;
  if (Fs <= 1) return;
  // The rows of the next PT_AHEAD steps are in flight while one step computes: the addresses of step t depend on t alone.  Every lane
  // loads -- the idle lanes of the last wave read bin 0 -- and past the last step the issue loads the last step's rows again, so it has
  // no branch around a load.  i_t and (t Q mod P) advance by Q / P and Q mod P in 32-bit scalar arithmetic: a 64-bit division per
  // step, which every lane would carry, cost more than the rest of the step (measured: 1.2 us a step with it).
  float q_a[PT_AHEAD], q_b[PT_AHEAD];
  unsigned q_tj[PT_AHEAD], q_tj1[PT_AHEAD], q_ti[PT_AHEAD];
  int q_r[PT_AHEAD];
  const int q_div = Q / P, q_rem = Q % P;
  long long n_t = 1;                    // the step the next issue is for
  int n_i = q_div, n_r = q_rem, n_j = 0;  // its i_t, t Q mod P (TAB: a_t mod 2^24) and i_{t-1}
  if constexpr (TAB) { n_i = pt_tab_i(ab[1], Fa); n_r = (int)(ab[1] & (PT_ONE - 1)); }
  auto issue = [&](int d) {
    q_r[d] = n_r;
    q_a[d] = mb[(long long)n_i * PT_NB]; q_b[d] = mb[(long long)(n_i + 1) * PT_NB];
    q_tj[d] = tb[(long long)n_j * PT_NB]; q_tj1[d] = tb[(long long)(n_j + 1) * PT_NB]; q_ti[d] = tb[(long long)n_i * PT_NB];
    if (n_t + 1 < Fs) {  // (uniform)
      ++n_t;
      n_j = n_i;
      if constexpr (TAB) {
        const long long a = ab[n_t];
        n_i = pt_tab_i(a, Fa); n_r = (int)(a & (PT_ONE - 1));
      } else {
        n_i += q_div; n_r += q_rem;
        if (n_r >= P) { n_r -= P; ++n_i; }
      }
    }
  };
#pragma unroll
  for (int d = 0; d < PT_AHEAD; ++d) issue(d);
  for (long long tau0 = 1; tau0 < Fs; tau0 += PT_AHEAD) {
#pragma unroll
   for (int d = 0; d < PT_AHEAD; ++d) {
    const long long tau = tau0 + d;
    if (tau >= Fs) break;  // (uniform)
    const float c_a = q_a[d], c_b = q_b[d];
    const unsigned c_tj = q_tj[d], c_tj1 = q_tj1[d], c_ti = q_ti[d];
    const int c_r = q_r[d];
    issue(d);
    const int pp = (int)(tau & 1);
    float alpha;
    if constexpr (TAB) alpha = (float)c_r * 5.9604644775390625e-08f;  // 2^-24: exact
    else alpha = __fdiv_rn((float)c_r, (float)P);
    const float m = pt_interp(c_a, c_b, alpha);
    const unsigned adv = ph + c_tj1 - c_tj;
    if (act) { s_m[pp][k + 2] = m; s_adv[pp][k] = adv; s_th[pp][k] = c_ti; }
    __syncthreads();
    bool pk = false;
    if (act) pk = m > s_m[pp][k + 1] && m > s_m[pp][k] && m >= s_m[pp][k + 3] && m >= s_m[pp][k + 4];
    const unsigned long long bal = __ballot(pk);
    if (lane == 0) s_pk[pp][wv] = bal;
    __syncthreads();
    if (act) {
      int lo = -1, hi = -1;  // the nearest peak at or below k, at or above k
      unsigned long long w = s_pk[pp][wv] & (~0ull >> (63 - lane));
      for (int ww = wv;;) {
        if (w) { lo = ww * 64 + 63 - __clzll((long long)w); break; }
        if (--ww < 0) break;
        w = s_pk[pp][ww];
      }
      w = s_pk[pp][wv] & (~0ull << lane);
      for (int ww = wv;;) {
        if (w) { hi = ww * 64 + __ffsll((unsigned long long)w) - 1; break; }
        if (++ww >= PT_WAVES) break;
        w = s_pk[pp][ww];
      }
      const int own = lo < 0 ? hi : (hi < 0 ? lo : (hi - k < k - lo ? hi : lo));  // a tie goes to the lower peak
      ph = own < 0 ? adv : s_adv[pp][own] + c_ti - s_th[pp][own];
      pb[tau * PT_NB] = ph;
    }
   }
  }
}

// Steps [0, F_s) of every item: wave w of workgroup blockIdx.x owns step blockIdx.x * SF_FPB + w.  fr: [B][fr_bstride], frame t at t * n.
template <bool TAB>
__global__ __launch_bounds__(64 * SF_FPB) void pitch_synth_kernel(const float* __restrict__ mag, long long a_bstride,
                                                                  const unsigned* __restrict__ phi, long long p_bstride, const Items it, int P, int Q,
                                                                  const long long* __restrict__ steps, long long s_bstride,
                                                                  const float* __restrict__ win, const float2* __restrict__ tw,
                                                                  float* __restrict__ fr, long long fr_bstride) {
  __shared__ float lds[SF_FPB][4][SF_PLANE];
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  const int b = blockIdx.y;
  const long long len = it.len_in(b);
  long long Fs;
  if constexpr (TAB) Fs = pt_tab_fs(steps + (long long)b * s_bstride, pt_frames_a(len));
  else Fs = pt_frames_s(len, P, Q);
  if ((long long)blockIdx.x * SF_FPB >= Fs) return;  // uniform over the workgroup
  const long long tau = (long long)blockIdx.x * SF_FPB + wv;
  const bool valid = tau < Fs;
  float *ar = lds[wv][0], *ai = lds[wv][1], *br = lds[wv][2], *bi = lds[wv][3];
  long long i;
  float alpha;
  if constexpr (TAB) {
    const long long a = valid ? steps[(long long)b * s_bstride + 1 + tau] : 0;
    i = pt_tab_i(a, pt_frames_a(len));
    alpha = (float)(int)(a & (PT_ONE - 1)) * 5.9604644775390625e-08f;
  } else {
    const long long tq = tau * Q;
    i = tq / P;
    alpha = __fdiv_rn((float)(int)(tq - i * P), (float)P);
  }
  const float* m0 = mag + (long long)b * a_bstride + i * PT_NB;
  const unsigned* pr = phi + (long long)b * p_bstride + tau * PT_NB;
  for (int k = t; k <= (PT_M >> 1); k += 64) {
    const int kp = PT_M - k;
    float xkr = 0.f, xki = 0.f, xpr = 0.f, xpi = 0.f;
    if (valid) {
      const float mk = pt_interp(m0[k], m0[PT_NB + k], alpha), mp = pt_interp(m0[kp], m0[PT_NB + kp], alpha);
      float s, c;
      sincospif(2.f * ((float)(int)pr[k] * 2.3283064365386963e-10f), &s, &c);  // 2^-32: the turn in [-0.5, 0.5)
      xkr = mk * c; xki = k > 0 ? mk * s : 0.f;
      sincospif(2.f * ((float)(int)pr[kp] * 2.3283064365386963e-10f), &s, &c);
      xpr = mp * c; xpi = k > 0 ? mp * s : 0.f;  // (kp = n/2 pairs with k = 0: both imaginary parts are dropped)
    }
    sf_pack(ar, ai, tw, PT_M, k, xkr, xki, xpr, xpi);
  }
  __syncthreads();
  sf_fft(ar, ai, br, bi, PT_M, PT_LOG2M, tw, t);
  if (!valid) return;
  sf_frame_store(ar, ai, PT_M, win, t, fr + (long long)b * fr_bstride + tau * PT_N);
}

// u[b][j], j < n_count: the overlap-add of the item's F_s frames, exactly 0 at and beyond N_u = H (F_s - 1).
template <bool TAB>
__global__ __launch_bounds__(256) void pitch_ola_kernel(const float* __restrict__ fr, long long fr_bstride, const Items it, int P, int Q,
                                                        const long long* __restrict__ steps, long long s_bstride, const float* __restrict__ inv_env,
                                                        float* __restrict__ u, long long u_bstride, long long n_count) {
  const int b = blockIdx.y;
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_count) return;
  const long long len = it.len_in(b);
  long long Fs;
  if constexpr (TAB) Fs = pt_tab_fs(steps + (long long)b * s_bstride, pt_frames_a(len));
  else Fs = pt_frames_s(len, P, Q);
  float v = 0.f;
  if (j < PT_H * (Fs - 1)) {
    const long long p = j + PT_M, fl = p / PT_H;  // fl in [2, F_s]
    const int r = (int)(p - fl * PT_H);
    int region;
    const float acc = sf_ola_sum(fr + (long long)b * fr_bstride, fl, r, PT_N, PT_H, Fs, 0, &region);
    float e;
    if (fl < 3 && fl >= Fs) {  // F_s = 2: frames 0 and 1 alone, head and tail at once
      const double s1 = sinpi((double)(r + PT_H) / PT_N), s2 = sinpi((double)(r + 2 * PT_H) / PT_N);
      e = (float)(1.0 / (s1 * s1 * s1 * s1 + s2 * s2 * s2 * s2));
    } else {
      e = inv_env[region * PT_H + r];
    }
    v = acc * e;
  }
  u[(long long)b * u_bstride + j] = v;
}

// nu[b] = N_u / H (the resampler's input length in units of H) and crop[b] = min(len, N_v); both 0 for an item below n/2 + 1
__global__ void pitch_geom_kernel(const Items it, int B, int P, int Q, int* __restrict__ nu, int* __restrict__ crop) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long len = it.len_in(b);
  const long long Fs = pt_frames_s(len, P, Q);
  const long long Nu = Fs ? PT_H * (Fs - 1) : 0, Nv = (Nu * Q + P - 1) / P;
  nu[b] = (int)(Nu / PT_H);
  crop[b] = (int)(len < Nv ? len : Nv);
}

// the items shorter than n/2 + 1 samples come back as they are (grid (2, B): 512 samples cover them)
__global__ __launch_bounds__(256) void pitch_short_kernel(const float* __restrict__ x, long long x_bstride, const Items it, float* __restrict__ y,
                                                          long long y_bstride, long long n_count) {
  const int b = blockIdx.y;
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long len = it.len_in(b);
  if (len >= PT_M + 1 || j >= len || j >= n_count) return;
  y[(long long)b * y_bstride + j] = x[(long long)b * x_bstride + j];
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct PitchReq { bool on = false; int P = 1, Q = 1; bool formant = false; float semitones = 0.f; };  // (semitones: what P / Q were planned from)

static int pitch_plan(float semitones, int* P, int* Q) {
  if (!(fabsf(semitones) <= (float)VITS_PITCH_MAX_SEMITONES))  // (NaN fails the comparison)
    return fail(VITS_ERR_ARG, "pitch: %g semitones outside [-%d, %d]", (double)semitones, VITS_PITCH_MAX_SEMITONES, VITS_PITCH_MAX_SEMITONES);
  const long p0 = lround(1000.0 * pow(2.0, (double)semitones / 12.0));
  long a = p0, b = 1000;
  while (b) { const long t = a % b; a = b; b = t; }
  *P = (int)(p0 / a);
  *Q = (int)(1000 / a);
  return VITS_OK;
}

// The resampler tables of the ratios in use, per (device, P, Q).  A server may see any of 1501 ratios, so unlike the output-rate tables
// (which captured graphs point into) these are evicted, least recently used first; a call in flight keeps its table alive.
// (Not a DevTabs of op_door.hip.h: that one never evicts and hands out plain pointers.)
#define PT_MAX_TABS 32
static std::mutex g_pt_mu;
static std::map<std::tuple<int, int, int>, std::pair<std::shared_ptr<ResampleTab>, uint64_t>> g_pt_tabs;
static uint64_t g_pt_tick = 0;

static int pitch_tab_get(int device, int P, int Q, std::shared_ptr<ResampleTab>* out) {
  std::lock_guard<std::mutex> g(g_pt_mu);
  const auto key = std::make_tuple(device, P, Q);
  auto it = g_pt_tabs.find(key);
  if (it == g_pt_tabs.end()) {
    std::shared_ptr<ResampleTab> T(new ResampleTab, [](ResampleTab* t) { if (t->d) hipFree(t->d); delete t; });
    TRY(resample_plan(P, Q, &T->P));
    HIP_TRY(hipSetDevice(device));
    TRY(resample_upload(device, *T));
    if (g_pt_tabs.size() >= PT_MAX_TABS) {
      auto old = g_pt_tabs.begin();
      for (auto i = g_pt_tabs.begin(); i != g_pt_tabs.end(); ++i) if (i->second.second < old->second.second) old = i;
      g_pt_tabs.erase(old);
    }
    it = g_pt_tabs.emplace(key, std::make_pair(T, 0)).first;
  }
  it->second.second = ++g_pt_tick;
  *out = it->second.first;
  return VITS_OK;
}

// bytes of scratch an item of `len` samples takes in a group (the strides of a group are those of its longest item)
static size_t pitch_item_bytes(long long len, int P, int Q, bool formant) {
  const long long Fa = pt_frames_a(len), Fs = pt_frames_s(len, P, Q);
  if (!Fa) return 2 * sizeof(int);
  return (size_t)(Fa + 2) * PT_NB * (formant ? 12 : 8) + (size_t)Fs * PT_NB * 4 + (size_t)Fs * PT_N * 4 + (size_t)(Fs - 1) * PT_H * 4 + 2 * sizeof(int) + 64;
}

// ---- the phase-vocoder group runner (this stage and contour.hip.h) -------------------------------------------------------
struct PvGroup { int b0, c; long long mx; };  // consecutive items whose scratch fits: the first, how many, the longest one's samples
struct PvCarve {  // the scratch of a group, handed out front to back
  char *base, *p;
  template <typename T>
  T* take(size_t n) { T* r = reinterpret_cast<T*>(p); p += sizeof(T) * n; return r; }
  void align8() { p += (8 - (p - base) % 8) % 8; }
};
struct PvGeom {  // what a stage's front() settles for a group
  Items it;                    // the group's items as the vocoder kernels see them
  long long Fa = 0, Fs = 0;    // analysis frames of the longest item (0: no vocoder launches); the steps the strides and grids hold
  int P = 1, Q = 1;            // the plain kernels' ratio
  long long *steps = nullptr, s_bs = 0;  // TAB: the group's step table, rows at s_bs
};

// B items of h_len samples through the vocoder on `stream`, group by group: one scratch of head_bytes + the largest group's bytes
// (item_bytes(len) of its longest item times its count, at most VITS_PITCH_MAX_SCRATCH), carved per group as front's own | mag | th |
// analysis' own | phi | (align 8) | frames | u | finish's own, then analysis -> phase -> synth -> ola.  Allocates, and waits for the
// stream before it frees: not capturable.  The stage supplies head(scr): its uploads in front of the groups; front(S, g, &v): its
// scratch in front and the group's geometry (both hipError_t; front may wait for the stream); analysis(S, g, v, D, mag, th, a_bs): step 1,
// returning the magnitudes the synthesis reads; finish(S, g, v, u, u_bs): what becomes of u [c][u_bs] (null: a group without frames).
// u_out (nullable): the stretch doors -- u of item b goes to u_out[b * u_bstride + j], j < u_bstride (zeros for a frameless group).
// `at`: what the refusal of an item that fits no group says behind "bytes of scratch".
template <bool TAB, typename ItemBytes, typename Head, typename Front, typename Analysis, typename Finish>
static int pv_run(const char* what, const char* at, int device, hipStream_t stream, const long long* h_len, int B, size_t head_bytes, float* u_out,
                  long long u_bstride, ItemBytes&& item_bytes, Head&& head, Front&& front, Analysis&& analysis, Finish&& finish) {
  const StftTab* D = nullptr;
  TRY(stft_tab_get(device, PT_N, &D));
  std::vector<PvGroup> groups;
  size_t need = 0;
  for (int b0 = 0; b0 < B;) {
    long long mx = 0;
    int c = 0;
    while (b0 + c < B && c < 65535) {
      const long long m2 = std::max(mx, h_len[b0 + c]);
      if (item_bytes(m2) * (size_t)(c + 1) > (size_t)VITS_PITCH_MAX_SCRATCH) break;
      mx = m2;
      ++c;
    }
    if (!c) return fail(VITS_ERR_UNSUPPORTED, "%s: an item of %lld samples needs %zu bytes of scratch%s (limit %lld)", what, h_len[b0],
                        item_bytes(h_len[b0]), at, (long long)VITS_PITCH_MAX_SCRATCH);
    need = std::max(need, item_bytes(mx) * (size_t)c);
    groups.push_back({b0, c, mx});
    b0 += c;
  }
  HIP_TRY(hipSetDevice(device));
  char* scr = nullptr;
  if (hipMalloc((void**)&scr, head_bytes + need) != hipSuccess) return fail(VITS_ERR_NOMEM, "%s: scratch alloc of %zu bytes failed", what, head_bytes + need);
  hipError_t e = head(scr);
  for (size_t gi = 0; gi < groups.size() && e == hipSuccess; ++gi) {
    const PvGroup& g = groups[gi];
    const int c = g.c;
    PvCarve S{scr, scr + head_bytes};
    PvGeom v;
    if ((e = front(S, g, &v)) != hipSuccess) break;
    float* u = nullptr;
    long long u_bs = 0;
    if (v.Fa) {
      const long long a_bs = (v.Fa + 2) * PT_NB, p_bs = v.Fs * PT_NB, f_bs = v.Fs * PT_N;
      float* mag = S.take<float>((size_t)c * a_bs);
      unsigned* th = S.take<unsigned>((size_t)c * a_bs);
      const float* magf = analysis(S, g, v, *D, mag, th, a_bs);
      unsigned* phi = S.take<unsigned>((size_t)c * p_bs);
      S.align8();  // (the frames are written as float2)
      float* fr = S.take<float>((size_t)c * f_bs);
      u_bs = u_out ? u_bstride : (v.Fs - 1) * PT_H;
      u = u_out ? u_out + (long long)g.b0 * u_bstride : S.take<float>((size_t)c * u_bs);
      hipLaunchKernelGGL(pitch_phase_kernel<TAB>, dim3(c), dim3(64 * PT_WAVES), 0, stream, mag, th, a_bs, v.it, v.P, v.Q, v.steps, v.s_bs, phi, p_bs);
      hipLaunchKernelGGL(pitch_synth_kernel<TAB>, dim3((unsigned)((v.Fs + SF_FPB - 1) / SF_FPB), c), dim3(64 * SF_FPB), 0, stream, magf, a_bs, phi,
                         p_bs, v.it, v.P, v.Q, v.steps, v.s_bs, D->d_win, D->d_tw, fr, f_bs);
      hipLaunchKernelGGL(pitch_ola_kernel<TAB>, dim3((unsigned)((u_bs + 255) / 256), c), dim3(256), 0, stream, fr, f_bs, v.it, v.P, v.Q, v.steps,
                         v.s_bs, D->d_env, u, u_bs, u_bs);
    } else if (u_out) {
      hipMemsetAsync(u_out + (long long)g.b0 * u_bstride, 0, sizeof(float) * (size_t)c * u_bstride, stream);
    }
    finish(S, g, v, u, u_bs);
  }
  if (e == hipSuccess) e = hipGetLastError();
  const hipError_t e2 = hipStreamSynchronize(stream);
  hipFree(scr);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) return fail(VITS_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
  return VITS_OK;
}

// y[b][0 .. n_count) = the shifted item b, for B items on `stream`; x / x_n / it as in denoise_launch (device pointers), h_len the
// items' lengths on the host.  pv_run's: not capturable.  y is not x.  u_out (nullable): the stretch door -- nothing is resampled.
// formant: steps 3a-3d -- the synthesis reads the corrected magnitudes, the phase recursion the plain ones.
static int pitch_run(int device, hipStream_t stream, const float* x, long long x_bstride, long long x_n, const Items& it, const long long* h_len,
                     int B, int P, int Q, bool formant, float* y, long long y_bstride, long long n_count, float* u_out, long long u_bstride) {
  if (B <= 0) return VITS_OK;
  std::shared_ptr<ResampleTab> R;  // (held until the stream has been waited for)
  if (!u_out) TRY(pitch_tab_get(device, P, Q, &R));
  char at[32];
  snprintf(at, sizeof at, " at %d/%d", P, Q);
  return pv_run<false>(
      "pitch", at, device, stream, h_len, B, 0, u_out, u_bstride, [&](long long len) { return pitch_item_bytes(len, P, Q, formant); },
      [](char*) { return hipSuccess; },
      [&](PvCarve&, const PvGroup& g, PvGeom* v) {
        *v = PvGeom{it.from(g.b0), pt_frames_a(g.mx), pt_frames_s(g.mx, P, Q), P, Q};
        return hipSuccess;
      },
      [&](PvCarve& S, const PvGroup& g, const PvGeom& v, const StftTab& D, float* mag, unsigned* th, long long a_bs) -> const float* {
        const float* xg = x + (long long)g.b0 * x_bstride;
        const dim3 grid((unsigned)((v.Fa + 2 + SF_FPB - 1) / SF_FPB), g.c);
        hipLaunchKernelGGL(pitch_analysis_kernel, grid, dim3(64 * SF_FPB), 0, stream, xg, x_bstride, x_n, v.it, D.d_win, D.d_tw, mag, th, a_bs);
        if (!formant) return mag;
        float* magf = S.take<float>((size_t)g.c * a_bs);
        hipLaunchKernelGGL(pitch_formant_kernel<false>, grid, dim3(64 * SF_FPB), 0, stream, xg, x_bstride, x_n, mag, a_bs, v.it, P, Q, magf);
        return magf;
      },
      [&](PvCarve& S, const PvGroup& g, const PvGeom& v, const float* u, long long u_bs) {
        if (u_out) return;
        float* yg = y + (long long)g.b0 * y_bstride;
        if (u) {  // N_u / H and the crop per item, then u -> y through the P -> Q resampler
          int* d_nu = S.take<int>(g.c);
          int* d_crop = S.take<int>(g.c);
          hipLaunchKernelGGL(pitch_geom_kernel, dim3((unsigned)((g.c + 63) / 64)), dim3(64), 0, stream, v.it, g.c, P, Q, d_nu, d_crop);
          resample_launch_crop(stream, *R, u, u_bs, u_bs, Items{d_nu, PT_H}, d_crop, g.c, yg, y_bstride, n_count);
        } else {
          for (int b = 0; b < g.c; ++b) hipMemsetAsync(yg + (long long)b * y_bstride, 0, sizeof(float) * (size_t)n_count, stream);
        }
        hipLaunchKernelGGL(pitch_short_kernel, dim3(2, g.c), dim3(256), 0, stream, x + (long long)g.b0 * x_bstride, x_bstride, v.it, yg, y_bstride, n_count);
      });
}

// what a shifting entry point of a vocoder needs checked before any work is queued
static int pitch_req(const vits_model* v, float semitones, bool formant, PitchReq* q) {
  q->on = false;
  int P = 1, Q = 1;
  TRY(pitch_plan(semitones, &P, &Q));
  if (P == Q) return VITS_OK;  // the identity: the call as it was
  if (v->hp.hop_length % PT_H)
    return fail(VITS_ERR_UNSUPPORTED, "pitch: the vocoder's hop_length %d is not a multiple of the pitch stage's hop %d", v->hp.hop_length, PT_H);
  ResamplePlan rp;
  TRY(resample_plan(P, Q, &rp));
  q->on = true; q->P = P; q->Q = Q; q->formant = formant; q->semitones = semitones;
  return VITS_OK;
}

// ---- entry points ----------------------------------------------------------------------------------------------------
int vits_pitch_plan(float semitones, int32_t* P, int32_t* Q) {
  int p = 1, q = 1;
  TRY(pitch_plan(semitones, &p, &q));
  if (P) *P = p;
  if (Q) *Q = q;
  return VITS_OK;
}

// the gains of step 3d for B items on the device (x [B][N], their lengths in dl): pitch_formant_kernel<true> into g [B][N / H + 3][NB],
// which the caller has zeroed (the rows at and beyond F_a + 2, and the items too short to have frames)
static int pitch_gain_run(int device, const float* dx, const int* dl, int B, long long N, int P, int Q, float* g) {
  const long long Fa = pt_frames_a(N), a_bs = (N / PT_H + 3) * PT_NB;
  if (!Fa) return VITS_OK;
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(pitch_formant_kernel<true>, dim3((unsigned)((Fa + 2 + SF_FPB - 1) / SF_FPB), B), dim3(64 * SF_FPB), 0, nullptr, dx, N, N,
                     (const float*)nullptr, a_bs, Items{dl, 1}, P, Q, g);
  hipError_t e = hipGetLastError();
  const hipError_t e2 = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) return fail(VITS_ERR_DEVICE, "pitch: %s", hipGetErrorString(e));
  return VITS_OK;
}

enum PitchDoor { PT_DOOR_SHIFT, PT_DOOR_STRETCH, PT_DOOR_GAIN };

static int pitch_op(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, float semitones, float* y, PitchDoor door,
                    bool formant) {
  const bool stretch = door == PT_DOOR_STRETCH;
  if (!y) return fail(VITS_ERR_ARG, "pitch: bad argument");
  std::vector<int> len32;
  TRY(op_items_check("pitch", x, lengths, B, N, &len32, "N = "));
  int P = 1, Q = 1;
  TRY(pitch_plan(semitones, &P, &Q));
  const std::vector<long long> len64(lengths, lengths + B);
  if (P == Q) {
    if (stretch) return fail(VITS_ERR_ARG, "pitch: %g semitones is the identity (P = Q): there is no stretch to return", (double)semitones);
    if (door == PT_DOOR_GAIN) return fail(VITS_ERR_ARG, "pitch: %g semitones is the identity (P = Q): there is no gain to return", (double)semitones);
    for (int b = 0; b < B; ++b) {
      memcpy(y + (size_t)b * N, x + (size_t)b * N, sizeof(float) * (size_t)lengths[b]);
      memset(y + (size_t)b * N + lengths[b], 0, sizeof(float) * (size_t)(N - lengths[b]));
    }
    return VITS_OK;
  }
  const long long Ny = stretch ? (long long)PT_H * (((N / PT_H + 2) * P + Q - 1) / Q - 1) : door == PT_DOOR_GAIN ? (N / PT_H + 3) * PT_NB : N;
  OpDoor d("pitch", device);
  float* dx = d.up_items(x, lengths, B, N);
  int* dl = d.up(len32.data(), B);
  // (the gain door's kernel writes rows [0, F_a + 2) only: the others are zeros from here)
  float* dy = d.out<float>((size_t)B * Ny, door == PT_DOOR_GAIN ? 0 : 0xff);
  const Items it{dl, 1};
  if (d.ok()) {
    if (door == PT_DOOR_GAIN) TRY(pitch_gain_run(device, dx, dl, B, N, P, Q, dy));
    else if (stretch) TRY(pitch_run(device, nullptr, dx, N, N, it, len64.data(), B, P, Q, formant, nullptr, 0, 0, dy, Ny));
    else TRY(pitch_run(device, nullptr, dx, N, N, it, len64.data(), B, P, Q, formant, dy, Ny, Ny, nullptr, 0));
  }
  d.finish();
  d.down(y, dy, (size_t)B * Ny);
  return d.rc();
}

int vits_op_pitch_shift(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, float semitones, float* y) {
  return pitch_op(device, x, lengths, B, N, semitones, y, PT_DOOR_SHIFT, false);
}
int vits_op_pitch_stretch(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, float semitones, float* y) {
  return pitch_op(device, x, lengths, B, N, semitones, y, PT_DOOR_STRETCH, false);
}
int vits_op_pitch_shift_formant(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, float semitones, float* y) {
  return pitch_op(device, x, lengths, B, N, semitones, y, PT_DOOR_SHIFT, true);
}
int vits_op_pitch_stretch_formant(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, float semitones, float* y) {
  return pitch_op(device, x, lengths, B, N, semitones, y, PT_DOOR_STRETCH, true);
}
int vits_op_pitch_formant_gain(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, float semitones, float* gain) {
  return pitch_op(device, x, lengths, B, N, semitones, gain, PT_DOOR_GAIN, false);
}
