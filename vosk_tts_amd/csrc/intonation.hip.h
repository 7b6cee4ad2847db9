// intonation.hip.h -- intonation range (include/vits_intonation.h): the F0 track of the finished waveform at the pitch stage's frame
// geometry, the integer offsets that scale its deviation from the median, and the frame tracks the contour stage then runs on.
// Part of the ONE translation unit engine.hip: included by contour.hip.h ahead of its host half (contour_run launches these kernels in
// place of contour_tracks_kernel where a call carries an IntonReq; the doors stand at the end of contour.hip.h).
//
// Launches per group of items, ahead of contour_steps_kernel:
//   f0_track_kernel          a wave per analysis row: the frame in LDS, lane l owns the lags l + 64 i; d, d', the decision, cents_f
//   intonation_item_kernel   a workgroup per item: the median by an LDS histogram, the unvoiced interpolation by two block scans, o_f, P_f
//                            and the item's word "some P_f is not 1000", which contour_run reads back
//   intonation_tracks_kernel contour_tracks_kernel with P_f in place of P_tok(f)
#pragma once
#include "../../include/vits_intonation.h"

#define IN_W VITS_INTONATION_WINDOW
#define IN_NI (IN_W / 64 + 1)            // lag blocks of a lane: tau = lane + 64 i <= IN_W
#define IN_CENTS VITS_INTONATION_MAX_CENTS
#define IN_TABN (2 * IN_CENTS + 1)
#define IN_BINS 8192                     // histogram bins of cents_f: f0 < 600 Hz at every accepted rate, 1200 log2(600 / 27.5) < 5400
#define IN_ITEM_T 256                    // threads of intonation_item_kernel
static_assert(IN_W == PT_M && IN_W + IN_W <= PT_N, "fr[j + tau], j < W, tau <= W stays inside the frame");

// What a call with the intonation flag hands the device (on: r_m != 1000); rate: the voice's own.
struct IntonReq {
  bool on = false;
  int r_m = 1000;
  int rate = 0;
};

__host__ __device__ __forceinline__ int in_tau_min(int rate) { const int t = rate / 550; return t < 2 ? 2 : t; }
__host__ __device__ __forceinline__ int in_tau_max(int rate) { const int t = (rate + 54) / 55; return t > IN_W - 1 ? IN_W - 1 : t; }
// rha(a / b), b > 0: round half away from zero
__host__ __device__ __forceinline__ long long in_rha(long long a, long long b) {
  const long long m = a < 0 ? -a : a, q = (2 * m + b) / (2 * b);
  return a < 0 ? -q : q;
}

// acc[i] += sum_{j < W} (fr[j] - fr[j + lane + 64 i])^2 for the NI lag blocks of a lane, in ascending j.  Block IN_NI - 1 holds the one lag
// IN_W: every lane computes it (one address, a broadcast), lane 0 owns it.
template <int NI>
__device__ __forceinline__ void in_diff(const float* __restrict__ fr, int lane, float* __restrict__ acc) {
  const float* fl = fr + lane;
#pragma unroll 4
  for (int j = 0; j < IN_W; ++j) {
    const float a = fr[j];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const float df = a - (i < IN_NI - 1 ? fl[j + 64 * i] : fr[j + IN_W]);
      acc[i] = fmaf(df, df, acc[i]);
    }
  }
}

// cents [B][c_bstride]: row f < 1 + len / H of every item (0: unvoiced, or an item below n/2 + 1 samples); the rows behind are the
// caller's zeros.  One wave per workgroup and row: a 50-token request is about 250 rows, one per compute unit.
// LDS: the fr[j] read is one address for the wave (a broadcast), fr[j + tau] are 64 consecutive words: neither conflicts.
__global__ __launch_bounds__(64) void f0_track_kernel(const float* __restrict__ x, long long x_bstride, long long x_n, const int* __restrict__ d_len,
                                                      int rate, int* __restrict__ cents, long long c_bstride) {
  __shared__ float s_fr[PT_N];
  __shared__ float s_dn[IN_W + 1];
  const int lane = threadIdx.x;
  const int b = blockIdx.y;
  const long long len = d_len[b];
  const long long f = blockIdx.x;
  if (len < 0 || f >= ct_frames(len) || f >= c_bstride) return;  // (uniform)
  int* out = cents + (long long)b * c_bstride + f;
  if (len < PT_M + 1) {  // (uniform) no track
    if (lane == 0) *out = 0;
    return;
  }
  const float* xb = x + (long long)b * x_bstride;
  for (int i = lane; i < PT_N; i += 64) s_fr[i] = sf_load(xb, f * PT_H + i, PT_M, len, 0, x_n);
  __syncthreads();
  const int tmin = in_tau_min(rate), tmax = in_tau_max(rate);
  const int ni = (tmax + 1) / 64 + 1;  // blocks that hold a lag <= tmax + 1 (uniform)
  // d(tau): one fp32 accumulator per lag, ascending j (the loop is compiled once per number of blocks: 3 at 8 kHz to 9 at 28 kHz and above)
  float acc[IN_NI];
#pragma unroll
  for (int i = 0; i < IN_NI; ++i) acc[i] = 0.f;
  switch (ni) {
    case 3: in_diff<3>(s_fr, lane, acc); break;
    case 4: in_diff<4>(s_fr, lane, acc); break;
    case 5: in_diff<5>(s_fr, lane, acc); break;
    case 6: in_diff<6>(s_fr, lane, acc); break;
    case 7: in_diff<7>(s_fr, lane, acc); break;
    case 8: in_diff<8>(s_fr, lane, acc); break;
    default: in_diff<IN_NI>(s_fr, lane, acc); break;
  }
  // d'(tau): the running sum in ascending tau, a wave scan per block of 64 lags with the carry of the blocks before
  float carry = 0.f;
#pragma unroll
  for (int i = 0; i < IN_NI; ++i) {
    if (i < ni) {
      const int tau = lane + 64 * i;
      const float v = (tau >= 1 && tau <= tmax + 1) ? acc[i] : 0.f;
      float s = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(s, o);
        if (lane >= o) s += t;
      }
      s += carry;
      carry = __shfl(s, 63);
      if (tau <= IN_W) s_dn[tau] = s > 0.f ? (v * (float)tau) / s : 1.f;
    }
  }
  __syncthreads();
  // the first lag under the threshold, by ballot over ascending blocks
  int first = 0;
  for (int i = 0; i < ni && !first; ++i) {
    const int tau = lane + 64 * i;
    const bool under = tau >= tmin && tau <= tmax && s_dn[tau] < VITS_INTONATION_THRESHOLD;
    const unsigned long long m = __ballot(under);
    if (m) first = 64 * i + __ffsll((long long)m) - 1;
  }
  if (lane != 0) return;
  int c = 0;
  if (first) {
    int t = first;
    while (t + 1 <= tmax && s_dn[t + 1] < s_dn[t]) ++t;
    const double y0 = (double)s_dn[t - 1], y1 = (double)s_dn[t], y2 = (double)s_dn[t + 1];  // (2 <= tmin <= t <= tmax <= W - 1)
    const double cv = y0 - 2.0 * y1 + y2;
    double off = 0.0;
    if (cv > 0.0) {
      off = (y0 - y2) / (2.0 * cv);
      off = off > 0.5 ? 0.5 : (off < -0.5 ? -0.5 : off);
    }
    c = (int)lround(1200.0 * log2((double)rate / ((double)t + off) / 27.5));
  }
  *out = c;
}

// Inclusive scan of one value per thread over the workgroup's IN_ITEM_T threads (MAX: the largest so far, else the smallest from the
// right); s: IN_ITEM_T ints of LDS.  Every thread calls it.
template <bool MAX>
__device__ __forceinline__ int in_block_scan(int v, int* s) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int o = 1; o < IN_ITEM_T; o <<= 1) {
    int w = v;
    if (MAX) { if (t >= o) w = s[t - o]; }
    else { if (t + o < IN_ITEM_T) w = s[t + o]; }
    __syncthreads();
    v = MAX ? (w > v ? w : v) : (w < v ? w : v);
    s[t] = v;
    __syncthreads();
  }
  return v;
}

// o_f and P_f of one item per workgroup.  cents [B][c_bstride]; o, Pf [B][t_bstride] (rows f < F = 1 + len / H <= t_bstride);
// flag [B]: 1 where some P_f != 1000.  tab: TAB of the header on the device.  The tokens as contour_tracks_kernel takes them.
__global__ __launch_bounds__(IN_ITEM_T) void intonation_item_kernel(const int* __restrict__ d_len, const int* __restrict__ cents, long long c_bstride,
                                                                    int r_m, const int* __restrict__ tab, const int* __restrict__ cum,
                                                                    long long cum_bstride, const int* __restrict__ tok_len, long long hop,
                                                                    const int* __restrict__ ptok, long long tok_bstride, int tok_max,
                                                                    int* __restrict__ o, int* __restrict__ Pf, long long t_bstride,
                                                                    int* __restrict__ flag) {
  __shared__ int s_hist[IN_BINS];
  __shared__ int s_scan[IN_ITEM_T];
  __shared__ int s_nv, s_med, s_any;
  const int b = blockIdx.x, t = threadIdx.x;
  const long long len = d_len[b];
  long long F = len > 0 ? ct_frames(len) : 0;
  if (F > t_bstride) F = t_bstride;
  const int* cb = cents + (long long)b * c_bstride;
  int* ob = o + (long long)b * t_bstride;
  int* pb = Pf + (long long)b * t_bstride;
  const bool tracked = len >= PT_M + 1;
  for (int i = t; i < IN_BINS; i += IN_ITEM_T) s_hist[i] = 0;
  if (t == 0) { s_nv = 0; s_med = 0; s_any = 0; }
  __syncthreads();
  // the lower median of the voiced cents: integer counts commute, so the histogram does not depend on the order of the adds
  if (tracked) {
    int mine = 0;
    for (long long f = t; f < F && f < c_bstride; f += IN_ITEM_T) {
      const int c = cb[f];
      if (c > 0) { atomicAdd(&s_hist[c < IN_BINS ? c : IN_BINS - 1], 1); ++mine; }
    }
    if (mine) atomicAdd(&s_nv, mine);
  }
  __syncthreads();
  const int nv = s_nv;
  if (nv > 0) {
    constexpr int per = IN_BINS / IN_ITEM_T;
    int part = 0;
    for (int i = 0; i < per; ++i) part += s_hist[t * per + i];
    s_scan[t] = part;
    __syncthreads();
    if (t == 0) {
      const int k = (nv - 1) / 2;  // the element of that index in ascending order
      int run = 0, bin = 0;
      for (int i = 0; i < IN_ITEM_T; ++i) {
        if (run + s_scan[i] > k) {
          for (bin = i * per; bin < (i + 1) * per; ++bin) {
            run += s_hist[bin];
            if (run > k) break;
          }
          break;
        }
        run += s_scan[i];
      }
      s_med = bin;
    }
    __syncthreads();
    const int med = s_med;
    const long long rm = (long long)r_m - 1000;
    // ascending chunks: l(f), the last voiced row <= f, parked in o
    int carry = -1;
    for (long long f0 = 0; f0 < F; f0 += IN_ITEM_T) {
      const long long f = f0 + t;
      const bool voiced = f < F && f < c_bstride && cb[f] > 0;
      int l = in_block_scan<true>(voiced ? (int)f : -1, s_scan);
      if (carry > l) l = carry;
      if (f < F) ob[f] = l;
      carry = s_scan[IN_ITEM_T - 1] > carry ? s_scan[IN_ITEM_T - 1] : carry;
      __syncthreads();
    }
    // descending chunks: g(f), the first voiced row >= f, and with both the offset (a thread reads and writes its own o[f] only)
    int carry_g = 0x7fffffff;
    for (long long f0 = (F - 1) / IN_ITEM_T * IN_ITEM_T; f0 >= 0; f0 -= IN_ITEM_T) {
      const long long f = f0 + t;
      const bool voiced = f < F && f < c_bstride && cb[f] > 0;
      int g = in_block_scan<false>(voiced ? (int)f : 0x7fffffff, s_scan);
      if (carry_g < g) g = carry_g;
      if (f < F) {
        const int l = ob[f];
        long long v;
        if (l == (int)f) v = in_rha(rm * (cb[f] - med), 1000);
        else if (l < 0) v = in_rha(rm * (cb[g] - med), 1000);  // (nv > 0: one of l, g exists)
        else if (g == 0x7fffffff) v = in_rha(rm * (cb[l] - med), 1000);
        else {
          const long long ol = in_rha(rm * (cb[l] - med), 1000), og = in_rha(rm * (cb[g] - med), 1000);
          v = ol + in_rha((og - ol) * (f - l), (long long)g - l);
        }
        ob[f] = (int)(v < -IN_CENTS ? -IN_CENTS : (v > IN_CENTS ? IN_CENTS : v));
      }
      carry_g = s_scan[0] < carry_g ? s_scan[0] : carry_g;
      __syncthreads();
    }
  } else {
    for (long long f = t; f < F; f += IN_ITEM_T) ob[f] = 0;
  }
  __syncthreads();  // (the workgroup's own global writes of o, read below by other threads)
  int n = tok_len ? tok_len[b] : 0;
  n = n < 0 ? 0 : (n > tok_max ? tok_max : n);
  const int* cumb = cum + (long long)b * cum_bstride;
  const int* ptb = ptok + (long long)b * tok_bstride;
  int any = 0;
  for (long long f = t; f < F; f += IN_ITEM_T) {
    long long p = f * PT_H;
    if (p > len - 1) p = len - 1;
    const int tk = ct_tok(cumb, n, hop, p);
    const long long P = tk < n ? ptb[tk] : 1000;
    long long v = (P * tab[ob[p >> 8] + IN_CENTS] + 500) / 1000;
    v = v < 500 ? 500 : (v > 2000 ? 2000 : v);
    pb[f] = (int)v;
    any |= v != 1000;
  }
  if (any) atomicOr(&s_any, 1);
  __syncthreads();
  if (t == 0) flag[b] = s_any;
}

// contour_tracks_kernel with the per-row ratios Pf [B][t_bstride] in place of the token's: inc [B][t_bstride] (rows f < F), gbar
// [B][t_bstride] (rows f <= F).  The gains are the tokens', found as there.
__global__ __launch_bounds__(256) void intonation_tracks_kernel(const int* __restrict__ d_len, const int* __restrict__ cum, long long cum_bstride,
                                                                const int* __restrict__ tok_len, long long hop, const float* __restrict__ gtok,
                                                                long long tok_bstride, int tok_max, const int* __restrict__ Pf,
                                                                long long* __restrict__ inc, float* __restrict__ gbar, long long t_bstride) {
  const int b = blockIdx.y;
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long len = d_len[b];
  const long long F = ct_frames(len);
  if (len <= 0 || f >= F || f + 1 >= t_bstride) return;
  int n = tok_len ? tok_len[b] : 0;
  n = n < 0 ? 0 : (n > tok_max ? tok_max : n);
  const int* cb = cum + (long long)b * cum_bstride;
  const float* gb = gtok + (long long)b * tok_bstride;
  const int* pb = Pf + (long long)b * t_bstride;
  long long sig = 0;
  double gs = 0.0;
#pragma unroll
  for (int j = -CT_R; j <= CT_R; ++j) {  // ascending j
    long long ff = f + j;
    ff = ff < 0 ? 0 : (ff > F - 1 ? F - 1 : ff);
    long long p = ff * PT_H;
    if (p > len - 1) p = len - 1;
    const int t = ct_tok(cb, n, hop, p);
    sig += pb[ff];
    gs += (double)(t < n ? gb[t] : 1.f);
  }
  long long v = sig > 0 ? (PT_ONE * 1000 * CT_K) / sig : CT_MIN_INC;
  if (v < CT_MIN_INC) v = CT_MIN_INC;
  inc[(long long)b * t_bstride + f] = v;
  const float g = (float)(gs / (double)CT_K);
  gbar[(long long)b * t_bstride + f] = g;
  if (f == F - 1) gbar[(long long)b * t_bstride + F] = g;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static int inton_range_arg(float pitch_range, int* r_m) {
  const double r = (double)pitch_range;
  if (!(r >= 0.0 && r <= (double)VITS_INTONATION_MAX_RANGE))  // (NaN fails the comparison)
    return fail(VITS_ERR_ARG, "intonation: pitch_range %g outside [0, %g]", r, (double)VITS_INTONATION_MAX_RANGE);
  *r_m = (int)lround(1000.0 * r);
  return VITS_OK;
}

static int inton_rate_arg(int rate) {
  if (rate < VITS_INTONATION_MIN_RATE || rate > VITS_INTONATION_MAX_RATE)
    return fail(VITS_ERR_UNSUPPORTED, "intonation: the F0 tracker takes rates from %d to %d Hz, not %d", VITS_INTONATION_MIN_RATE,
                VITS_INTONATION_MAX_RATE, rate);
  return VITS_OK;
}

// TAB of include/vits_intonation.h on the device, one copy per device (uploaded on first use, outside any capture; never freed)
static DevTabs<int, int*> g_in_tabs;

static int inton_tab_get(int device, const int** out) {
  int* const* d = nullptr;
  TRY(g_in_tabs.get(device, &d, [&](int*& tab) {
    std::vector<int> T(IN_TABN);
    for (int j = 0; j < IN_TABN; ++j) T[j] = (int)lround(1000.0 * pow(2.0, (double)(j - IN_CENTS) / 1200.0));
    return dev_table_upload(device, "intonation", T.data(), sizeof(int) * IN_TABN, (void**)&tab);
  }));
  *out = *d;
  return VITS_OK;
}

// the track of c items whose longest has F rows, behind whatever `stream` holds; cents [c][c_bstride] is zeroed first
static void inton_track_launch(hipStream_t stream, const float* x, long long x_bstride, const int* d_len, int c, long long F, int rate, int* cents,
                               long long c_bstride) {
  hipMemsetAsync(cents, 0, sizeof(int) * (size_t)c * c_bstride, stream);
  hipLaunchKernelGGL(f0_track_kernel, dim3((unsigned)F, c), dim3(64), 0, stream, x, x_bstride, x_bstride, d_len, rate, cents, c_bstride);
}
