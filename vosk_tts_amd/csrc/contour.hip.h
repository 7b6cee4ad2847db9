// contour.hip.h -- per-token pitch and volume contours (include/vits_contour.h): frame tracks from the tokens, the position recurrence,
// the vocoder of pitch.hip.h driven by its step table, a warping windowed-sinc resampler and the gain curve.  Part of the ONE
// translation unit engine.hip (included there, after pitch.hip.h, whose group runner pv_run and TAB instantiations it runs on).
//
// Launches per group of items (d_len: every item's samples; d_vlen: the same for the items that go through the vocoder, 0 for the
// items of cases (b) and (c), which every vocoder kernel then leaves at once):
//   contour_tracks_kernel   a thread per analysis row: Sigma_f by 2 R + 1 binary searches in cum, inc_f, gbar_f
//   contour_steps_kernel    one wave per item, lane 0 walks the recurrence: F_s, a_0 .. a_{F_s}
//   contour_analysis_kernel step 1 of the vocoder with the frame's transform in double (stft.hip.h; the reason stands at the kernel)
//   pitch_phase_kernel<true>, pitch_synth_kernel<true>, pitch_ola_kernel<true>
//   contour_warp_kernel     a workgroup per CT_TILE consecutive outputs of one item: u window, step slice and filter table in LDS
//   contour_gain_kernel     the items of cases (b) and (c): y = G x
#pragma once
#include "../../include/vits_contour.h"

#define CT_R VITS_CONTOUR_RAMP
#define CT_K (2 * CT_R + 1)
#define CT_RES VITS_CONTOUR_TABLE_RES
#define CT_TAB (RS_Z * CT_RES + 2)       // floats of the filter table
#define CT_TILE 256                      // outputs of one workgroup of contour_warp_kernel, one per thread
#define CT_ASL 8                         // steps of the table a tile stages: it spans one analysis frame, a step is at least half of one
#define CT_REACH (2 * RS_Z)              // Z / s at rho = 2
#define CT_SPAN (2 * CT_TILE + 2 * CT_REACH + 16)  // u samples a tile stages (2 * 256 + 2 * 32 + 2 are needed at rho <= 2)
#define CT_MIN_INC (1LL << 23)
static_assert(PT_H == 256 && CT_TILE == PT_H, "a tile of the warp is one analysis hop: A = n << 16");

__host__ __device__ __forceinline__ long long ct_frames(long long len) { return 1 + len / PT_H; }

// the first t < n with cum[t] * hop > p, or n (cum is non-decreasing; at most 32 halvings)
__device__ __forceinline__ int ct_tok(const int* __restrict__ cum, int n, long long hop, long long p) {
  int lo = 0, hi = n;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi) >> 1;
    if ((long long)cum[mid] * hop > p) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// inc [B][t_bstride] (rows f < F), gbar [B][t_bstride] (rows f <= F), F = 1 + len / H <= t_bstride - 1
__global__ __launch_bounds__(256) void contour_tracks_kernel(const int* __restrict__ d_len, const int* __restrict__ cum, long long cum_bstride,
                                                             const int* __restrict__ tok_len, long long hop, const int* __restrict__ ptok,
                                                             const float* __restrict__ gtok, long long tok_bstride, int tok_max,
                                                             long long* __restrict__ inc, float* __restrict__ gbar, long long t_bstride) {
  const int b = blockIdx.y;
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long len = d_len[b];
  const long long F = ct_frames(len);
  if (len <= 0 || f >= F || f + 1 >= t_bstride) return;
  int n = tok_len[b];
  n = n < 0 ? 0 : (n > tok_max ? tok_max : n);
  const int* cb = cum + (long long)b * cum_bstride;
  const int* pb = ptok + (long long)b * tok_bstride;
  const float* gb = gtok + (long long)b * tok_bstride;
  long long sig = 0;
  double gs = 0.0;
#pragma unroll
  for (int j = -CT_R; j <= CT_R; ++j) {  // ascending j
    long long ff = f + j;
    ff = ff < 0 ? 0 : (ff > F - 1 ? F - 1 : ff);
    long long p = ff * PT_H;
    if (p > len - 1) p = len - 1;
    const int t = ct_tok(cb, n, hop, p);
    sig += t < n ? pb[t] : 1000;
    gs += (double)(t < n ? gb[t] : 1.f);
  }
  long long v = sig > 0 ? (PT_ONE * 1000 * CT_K) / sig : CT_MIN_INC;
  if (v < CT_MIN_INC) v = CT_MIN_INC;  // (never for the P the host hands over: Sigma <= 2000 K)
  inc[(long long)b * t_bstride + f] = v;
  const float g = (float)(gs / (double)CT_K);
  gbar[(long long)b * t_bstride + f] = g;
  if (f == F - 1) gbar[(long long)b * t_bstride + F] = g;
}

// steps [B][s_bstride]: row b = F_s, a_0 .. a_{F_s}.  The loop is bounded by 2 (F_a + 1) + 1 and every step is at least 2^23, so it ends
// whatever inc holds; s_bstride >= 2 (F_a + 1) + 2.
__global__ __launch_bounds__(64) void contour_steps_kernel(const int* __restrict__ d_vlen, const long long* __restrict__ inc, long long t_bstride,
                                                           long long* __restrict__ steps, long long s_bstride) {
  const int b = blockIdx.x;
  if (threadIdx.x != 0) return;
  long long* row = steps + (long long)b * s_bstride;
  const long long Fa = pt_frames_a(d_vlen[b]);
  long long cap = 2 * (Fa + 1);
  if (cap > s_bstride - 2) cap = s_bstride - 2;
  if (!Fa || cap < 0) { row[0] = 0; return; }
  const long long* ib = inc + (long long)b * t_bstride;
  const long long end = (Fa + 1) << 24;
  long long a = 0, fs = 0;
  for (long long t = 0; t <= cap; ++t) {
    row[1 + t] = a;
    if (a >= end) break;
    fs = t + 1;
    long long i = a >> 24;
    if (i > Fa - 1) i = Fa - 1;
    long long v = ib[i];
    if (v < CT_MIN_INC) v = CT_MIN_INC;
    a += v;
  }
  if (fs > cap) fs = cap;  // (a table cut short by s_bstride: never with the strides contour_run forms)
  row[0] = fs;
}

// Step 1 of include/vits_pitch.h for the contour stage: rows [0, F_a + 2) of every item, the grid, the row ownership and the outputs of
// pitch_analysis_kernel (mag / th: [B][a_bstride], row f at f * PT_NB; zeros in the two rows behind the last frame), with the transform of
// the frame formed in double and the magnitude and the 32-bit turn rounded once.  The fp32 transform of pitch_analysis_kernel leaves
// every bin a few 1e-7 of the frame's level from the exact spectrum; in the phases that error is added twice a step by the recursion,
// and a contour runs up to two steps per analysis frame with weights that are exact: measured through vits_op_contour_stretch, u sat
// at 4.8 to 4.9 times the float32 restatement's distance from float64 with it (and the same with atan2 alone taken in double).  The
// transform is sf_frame_spectrum_f64 and sf_bin_f64 of stft.hip.h.
__global__ __launch_bounds__(64 * SF_FPB) void contour_analysis_kernel(const float* __restrict__ x, long long x_bstride, long long x_n,
                                                                       const int* __restrict__ d_vlen, float* __restrict__ mag,
                                                                       unsigned* __restrict__ th, long long a_bstride) {
  __shared__ double2 s_tw[PT_M];  // exp(-2 pi i t / n), t < n/2
  __shared__ double2 s_z[SF_FPB][PT_M];
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  const int b = blockIdx.y;
  const long long len = d_vlen[b];
  const long long Fa = pt_frames_a(len);
  if (Fa == 0 || (long long)blockIdx.x * SF_FPB >= Fa + 2) return;  // uniform over the workgroup
  const long long f = (long long)blockIdx.x * SF_FPB + wv;
  const bool valid = f < Fa;
  double2* Z = s_z[wv];
  sf_frame_spectrum_f64(x + (long long)b * x_bstride, f * PT_H, len, x_n, valid, t, s_tw, Z);
  if (f >= Fa + 2) return;
  float* mo = mag + (long long)b * a_bstride + f * PT_NB;
  unsigned* to = th + (long long)b * a_bstride + f * PT_NB;
  for (int k = t; k < PT_NB; k += 64) {
    float m = 0.f;
    unsigned a = 0u;
    if (valid) {
      const double2 X = sf_bin_f64(Z, s_tw, k);
      m = (float)sqrt(X.x * X.x + X.y * X.y);
      if (X.x != 0.0 || X.y != 0.0) a = (unsigned)(long long)rint(atan2(X.y, X.x) * 0.15915494309189533577 * 4294967296.0);  // the low 32 bits
    }
    mo[k] = m;
    to[k] = a;
  }
}

// G[n] of include/vits_contour.h: one rounding per operation, as the restatement has them
__device__ __forceinline__ float ct_gain(const float* __restrict__ gb, long long n) {
  const long long f = n >> 8;
  const float fr = (float)(int)(n & 255) * (1.f / 256.f);
  return __fadd_rn(__fmul_rn(__fsub_rn(1.f, fr), gb[f]), __fmul_rn(fr, gb[f + 1]));
}

template <typename OUT>
__device__ __forceinline__ void ct_store(OUT* __restrict__ y, float v, float scale) {
  if constexpr (sizeof(OUT) == sizeof(int16_t)) *y = pcm16_of(v, scale);
  else *y = v;
}

// Outputs [0, n_count) of the items with d_vlen[b] > 0; u: [B][u_bstride]; y exactly 0 at and beyond len.
template <typename OUT>
__global__ __launch_bounds__(CT_TILE) void contour_warp_kernel(const float* __restrict__ u, long long u_bstride, const long long* __restrict__ steps,
                                                               long long s_bstride, const float* __restrict__ gbar, long long t_bstride,
                                                               const int* __restrict__ d_len, const int* __restrict__ d_vlen,
                                                               const float* __restrict__ tab, OUT* __restrict__ y, long long y_bstride,
                                                               long long n_count, float scale) {
  __shared__ long long s_a[CT_ASL];
  __shared__ float s_u[CT_SPAN];
  __shared__ float s_T[CT_TAB];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long vlen = d_vlen[b], len = d_len[b];
  if (vlen <= 0) return;  // (uniform) contour_gain_kernel's item
  const long long n0 = (long long)blockIdx.x * CT_TILE, n = n0 + tid;
  OUT* yo = y + (long long)b * y_bstride + n;
  const long long Fa = pt_frames_a(vlen);
  const long long* row = steps + (long long)b * s_bstride;
  const long long Fs = pt_tab_fs(row, Fa);
  if (n0 >= len || Fs < 2) {  // (uniform)
    if (n < n_count) ct_store<OUT>(yo, 0.f, scale);
    return;
  }
  const long long* ab = row + 1;  // a_0 .. a_{F_s}
  const long long Nu = PT_H * (Fs - 1);
  // the tile's first step: the largest t <= F_s - 1 with a_t <= A0 (a_0 = 0 <= A0); every thread runs the same search
  const long long A0 = n0 << 16;
  long long lo = 0, hi = Fs - 1;
  for (int it = 0; it < 48 && lo < hi; ++it) {
    const long long mid = (lo + hi + 1) >> 1;
    if (ab[mid] <= A0) lo = mid;
    else hi = mid - 1;
  }
  const long long t0 = lo;
  if (tid < CT_ASL) s_a[tid] = ab[t0 + tid < Fs ? t0 + tid : Fs];
  for (int j = tid; j < CT_TAB; j += CT_TILE) s_T[j] = tab[j];
  // the u window of the tile: from floor(tau(n0)) - reach - 2
  const long long a0 = ab[t0], d0 = ab[t0 + 1] - a0;  // (t0 + 1 <= F_s)
  const double tau0 = d0 > 0 ? (double)PT_H * ((double)t0 + (double)(A0 - a0) / (double)d0) : 0.0;
  const long long w_lo = (long long)floor(tau0) - CT_REACH - 2;
  const float* ub = u + (long long)b * u_bstride;
  const long long u_end = Nu < u_bstride ? Nu : u_bstride;
  for (int j = tid; j < CT_SPAN; j += CT_TILE) {
    const long long k = w_lo + j;
    s_u[j] = (k >= 0 && k < u_end) ? ub[k] : 0.f;
  }
  __syncthreads();
  if (n >= n_count) return;
  float acc = 0.f;
  bool live = n < len;
  if (live) {
    const long long A = n << 16;
    int t = 0;
#pragma unroll
    for (int it = 0; it < CT_ASL - 2; ++it)
      if (s_a[t + 1] <= A) ++t;
    const long long at = s_a[t], d = s_a[t + 1] - at;
    if (at <= A && d > 0 && A - at < d) {  // (else: a table that does not cover the tile; never with contour_steps_kernel's)
      const double tau = (double)PT_H * ((double)(t0 + t) + (double)(A - at) / (double)d);
      if (tau < (double)Nu) {
        const double s = fmin(1.0, (double)d * (1.0 / (double)PT_ONE));
        const double hw = (double)RS_Z / s;
        long long klo = (long long)ceil(tau - hw), khi = (long long)floor(tau + hw);
        if (klo < 0) klo = 0;
        if (khi > u_end - 1) khi = u_end - 1;
        if (khi - klo > 2 * CT_REACH + 2) khi = klo + 2 * CT_REACH + 2;  // (never: Z / s <= 2 Z)
        const double sR = s * (double)CT_RES;
        const float sf = (float)s;
        for (long long k = klo; k <= khi; ++k) {  // ascending k
          const double p = fabs(tau - (double)k) * sR;
          int j = (int)p;
          if (j > RS_Z * CT_RES) j = RS_Z * CT_RES;
          const float fr = (float)(p - (double)j);
          const float T0 = s_T[j];
          const float h = sf * (T0 + fr * (s_T[j + 1] - T0));
          const long long w = k - w_lo;
          const float uu = (w >= 0 && w < CT_SPAN) ? s_u[w] : ub[k];  // (the window holds every tap at rho <= 2)
          acc += uu * h;
        }
      }
    }
    acc = __fmul_rn(ct_gain(gbar + (long long)b * t_bstride, n), acc);
  }
  ct_store<OUT>(yo, acc, scale);
}

// Outputs [0, n_count) of the items with d_vlen[b] == 0: y[n] = G[n] x[n], exactly 0 at and beyond len.
template <typename OUT>
__global__ __launch_bounds__(256) void contour_gain_kernel(const float* __restrict__ x, long long x_bstride, const float* __restrict__ gbar,
                                                           long long t_bstride, const int* __restrict__ d_len, const int* __restrict__ d_vlen,
                                                           OUT* __restrict__ y, long long y_bstride, long long n_count, float scale) {
  const int b = blockIdx.y;
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (d_vlen[b] > 0 || n >= n_count) return;
  const long long len = d_len[b];
  float v = 0.f;
  if (n < len && n < x_bstride) v = __fmul_rn(ct_gain(gbar + (long long)b * t_bstride, n), x[(long long)b * x_bstride + n]);
  ct_store<OUT>(y + (long long)b * y_bstride + n, v, scale);
}

// the frame table from the signal instead of the tokens (include/vits_intonation.h): its kernels, IntonReq and the table of its ratios
#include "intonation.hip.h"

// ---- host ---------------------------------------------------------------------------------------------------------------
// What a contoured call hands the device: P_t and g_t per token [B][Tx] (neutral beyond an item's tokens), and per item whether any of
// its tokens is shifted.  on: some token of the call is not neutral (case (a) of the header otherwise).
struct ContourReq {
  bool on = false;
  int Tx = 0;
  std::vector<int> P;
  std::vector<float> g;
  std::vector<char> shift;
};

static int contour_plan(const float* semitones, const float* gain_db, float add_semitones, const int64_t* tok_lengths, int B, int Tx, ContourReq* q) {
  *q = ContourReq();
  q->Tx = Tx;
  q->P.assign((size_t)B * Tx, 1000);
  q->g.assign((size_t)B * Tx, 1.f);
  q->shift.assign(B, 0);
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < tok_lengths[b]; ++t) {
      const size_t i = (size_t)b * Tx + t;
      const double s = (semitones ? (double)semitones[i] : 0.0) + (double)add_semitones;
      const double v = gain_db ? (double)gain_db[i] : 0.0;
      if (!(fabs(s) <= (double)VITS_PITCH_MAX_SEMITONES))  // (NaN fails the comparison)
        return fail(VITS_ERR_ARG, "contour: %g semitones at item %d, token %d outside [-%d, %d]", s, b, t, VITS_PITCH_MAX_SEMITONES, VITS_PITCH_MAX_SEMITONES);
      if (!(v >= (double)VITS_CONTOUR_MIN_DB && v <= (double)VITS_CONTOUR_MAX_DB))
        return fail(VITS_ERR_ARG, "contour: %g dB at item %d, token %d outside [%g, %g]", v, b, t, (double)VITS_CONTOUR_MIN_DB, (double)VITS_CONTOUR_MAX_DB);
      q->P[i] = (int)lround(1000.0 * pow(2.0, s / 12.0));
      q->g[i] = (float)pow(10.0, v / 20.0);
      if (q->P[i] != 1000) q->shift[b] = 1;
      if (q->P[i] != 1000 || q->g[i] != 1.f) q->on = true;
    }
  return VITS_OK;
}

// h_1 of include/vits_contour.h on the device, one copy per device (uploaded on first use, outside any capture; never freed)
static DevTabs<int, float*> g_ct_tabs;

static int contour_tab_get(int device, const float** out) {
  float* const* d = nullptr;
  TRY(g_ct_tabs.get(device, &d, [&](float*& tab) {
    std::vector<float> T(CT_TAB, 0.f);
    const double i0b = rs_bessel_i0(RS_BETA);
    for (int j = 0; j <= RS_Z * CT_RES; ++j) {
      const double yv = (double)j / (double)CT_RES, v = RS_RHO * yv, pv = M_PI * v;
      const double sinc = j == 0 ? 1.0 : sin(pv) / pv;
      const double r2 = std::max(1.0 - (yv / RS_Z) * (yv / RS_Z), 0.0);
      T[j] = (float)(RS_RHO * sinc * rs_bessel_i0(RS_BETA * sqrt(r2)) / i0b);
    }
    return dev_table_upload(device, "contour", T.data(), sizeof(float) * CT_TAB, (void**)&tab);
  }));
  *out = *d;
  return VITS_OK;
}

// bytes of scratch an item of `len` samples takes in a group (the strides of a group are those of its longest item); F_s <= 2 (F_a + 1)
// inton: with the track, the offsets and the ratios of include/vits_intonation.h (three ints a row)
static size_t contour_item_bytes(long long len, bool inton = false) {
  const long long Fa = pt_frames_a(len), F = ct_frames(len), cap = 2 * (Fa + 1);
  size_t n = (size_t)(F + 1) * 12 + (size_t)(cap + 2) * 8 + 64;
  if (inton) n += (size_t)(F + 1) * 12 + 16;
  if (Fa) n += (size_t)(Fa + 2) * PT_NB * 8 + (size_t)cap * PT_NB * 4 + (size_t)cap * PT_N * 4 + (size_t)(cap - 1) * PT_H * 4;
  return n;
}

// y[b][0 .. n_count) = the contoured item b, for B items on `stream`: x [B][x_bstride] float on the device, h_len their lengths on the
// host; d_cum [B][cum_bstride], d_toklen [B] on the device.  y is float, or int16 (pcm: pcm16_of at pcm_scale).
// Allocates its scratch and waits for the stream before it frees it: not capturable.  y is not x.
// u_out / steps_out (both or neither; device): the stretch door -- u goes to u_out[b * u_bstride + j], the step tables to
// steps_out[b * s_bstride + ..] (zeroed by the caller), and nothing is warped.
// in (optional): the frame table comes from the item's own F0 track (include/vits_intonation.h) -- the tokens' ratios times the track's,
// row by row; which items go through the vocoder is then the device's word, read back once per group.  cents_out (with `in` only, or
// null; device, [B][c_bstride] with c_bstride >= 1 + (the longest length) / H): where the track is left.  q.Tx may be 0 with `in`.
static int contour_run(int device, hipStream_t stream, const float* x, long long x_bstride, const long long* h_len, int B, const ContourReq& q,
                       const int* d_cum, long long cum_bstride, const int* d_toklen, int hop, void* y, bool pcm, float pcm_scale,
                       long long y_bstride, long long n_count, float* u_out, long long u_bstride, long long* steps_out, long long s_bstride,
                       const IntonReq* in = nullptr, int* cents_out = nullptr, long long c_bstride = 0) {
  if (B <= 0) return VITS_OK;
  const float* d_T = nullptr;
  TRY(contour_tab_get(device, &d_T));
  const int* d_R = nullptr;
  if (in) TRY(inton_tab_get(device, &d_R));
  std::vector<int> len32(B), vlen32(B);
  for (int b = 0; b < B; ++b) {
    if (h_len[b] < 0 || h_len[b] >= (1LL << 31)) return fail(VITS_ERR_ARG, "contour: length %lld of item %d", h_len[b], b);
    len32[b] = (int)h_len[b];
    vlen32[b] = (q.shift[b] && h_len[b] >= PT_M + 1) ? (int)h_len[b] : 0;  // (with `in`: set from the device's word, group by group)
  }
  // in front of the groups: len | vlen | P | g
  const size_t tok_bytes = (size_t)B * q.Tx * 4, head = (2 * (size_t)B * 4 + 2 * tok_bytes + 63) / 64 * 64;
  struct { int *len, *vlen, *P; float* g; } hd{};     // what head() lays out, for every group
  struct { float* gbar; long long t_bs; } grp{};      // the group's gain rows: front() sets them, finish() reads them
  std::vector<int> h_flag(in ? B : 0);
  return pv_run<true>(
      "contour", "", device, stream, h_len, B, head, u_out, u_bstride, [&](long long len) { return contour_item_bytes(len, in != nullptr); },
      [&](char* scr) {
        hd.len = reinterpret_cast<int*>(scr); hd.vlen = hd.len + B; hd.P = hd.vlen + B; hd.g = reinterpret_cast<float*>(hd.P + (size_t)B * q.Tx);
        hipError_t e = hipMemcpyAsync(hd.len, len32.data(), sizeof(int) * B, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && !in) e = hipMemcpyAsync(hd.vlen, vlen32.data(), sizeof(int) * B, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && tok_bytes) e = hipMemcpyAsync(hd.P, q.P.data(), tok_bytes, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && tok_bytes) e = hipMemcpyAsync(hd.g, q.g.data(), tok_bytes, hipMemcpyHostToDevice, stream);
        return e;
      },
      // inc | gbar | (in: cents | o | Pf | flag) | (align 8) | steps | (align 8); the tracks, and which of the group's items the vocoder takes
      [&](PvCarve& S, const PvGroup& g, PvGeom* v) {
        const int b0 = g.b0, c = g.c;
        const long long F = ct_frames(g.mx);
        const long long t_bs = grp.t_bs = F + 1;
        const int *lg = hd.len + b0, *cumg = d_cum ? d_cum + (long long)b0 * cum_bstride : nullptr, *tlg = d_toklen ? d_toklen + b0 : nullptr;
        long long* d_inc = S.take<long long>((size_t)c * t_bs);
        float* d_gbar = grp.gbar = S.take<float>((size_t)c * t_bs);
        int* d_Pf = nullptr;
        if (in) {  // the track, the offsets, the ratios and the items' words; then which items the vocoder takes
          int* d_track = S.take<int>((size_t)c * t_bs);
          int* d_cents = cents_out ? cents_out + (long long)b0 * c_bstride : d_track;
          const long long c_bs = cents_out ? c_bstride : t_bs;
          int* d_o = S.take<int>((size_t)c * t_bs);
          d_Pf = S.take<int>((size_t)c * t_bs);
          int* d_flag = S.take<int>(c);
          inton_track_launch(stream, x + (long long)b0 * x_bstride, x_bstride, lg, c, F, in->rate, d_cents, c_bs);
          hipLaunchKernelGGL(intonation_item_kernel, dim3(c), dim3(IN_ITEM_T), 0, stream, lg, d_cents, c_bs, in->r_m, d_R, cumg, cum_bstride, tlg,
                             (long long)hop, hd.P + (size_t)b0 * q.Tx, (long long)q.Tx, q.Tx, d_o, d_Pf, t_bs, d_flag);
          hipError_t e = hipMemcpyAsync(h_flag.data() + b0, d_flag, sizeof(int) * c, hipMemcpyDeviceToHost, stream);
          if (e == hipSuccess) e = hipStreamSynchronize(stream);
          if (e != hipSuccess) return e;
          for (int b = b0; b < b0 + c; ++b) vlen32[b] = (h_flag[b] && h_len[b] >= PT_M + 1) ? (int)h_len[b] : 0;
          e = hipMemcpyAsync(hd.vlen + b0, vlen32.data() + b0, sizeof(int) * c, hipMemcpyHostToDevice, stream);
          if (e != hipSuccess) return e;
        }
        long long vmx = 0;
        for (int b = 0; b < c; ++b) vmx = std::max(vmx, (long long)vlen32[b0 + b]);
        const long long Fa = pt_frames_a(vmx), cap = 2 * (Fa + 1);
        v->s_bs = steps_out ? s_bstride : cap + 2;
        S.align8();
        long long* d_steps = S.take<long long>((size_t)c * (cap + 2));
        v->steps = steps_out ? steps_out + (long long)b0 * s_bstride : d_steps;
        S.align8();
        if (in)
          hipLaunchKernelGGL(intonation_tracks_kernel, dim3((unsigned)((F + 255) / 256), c), dim3(256), 0, stream, lg, cumg, cum_bstride, tlg,
                             (long long)hop, hd.g + (size_t)b0 * q.Tx, (long long)q.Tx, q.Tx, d_Pf, d_inc, d_gbar, t_bs);
        else
          hipLaunchKernelGGL(contour_tracks_kernel, dim3((unsigned)((F + 255) / 256), c), dim3(256), 0, stream, lg, cumg, cum_bstride, tlg, (long long)hop,
                             hd.P + (size_t)b0 * q.Tx, hd.g + (size_t)b0 * q.Tx, (long long)q.Tx, q.Tx, d_inc, d_gbar, t_bs);
        v->it = Items{hd.vlen + b0, 1}; v->Fs = cap;
        if (Fa && v->s_bs >= cap + 2) {
          v->Fa = Fa;
          hipLaunchKernelGGL(contour_steps_kernel, dim3(c), dim3(64), 0, stream, v->it.units, d_inc, t_bs, v->steps, v->s_bs);
        }
        return hipSuccess;
      },
      [&](PvCarve&, const PvGroup& g, const PvGeom& v, const StftTab&, float* mag, unsigned* th, long long a_bs) -> const float* {
        hipLaunchKernelGGL(contour_analysis_kernel, dim3((unsigned)((v.Fa + 2 + SF_FPB - 1) / SF_FPB), g.c), dim3(64 * SF_FPB), 0, stream,
                           x + (long long)g.b0 * x_bstride, x_bstride, x_bstride, v.it.units, mag, th, a_bs);
        return mag;
      },
      // u warped along the step table and scaled by the gain curve; the items the vocoder left alone are y = G x
      [&](PvCarve&, const PvGroup& g, const PvGeom& v, const float* u, long long u_bs) {
        if (u_out || n_count <= 0) return;
        const dim3 grid((unsigned)((n_count + CT_TILE - 1) / CT_TILE), g.c);
        const float* xg = x + (long long)g.b0 * x_bstride;
        const int *lg = hd.len + g.b0, *vg = v.it.units;
        auto out = [&](auto* y0, float scale) {
          using OUT = std::remove_pointer_t<decltype(y0)>;
          OUT* yg = y0 + (long long)g.b0 * y_bstride;
          if (u) hipLaunchKernelGGL(contour_warp_kernel<OUT>, grid, dim3(CT_TILE), 0, stream, u, u_bs, v.steps, v.s_bs, grp.gbar, grp.t_bs, lg, vg, d_T, yg, y_bstride, n_count, scale);
          hipLaunchKernelGGL(contour_gain_kernel<OUT>, grid, dim3(256), 0, stream, xg, x_bstride, grp.gbar, grp.t_bs, lg, vg, yg, y_bstride, n_count, scale);
        };
        if (pcm) out(static_cast<int16_t*>(y), pcm_scale);
        else out(static_cast<float*>(y), 1.f);
      });
}

// ---- the parity doors ---------------------------------------------------------------------------------------------------
static int contour_op(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, const int32_t* cum, const int64_t* tok_lengths,
                      int32_t Tx, int32_t hop, const float* token_semitones, const float* token_gain_db, float* y, float* u, int64_t* steps,
                      const IntonReq* in = nullptr, int32_t* cents = nullptr) {
  const bool stretch = u != nullptr;
  const char* what = in ? "intonation" : "contour";
  const bool no_tokens = in && !cum && Tx == 0;  // (include/vits_intonation.h: the stage without a contour)
  if ((!stretch && !y) || (stretch && !steps) || hop <= 0 || (!no_tokens && (!cum || !tok_lengths || Tx <= 0))) return fail(VITS_ERR_ARG, "%s: bad argument", what);
  std::vector<int> len32;
  TRY(op_items_check(what, x, lengths, B, N, &len32, "N = "));
  std::vector<int> tl32(B, 0);
  const std::vector<int64_t> no_tl(B, 0);
  if (no_tokens) tok_lengths = no_tl.data();
  for (int b = 0; b < B && !no_tokens; ++b) {
    if (tok_lengths[b] < 0 || tok_lengths[b] > Tx) return fail(VITS_ERR_ARG, "contour: token length %lld of item %d outside [0, T_x = %d]", (long long)tok_lengths[b], b, Tx);
    tl32[b] = (int)tok_lengths[b];
    for (int t = 0; t < tl32[b]; ++t) {
      const int32_t c0 = t ? cum[(size_t)b * Tx + t - 1] : 0, c1 = cum[(size_t)b * Tx + t];
      if (c1 < c0) return fail(VITS_ERR_ARG, "contour: cum of item %d decreases at token %d (%d after %d)", b, t, c1, c0);
    }
  }
  ContourReq q;
  TRY(contour_plan(token_semitones, token_gain_db, 0.f, tok_lengths, B, Tx, &q));
  const std::vector<long long> len64(lengths, lengths + B);
  const long long Nu = (long long)PT_H * (2 * (N / PT_H + 2) - 1), Ns = 2 * (N / PT_H + 2) + 2, Nc = 1 + N / PT_H;
  OpDoor d(what, device);
  float* dx = d.up_items(x, lengths, B, N);
  int* dc = no_tokens ? nullptr : d.up(cum, (size_t)B * Tx);
  int* dt = d.up(tl32.data(), B);
  float* dy = stretch ? d.out<float>((size_t)B * Nu) : d.out<float>((size_t)B * N);
  long long* ds = stretch ? d.out<long long>((size_t)B * Ns, 0) : nullptr;
  int* dcents = cents ? d.out<int>((size_t)B * Nc, 0) : nullptr;
  if (d.ok())
    TRY(stretch ? contour_run(device, nullptr, dx, N, len64.data(), B, q, dc, Tx, dt, hop, nullptr, false, 1.f, 0, 0, dy, Nu, ds, Ns, in, dcents, Nc)
                : contour_run(device, nullptr, dx, N, len64.data(), B, q, dc, Tx, dt, hop, dy, false, 1.f, N, N, nullptr, 0, nullptr, 0, in, dcents, Nc));
  d.finish();
  d.down(stretch ? u : y, dy, stretch ? (size_t)B * Nu : (size_t)B * N);
  if (stretch) d.down(reinterpret_cast<long long*>(steps), ds, (size_t)B * Ns);
  if (cents) d.down(reinterpret_cast<int*>(cents), dcents, (size_t)B * Nc);
  return d.rc();
}

int vits_op_contour(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, const int32_t* cum, const int64_t* tok_lengths,
                    int32_t T_x, int32_t hop, const float* token_semitones, const float* token_gain_db, float* y) {
  return contour_op(device, x, lengths, B, N, cum, tok_lengths, T_x, hop, token_semitones, token_gain_db, y, nullptr, nullptr);
}
int vits_op_contour_stretch(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, const int32_t* cum,
                            const int64_t* tok_lengths, int32_t T_x, int32_t hop, const float* token_semitones, const float* token_gain_db,
                            float* u, int64_t* steps) {
  if (!u) return fail(VITS_ERR_ARG, "contour: bad argument");
  return contour_op(device, x, lengths, B, N, cum, tok_lengths, T_x, hop, token_semitones, token_gain_db, nullptr, u, steps);
}

// ---- the doors of include/vits_intonation.h -------------------------------------------------------------------------------
int vits_op_f0_track(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, int32_t* cents) {
  if (!cents) return fail(VITS_ERR_ARG, "f0 track: bad argument");
  std::vector<int> len32;
  TRY(op_items_check("f0 track", x, lengths, B, N, &len32, "N = "));
  TRY(inton_rate_arg(rate));
  const long long Nc = 1 + N / PT_H;
  OpDoor d("f0 track", device);
  float* dx = d.up_items(x, lengths, B, N);
  int* dl = d.up(len32.data(), B);
  int* dc = d.dev<int>((size_t)B * Nc);
  if (d.ok()) inton_track_launch(nullptr, dx, N, dl, B, Nc, rate, dc, Nc);
  d.finish();
  d.down(reinterpret_cast<int*>(cents), dc, (size_t)B * Nc);
  return d.rc();
}

static int inton_op(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, const int32_t* cum,
                    const int64_t* tok_lengths, int32_t T_x, int32_t hop, const float* token_semitones, const float* token_gain_db, float pitch_range,
                    float* y, float* u, int64_t* steps, int32_t* cents) {
  IntonReq in;
  TRY(inton_range_arg(pitch_range, &in.r_m));
  TRY(inton_rate_arg(rate));
  in.on = true;  // (a door runs the stage at r_m == 1000 too: every R_f is 1000 then)
  in.rate = rate;
  return contour_op(device, x, lengths, B, N, cum, tok_lengths, T_x, hop, token_semitones, token_gain_db, y, u, steps, &in, cents);
}

int vits_op_intonation(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, const int32_t* cum,
                       const int64_t* tok_lengths, int32_t T_x, int32_t hop, const float* token_semitones, const float* token_gain_db,
                       float pitch_range, float* y) {
  return inton_op(device, x, lengths, B, N, rate, cum, tok_lengths, T_x, hop, token_semitones, token_gain_db, pitch_range, y, nullptr, nullptr, nullptr);
}
int vits_op_intonation_stretch(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, const int32_t* cum,
                               const int64_t* tok_lengths, int32_t T_x, int32_t hop, const float* token_semitones,
                               const float* token_gain_db, float pitch_range, float* u, int64_t* steps, int32_t* cents) {
  if (!u || !cents) return fail(VITS_ERR_ARG, "intonation: bad argument");
  return inton_op(device, x, lengths, B, N, rate, cum, tok_lengths, T_x, hop, token_semitones, token_gain_db, pitch_range, nullptr, u, steps, cents);
}
