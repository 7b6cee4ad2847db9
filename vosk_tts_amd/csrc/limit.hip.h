// limit.hip.h -- the look-ahead peak limiter of include/vits_limit.h: envelope (sample peak, or true peak through the 4x polyphase
// interpolator), look-ahead minimum, release, box attack and the gain applied, for every item of a batch on the device.  Part of the ONE
// translation unit engine.hip (included there, behind loudness.hip.h, whose measurement and profiling scope it uses).
//
// Index shift: the definition runs k over [-W, len); here j = k + W >= 0, so e[k] is d-space value j and s[n] averages j in [n, n + W].
// m[k] = min r[k .. k+W] is r(max p[j-W .. j]): a trailing window in j, and r is non-increasing in p, so the maximum is slid over fp32 p.
// The serial part is the release d[j] = max(q[j], a d[j-1]) on the deficit d = 1 - e, q = 1 - m: maps v -> max(C, A v), which compose
// as (A2 A1, max(C2, A2 C1)).  A run of R consecutive j has A = a^R whatever its data, so a scan needs only C and the powers
// a^(R 2^k), which the host forms in double.
//
// Decomposition: a workgroup of LM_THREADS threads owns VITS_LIMIT_TILE consecutive samples (or j) of one item; grid (tiles, items).
// Dependencies between tiles are launch boundaries:
//   1. limit_env_kernel     p[b][n] and the tile's maximum of p; true-peak mode stages the tile plus LM_HALF of halo either side and the
//                           4 x 33 table in LDS.  Does not depend on the gain: runs once per call.
//   2. limit_gain_kernel    one wave per item: max p over its tiles and the pass's pre-gain -> gv[b] = {g, max p}
//   3. limit_scan_kernel    j-tile kt: the sliding maximum over the tile plus W of backward halo, runs of 8 from zero state, Kogge-Stone
//                           in LDS -> cend[b][kt], the tile's C (its A is a^TILE)
//   4. limit_carry_kernel   one wave per item: cin[b][0] = 0, cin[b][kt + 1] = max(cend[b][kt], a^TILE cin[b][kt])
//   5. limit_apply_kernel   sample tile kn needs d over j in [kn TILE, kn TILE + TILE + W): 256 runs of 12 from cin[b][kn], each run again
//                           from its true incoming value, an LDS prefix sum in double, s[n] = 1 - (D[n+W] - D[n-1]) / (W + 1), then
//                           y = fp32(g s) x (or pcm16_of) and the tile's min s
//   6. limit_final_kernel   (the entry points only) one wave per item: min s over its tiles and the gain into the call's result row
// Cost written down: p is written once and read twice per pass with up to W (2 W in 5) samples of halo; the sliding maximum is log2(W + 1)
// doubling levels over the staged span.  No atomics, no waiting between workgroups, fixed slots and fixed order.
//
// LDS of limit_apply_kernel: 2 x 4096 floats (the doubling levels ping-pong) + 256 rows of 12 + 1 doubles (a thread walks its own row;
// the odd row length in 8-byte words keeps the 64-bit reads of consecutive lanes on different bank pairs) + 2 x 256 doubles of scan
// = 63488 bytes.
#pragma once
#include <optional>
#include "../../include/vits_limit.h"

#define LM_THREADS 256
#define LM_LEVELS 8  // log2(LM_THREADS)
#define LM_HALF 16   // half width of the 4x interpolator in input samples
#define LM_TAPS 33
#define LM_RS 8      // run of limit_scan_kernel
#define LM_RA 12     // run of limit_apply_kernel
static_assert(LM_RS * LM_THREADS == VITS_LIMIT_TILE, "scan tile = threads x run");
static_assert(LM_RA * LM_THREADS == VITS_LIMIT_TILE + VITS_LIMIT_MAX_LOOKAHEAD, "apply span = threads x run");
static_assert((1 << LM_LEVELS) == LM_THREADS, "scan levels");
static_assert(VITS_LIMIT_TILE == VITS_LOUDNESS_TILE, "one tile count serves both scratch layouts");

struct LimTab { float t[VITS_LIMIT_OVERSAMPLE][LM_TAPS]; };
struct LimPrm {
  int mode = 0, W = 1;
  float ceiling = 1.f, gain = 1.f;
  double a = 0.0;
  double PS[LM_LEVELS], PA[LM_LEVELS];  // a^(LM_RS 2^k), a^(LM_RA 2^k)
  double aT = 0.0;                      // a^VITS_LIMIT_TILE
};

static int limit_plan(int rate, float lookahead_ms, float release_ms, int* W, double* a) {
  if (rate < 1 || rate > (1 << 24)) return fail(VITS_ERR_UNSUPPORTED, "limit: rate %d Hz outside [1, %d]", rate, 1 << 24);
  if (!(lookahead_ms > 0.f && lookahead_ms <= 10.f)) return fail(VITS_ERR_ARG, "limit: lookahead %g ms outside (0, 10]", (double)lookahead_ms);
  if (!(release_ms >= 1.f && release_ms <= 1000.f)) return fail(VITS_ERR_ARG, "limit: release %g ms outside [1, 1000]", (double)release_ms);
  const long long w = llround((double)lookahead_ms * (double)rate / 1000.0);
  if (w < 1 || w > VITS_LIMIT_MAX_LOOKAHEAD)
    return fail(VITS_ERR_UNSUPPORTED, "limit: look-ahead W = %lld samples (%g ms at %d Hz) outside [1, %d]", w, (double)lookahead_ms, rate, VITS_LIMIT_MAX_LOOKAHEAD);
  if (W) *W = (int)w;
  if (a) *a = exp(-1.0 / ((double)release_ms * (double)rate / 1000.0));
  return VITS_OK;
}

static int limit_params(int rate, int mode, float ceiling, float lookahead_ms, float release_ms, float gain, LimPrm* out) {
  LimPrm p;
  if (mode != VITS_LIMIT_SAMPLE && mode != VITS_LIMIT_TRUE)
    return fail(VITS_ERR_ARG, "limit: mode %d is neither VITS_LIMIT_SAMPLE (1) nor VITS_LIMIT_TRUE (2)", mode);
  if (!(ceiling > 0.f && ceiling <= 1.f)) return fail(VITS_ERR_ARG, "limit: ceiling %g outside (0, 1]", (double)ceiling);
  if (!(gain >= 0.f && gain <= 64.f)) return fail(VITS_ERR_ARG, "limit: gain %g outside [0, 64]", (double)gain);
  TRY(limit_plan(rate, lookahead_ms, release_ms, &p.W, &p.a));
  p.mode = mode; p.ceiling = ceiling; p.gain = gain;
  double ps = 1.0, pa = 1.0;
  for (int i = 0; i < LM_RS; ++i) ps *= p.a;
  for (int i = 0; i < LM_RA; ++i) pa *= p.a;
  for (int k = 0; k < LM_LEVELS; ++k) {
    p.PS[k] = ps; p.PA[k] = pa;
    ps *= ps; pa *= pa;
  }
  p.aT = ps;  // a^(LM_RS 2^LM_LEVELS)
  *out = p;
  return VITS_OK;
}

// the fp32 table of vits_resample_table(rate, 4 rate)
static int limit_tab(int rate, LimTab* out) {
  if (rate < 1 || rate > (1 << 24)) return fail(VITS_ERR_UNSUPPORTED, "limit: rate %d Hz outside [1, %d]", rate, 1 << 24);
  ResamplePlan P;
  TRY(resample_plan(rate, VITS_LIMIT_OVERSAMPLE * rate, &P));
  if (P.L != VITS_LIMIT_OVERSAMPLE || P.M != 1 || P.taps != LM_TAPS || P.half != LM_HALF)
    return fail(VITS_ERR_DEVICE, "limit: the 4x interpolator is %d/%d with %d taps, half width %d", P.L, P.M, P.taps, P.half);
  resample_fill(P, &out->t[0][0]);
  return VITS_OK;
}

// ---- device ---------------------------------------------------------------------------------------------------------------
// step 2 from fp32 values, in double
__device__ __forceinline__ double lm_need(double c, double g, float p) {
  const double gp = g * (double)p;
  return gp > 0.0 ? fmin(1.0, c / gp) : 1.0;
}

// p [B, it.cap]; tpeak [B, ntiles], written for the tiles that hold samples of the item
__global__ __launch_bounds__(LM_THREADS) void limit_env_kernel(const float* __restrict__ x, long long x_bstride, const Items it, int mode,
                                                               const LimTab tab, int ntiles, float* __restrict__ p, float* __restrict__ tpeak) {
  __shared__ float xs[VITS_LIMIT_TILE + 2 * LM_HALF];
  __shared__ float tb[VITS_LIMIT_OVERSAMPLE * LM_TAPS];
  __shared__ float pk[LM_THREADS];
  const int b = blockIdx.y, k = blockIdx.x, t = threadIdx.x;
  const long long len = it.len_out(b), n0 = (long long)k * VITS_LIMIT_TILE;
  if (n0 >= len) return;  // (the whole workgroup)
  const float* xb = x + (long long)b * x_bstride;
  for (int i = t; i < VITS_LIMIT_TILE + 2 * LM_HALF; i += LM_THREADS) {
    const long long n = n0 - LM_HALF + i;
    xs[i] = (n >= 0 && n < len) ? xb[n] : 0.f;
  }
  if (t < VITS_LIMIT_OVERSAMPLE * LM_TAPS) tb[t] = tab.t[t / LM_TAPS][t % LM_TAPS];
  __syncthreads();
  float pm = 0.f;
  for (int i = 0; i < VITS_LIMIT_TILE / LM_THREADS; ++i) {
    const int l = t + i * LM_THREADS;
    if (n0 + l >= len) break;
    float v = fabsf(xs[l + LM_HALF]);
    if (mode == VITS_LIMIT_TRUE) {
#pragma unroll
      for (int ph = 0; ph < VITS_LIMIT_OVERSAMPLE; ++ph) {  // resample_kernel at L = 4, M = 1: lo = (64 - ph) / 4, hi = 16
        const int lo = ph ? LM_HALF - 1 : LM_HALF, nt = lo + LM_HALF + 1;
        const float* xr = xs + l + LM_HALF - lo;  // (the last one read is l + 2 LM_HALF: inside xs)
        float acc = 0.f;
        for (int j = 0; j < nt; ++j) acc = fmaf(tb[ph * LM_TAPS + j], xr[j], acc);
        v = fmaxf(v, fabsf(acc));
      }
    }
    p[(long long)b * it.cap + n0 + l] = v;
    pm = fmaxf(pm, v);
  }
  pk[t] = pm;
  __syncthreads();
  for (int w = LM_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) pk[t] = fmaxf(pk[t], pk[t + w]);
    __syncthreads();
  }
  if (t == 0) tpeak[(long long)b * ntiles + k] = pk[0];
}

// gv[b] = {g, max p}.  src 0: prm.gain; 1: res0[b].gain (pass 1 of the LUFS form); 2: pass 2, res1 the measurement of y_0.
__global__ __launch_bounds__(64) void limit_gain_kernel(const Items it, int ntiles, const float* __restrict__ tpeak, int src, const LimPrm prm,
                                                        const float* __restrict__ res0, const float* __restrict__ res1, float* __restrict__ gv) {
  const int b = blockIdx.x, t = threadIdx.x;
  const long long len = it.len_out(b);
  const int nt = (int)((len + VITS_LIMIT_TILE - 1) / VITS_LIMIT_TILE);
  float pm = 0.f;
  for (int k = t; k < nt; k += 64) pm = fmaxf(pm, tpeak[(long long)b * ntiles + k]);
  for (int o = 32; o > 0; o >>= 1) pm = fmaxf(pm, __shfl_xor(pm, o));
  if (t == 0) {
    float g = prm.gain;
    if (src >= 1) g = res0[b * 4 + 2];
    if (src == 2 && lm_need((double)prm.ceiling, (double)g, pm) < 1.0) g = (float)((double)g * (double)res1[b * 4 + 2]);
    gv[b * 2 + 0] = g;
    gv[b * 2 + 1] = pm;
  }
}

// pa[i] = p of sample s0 + i for i < span, 0 outside the item
__device__ __forceinline__ void lm_fill(float* pa, const float* __restrict__ pb, long long s0, int span, long long len) {
  for (int i = threadIdx.x; i < span; i += LM_THREADS) {
    const long long n = s0 + i;
    pa[i] = (n >= 0 && n < len) ? pb[n] : 0.f;
  }
  __syncthreads();
}

// in: pa filled over `span` and published.  out: a buffer M (pa or pb) and off2 with max p[i .. i + w) = max(M[i], M[i + off2]) for every
// i + w <= span.  Doubling: level v holds maxima over 2^v; beyond the span counts as 0 (p >= 0).
__device__ __forceinline__ const float* lm_wmax(float* pa, float* pb, int span, int w, int* off2) {
  int q = 0;
  while ((2 << q) <= w) ++q;  // 2^q <= w < 2^(q+1)
  float *src = pa, *dst = pb;
  for (int v = 0; v < q; ++v) {
    const int step = 1 << v;
    for (int i = threadIdx.x; i < span; i += LM_THREADS) dst[i] = fmaxf(src[i], i + step < span ? src[i + step] : 0.f);
    __syncthreads();
    float* tmp = src; src = dst; dst = tmp;
  }
  *off2 = w - (1 << q);
  return src;
}

// The release over this thread's run of R consecutive j (local l0 = t R ..), the tile entered with deficit cin.  Returns the tile's end
// value; with RERUN d[i] is the deficit at each of the run's j.
template <int R, bool RERUN>
__device__ __forceinline__ double lm_release(const LimPrm& prm, const double* Pk, const float* mq, int off2, double g, double cin,
                                             double (*sc)[LM_THREADS], double* d) {
  const int t = threadIdx.x, l0 = t * R;
  double q[R];
#pragma unroll
  for (int i = 0; i < R; ++i) q[i] = 1.0 - lm_need((double)prm.ceiling, g, fmaxf(mq[l0 + i], mq[l0 + i + off2]));
  double v = t == 0 ? cin : 0.0;
#pragma unroll
  for (int i = 0; i < R; ++i) v = fmax(q[i], prm.a * v);
  int cur = 0;
  sc[0][t] = v;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < LM_LEVELS; ++k) {
    const int off = 1 << k;
    double u = sc[cur][t];
    if (t >= off) u = fmax(u, Pk[k] * sc[cur][t - off]);
    sc[cur ^ 1][t] = u;
    __syncthreads();
    cur ^= 1;
  }
  if constexpr (RERUN) {
    v = t == 0 ? cin : sc[cur][t - 1];
#pragma unroll
    for (int i = 0; i < R; ++i) { v = fmax(q[i], prm.a * v); d[i] = v; }
  }
  return sc[cur][LM_THREADS - 1];
}

// cend [B, ntj]: the deficit at the end of j-tile kt entered with 0; written for kt TILE < len + W
__global__ __launch_bounds__(LM_THREADS) void limit_scan_kernel(const float* __restrict__ p, const Items it, const LimPrm prm,
                                                                const float* __restrict__ gv, int ntj, double* __restrict__ cend) {
  constexpr int SPAN = VITS_LIMIT_TILE + VITS_LIMIT_MAX_LOOKAHEAD;
  __shared__ float pa[SPAN], pb[SPAN];
  __shared__ double sc[2][LM_THREADS];
  const int b = blockIdx.y, kt = blockIdx.x;
  const long long len = it.len_out(b), j0 = (long long)kt * VITS_LIMIT_TILE;
  if (j0 >= len + prm.W) return;  // (the whole workgroup)
  lm_fill(pa, p + (long long)b * it.cap, j0 - prm.W, SPAN, len);
  int off2;
  const float* mq = lm_wmax(pa, pb, SPAN, prm.W + 1, &off2);
  const double e = lm_release<LM_RS, false>(prm, prm.PS, mq, off2, (double)gv[b * 2], 0.0, sc, nullptr);
  if (threadIdx.x == 0) cend[(long long)b * ntj + kt] = e;
}

// cin [B, ntj]: the deficit j-tile kt is entered with.  One wave per item.
__global__ __launch_bounds__(64) void limit_carry_kernel(const Items it, const LimPrm prm, int ntj, const double* __restrict__ cend,
                                                         double* __restrict__ cin) {
  __shared__ double es[64];
  const int b = blockIdx.x, t = threadIdx.x;
  const long long len = it.len_out(b);
  const int nt = (int)((len + prm.W + VITS_LIMIT_TILE - 1) / VITS_LIMIT_TILE);
  double v = 0.0;
  for (int k0 = 0; k0 < nt; k0 += 64) {
    if (k0 + t < nt) es[t] = cend[(long long)b * ntj + k0 + t];
    __syncthreads();
    if (t == 0) {
      const int n = nt - k0 < 64 ? nt - k0 : 64;
      for (int i = 0; i < n; ++i) {
        cin[(long long)b * ntj + k0 + i] = v;
        v = fmax(es[i], prm.aT * v);
      }
    }
    __syncthreads();
  }
}

// y[b, n] for 0 <= n < n_count (exactly 0 at and beyond len, where x and p are not read); s_out (nullable) [B, it.cap]: fp32(s), 1 beyond len;
// smin [B, ntiles]: min fp32(s) over the tile's samples of the item, written for the tiles that hold some.
template <typename OUT>
__global__ __launch_bounds__(LM_THREADS) void limit_apply_kernel(const float* __restrict__ x, long long x_bstride, const Items it,
                                                                 const float* __restrict__ p, const LimPrm prm, const float* __restrict__ gv,
                                                                 int ntiles, int ntj, const double* __restrict__ cin, OUT* __restrict__ y,
                                                                 long long y_bstride, long long n_count, float scale, float* __restrict__ s_out,
                                                                 float* __restrict__ smin) {
  constexpr int NJ = LM_RA * LM_THREADS, SPAN = NJ + VITS_LIMIT_MAX_LOOKAHEAD, ROW = LM_RA + 1;
  __shared__ float pa[SPAN], pb[SPAN];
  __shared__ double dd[LM_THREADS * ROW];
  __shared__ double sc[2][LM_THREADS];
  const int b = blockIdx.y, kn = blockIdx.x, t = threadIdx.x;
  const long long len = it.len_out(b), n0 = (long long)kn * VITS_LIMIT_TILE;
  if (n0 >= len) {  // (the whole workgroup)
    for (int i = 0; i < VITS_LIMIT_TILE / LM_THREADS; ++i) {
      const long long n = n0 + t + i * LM_THREADS;
      if (n < n_count) y[(long long)b * y_bstride + n] = (OUT)0;
      if (s_out && n < it.cap) s_out[(long long)b * it.cap + n] = 1.f;
    }
    return;
  }
  const int W = prm.W;
  const double g = (double)gv[b * 2];
  lm_fill(pa, p + (long long)b * it.cap, n0 - W, SPAN, len);
  int off2;
  const float* mq = lm_wmax(pa, pb, SPAN, W + 1, &off2);
  double d[LM_RA];
  lm_release<LM_RA, true>(prm, prm.PA, mq, off2, g, cin[(long long)b * ntj + kn], sc, d);
  // inclusive prefix sums of d over the span: the run, a Kogge-Stone sum over the runs, the run again
  double run = 0.0;
#pragma unroll
  for (int i = 0; i < LM_RA; ++i) run += d[i];
  int cur = 0;
  __syncthreads();  // (lm_release's last reads of sc)
  sc[0][t] = run;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < LM_LEVELS; ++k) {
    const int off = 1 << k;
    double u = sc[cur][t];
    if (t >= off) u += sc[cur][t - off];
    sc[cur ^ 1][t] = u;
    __syncthreads();
    cur ^= 1;
  }
  double acc = t ? sc[cur][t - 1] : 0.0;
#pragma unroll
  for (int i = 0; i < LM_RA; ++i) { acc += d[i]; dd[t * ROW + i] = acc; }
  __syncthreads();
  const double inv = 1.0 / (double)(W + 1);
  const float* xb = x + (long long)b * x_bstride;
  float sm = 1.f;
  for (int i = 0; i < VITS_LIMIT_TILE / LM_THREADS; ++i) {
    const int l = t + i * LM_THREADS;
    const long long n = n0 + l;
    float v = 0.f, s32 = 1.f;
    if (n < len) {
      const int hi = l + W, lo = l - 1;
      const double sum = dd[(hi / LM_RA) * ROW + hi % LM_RA] - (l ? dd[(lo / LM_RA) * ROW + lo % LM_RA] : 0.0);
      const double s = 1.0 - sum * inv;
      s32 = (float)s;
      sm = fminf(sm, s32);
      v = (float)(g * s) * xb[n];
    }
    if (s_out && n < it.cap) s_out[(long long)b * it.cap + n] = s32;
    if (n < n_count) {
      if constexpr (sizeof(OUT) == sizeof(int16_t)) y[(long long)b * y_bstride + n] = pcm16_of(v, scale);
      else y[(long long)b * y_bstride + n] = v;
    }
  }
  float* red = pa;  // (every read of pa / pb lies before lm_release's barriers)
  red[t] = sm;
  __syncthreads();
  for (int w = LM_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) red[t] = fminf(red[t], red[t + w]);
    __syncthreads();
  }
  if (t == 0) smin[(long long)b * ntiles + kn] = red[0];
}

// ---- launches ----------------------------------------------------------------------------------------------------------------
// device scratch of a limited call over [B, N]: p | tpeak | smin | gv | cend | cin | y0 (the LUFS form only)
struct LimScratch {
  float *p, *tpeak, *smin, *gv, *y0;
  double *cend, *cin;
  int ntiles, ntj;
};
static size_t lim_scratch_layout(int B, long long N, bool two_pass, char* base, LimScratch* out) {
  const long long nt = (N + VITS_LIMIT_TILE - 1) / VITS_LIMIT_TILE, ntj = (N + VITS_LIMIT_MAX_LOOKAHEAD + VITS_LIMIT_TILE - 1) / VITS_LIMIT_TILE;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return base ? base + o : nullptr; };
  LimScratch S;
  S.p = reinterpret_cast<float*>(take(sizeof(float) * (size_t)B * N));
  S.tpeak = reinterpret_cast<float*>(take(sizeof(float) * (size_t)B * nt));
  S.smin = reinterpret_cast<float*>(take(sizeof(float) * (size_t)B * nt));
  S.gv = reinterpret_cast<float*>(take(sizeof(float) * (size_t)B * 2));
  S.cend = reinterpret_cast<double*>(take(sizeof(double) * (size_t)B * ntj));
  S.cin = reinterpret_cast<double*>(take(sizeof(double) * (size_t)B * ntj));
  S.y0 = two_pass ? reinterpret_cast<float*>(take(sizeof(float) * (size_t)B * N)) : nullptr;
  S.ntiles = (int)nt;
  S.ntj = (int)ntj;
  if (out) *out = S;
  return off;
}

// a launch counted / timed under the operation "out.limit" where a session is given (the parity doors have none)
struct LimProf {
  std::optional<ProfScope> p;
  LimProf(vits_session* s, const char* kernel) { if (s) p.emplace(s, "out.limit", 0, kernel); }
};

// step 1 of B items x[b, 0 : it.len_out(b)) of capacity it.cap on `stream` (no allocation, no synchronisation)
static void lim_env_launch(hipStream_t stream, int mode, const LimTab& tab, const LimScratch& S, const float* x, long long x_bstride, const Items& it,
                           int B, vits_session* ps = nullptr) {
  if (B <= 0 || S.ntiles <= 0) return;
  LimProf lp(ps, "limit_env_kernel");
  hipLaunchKernelGGL(limit_env_kernel, dim3(S.ntiles, B), dim3(LM_THREADS), 0, stream, x, x_bstride, it, mode, tab, S.ntiles, S.p, S.tpeak);
}

// one pass behind lim_env_launch: the gain (src as limit_gain_kernel takes it), steps 2-6 into y[b, 0 : n_count), n_count <= it.cap
template <typename OUT>
static void lim_pass_launch(hipStream_t stream, const LimPrm& prm, const LimScratch& S, int src, const float* res0, const float* res1, const float* x,
                            long long x_bstride, const Items& it, int B, OUT* y, long long y_bstride, long long n_count, float scale, float* s_out,
                            vits_session* ps = nullptr) {
  if (B <= 0 || S.ntiles <= 0) return;
  { LimProf lp(ps, "limit_gain_kernel");
  hipLaunchKernelGGL(limit_gain_kernel, dim3(B), dim3(64), 0, stream, it, S.ntiles, S.tpeak, src, prm, res0, res1, S.gv); }
  { LimProf lp(ps, "limit_scan_kernel");
  hipLaunchKernelGGL(limit_scan_kernel, dim3(S.ntj, B), dim3(LM_THREADS), 0, stream, S.p, it, prm, S.gv, S.ntj, S.cend); }
  { LimProf lp(ps, "limit_carry_kernel");
  hipLaunchKernelGGL(limit_carry_kernel, dim3(B), dim3(64), 0, stream, it, prm, S.ntj, S.cend, S.cin); }
  LimProf lp(ps, sizeof(OUT) == sizeof(int16_t) ? "limit_apply_kernel<int16>" : "limit_apply_kernel<float>");
  hipLaunchKernelGGL(limit_apply_kernel<OUT>, dim3((unsigned)((n_count + VITS_LIMIT_TILE - 1) / VITS_LIMIT_TILE), B), dim3(LM_THREADS), 0, stream, x,
                     x_bstride, it, S.p, prm, S.gv, S.ntiles, S.ntj, S.cin, y, y_bstride, n_count, scale, s_out, S.smin);
}

// res[b] = {L, peak, gain, 0} of a measurement becomes {L, peak, g, min s} of the limited call (keep), or {0, max p, g, min s}.  One wave
// per item.
__global__ __launch_bounds__(64) void limit_final_kernel(const Items it, int ntiles, const float* __restrict__ smin, const float* __restrict__ gv,
                                                         int keep, float* __restrict__ res) {
  const int b = blockIdx.x, t = threadIdx.x;
  const long long len = it.len_out(b);
  const int nt = (int)((len + VITS_LIMIT_TILE - 1) / VITS_LIMIT_TILE);
  float sm = 1.f;
  for (int k = t; k < nt; k += 64) sm = fminf(sm, smin[(long long)b * ntiles + k]);
  for (int o = 32; o > 0; o >>= 1) sm = fminf(sm, __shfl_xor(sm, o));
  if (t == 0) {
    if (!keep) { res[b * 4 + 0] = 0.f; res[b * 4 + 1] = gv[b * 2 + 1]; }
    res[b * 4 + 2] = gv[b * 2 + 0];
    res[b * 4 + 3] = sm;
  }
}

// ---- a call's request (the fields behind VITS_FLAG_LIMIT / STTS_FLAG_LIMIT) ---------------------------------------------------------
struct LimReq {
  bool on = false;
  LimPrm prm;
  LimTab tab;
  int rate = 0;
  float* out_reduction = nullptr;
};
// What a call asks of its last stage: a loudness request, a limiter, both (the two-pass form) or neither.
struct NormReq {
  LoudReq loud;
  LimReq lim;
  bool on() const { return loud.on || lim.on; }
};
// q->loud as loud_req left it (on or off) for the same call at `rate`; loud_ceiling the call's loudness_ceiling where q->loud.on
static int lim_req(bool flagged, int mode, float ceiling, float lookahead_ms, float release_ms, float gain, float* out_reduction, int rate,
                   float loud_ceiling, NormReq* q) {
  q->lim.on = false;
  if (!flagged) return VITS_OK;
  if (q->loud.on && q->loud.prm.mode == VITS_LOUDNESS_PEAK)
    return fail(VITS_ERR_ARG, "limit: loudness_mode VITS_LOUDNESS_PEAK with the limit flag: a peak target leaves a limiter nothing to do (use VITS_LOUDNESS_LUFS, or the limiter alone)");
  if (q->loud.on && loud_ceiling != 0.f)
    return fail(VITS_ERR_ARG, "limit: loudness_ceiling %g with the limit flag: limit_ceiling %g is the call's ceiling, loudness_ceiling must be 0", (double)loud_ceiling, (double)ceiling);
  LimReq& l = q->lim;
  TRY(limit_params(rate, mode, ceiling, lookahead_ms, release_ms, q->loud.on ? 1.f : gain, &l.prm));
  memset(&l.tab, 0, sizeof(l.tab));
  if (mode == VITS_LIMIT_TRUE) TRY(limit_tab(rate, &l.tab));
  l.rate = rate;
  l.out_reduction = out_reduction;
  l.on = true;
  return VITS_OK;
}
// res_h [B, 4] = {L, peak, gain, min s} of a finished call into the caller's result arrays
static void norm_req_results(const NormReq& q, const float* res_h, int B) {
  if (q.loud.on) loud_req_results(q.loud, res_h, B);
  if (q.lim.on && q.lim.out_reduction)
    for (int b = 0; b < B; ++b) q.lim.out_reduction[b] = res_h[b * 4 + 3];
}

// device scratch of a normalised and / or limited call over [B, N]: the loudness scratch | the limiter's | a second loudness scratch
struct NormScratch { LoudScratch LS, LS1; LimScratch MS; };
static size_t lim_extra_layout(int B, long long N, char* base, NormScratch* out) {
  const size_t a = lim_scratch_layout(B, N, true, base, out ? &out->MS : nullptr);
  return a + loud_scratch_layout(B, N, base ? base + a : nullptr, out ? &out->LS1 : nullptr);
}
static size_t norm_scratch_layout(const NormReq& lq, int B, long long N, char* base, NormScratch* out) {
  const size_t a = loud_scratch_layout(B, N, base, out ? &out->LS : nullptr);
  return lq.lim.on ? a + lim_extra_layout(B, N, base ? base + a : nullptr, out) : a;
}
static size_t norm_scratch_bytes(const NormReq& lq, int B, long long N) { return norm_scratch_layout(lq, B, N, nullptr, nullptr); }

// the limiter's part of a cached context's buffers (loud_ws_ensure first)
static int lim_ws_ensure(LoudWs* w, int B, long long N) {
  if (w->dm) return VITS_OK;
  w->dm_bytes = lim_extra_layout(B, N, nullptr, nullptr);
  if (hipMalloc((void**)&w->dm, w->dm_bytes) != hipSuccess) {
    w->dm = nullptr;
    (void)hipGetLastError();
    const size_t n = w->dm_bytes;
    w->dm_bytes = 0;
    return fail(VITS_ERR_NOMEM, "limiter buffers (%zu bytes)", n);
  }
  return VITS_OK;
}
static void norm_ws_layout(const NormReq& lq, const LoudWs& W, int B, long long N, NormScratch* out) {
  out->LS = W.S;
  if (lq.lim.on) lim_extra_layout(B, N, W.dm, out);
}

// The last stage of a flagged call on `stream` (no allocation, no synchronisation): B items x[b, 0 : it.len_out(b)) of capacity it.cap measured,
// normalised and / or limited into y[b, 0 : n_count), NS.LS.res[b] = {L, peak, gain, min s}.  Without a limiter these are exactly
// loud_measure_launch and loud_apply_launch.
template <typename OUT>
static void norm_launch(hipStream_t stream, const NormReq& nq, const NormScratch& NS, const float* x, long long x_bstride, const Items& it, int B,
                        OUT* y, long long y_bstride, long long n_count, float scale, vits_session* ps = nullptr) {
  const LoudReq& lq = nq.loud;
  if (!nq.lim.on) {
    loud_measure_launch(stream, lq.P, lq.prm, NS.LS, x, x_bstride, it, B, ps);
    loud_apply_launch<OUT>(stream, NS.LS, x, x_bstride, it, B, y, y_bstride, n_count, scale, ps);
    return;
  }
  if (B <= 0 || n_count <= 0) return;
  const LimReq& q = nq.lim;
  const bool lufs = lq.on;  // (with a limiter a loudness request is a LUFS target: lim_req refuses the peak mode)
  lim_env_launch(stream, q.prm.mode, q.tab, NS.MS, x, x_bstride, it, B, ps);
  if (lufs) {
    loud_measure_launch(stream, lq.P, lq.prm, NS.LS, x, x_bstride, it, B, ps);
    lim_pass_launch<float>(stream, q.prm, NS.MS, 1, NS.LS.res, nullptr, x, x_bstride, it, B, NS.MS.y0, it.cap, it.cap, 1.f, nullptr, ps);
    loud_measure_launch(stream, lq.P, lq.prm, NS.LS1, NS.MS.y0, it.cap, it, B, ps);
    lim_pass_launch<OUT>(stream, q.prm, NS.MS, 2, NS.LS.res, NS.LS1.res, x, x_bstride, it, B, y, y_bstride, n_count, scale, nullptr, ps);
  } else {
    lim_pass_launch<OUT>(stream, q.prm, NS.MS, 0, nullptr, nullptr, x, x_bstride, it, B, y, y_bstride, n_count, scale, nullptr, ps);
  }
  LimProf lp(ps, "limit_final_kernel");
  hipLaunchKernelGGL(limit_final_kernel, dim3(B), dim3(64), 0, stream, it, NS.MS.ntiles, NS.MS.smin, NS.MS.gv, lufs ? 1 : 0, NS.LS.res);
}

// ---- host-only entry point and the kernel-level parity doors --------------------------------------------------------------------
int vits_limit_plan(int32_t rate, float lookahead_ms, float release_ms, int32_t* W, double* a) {
  int w = 0;
  double aa = 0.0;
  TRY(limit_plan(rate, lookahead_ms, release_ms, &w, &aa));
  if (W) *W = w;
  if (a) *a = aa;
  return VITS_OK;
}

// x [B, N] on the host through step 1 (prm null: true peak only) or a whole limited call; lufs: the two-pass form at `target`
static int lim_op(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, const LimPrm* prm, bool lufs,
                  float target, float* tp, float* s, float* y, float* reduction, float* loudness, float* gain) {
  std::vector<int> len32;
  TRY(op_items_check("limit", x, lengths, B, N, &len32));
  const int mode = prm ? prm->mode : VITS_LIMIT_TRUE;
  LimTab tab;
  memset(&tab, 0, sizeof(tab));
  if (mode == VITS_LIMIT_TRUE) TRY(limit_tab(rate, &tab));
  LoudPlan LP;
  LoudParams lprm;
  if (lufs) {
    TRY(loud_params(VITS_LOUDNESS_LUFS, target, 0.f, &lprm));
    TRY(loud_plan(rate, &LP));
  }
  OpDoor d("limit", device);
  const size_t lscr = align_up(loud_scratch_bytes(B, N), 256), scr = lim_scratch_layout(B, N, lufs, nullptr, nullptr), nx = (size_t)B * N;
  char* dscr = d.dev<char>(scr + 2 * lscr);
  float* dx = d.up(x, nx);
  int* dl = d.up(len32.data(), B);
  float* dy = prm ? d.out<float>(nx) : nullptr;
  float* ds = s ? d.out<float>(nx) : nullptr;
  LimScratch S;
  LoudScratch S0, S1;
  lim_scratch_layout(B, N, lufs, dscr, &S);
  loud_scratch_layout(B, N, dscr ? dscr + scr : nullptr, &S0);
  loud_scratch_layout(B, N, dscr ? dscr + scr + lscr : nullptr, &S1);
  std::vector<float> res0((size_t)B * 4), gv((size_t)B * 2), tiles((size_t)B * S.ntiles);
  const Items it{dl, 1, 1, 1, N};
  if (d.ok()) {
    lim_env_launch(nullptr, mode, tab, S, dx, N, it, B);
    if (prm && !lufs) {
      lim_pass_launch<float>(nullptr, *prm, S, 0, nullptr, nullptr, dx, N, it, B, dy, N, N, 1.f, ds);
    } else if (prm) {
      loud_measure_launch(nullptr, LP, lprm, S0, dx, N, it, B);
      lim_pass_launch<float>(nullptr, *prm, S, 1, S0.res, nullptr, dx, N, it, B, S.y0, N, N, 1.f, (float*)nullptr);
      loud_measure_launch(nullptr, LP, lprm, S1, S.y0, N, it, B);
      lim_pass_launch<float>(nullptr, *prm, S, 2, S0.res, S1.res, dx, N, it, B, dy, N, N, 1.f, ds);
    }
  }
  d.finish();
  d.down(tiles.data(), prm ? S.smin : S.tpeak, tiles.size());
  if (prm) d.down(gv.data(), S.gv, gv.size());
  if (lufs) d.down(res0.data(), S0.res, res0.size());
  if (y) d.down(y, dy, nx);
  if (s) d.down(s, ds, nx);
  if (!d.ok()) return d.rc();
  for (int b = 0; b < B; ++b) {  // the tiles of an item: max p, or min s (both exact in any order)
    const int nt = (int)((lengths[b] + VITS_LIMIT_TILE - 1) / VITS_LIMIT_TILE);
    float v = prm ? 1.f : 0.f;
    for (int k = 0; k < nt; ++k) {
      const float w = tiles[(size_t)b * S.ntiles + k];
      v = prm ? std::min(v, w) : std::max(v, w);
    }
    if (tp) tp[b] = v;
    if (reduction) reduction[b] = v;
    if (loudness) loudness[b] = res0[(size_t)b * 4 + 0];
    if (gain) gain[b] = gv[(size_t)b * 2];
  }
  return VITS_OK;
}

int vits_op_true_peak(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, float* tp) {
  if (!tp) return fail(VITS_ERR_ARG, "limit: null output");
  return lim_op(device, x, lengths, B, N, rate, nullptr, false, 0.f, tp, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int vits_op_limit_gain(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, int32_t mode, float ceiling,
                       float lookahead_ms, float release_ms, float gain, float* s) {
  if (!s) return fail(VITS_ERR_ARG, "limit: null output");
  LimPrm prm;
  TRY(limit_params(rate, mode, ceiling, lookahead_ms, release_ms, gain, &prm));
  return lim_op(device, x, lengths, B, N, rate, &prm, false, 0.f, nullptr, s, nullptr, nullptr, nullptr, nullptr);
}

int vits_op_limit(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, int32_t mode, float ceiling,
                  float lookahead_ms, float release_ms, float gain, float* y, float* reduction) {
  if (!y) return fail(VITS_ERR_ARG, "limit: null output");
  LimPrm prm;
  TRY(limit_params(rate, mode, ceiling, lookahead_ms, release_ms, gain, &prm));
  return lim_op(device, x, lengths, B, N, rate, &prm, false, 0.f, nullptr, nullptr, y, reduction, nullptr, nullptr);
}

int vits_op_loudness_limit(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, float target, int32_t mode,
                           float ceiling, float lookahead_ms, float release_ms, float* y, float* loudness, float* gain, float* reduction) {
  if (!y) return fail(VITS_ERR_ARG, "limit: null output");
  LimPrm prm;
  TRY(limit_params(rate, mode, ceiling, lookahead_ms, release_ms, 1.f, &prm));
  return lim_op(device, x, lengths, B, N, rate, &prm, true, target, nullptr, nullptr, y, reduction, loudness, gain);
}
