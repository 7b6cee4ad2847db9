// loudness.hip.h -- loudness-normalised output (include/vits_loudness.h): the BS.1770 K-weighting, gated block statistics, peak and gain
// of every item of a batch on the device, and the gain applied behind them.  Part of the ONE translation unit engine.hip (included
// there, after the resampler and the denoiser).
//
// The serial part is the 4th-order recurrence.  The cascade of the two biquads (transposed direct form II) is a linear system with the
// state s = (p1, p2, q1, q2):  s' = A s + B x,  y = C s + D x.  So the end state of a run of samples is (its end state from zero
// state) + A^run (its incoming state), and the incoming states of all runs follow from a scan over the zero-state end states with the
// matrices A^(LD_S 2^k), which the host forms in double from the fp32 coefficients.
//
// Decomposition: a thread owns LD_S consecutive samples, a workgroup LD_THREADS threads = VITS_LOUDNESS_TILE samples of one item; grid
// (tiles, items).  Dependencies between tiles are launch boundaries:
//   1. loud_tile_kernel     zero-state runs + Kogge-Stone scan in LDS -> the tile's zero-state end state E[b][k], the tile's peak
//   2. loud_carry_kernel    one wave per item: c[b][0] = 0, c[b][k + 1] = A^TILE c[b][k] + E[b][k] (lane 0 walks the tiles; the other
//                           lanes stage E through LDS 64 tiles at a time so the chain never waits for memory)
//   3. loud_square_kernel   the same runs with thread 0 starting from c[b][k], the scan, then every run again from its true incoming
//                           state: y^2 summed per 100 ms hop into fixed slots part[b][k][hop - first hop of the tile]
//   4. loud_final_kernel    one workgroup per item, in double: hop energies (the tiles of a hop added in ascending order), both gates,
//                           L, the peak over tiles and the gain -> res[b] = {L, peak, gain}
//   5. loud_apply_kernel    y = gain[b] * x, float or with pcm16_of
// Cost written down: the x tile is read from memory three times (1, 3, 5) and the runs are computed three times (once in 1, twice in 3)
// rather than storing 4 words of state per LD_S samples; 2 (one lane per item) is 64 + 20 k cycles for k tiles, 15 us for a
// 2000-token utterance.  No atomics and no waiting between workgroups; every sum has a fixed order.
//
// LDS: a thread walks xs[t * LD_ROW + i], i = 0 .. LD_S - 1.  ds_read_b32 banks are (address / 4) % 32 over the lanes of a 32-lane half;
// with LD_ROW = LD_S + 1 = 9, odd, lanes t .. t + 31 fall on 32 different banks for every i.  (Unpadded, stride 8, they would fall on 4.)
// The coalesced staging writes go to j + j / 8: 32 consecutive j cover 35 addresses, so 3 banks are hit twice -- 2-way on 3 of 32 lanes.
#pragma once
#include "../../include/vits_loudness.h"

#define LD_S 8
#define LD_THREADS 256
#define LD_ROW (LD_S + 1)
#define LD_LEVELS 8  // log2(LD_THREADS)
#define LD_SLOTS 8   // hops one tile can touch: (hop - 1 + TILE - 1) / hop + 1 <= 7 at hop >= 400, + 1 for a run's (empty) second part
#define LD_MIN_HOP ((VITS_LOUDNESS_MIN_RATE + 5) / 10)
static_assert(LD_S * LD_THREADS == VITS_LOUDNESS_TILE, "tile = threads x run");
static_assert((1 << LD_LEVELS) == LD_THREADS, "scan levels");
static_assert((LD_MIN_HOP - 1 + VITS_LOUDNESS_TILE - 1) / LD_MIN_HOP + 2 <= LD_SLOTS, "hop slots of a tile");
static_assert(LD_MIN_HOP > LD_S, "a run touches at most two hops");

// The recurrence runs in double: the high-pass stage's poles lie within 0.005 of the unit circle at 48 kHz, and a DC offset in the input
// parks the transposed-form states at the size of the offset while the output is its small difference.  An fp32 recurrence measured
// 5.7e-3 LU from the float64 restatement on the worst test item at 48 kHz (8.8e-4 at 22050 Hz, 2.1e-4 at 8000 Hz), this one 2e-6.  The
// coefficients are still the fp32 values of the definition; the kernels are bound by the serial chain and by memory, not by the fp64 rate.
typedef double ld_t;
struct LoudCoef {
  ld_t b[3], a[2];  // stage 1: b0 b1 b2, a1 a2 (each the fp32 value)
  ld_t d[2];        // stage 2: a1 a2 (its b is 1, -2, 1)
  ld_t P[LD_LEVELS][16];  // A^(LD_S 2^k), row-major
  ld_t PT[16];            // A^VITS_LOUDNESS_TILE
  int hop;
};
struct LoudParams { int mode = 0; float target = 0.f, ceiling = 0.f; };  // mode 0: measure only (gain 1)

struct LoudPlan {
  int rate = 0, hop = 0;
  double sos[2][6];
  LoudCoef c;
};

static void ld_matmul(const double* a, const double* b, double* out) {
  double r[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0;
      for (int k = 0; k < 4; ++k) s += a[i * 4 + k] * b[k * 4 + j];
      r[i * 4 + j] = s;
    }
  memcpy(out, r, sizeof(r));
}

static int loud_plan(int rate, LoudPlan* out) {
  if (rate < VITS_LOUDNESS_MIN_RATE) return fail(VITS_ERR_UNSUPPORTED, "loudness: rate %d Hz is below %d Hz", rate, VITS_LOUDNESS_MIN_RATE);
  LoudPlan P;
  P.rate = rate;
  P.hop = (int)(((long long)rate + 5) / 10);
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = tan(M_PI * f0 / rate), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
    double* s = P.sos[0];
    s[0] = (Vh + Vb * K / Q + K * K) / a0; s[1] = 2.0 * (K * K - Vh) / a0; s[2] = (Vh - Vb * K / Q + K * K) / a0;
    s[3] = 1.0; s[4] = 2.0 * (K * K - 1.0) / a0; s[5] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = tan(M_PI * f0 / rate), a0 = 1.0 + K / Q + K * K;
    double* s = P.sos[1];
    s[0] = 1.0; s[1] = -2.0; s[2] = 1.0;
    s[3] = 1.0; s[4] = 2.0 * (K * K - 1.0) / a0; s[5] = (1.0 - K / Q + K * K) / a0;
  }
  LoudCoef& c = P.c;
  for (int i = 0; i < 3; ++i) c.b[i] = (float)P.sos[0][i];  // (rounded once to fp32, as the definition says)
  c.a[0] = (float)P.sos[0][4]; c.a[1] = (float)P.sos[0][5];
  c.d[0] = (float)P.sos[1][4]; c.d[1] = (float)P.sos[1][5];
  c.hop = P.hop;
  // A of those coefficients (x = 0: y1 = p1, y2 = p1 + q1) and its powers
  const double a1 = c.a[0], a2 = c.a[1], d1 = c.d[0], d2 = c.d[1];
  double A[16] = {-a1, 1, 0, 0,
                  -a2, 0, 0, 0,
                  -2.0 - d1, 0, -d1, 1,
                  1.0 - d2, 0, -d2, 0};
  double M[16];
  memcpy(M, A, sizeof(M));
  for (int s = 1; s < LD_S; s *= 2) ld_matmul(M, M, M);  // A^LD_S
  for (int k = 0; k < LD_LEVELS; ++k) {
    for (int i = 0; i < 16; ++i) c.P[k][i] = M[i];
    ld_matmul(M, M, M);
  }
  for (int i = 0; i < 16; ++i) c.PT[i] = M[i];  // A^(LD_S 2^LD_LEVELS)
  *out = P;
  return VITS_OK;
}

static int loud_params(int mode, float target, float ceiling, LoudParams* out) {
  LoudParams p;
  p.mode = mode;
  p.target = target;
  p.ceiling = 0.f;
  if (mode == VITS_LOUDNESS_LUFS) {
    if (!(target >= -70.f && target <= 0.f)) return fail(VITS_ERR_ARG, "loudness: LUFS target %g outside [-70, 0]", (double)target);
    if (!(ceiling >= 0.f) || std::isinf(ceiling)) return fail(VITS_ERR_ARG, "loudness: ceiling %g must be >= 0 (0 = none)", (double)ceiling);
    p.ceiling = ceiling;
  } else if (mode == VITS_LOUDNESS_PEAK) {
    if (!(target > 0.f && target <= 1.f)) return fail(VITS_ERR_ARG, "loudness: peak target %g outside (0, 1]", (double)target);
  } else {
    return fail(VITS_ERR_ARG, "loudness: mode %d is neither VITS_LOUDNESS_LUFS (1) nor VITS_LOUDNESS_PEAK (2)", mode);
  }
  *out = p;
  return VITS_OK;
}

// ---- device ---------------------------------------------------------------------------------------------------------------
struct LdState { ld_t p1, p2, q1, q2; };

// one sample through the cascade; returns the K-weighted sample
__device__ __forceinline__ ld_t ld_step(const LoudCoef& c, LdState& s, ld_t x) {
  const ld_t y1 = fma(c.b[0], x, s.p1);
  s.p1 = fma(c.b[1], x, s.p2) - c.a[0] * y1;
  s.p2 = fma(c.b[2], x, -c.a[1] * y1);
  const ld_t y2 = y1 + s.q1;
  s.q1 = fma((ld_t)-2, y1, s.q2) - c.d[0] * y2;
  s.q2 = fma(-c.d[1], y2, y1);
  return y2;
}

__device__ __forceinline__ LdState ld_mv(const ld_t* M, const LdState& v) {
  LdState r;
  r.p1 = M[0] * v.p1 + M[1] * v.p2 + M[2] * v.q1 + M[3] * v.q2;
  r.p2 = M[4] * v.p1 + M[5] * v.p2 + M[6] * v.q1 + M[7] * v.q2;
  r.q1 = M[8] * v.p1 + M[9] * v.p2 + M[10] * v.q1 + M[11] * v.q2;
  r.q2 = M[12] * v.p1 + M[13] * v.p2 + M[14] * v.q1 + M[15] * v.q2;
  return r;
}

// stages samples [n0, n0 + TILE) of the item, zero at and beyond len (those are never read), padded rows
__device__ __forceinline__ void ld_stage(float* xs, const float* __restrict__ xb, long long n0, long long len) {
  for (int j = threadIdx.x; j < VITS_LOUDNESS_TILE; j += LD_THREADS) {
    const long long n = n0 + j;
    xs[(j / LD_S) * LD_ROW + (j % LD_S)] = n < len ? xb[n] : 0.f;
  }
}

// in: every thread's end state of its own run.  out: the state at the end of thread t's run given all runs before it in the tile
// (inclusive scan, v[t] = sum_u<=t A^(LD_S (t - u)) e[u]), in sc[cur][t]; returns cur.  Kogge-Stone: the order of the additions is fixed.
__device__ __forceinline__ int ld_scan(const LoudCoef& c, LdState (*sc)[LD_THREADS], LdState e) {
  const int t = threadIdx.x;
  int cur = 0;
  sc[0][t] = e;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < LD_LEVELS; ++k) {
    const int off = 1 << k;
    LdState v = sc[cur][t];
    if (t >= off) {
      const LdState w = ld_mv(c.P[k], sc[cur][t - off]);
      v.p1 += w.p1; v.p2 += w.p2; v.q1 += w.q1; v.q2 += w.q2;
    }
    sc[cur ^ 1][t] = v;
    __syncthreads();
    cur ^= 1;
  }
  return cur;
}

// E / tpeak: [B, ntiles]; written for the tiles that hold samples of the item (k < ceil(len / TILE)), the only ones read later
__global__ __launch_bounds__(LD_THREADS) void loud_tile_kernel(const float* __restrict__ x, long long x_bstride, const Items it, const LoudCoef c,
                                                               int ntiles, LdState* __restrict__ E, float* __restrict__ tpeak) {
  __shared__ float xs[LD_THREADS * LD_ROW];
  __shared__ LdState sc[2][LD_THREADS];
  __shared__ float pk[LD_THREADS];
  const int b = blockIdx.y, k = blockIdx.x, t = threadIdx.x;
  const long long len = it.len_out(b), n0 = (long long)k * VITS_LOUDNESS_TILE;
  if (n0 >= len) return;  // (the whole workgroup)
  ld_stage(xs, x + (long long)b * x_bstride, n0, len);
  __syncthreads();
  LdState s = {0, 0, 0, 0};
  float p = 0.f;
#pragma unroll
  for (int i = 0; i < LD_S; ++i) {
    const float v = xs[t * LD_ROW + i];
    p = fmaxf(p, fabsf(v));
    ld_step(c, s, v);
  }
  pk[t] = p;
  const int cur = ld_scan(c, sc, s);  // (its barriers also publish pk)
  for (int w = LD_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) pk[t] = fmaxf(pk[t], pk[t + w]);
    __syncthreads();
  }
  if (t == 0) {
    E[(long long)b * ntiles + k] = sc[cur][LD_THREADS - 1];
    tpeak[(long long)b * ntiles + k] = pk[0];
  }
}

// C[b][k]: the state the item's tile k starts from.  One wave per item.
__global__ __launch_bounds__(64) void loud_carry_kernel(const Items it, const LoudCoef c, int ntiles, const LdState* __restrict__ E,
                                                        LdState* __restrict__ C) {
  __shared__ LdState es[64];
  const int b = blockIdx.x, t = threadIdx.x;
  const long long len = it.len_out(b);
  const int nt = (int)((len + VITS_LOUDNESS_TILE - 1) / VITS_LOUDNESS_TILE);
  LdState s = {0, 0, 0, 0};
  for (int k0 = 0; k0 < nt; k0 += 64) {
    if (k0 + t < nt) es[t] = E[(long long)b * ntiles + k0 + t];
    __syncthreads();
    if (t == 0) {
      const int n = nt - k0 < 64 ? nt - k0 : 64;
      for (int i = 0; i < n; ++i) {
        C[(long long)b * ntiles + k0 + i] = s;
        const LdState w = ld_mv(c.PT, s), e = es[i];
        s.p1 = w.p1 + e.p1; s.p2 = w.p2 + e.p2; s.q1 = w.q1 + e.q1; s.q2 = w.q2 + e.q2;
      }
    }
    __syncthreads();
  }
}

// part[b][k][j]: the sum of y[n]^2 over the samples n < len of tile k that lie in hop (k TILE) / hop + j
__global__ __launch_bounds__(LD_THREADS) void loud_square_kernel(const float* __restrict__ x, long long x_bstride, const Items it, const LoudCoef c,
                                                                 int ntiles, const LdState* __restrict__ C, ld_t* __restrict__ part) {
  __shared__ float xs[LD_THREADS * LD_ROW];
  __shared__ LdState sc[2][LD_THREADS];
  __shared__ ld_t ca[LD_THREADS], cb[LD_THREADS];
  __shared__ int sl[LD_THREADS];
  const int b = blockIdx.y, k = blockIdx.x, t = threadIdx.x;
  const long long len = it.len_out(b), n0 = (long long)k * VITS_LOUDNESS_TILE;
  if (n0 >= len) return;
  ld_stage(xs, x + (long long)b * x_bstride, n0, len);
  __syncthreads();
  const LdState zero = {0, 0, 0, 0};
  const LdState cin = C[(long long)b * ntiles + k];
  LdState s = t == 0 ? cin : zero;
#pragma unroll
  for (int i = 0; i < LD_S; ++i) ld_step(c, s, xs[t * LD_ROW + i]);
  const int cur = ld_scan(c, sc, s);
  s = t == 0 ? cin : sc[cur][t - 1];
  // the run again, from its true incoming state: squares into the (at most two) hops it touches
  const long long nt0 = n0 + (long long)t * LD_S;
  const long long h0 = nt0 / c.hop, nb = (h0 + 1) * c.hop;  // nb: first sample of the next hop
  ld_t sa = 0, sb = 0;
#pragma unroll
  for (int i = 0; i < LD_S; ++i) {
    const ld_t y = ld_step(c, s, xs[t * LD_ROW + i]);
    const long long n = nt0 + i;
    const ld_t q = n < len ? y * y : (ld_t)0;
    if (n < nb) sa += q; else sb += q;
  }
  ca[t] = sa; cb[t] = sb;
  sl[t] = (int)(h0 - n0 / c.hop);
  __syncthreads();
  // wave w adds slots w and w + 4: lane l takes threads l, l + 64, l + 128, l + 192 in that order, then a butterfly over the lanes
  const int w = t >> 6, l = t & 63;
  for (int j = w; j < LD_SLOTS; j += LD_THREADS / 64) {
    ld_t acc = 0;
    for (int u = l; u < LD_THREADS; u += 64) {
      const int su = sl[u];
      acc += (su == j ? ca[u] : (ld_t)0) + (su + 1 == j ? cb[u] : (ld_t)0);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (l == 0) part[((long long)b * ntiles + k) * LD_SLOTS + j] = acc;
  }
}

__device__ __forceinline__ double ld_block_sum(double* red, double v) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int w = LD_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  return red[0];
}

// Eh: double [B, eh_stride] scratch (hop energies); res: float [B, 4] = {L, peak, gain, 0}
__global__ __launch_bounds__(LD_THREADS) void loud_final_kernel(const Items it, int hop, int ntiles, const ld_t* __restrict__ part,
                                                                const float* __restrict__ tpeak, double* __restrict__ Eh, long long eh_stride,
                                                                const LoudParams prm, float* __restrict__ res) {
  __shared__ double red[LD_THREADS];
  __shared__ float pk[LD_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  const long long len = it.len_out(b);
  const int nt = (int)((len + VITS_LOUDNESS_TILE - 1) / VITS_LOUDNESS_TILE);
  const long long nh = len / hop, nh_all = (len + hop - 1) / hop;
  double* eh = Eh + (long long)b * eh_stride;
  const ld_t* pb = part + (long long)b * ntiles * LD_SLOTS;
  for (long long i = t; i < nh_all; i += LD_THREADS) {  // hop i: its tiles in ascending order
    const long long first = i * hop, last = ((i + 1) * hop < len ? (i + 1) * hop : len) - 1;
    double e = 0.0;
    for (long long k = first / VITS_LOUDNESS_TILE; k <= last / VITS_LOUDNESS_TILE; ++k)
      e += (double)pb[k * LD_SLOTS + (i - (k * VITS_LOUDNESS_TILE) / hop)];
    eh[i] = e;
  }
  float p = 0.f;
  for (int k = t; k < nt; k += LD_THREADS) p = fmaxf(p, tpeak[(long long)b * ntiles + k]);
  pk[t] = p;
  __syncthreads();  // (eh is read below by other threads of this workgroup)
  for (int w = LD_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) pk[t] = fmaxf(pk[t], pk[t + w]);
    __syncthreads();
  }
  const float peak = pk[0];
  // blocks
  long long nblk = 0;
  double z_short = 0.0;
  if (nh >= 4) {
    nblk = nh - 3;
  } else if (len >= 1) {
    nblk = 1;
    for (long long i = 0; i < nh_all; ++i) z_short += eh[i];
    z_short /= (double)len;
  }
  const double inv = 1.0 / (4.0 * (double)hop);
  double gamma = -70.0, loud = -INFINITY;
  for (int pass = 0; pass < 2; ++pass) {  // 0: the absolute gate, 1: both
    double s = 0.0, cnt = 0.0;
    for (long long j = t; j < nblk; j += LD_THREADS) {
      const double z = nh >= 4 ? (eh[j] + eh[j + 1] + eh[j + 2] + eh[j + 3]) * inv : z_short;
      if (z > 0.0) {
        const double lj = -0.691 + 10.0 * log10(z);
        if (lj > -70.0 && (pass == 0 || lj > gamma)) { s += z; cnt += 1.0; }
      }
    }
    s = ld_block_sum(red, s);
    cnt = ld_block_sum(red, cnt);
    if (cnt == 0.0) { loud = -INFINITY; break; }  // (uniform over the workgroup)
    loud = -0.691 + 10.0 * log10(s / cnt);
    gamma = loud - 10.0;
  }
  if (t == 0) {
    double g = 1.0;
    if (prm.mode == VITS_LOUDNESS_LUFS) {
      if (loud > -INFINITY) g = pow(10.0, ((double)prm.target - loud) / 20.0);
      if (prm.ceiling > 0.f && g * (double)peak > (double)prm.ceiling) g = (double)prm.ceiling / (double)peak;
    } else if (prm.mode == VITS_LOUDNESS_PEAK) {
      if (peak > 0.f) g = (double)prm.target / (double)peak;
    }
    res[b * 4 + 0] = (float)loud;
    res[b * 4 + 1] = peak;
    res[b * 4 + 2] = (float)g;
    res[b * 4 + 3] = 0.f;
  }
}

// y[b, j] = res[b].gain * x[b, j] for j < len, 0 beyond (x is not read there), 0 <= j < n_count.  OUT = int16_t: pcm16_of.
template <typename OUT>
__global__ __launch_bounds__(256) void loud_apply_kernel(const float* __restrict__ x, long long x_bstride, const Items it,
                                                         const float* __restrict__ res, OUT* __restrict__ y, long long y_bstride, long long n_count,
                                                         float scale) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (j >= n_count) return;
  const long long len = it.len_out(b);
  const float v = j < len ? res[b * 4 + 2] * x[(long long)b * x_bstride + j] : 0.f;
  if constexpr (sizeof(OUT) == sizeof(int16_t)) y[(long long)b * y_bstride + j] = pcm16_of(v, scale);
  else y[(long long)b * y_bstride + j] = v;
}

// ---- launches ----------------------------------------------------------------------------------------------------------------
// device scratch of a measurement over [B, N]: E | C | tpeak | part | Eh | res (sized for the smallest hop, so it serves every rate)
struct LoudScratch {
  LdState *E, *C;
  float *tpeak, *res;
  ld_t* part;
  double* Eh;
  long long eh_stride;
  int ntiles;
};
static size_t loud_scratch_layout(int B, long long N, char* base, LoudScratch* out) {
  const long long nt = (N + VITS_LOUDNESS_TILE - 1) / VITS_LOUDNESS_TILE, ehs = N / LD_MIN_HOP + 2;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return base ? base + o : nullptr; };
  LoudScratch S;
  S.E = reinterpret_cast<LdState*>(take(sizeof(LdState) * (size_t)B * nt));
  S.C = reinterpret_cast<LdState*>(take(sizeof(LdState) * (size_t)B * nt));
  S.tpeak = reinterpret_cast<float*>(take(sizeof(float) * (size_t)B * nt));
  S.part = reinterpret_cast<ld_t*>(take(sizeof(ld_t) * (size_t)B * nt * LD_SLOTS));
  S.Eh = reinterpret_cast<double*>(take(sizeof(double) * (size_t)B * ehs));
  S.res = reinterpret_cast<float*>(take(sizeof(float) * (size_t)B * 4));
  S.eh_stride = ehs;
  S.ntiles = (int)nt;
  if (out) *out = S;
  return off;
}
static size_t loud_scratch_bytes(int B, long long N) { return loud_scratch_layout(B, N, nullptr, nullptr); }

// a launch counted / timed under the operation "out.loudness" where a session is given (the parity doors have none)
struct LoudProf {
  char buf[sizeof(ProfScope)];
  ProfScope* p = nullptr;
  LoudProf(vits_session* s, const char* kernel) { if (s) p = new (buf) ProfScope(s, "out.loudness", 0, kernel); }
  ~LoudProf() { if (p) p->~ProfScope(); }
};

// Measures B items x[b, 0 : it.len_out(b)) of capacity it.cap on `stream` (no allocation, no synchronisation): S.res[b] = {L, peak, gain}.
static void loud_measure_launch(hipStream_t stream, const LoudPlan& P, const LoudParams& prm, const LoudScratch& S, const float* x,
                                long long x_bstride, const Items& it, int B, vits_session* ps = nullptr) {
  if (B <= 0) return;
  if (S.ntiles > 0) {
    { LoudProf lp(ps, "loud_tile_kernel");
    hipLaunchKernelGGL(loud_tile_kernel, dim3(S.ntiles, B), dim3(LD_THREADS), 0, stream, x, x_bstride, it, P.c, S.ntiles, S.E, S.tpeak); }
    { LoudProf lp(ps, "loud_carry_kernel");
    hipLaunchKernelGGL(loud_carry_kernel, dim3(B), dim3(64), 0, stream, it, P.c, S.ntiles, S.E, S.C); }
    { LoudProf lp(ps, "loud_square_kernel");
    hipLaunchKernelGGL(loud_square_kernel, dim3(S.ntiles, B), dim3(LD_THREADS), 0, stream, x, x_bstride, it, P.c, S.ntiles, S.C, S.part); }
  }
  LoudProf lp(ps, "loud_final_kernel");
  hipLaunchKernelGGL(loud_final_kernel, dim3(B), dim3(LD_THREADS), 0, stream, it, P.hop, S.ntiles, S.part, S.tpeak, S.Eh, S.eh_stride, prm, S.res);
}

template <typename OUT>
static void loud_apply_launch(hipStream_t stream, const LoudScratch& S, const float* x, long long x_bstride, const Items& it, int B, OUT* y,
                              long long y_bstride, long long n_count, float scale, vits_session* ps = nullptr) {
  if (B <= 0 || n_count <= 0) return;
  LoudProf lp(ps, sizeof(OUT) == sizeof(int16_t) ? "loud_apply_kernel<int16>" : "loud_apply_kernel<float>");
  hipLaunchKernelGGL(loud_apply_kernel<OUT>, dim3((unsigned)((n_count + 255) / 256), B), dim3(256), 0, stream, x, x_bstride, it, S.res, y, y_bstride, n_count, scale);
}

// ---- a call's request (the fields behind VITS_FLAG_LOUDNESS / STTS_FLAG_LOUDNESS) ----------------------------------------------
struct LoudReq {
  bool on = false;
  LoudParams prm;
  float *out_loudness = nullptr, *out_gain = nullptr;
  LoudPlan P;  // of the rate the call returns
};
static int loud_req(bool flagged, int mode, float target, float ceiling, float* out_loudness, float* out_gain, int rate, LoudReq* q) {
  q->on = false;
  if (!flagged) return VITS_OK;
  TRY(loud_params(mode, target, ceiling, &q->prm));
  TRY(loud_plan(rate, &q->P));
  q->out_loudness = out_loudness; q->out_gain = out_gain;
  q->on = true;
  return VITS_OK;
}
static void loud_req_results(const LoudReq& q, const float* res_h, int B) {
  for (int b = 0; b < B; ++b) {
    if (q.out_loudness) q.out_loudness[b] = res_h[b * 4 + 0];
    if (q.out_gain) q.out_gain[b] = res_h[b * 4 + 2];
  }
}

// device + pinned buffers of the flagged calls of one cached context (a back session, one of its rates, a multistream back): the
// scratch, the normalised output (float or int16, sized for float) and the pinned copies.  Allocated by the first flagged request.
struct LoudWs {
  char* d = nullptr;    // scratch | y
  char* h = nullptr;    // pinned: res [B, 4] | y
  char* dm = nullptr;   // limit.hip.h: the limiter's scratch, allocated by the context's first limited request
  size_t scr_bytes = 0, y_bytes = 0, dm_bytes = 0;
  LoudScratch S;
  void* y_d() const { return d + scr_bytes; }
  float* res_h() const { return reinterpret_cast<float*>(h); }
  char* y_h() const { return h + 4096; }
};
static void loud_ws_free(LoudWs* w) {
  if (w->d) hipFree(w->d);
  if (w->dm) hipFree(w->dm);
  if (w->h) hipHostFree(w->h);
  *w = LoudWs();
}
static void loud_ws_delete(LoudWs* w) {
  if (!w) return;
  loud_ws_free(w);
  delete w;
}
static size_t loud_ws_bytes(const LoudWs* w) { return w ? w->scr_bytes + w->y_bytes + w->dm_bytes : 0; }
static int loud_ws_ensure(LoudWs** pw, int B, long long N) {
  if (!*pw) *pw = new LoudWs();
  LoudWs* w = *pw;
  if (w->d) return VITS_OK;
  if (B > 256) return fail(VITS_ERR_UNSUPPORTED, "loudness: batch of %d items (at most 256)", B);
  w->scr_bytes = loud_scratch_bytes(B, N);
  w->y_bytes = sizeof(float) * (size_t)B * (size_t)N;
  if (hipMalloc((void**)&w->d, w->scr_bytes + w->y_bytes) != hipSuccess || hipHostMalloc((void**)&w->h, 4096 + w->y_bytes) != hipSuccess) {
    loud_ws_free(w);
    (void)hipGetLastError();
    return fail(VITS_ERR_NOMEM, "loudness buffers (%zu bytes)", w->scr_bytes + w->y_bytes);
  }
  loud_scratch_layout(B, N, w->d, &w->S);
  return VITS_OK;
}

// ---- host-only entry point and the kernel-level parity doors --------------------------------------------------------------------
int vits_loudness_plan(int32_t rate, double sos[2][6], int32_t* hop) {
  LoudPlan P;
  TRY(loud_plan(rate, &P));
  if (sos) memcpy(sos, P.sos, sizeof(P.sos));
  if (hop) *hop = P.hop;
  return VITS_OK;
}

// x [B, N] on the host measured (prm.mode 0) or normalised into y; results for every item
static int loud_op(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, const LoudParams& prm, float* y,
                   float* loudness, float* peak, float* gain) {
  std::vector<int> len32;
  TRY(op_items_check("loudness", x, lengths, B, N, &len32));
  LoudPlan P;
  TRY(loud_plan(rate, &P));
  OpDoor d("loudness", device);
  const size_t nx = (size_t)B * N;
  char* dscr = d.dev<char>(loud_scratch_bytes(B, N));
  float* dx = d.up(x, nx);
  int* dl = d.up(len32.data(), B);
  float* dy = y ? d.out<float>(nx) : nullptr;
  std::vector<float> res((size_t)B * 4);
  LoudScratch S;
  loud_scratch_layout(B, N, dscr, &S);
  const Items it{dl, 1, 1, 1, N};
  if (d.ok()) {
    loud_measure_launch(nullptr, P, prm, S, dx, N, it, B);
    if (y) loud_apply_launch<float>(nullptr, S, dx, N, it, B, dy, N, N, 1.f);
  }
  d.finish();
  d.down(res.data(), S.res, res.size());
  if (y) d.down(y, dy, nx);
  if (!d.ok()) return d.rc();
  for (int b = 0; b < B; ++b) {
    if (loudness) loudness[b] = res[(size_t)b * 4 + 0];
    if (peak) peak[b] = res[(size_t)b * 4 + 1];
    if (gain) gain[b] = res[(size_t)b * 4 + 2];
  }
  return VITS_OK;
}

int vits_op_loudness(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, float* loudness, float* peak) {
  return loud_op(device, x, lengths, B, N, rate, LoudParams(), nullptr, loudness, peak, nullptr);
}

int vits_op_loudness_normalize(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate, int32_t mode, float target,
                               float ceiling, float* y, float* loudness, float* gain) {
  if (!y) return fail(VITS_ERR_ARG, "loudness: null output");
  LoudParams prm;
  TRY(loud_params(mode, target, ceiling, &prm));
  return loud_op(device, x, lengths, B, N, rate, prm, y, loudness, nullptr, gain);
}
