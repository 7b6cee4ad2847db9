// resample.hip.h -- synthesis at the caller's sample rate (include/vits_resample.h): the polyphase windowed-sinc resampler behind the
// decoder.  Part of the ONE translation unit engine.hip (included there, after the session / launch helpers).
//
// Geometry (host, exact integer arithmetic): output n of an item has phase p = (n*M) mod L and position q = floor(n*M / L) and is
//     y[n] = sum_i table[p][i] * x[q - lo(p) + i],   lo(p) = (W - p) / L,   W = 16 * max(L, M)
// Access pattern: consecutive outputs step through the phases in the order p = (r*M) mod L, r = n mod L -- a bijection, as
// gcd(L, M) = 1 -- so a lane per output reading row p would stride through the table.  The device copy of the table is therefore
// stored by r and transposed, dev[i][r] = table[(r*M) mod L][i]: tap i of 64 consecutive outputs is 64 consecutive floats (wrapping at
// L).  The input span of a workgroup's VITS_RESAMPLE_TILE outputs is staged once in LDS, zero outside the item's own [0, len).
#pragma once
#include "../../include/vits_resample.h"

#define RS_Z 16
#define RS_RHO 0.9
#define RS_BETA 10.0
// LDS floats of one workgroup: (TILE - 1) * M / L + 1 positions + 2 * ceil(Hw) reach + 1, at M / L <= 4 and ceil(Hw) <= 64
#define RS_SPAN_MAX ((VITS_RESAMPLE_TILE - 1) * 4 + 2 * 4 * RS_Z + 4)

struct ResamplePlan {
  int rate_in = 0, rate_out = 0;
  int L = 1, M = 1, taps = 1, half = 0;
  long long W = 0;  // Hw = W / L
  int span = 0;     // LDS floats one workgroup stages
  long long n_out(long long len) const { return ::n_out(len, L, M); }
};

static int resample_plan(int rate_in, int rate_out, ResamplePlan* out) {
  if (rate_in <= 0 || rate_out <= 0) return fail(VITS_ERR_UNSUPPORTED, "resample: rates must be positive (rate_in %d, rate_out %d)", rate_in, rate_out);
  if ((long long)rate_out * 4 < rate_in || rate_out > (long long)rate_in * 4)
    return fail(VITS_ERR_UNSUPPORTED, "resample: rate_out %d outside [rate_in / 4, 4 * rate_in] of rate_in %d", rate_out, rate_in);
  int a = rate_in, b = rate_out;
  while (b) { const int t = a % b; a = b; b = t; }
  ResamplePlan P;
  P.rate_in = rate_in; P.rate_out = rate_out;
  P.L = rate_out / a; P.M = rate_in / a;
  P.W = (long long)RS_Z * (P.L > P.M ? P.L : P.M);
  // lo(p) + hi(p) + 1 over the phases; (W - p) / L and (W + p) / L only change where p crosses a residue of W, so the scan is cheap
  // enough to do in full for every L that can pass the table limit (taps >= 2 Z + 1 bounds L below 2000)
  if ((long long)P.L * (2 * RS_Z + 1) > VITS_RESAMPLE_MAX_TABLE)
    return fail(VITS_ERR_UNSUPPORTED, "resample: %d -> %d Hz needs %d phases: the phase table would exceed %d floats", rate_in, rate_out, P.L, VITS_RESAMPLE_MAX_TABLE);
  int taps = 0;
  for (int p = 0; p < P.L; ++p) {
    const int t = (int)((P.W - p) / P.L + (P.W + p) / P.L + 1);
    if (t > taps) taps = t;
  }
  P.taps = taps;
  P.half = (int)((P.W + P.L - 1) / P.L);
  if ((long long)P.L * taps > VITS_RESAMPLE_MAX_TABLE)
    return fail(VITS_ERR_UNSUPPORTED, "resample: %d -> %d Hz needs a phase table of %d x %d floats (limit %d)", rate_in, rate_out, P.L, taps, VITS_RESAMPLE_MAX_TABLE);
  P.span = (int)(((long long)(VITS_RESAMPLE_TILE - 1) * P.M + P.L - 1) / P.L) + 2 * P.half + 2;
  if (P.span > RS_SPAN_MAX) return fail(VITS_ERR_UNSUPPORTED, "resample: %d -> %d Hz: input span %d of one tile exceeds %d", rate_in, rate_out, P.span, RS_SPAN_MAX);
  *out = P;
  return VITS_OK;
}

// I0 by its power series: every term is positive, so the sum is good to a few ulp for the arguments used here (<= beta)
static double rs_bessel_i0(double x) {
  const double q = x * x / 4;
  double term = 1, sum = 1;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * k);
    sum += term;
    if (term < sum * 1e-18) break;
  }
  return sum;
}

// h at t = num / L.  The window's argument is formed from integers: 1 - (t / Hw)^2 = (W - num)(W + num) / W^2.
static double rs_tap(const ResamplePlan& P, long long num) {
  if (num > P.W || num < -P.W) return 0.0;
  const double s = P.L < P.M ? (double)P.L / (double)P.M : 1.0;
  const double c = RS_RHO * s;
  const double t = (double)num / (double)P.L;
  const double v = c * t;
  const double pv = M_PI * v;
  const double sinc = num == 0 ? 1.0 : sin(pv) / pv;
  const double r2 = (double)((P.W - num) * (P.W + num)) / (double)(P.W * P.W);
  return c * sinc * rs_bessel_i0(RS_BETA * sqrt(r2)) / rs_bessel_i0(RS_BETA);
}

static void resample_fill(const ResamplePlan& P, float* table) {
  for (int p = 0; p < P.L; ++p) {
    const long long lo = (P.W - p) / P.L;
    for (int i = 0; i < P.taps; ++i) table[(size_t)p * P.taps + i] = (float)rs_tap(P, (lo - i) * P.L + p);
  }
}

// ---- the kernel -----------------------------------------------------------------------------------------------------
// One workgroup = VITS_RESAMPLE_TILE consecutive outputs [n0, n0 + TILE) of item blockIdx.y, one per thread.
//   x        item b's input at x + b * x_bstride; x[j] is input sample x_off + j, and only 0 <= j < x_n is ever read
//   len      valid input samples of item b: it.len_in(b) (ragged.hip.h); samples >= len count as 0
//   tab      the device table [taps][L] described at the top
//   y        item b's output at y + b * y_bstride; y[j] is output n_begin + j, written for 0 <= j < n_count
//            (exactly 0 for outputs at and beyond ceil(len * L / M))
// OUT = int16_t: pcm16_of; dv (nullable) carries the per-call scale.
// CROP (the pitch stage, include/vits_pitch.h): item b's outputs at and beyond crop[b] are 0 as well; without it crop is not read.
template <typename OUT, bool CROP = false>
__global__ __launch_bounds__(VITS_RESAMPLE_TILE) void resample_kernel(const float* __restrict__ x, long long x_bstride, long long x_off,
                                                                      long long x_n, const Items it, const float* __restrict__ tab, int L, int M,
                                                                      int taps, int half, long long W, OUT* __restrict__ y, long long y_bstride,
                                                                      long long n_begin, long long n_count, float scale, const SynthDev* dv,
                                                                      const int* __restrict__ crop) {
  __shared__ float xs[RS_SPAN_MAX];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long len = it.len_in(b);
  const long long n0 = n_begin + (long long)blockIdx.x * VITS_RESAMPLE_TILE;
  const long long nm0 = n0 * M;  // 64-bit: n * M passes 2^31 within minutes of audio
  const long long q0 = nm0 / L;
  const int p0 = (int)(nm0 - q0 * L), r0 = (int)(n0 % L);
  // positions of this tile: q0 .. q0 + (p0 + (TILE - 1) * M) / L; reaches of at most `half` either side
  const long long k_lo = q0 - half;
  int span = (int)((p0 + (long long)(VITS_RESAMPLE_TILE - 1) * M) / L) + 2 * half + 2;
  if (span > RS_SPAN_MAX) span = RS_SPAN_MAX;  // (never: resample_plan refuses such a geometry)
  const float* xb = x + (long long)b * x_bstride;
  for (int j = tid; j < span; j += VITS_RESAMPLE_TILE) {
    const long long k = k_lo + j, kk = k - x_off;
    xs[j] = (k >= 0 && k < len && kk >= 0 && kk < x_n) ? xb[kk] : 0.f;
  }
  __syncthreads();
  const long long j_out = (long long)blockIdx.x * VITS_RESAMPLE_TILE + tid;
  if (j_out >= n_count) return;
  const long long n = n0 + tid;
  float acc = 0.f;
  long long n_end = n_out(len, L, M);
  if constexpr (CROP) n_end = n_end < crop[b] ? n_end : crop[b];
  if (n < n_end) {
    const int v = p0 + tid * M;  // < L + 255 * M: 32-bit
    const int dq = v / L, p = v - dq * L;
    int r = r0 + tid;
    r -= (r / L) * L;
    const int lo = (int)((W - p) / L), hi = (int)((W + p) / L);
    const int base = dq + half - lo;  // index in xs of x[q - lo]; the last one read is dq + half + hi <= span - 2
    int nt = lo + hi + 1;             // this phase's own taps (<= taps; the rest of its row is 0)
    if (nt > taps) nt = taps;
    if (base + nt > RS_SPAN_MAX) nt = RS_SPAN_MAX - base;  // (never, as above)
    const float* tr = tab + r;
    for (int i = 0; i < nt; ++i) acc = fmaf(tr[(long long)i * L], xs[base + i], acc);
  }
  if constexpr (sizeof(OUT) == sizeof(int16_t)) {
    if (dv) scale = dv->pcm_scale;
    y[(long long)b * y_bstride + j_out] = pcm16_of(acc, scale);
  } else {
    y[(long long)b * y_bstride + j_out] = acc;
  }
}

// ---- device tables, cached per (device, rate_in, rate_out) ------------------------------------------------------------
struct ResampleTab { ResamplePlan P; float* d = nullptr; };
static DevTabs<std::tuple<int, int, int>, ResampleTab> g_rs_tabs;
#define RS_MAX_TABS 64  // per process: captured graphs hold the pointers, so entries are never evicted
// L / M of the rate T returns at (null: the native rate, 1 / 1), and the items of a call returned at it
struct Rate { int L, M; };
static Rate rate_of(const ResampleTab* T) { return T ? Rate{T->P.L, T->P.M} : Rate{1, 1}; }
static Items items_at(const ResampleTab* T, const int* units, long long mul, long long cap) { return Items{units, mul, rate_of(T).L, rate_of(T).M, cap}; }

// the device copy of T.P's table (hipMalloc + a synchronous copy)
static int resample_upload(int device, ResampleTab& T) {
  const ResamplePlan& P = T.P;
  std::vector<float> tab((size_t)P.L * P.taps), dev((size_t)P.L * P.taps);
  resample_fill(P, tab.data());
  for (int r = 0; r < P.L; ++r) {
    const int p = (int)(((long long)r * P.M) % P.L);
    for (int i = 0; i < P.taps; ++i) dev[(size_t)i * P.L + r] = tab[(size_t)p * P.taps + i];
  }
  return dev_table_upload(device, "resample", dev.data(), dev.size() * sizeof(float), (void**)&T.d);
}

// Uploads on first use (call it outside stream capture).
static int resample_get(int device, int rate_in, int rate_out, const ResampleTab** out) {
  return g_rs_tabs.get(std::make_tuple(device, rate_in, rate_out), out, [&](ResampleTab& T) {
    TRY(resample_plan(rate_in, rate_out, &T.P));
    if (g_rs_tabs.size() >= RS_MAX_TABS) return fail(VITS_ERR_UNSUPPORTED, "resample: more than %d distinct rate pairs in one process", RS_MAX_TABS);
    return resample_upload(device, T);
  });
}

// Outputs [n_begin, n_begin + n_count) of B items on `stream` (capturable: no allocation, no synchronisation).
template <typename OUT>
static void resample_launch(hipStream_t stream, const ResampleTab& T, const float* x, long long x_bstride, long long x_off, long long x_n,
                            const Items& it, int B, OUT* y, long long y_bstride, long long n_begin, long long n_count, float scale,
                            const SynthDev* dv) {
  if (n_count <= 0 || B <= 0) return;
  const ResamplePlan& P = T.P;
  const unsigned gx = (unsigned)((n_count + VITS_RESAMPLE_TILE - 1) / VITS_RESAMPLE_TILE);
  hipLaunchKernelGGL(resample_kernel<OUT>, dim3(gx, B), dim3(VITS_RESAMPLE_TILE), 0, stream, x, x_bstride, x_off, x_n, it, T.d, P.L, P.M, P.taps,
                     P.half, P.W, y, y_bstride, n_begin, n_count, scale, dv, nullptr);
}

// The form of the pitch stage (include/vits_pitch.h): float outputs [0, n_count) of B items whose input lengths are it.len_in(b) and
// whose outputs at and beyond crop[b] are 0 (a device array).
static void resample_launch_crop(hipStream_t stream, const ResampleTab& T, const float* x, long long x_bstride, long long x_n, const Items& it,
                                 const int* crop, int B, float* y, long long y_bstride, long long n_count) {
  if (n_count <= 0 || B <= 0) return;
  const ResamplePlan& P = T.P;
  const unsigned gx = (unsigned)((n_count + VITS_RESAMPLE_TILE - 1) / VITS_RESAMPLE_TILE);
  hipLaunchKernelGGL((resample_kernel<float, true>), dim3(gx, B), dim3(VITS_RESAMPLE_TILE), 0, stream, x, x_bstride, 0LL, x_n, it, T.d, P.L, P.M,
                     P.taps, P.half, P.W, y, y_bstride, 0LL, n_count, 1.f, (const SynthDev*)nullptr, crop);
}

// 0 / the native rate -> 0 (the entry point's own path); anything else must have a plan
static int resample_rate_arg(const vits_model* m, int32_t sample_rate, int* rate) {
  *rate = 0;
  if (sample_rate == 0 || sample_rate == m->hp.sampling_rate) return VITS_OK;
  ResamplePlan P;
  TRY(resample_plan(m->hp.sampling_rate, sample_rate, &P));
  *rate = sample_rate;
  return VITS_OK;
}

// ---- host-only entry points and the kernel-level parity door -------------------------------------------------------------
int vits_resample_plan(int32_t rate_in, int32_t rate_out, int32_t* L, int32_t* M, int32_t* taps, int32_t* half_width_in) {
  ResamplePlan P;
  TRY(resample_plan(rate_in, rate_out, &P));
  if (L) *L = P.L;
  if (M) *M = P.M;
  if (taps) *taps = P.taps;
  if (half_width_in) *half_width_in = P.half;
  return VITS_OK;
}

int vits_resample_table(int32_t rate_in, int32_t rate_out, float* table, int64_t cap) {
  if (!table) return fail(VITS_ERR_ARG, "resample: null table");
  ResamplePlan P;
  TRY(resample_plan(rate_in, rate_out, &P));
  if (cap < (int64_t)P.L * P.taps) return fail(VITS_ERR_ARG, "resample: table capacity %lld < %d x %d floats", (long long)cap, P.L, P.taps);
  resample_fill(P, table);
  return VITS_OK;
}

int vits_op_resample(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, int32_t rate_in, int32_t rate_out, float* y) {
  if (!y) return fail(VITS_ERR_ARG, "resample: bad argument");
  std::vector<int> len32;
  TRY(op_items_check("resample", x, lengths, B, N, &len32));
  if (rate_in > 0 && rate_in == rate_out) {  // the identity (zeros beyond each item's end, like every other rate)
    for (int b = 0; b < B; ++b) {
      memcpy(y + (size_t)b * N, x + (size_t)b * N, sizeof(float) * (size_t)lengths[b]);
      memset(y + (size_t)b * N + lengths[b], 0, sizeof(float) * (size_t)(N - lengths[b]));
    }
    return VITS_OK;
  }
  ResamplePlan P;
  TRY(resample_plan(rate_in, rate_out, &P));
  const ResampleTab* T = nullptr;
  TRY(resample_get(device, rate_in, rate_out, &T));
  OpDoor d("resample", device);
  const size_t Ny = (size_t)P.n_out(N);
  float* dx = d.up(x, (size_t)B * N);
  int* dl = d.up(len32.data(), B);
  float* dy = d.out<float>(B * Ny);
  if (d.ok()) resample_launch<float>(nullptr, *T, dx, N, 0, N, Items{dl, 1}, B, dy, Ny, 0, Ny, 1.f, nullptr);
  d.finish();
  d.down(y, dy, B * Ny);
  return d.rc();
}
