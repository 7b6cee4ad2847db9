// prosody.hip.h -- the controlled length regulator (include/vits_prosody.h): durations_kernel plus per-item length scales, per-token
// rates, pauses and the fit to a frame count.  Part of the ONE translation unit engine.hip (included there behind kernels_misc.hip.h;
// not a standalone header).  An uncontrolled call never launches this kernel: it runs durations_kernel as before.
#pragma once

// The controls of one call on the device; every array is nullable but `ratio`.
struct RegCtl {
  const float* item_scales;  // [B, 3]: ls_b = item_scales[b, 1] replaces length_scale
  const float* tls;          // [B, T]: token_length_scale (the launcher passes null with forced durations)
  const int* pause;          // [B, T] frames
  const int* fit;            // [B]: F_b, 0 = not fitted
  float* ratio;              // out: s [B], and behind it int [B]: 1 where the fit of item b was refused (error bit REG_ERR_FIT)
};
#define REG_ERR_FIT 16  // bit in the session error word: a fit was refused (F_b <= P, U == 0 or s outside [0.25, 4])

// One workgroup per item, as durations_kernel; thread `tid` owns the tokens [tid * per, (tid + 1) * per), per = ceil(T / 256).
// Pass 1 sums u (double), the pauses and the unfitted frames of the thread's run; one serial scan of the 256 partials through LDS gives
// every thread its three exclusive prefixes, U, P and with them s; pass 2 recomputes the run's tokens (the same instructions on the same
// inputs: the same bits) and carries both scans -- the double prefix of u behind c_t and the integer prefix behind cum -- in registers.
// Writes dur, cum, ylen32 / ylen64 and ratio.  A refused fit raises REG_ERR_FIT and leaves the unfitted durations, so everything
// downstream of a call that is about to fail stays in bounds.
__global__ void __launch_bounds__(256) regulate_ctl_kernel(const float* logw, const int* forced, const int* len, float length_scale, int T,
                                                           int* dur, int* cum, int* ylen32, int64_t* ylen64, int Tcap, int* err,
                                                           const SynthDev* dv, const float* ea_z, int ea_row, const float* ea_m,
                                                           const float* ea_logs, RegCtl c) {
  __shared__ double part_u[256];
  __shared__ int part_d[256], part_p[256];
  __shared__ double sh_s;
  __shared__ int sh_fit;
  const int b = blockIdx.x, tid = threadIdx.x, B = gridDim.x;
  if (dv) length_scale = dv->scales[1];
  if (c.item_scales) length_scale = c.item_scales[(long long)b * 3 + 1];
  const float ea_mu = ea_z ? ea_m[0] : 0.f, ea_sc = ea_z ? expf(-ea_logs[0]) : 0.f;
  const int L = len[b];
  const int per = (T + 255) / 256;
  const int t0 = tid * per;
  // d0_t, u_t and pause_t of token t < L
  auto token = [&](int t, double* u, int* p) -> int {
    const long long o = (long long)b * T + t;
    *p = c.pause ? c.pause[o] : 0;
    if (forced) {
      int d = forced[o];
      if (d < 0) d = 0;
      *u = (double)d;
      return d;
    }
    const float lw = ea_z ? (ea_z[((long long)b * 2 + ea_row) * T + t] - ea_mu) * ea_sc : logw[o];
    float w = expf(lw) * length_scale;
    if (c.tls) w = w * c.tls[o];
    *u = (double)w;
    const int d = (int)ceilf(w);
    return d < 0 ? 0 : d;
  };
  double su = 0.0;
  int sd = 0, sp = 0;
  for (int t = t0; t < t0 + per && t < T && t < L; ++t) {
    double u; int p;
    const int d0 = token(t, &u, &p);
    su += u; sp += p; sd += d0 + p;
  }
  part_u[tid] = su; part_d[tid] = sd; part_p[tid] = sp;
  __syncthreads();
  if (tid == 0) {
    double U = 0.0;
    int D = 0, P = 0;
    for (int i = 0; i < 256; ++i) {
      const double vu = part_u[i]; part_u[i] = U; U += vu;
      const int vd = part_d[i]; part_d[i] = D; D += vd;
      const int vp = part_p[i]; part_p[i] = P; P += vp;
    }
    const int F = c.fit ? c.fit[b] : 0;
    int fit = F > 0;
    double s = 1.0;
    int bad = 0;
    if (fit) {
      s = ((double)F - (double)P) / U;
      bad = !(F > P) || !(U > 0.0) || !(s >= 0.25 && s <= 4.0);
      if (bad) { atomicOr(err, REG_ERR_FIT); fit = 0; }
    }
    c.ratio[b] = (float)s;
    reinterpret_cast<int*>(c.ratio)[B + b] = bad;
    int yl = fit ? F : D;
    if (yl < 1) yl = 1;
    if (Tcap > 0 && yl > Tcap) { atomicOr(err, 4); yl = Tcap; }
    ylen32[b] = yl;
    if (ylen64) ylen64[b] = yl;
    sh_s = s; sh_fit = fit;
  }
  __syncthreads();
  const bool fit = sh_fit != 0;
  const double s = sh_s;
  double run_u = part_u[tid];
  int run = fit ? part_p[tid] : part_d[tid];  // frames in front of the run that the fit does not place: pauses, or everything
  long long c_prev = fit ? (long long)rint(s * run_u) : 0;
  for (int t = t0; t < t0 + per && t < T; ++t) {
    int d = 0;
    if (t < L) {
      double u; int p;
      const int d0 = token(t, &u, &p);
      if (fit) {
        run_u += u;
        const long long ct = (long long)rint(s * run_u);
        d = (int)(ct - c_prev) + p;
        c_prev = ct;
        run += p;
      } else {
        d = d0 + p;
        run += d;
      }
    }
    dur[(long long)b * T + t] = d;
    cum[(long long)b * T + t] = (fit ? (int)c_prev : 0) + run;
  }
}
