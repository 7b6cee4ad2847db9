// marks.hip.h -- speech marks (include/vits_marks.h): the end of every token on the output time axis, from the cumulative frame counts
// the length regulator already left behind.  Part of the ONE translation unit engine.hip (included there, after resample.hip.h).
//
// Nothing is predicted here: frame f belongs to token j with cum[j-1] <= f < cum[j], so token t ends at output sample
// n_out(cum[t] * hop), n_out(x) = ceil(x * L / M) being the resampler's length rule (the identity at L = M = 1).  The rule is stated
// once, in ragged.hip.h; marks_end applies it in the kernel of the graph-replayed path and in the host function of the paths that have
// the counts on the host anyway (the eager VITS path, streams, every multistream call).
#pragma once
#include "../../include/vits_marks.h"

__host__ __device__ static inline long long marks_end(long long cum, long long hop, long long L, long long M) {
  return n_out(cum * hop, L, M);
}

// Host: token_ends[t] for the T tokens of one item from its inclusive cumulative frame counts; entries at and beyond `len` repeat the
// last valid one (0 when len == 0).
static void marks_fill_host(const int* cum, long long len, int T, int hop, long long L, long long M, int64_t* token_ends) {
  if (len > T) len = T;
  for (int t = 0; t < T; ++t) token_ends[t] = len <= 0 ? 0 : marks_end(cum[t < len ? t : len - 1], hop, L, M);
}

// ---- the kernel -----------------------------------------------------------------------------------------------------
// One thread per token, blockIdx.y = item.  cum is the plain int32 [B, T] that durations_kernel writes -- and that the persistent
// front program's PK_DUR step writes as well, next to its {value, epoch} cells (persist.hip.h: the launch-path back phase reads the
// plain array too), so both fronts are read in one form and no epoch has to be known here.  len: int32 [B], the items' token counts.
// L / M come by value, or from the per-call block when dv is given (graph replay: a graph depends on shapes only).
__global__ void __launch_bounds__(256) token_ends_kernel(const int* __restrict__ cum, const int* __restrict__ len, int T, int hop, long long L,
                                                         long long M, const SynthDev* __restrict__ dv, long long* __restrict__ token_ends) {
  const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (t >= T) return;
  if (dv) { L = dv->rate_L; M = dv->rate_M; }
  int n = len[b];
  if (n > T) n = T;
  long long e = 0;
  if (n > 0) e = marks_end(cum[(long long)b * T + (t < n ? t : n - 1)], hop, L, M);
  token_ends[(long long)b * T + t] = e;
}

static void token_ends_launch(vits_session* s, const int* cum, const int* len, int B, int T, int hop, long long L, long long M, const SynthDev* dv,
                              long long* token_ends) {
  ProfScope ps(s, "marks.token_ends", 0, "token_ends_kernel");
  hipLaunchKernelGGL(token_ends_kernel, dim3(cdiv(T, 256), B), dim3(256), 0, s->stream, cum, len, T, hop, L, M, dv, token_ends);
}
