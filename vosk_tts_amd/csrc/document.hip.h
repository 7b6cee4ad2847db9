// document.hip.h -- documents (include/vits_document.h): the B finished items of one batch call joined into one piece of audio on the
// device.  Part of the ONE translation unit engine.hip (included there, behind contour.hip.h; not a standalone header).
//
// Three kernels, all on the call's stream, none of which the host waits for:
//   doc_edges_kernel   (trim only) the peak of every frame and, per strip of DOC_STRIP frames of an item, its first / last loud frame
//   doc_layout_kernel  one workgroup: lo / hi / n per item, the integer scan of n_b + gap_b, the block {F, start[B], lo[B], hi[B]}
//   doc_join_kernel    every workgroup owns DOC_TILE samples of the joined signal: segment samples (faded), zeros in the gaps
// The block's first int, F, is the `len_y` of every stage behind the join; the whole block goes to the host with the call's final
// copies, where the marks are filled from it (doc_results).  Buffers are sized by the untrimmed bound, which the host knows.
#pragma once
#include "../../include/vits_document.h"
#include "marks.hip.h"

#define DOC_STRIP 64      // frames per workgroup of doc_edges_kernel
#define DOC_TILE 4096     // samples per workgroup of doc_join_kernel: 4 rounds of 256 lanes x 4 samples
#define DOC_LDS_SEG 1024  // documents of up to this many segments keep their tables in LDS (12 KB); longer ones search them in global memory

// ---- the request ------------------------------------------------------------------------------------------------------------
struct DocReq {
  bool on = false;
  int B = 0, lead = 0, fade = 0, keep = 0;
  bool trim = false;
  float thr = 0.f;
  std::vector<int> gap;  // [B]
  std::vector<float> w;  // [fade]
  int64_t *out_seg_start = nullptr, *out_seg_end = nullptr, *token_ends = nullptr;
  int32_t* out_trim = nullptr;
  // set by doc_prepare, in front of the decoder
  long long bound = 0;  // frames: lead + sum(len_b + gap_b)
  int nstrips = 0;
  int *d_gap = nullptr, *d_blk = nullptr;
  int2* d_edge = nullptr;
  float* d_w = nullptr;
  size_t blk_ints() const { return 1 + 3 * (size_t)B; }
};

// Checked before anything is launched.  The size bound is tested here with every len_b at its least, 1, and again by doc_prepare with
// the frame counts themselves.
static int doc_req(const vits_document* doc, int B, int hop, DocReq* out) {
  *out = DocReq();
  if (!doc) return fail(VITS_ERR_ARG, "document: the vits_document pointer is NULL (include/vits_document.h)");
  if (B <= 0 || hop <= 0) return fail(VITS_ERR_ARG, "document: bad argument");
  if (doc->lead_frames < 0) return fail(VITS_ERR_ARG, "document: lead_frames %d is negative", doc->lead_frames);
  if (doc->fade_samples < 0 || doc->fade_samples > hop / 2)
    return fail(VITS_ERR_ARG, "document: fade_samples %d outside [0, hop/2 = %d]", doc->fade_samples, hop / 2);
  if (doc->trim_keep_frames < 0) return fail(VITS_ERR_ARG, "document: trim_keep_frames %d is negative", doc->trim_keep_frames);
  if (!(doc->trim_db <= 0.f) || !std::isfinite(doc->trim_db))
    return fail(VITS_ERR_ARG, "document: trim_db %g: 0 (off) or a negative finite dBFS value", (double)doc->trim_db);
  out->B = B; out->lead = doc->lead_frames; out->fade = doc->fade_samples; out->keep = std::min(doc->trim_keep_frames, 1 << 30);  // (no item has that many frames)
  out->trim = doc->trim_db != 0.f;
  if (out->trim) out->thr = (float)pow(10.0, (double)doc->trim_db / 20.0);
  out->gap.assign(B, 0);
  long long least = (long long)doc->lead_frames + B;
  for (int b = 0; b < B && doc->gap_frames; ++b) {
    if (doc->gap_frames[b] < 0) return fail(VITS_ERR_ARG, "document: gap_frames %d of segment %d is negative", doc->gap_frames[b], b);
    out->gap[b] = doc->gap_frames[b];
    least += doc->gap_frames[b];
  }
  if (least * hop >= (1LL << 31))
    return fail(VITS_ERR_ARG, "document: lead and gaps alone make %lld samples, beyond the limit of 2^31 - 1", least * hop);
  out->w.resize(out->fade);
  for (int j = 0; j < out->fade; ++j) out->w[j] = (float)(0.5 - 0.5 * cos(M_PI * (j + 0.5) / out->fade));
  out->out_seg_start = doc->out_seg_start; out->out_seg_end = doc->out_seg_end; out->out_trim = doc->out_trim;
  out->on = true;
  return VITS_OK;
}

// ---- the kernels ------------------------------------------------------------------------------------------------------------
// grid (nstrips, B), 256 threads: wave w of the workgroup takes frames w, w + 4, ... of its strip; its 64 lanes read the frame as
// consecutive float4 (vec) or floats, and reduce |x| with a fixed butterfly.  max is exact, so the order is only fixed, not needed.
// edge [B, nstrips]: {first, last} loud frame of the strip, {-1, -1} without one.
template <bool VEC>
__global__ void __launch_bounds__(256) doc_edges_kernel(const float* __restrict__ x, long long x_bstride, const int* __restrict__ len_frames,
                                                        int hop, float thr, int nstrips, int2* __restrict__ edge) {
  __shared__ int s_first[4], s_last[4];
  const int b = blockIdx.y, strip = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int len = len_frames[b];
  const int f_begin = strip * DOC_STRIP, f_end = min(f_begin + DOC_STRIP, len);
  int first = 0x7fffffff, last = -1;
  for (int f = f_begin + wave; f < f_end; f += 4) {
    const float* p = x + (long long)b * x_bstride + (long long)f * hop;
    float m = 0.f;
    if constexpr (VEC) {
      for (int i = lane * 4; i < hop; i += 256) {
        const float4 v = *reinterpret_cast<const float4*>(p + i);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
      }
    } else {
      for (int i = lane; i < hop; i += 64) m = fmaxf(m, fabsf(p[i]));
    }
    for (int off = 32; off; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (m > thr) {
      first = min(first, f);
      last = f;
    }
  }
  if (lane == 0) { s_first[wave] = first; s_last[wave] = last; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) { first = min(first, s_first[w]); last = max(last, s_last[w]); }
    edge[(long long)b * nstrips + strip] = make_int2(last < 0 ? -1 : first, last);
  }
}

// One workgroup of 256 threads; thread t owns the items [t * chunk, (t + 1) * chunk).  blk: {F, start[B], lo[B], hi[B]}.
template <bool TRIM>
__global__ void __launch_bounds__(256) doc_layout_kernel(const int* __restrict__ len_frames, const int* __restrict__ gap,
                                                         const int2* __restrict__ edge, int nstrips, int keep, int lead, int B,
                                                         int* __restrict__ blk) {
  __shared__ int s_sum[256];
  int *start = blk + 1, *lo = blk + 1 + B, *hi = blk + 1 + 2 * B;
  const int chunk = (B + 255) / 256;
  const int b0 = min((int)threadIdx.x * chunk, B), b1 = min(b0 + chunk, B);
  int sum = 0;
  for (int b = b0; b < b1; ++b) {
    const int len = len_frames[b];
    int l = 0, h = len;
    if constexpr (TRIM) {  // the strips in order
      int f0 = -1, f1 = -1;
      for (int s = 0; s * DOC_STRIP < len; ++s) {
        const int2 e = edge[(long long)b * nstrips + s];
        if (e.y >= 0) {
          if (f0 < 0) f0 = e.x;
          f1 = e.y;
        }
      }
      l = f1 < 0 ? 0 : max(f0 - keep, 0);
      h = f1 < 0 ? 0 : min(f1 + 1 + keep, len);
    }
    lo[b] = l;
    hi[b] = h;
    sum += h - l + gap[b];
  }
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = lead;
    for (int t = 0; t < 256; ++t) {
      const int v = s_sum[t];
      s_sum[t] = acc;
      acc += v;
    }
    blk[0] = acc;
  }
  __syncthreads();
  int at = s_sum[threadIdx.x];
  for (int b = b0; b < b1; ++b) {
    start[b] = at;
    at += hi[b] - lo[b] + gap[b];  // (this thread's own writes)
  }
}

template <typename T>
__device__ __forceinline__ T doc_out(float v, float scale) {
  if constexpr (sizeof(T) == sizeof(int16_t)) return pcm16_of(v, scale);
  else return v;
}

// The segment tables of one workgroup: LDS copies for documents of up to DOC_LDS_SEG segments, the device block itself beyond.
struct DocTab {
  const int *start, *lo, *hi;
  int B;
  // the largest b with start[b] <= frame, -1 when the frame lies in the lead.  Segments do not overlap and start is non-decreasing, so
  // that one is the only segment that can hold the frame (an empty segment in front of it shares its start and is passed over).
  __device__ __forceinline__ int find(int frame) const {
    int a = 0, n = B;
    while (n > 0) {
      const int h = n >> 1;
      if (start[a + h] <= frame) { a += h + 1; n -= h + 1; }
      else n = h;
    }
    return a - 1;
  }
  // one joined sample: x_b[lo_b*hop + i] * h(i) * t(i) inside segment b, i the offset in it, nh = n_b * hop
  __device__ __forceinline__ float fade(float v, long long i, long long nh, const float* __restrict__ w, int fade) const {
    if (i < fade) v = v * w[i];
    else if (i >= nh - fade) v = v * w[nh - 1 - i];
    return v;
  }
};

// grid cdiv(bound * hop, DOC_TILE), 256 threads.  vec: hop, x_bstride and both base addresses allow 16-byte accesses; every segment
// and gap then begins on a multiple of 4 samples, so a lane's 4 samples lie in one segment or in one gap.  Without vec every sample is
// placed on its own.  Nothing at or beyond F * hop is written.
template <typename T>
__global__ void __launch_bounds__(256) doc_join_kernel(const float* __restrict__ x, long long x_bstride, const int* __restrict__ blk, int B,
                                                       int hop, const float* __restrict__ w, int fade, int vec, float scale,
                                                       T* __restrict__ y) {
  __shared__ int s_tab[3 * DOC_LDS_SEG];
  const long long total = (long long)blk[0] * hop;
  const long long t0 = (long long)blockIdx.x * DOC_TILE;
  if (t0 >= total) return;  // (the whole workgroup)
  DocTab tab{blk + 1, blk + 1 + B, blk + 1 + 2 * B, B};
  if (B <= DOC_LDS_SEG) {
    for (int i = threadIdx.x; i < 3 * B; i += 256) s_tab[i] = blk[1 + i];
    __syncthreads();
    tab = DocTab{s_tab, s_tab + B, s_tab + 2 * B, B};
  }
  for (int r = 0; r < DOC_TILE / 1024; ++r) {
    const long long pos = t0 + r * 1024 + (long long)threadIdx.x * 4;
    if (pos >= total) break;
    if (vec) {
      const int b = tab.find((int)(pos / hop));
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (b >= 0) {
        const long long i = pos - (long long)tab.start[b] * hop, nh = (long long)(tab.hi[b] - tab.lo[b]) * hop;
        if (i < nh) {
          v = *reinterpret_cast<const float4*>(x + (long long)b * x_bstride + (long long)tab.lo[b] * hop + i);
          if (i < fade || i + 4 > nh - fade) {
            v.x = tab.fade(v.x, i, nh, w, fade);
            v.y = tab.fade(v.y, i + 1, nh, w, fade);
            v.z = tab.fade(v.z, i + 2, nh, w, fade);
            v.w = tab.fade(v.w, i + 3, nh, w, fade);
          }
        }
      }
      if constexpr (sizeof(T) == sizeof(int16_t)) {
        short4 o;
        o.x = doc_out<T>(v.x, scale); o.y = doc_out<T>(v.y, scale); o.z = doc_out<T>(v.z, scale); o.w = doc_out<T>(v.w, scale);
        *reinterpret_cast<short4*>(y + pos) = o;
      } else {
        *reinterpret_cast<float4*>(y + pos) = v;
      }
    } else {
      for (int k = 0; k < 4; ++k) {
        const long long p = pos + k;
        if (p >= total) break;
        const int b = tab.find((int)(p / hop));
        float v = 0.f;
        if (b >= 0) {
          const long long i = p - (long long)tab.start[b] * hop, nh = (long long)(tab.hi[b] - tab.lo[b]) * hop;
          if (i < nh) v = tab.fade(x[(long long)b * x_bstride + (long long)tab.lo[b] * hop + i], i, nh, w, fade);
        }
        y[p] = doc_out<T>(v, scale);
      }
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// The device side of a request, in front of the decoder (the uploads are of pageable memory): h_len [B] are the items' lengths in
// samples as the host has them after phase 1.  alloc as in tail_run.
template <typename Alloc>
static int doc_prepare(Alloc&& alloc, hipStream_t stream, DocReq& q, const long long* h_len, int hop) {
  long long bound = q.lead, mx = 1;
  for (int b = 0; b < q.B; ++b) {
    const long long f = h_len[b] / hop;
    if (f < 1) return fail(VITS_ERR_ARG, "document: segment %d has no frame", b);
    bound += f + q.gap[b];
    mx = std::max(mx, f);
  }
  if (bound * hop >= (1LL << 31))
    return fail(VITS_ERR_ARG, "document: %lld samples before trimming, beyond the limit of 2^31 - 1", bound * hop);
  q.bound = bound;
  q.nstrips = (int)((mx + DOC_STRIP - 1) / DOC_STRIP);
  q.d_gap = static_cast<int*>(alloc(sizeof(int) * (size_t)q.B));
  q.d_blk = static_cast<int*>(alloc(sizeof(int) * q.blk_ints()));
  q.d_w = q.fade ? static_cast<float*>(alloc(sizeof(float) * (size_t)q.fade)) : nullptr;
  q.d_edge = q.trim ? static_cast<int2*>(alloc(sizeof(int2) * (size_t)q.B * q.nstrips)) : nullptr;
  if (!q.d_gap || !q.d_blk || (q.fade && !q.d_w) || (q.trim && !q.d_edge)) return fail(VITS_ERR_NOMEM, "device alloc failed");
  HIP_TRY(hipMemcpyAsync(q.d_gap, q.gap.data(), sizeof(int) * (size_t)q.B, hipMemcpyHostToDevice, stream));
  if (q.fade) HIP_TRY(hipMemcpyAsync(q.d_w, q.w.data(), sizeof(float) * (size_t)q.fade, hipMemcpyHostToDevice, stream));
  return VITS_OK;
}

// (a door has no session to count its launches under)
struct DocProf {
  std::optional<ProfScope> p;
  DocProf(vits_session* s, const char* name, const char* kernel) { if (s) p.emplace(s, name, 0, kernel); }
};

// The three launches, behind doc_prepare: x [B, x_bstride] with len_frames [B] on the device -> y [q.bound * hop] (float, or int16
// where pcm), of which [0, F * hop) are written.
static void doc_join_launch(vits_session* s, hipStream_t stream, const float* x, long long x_bstride, const int* len_frames, int hop, const DocReq& q,
                            void* y, bool pcm, float pcm_scale) {
  const int vec = hop % 4 == 0 && x_bstride % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0;
  if (q.trim) {
    DocProf ps(s, "doc.edges", "doc_edges_kernel");
    if (vec) hipLaunchKernelGGL(doc_edges_kernel<true>, dim3(q.nstrips, q.B), dim3(256), 0, stream, x, x_bstride, len_frames, hop, q.thr, q.nstrips, q.d_edge);
    else hipLaunchKernelGGL(doc_edges_kernel<false>, dim3(q.nstrips, q.B), dim3(256), 0, stream, x, x_bstride, len_frames, hop, q.thr, q.nstrips, q.d_edge);
  }
  {
    DocProf ps(s, "doc.layout", "doc_layout_kernel");
    if (q.trim)
      hipLaunchKernelGGL(doc_layout_kernel<true>, dim3(1), dim3(256), 0, stream, len_frames, (const int*)q.d_gap, (const int2*)q.d_edge, q.nstrips, q.keep,
                         q.lead, q.B, q.d_blk);
    else
      hipLaunchKernelGGL(doc_layout_kernel<false>, dim3(1), dim3(256), 0, stream, len_frames, (const int*)q.d_gap, (const int2*)q.d_edge, q.nstrips, q.keep,
                         q.lead, q.B, q.d_blk);
  }
  const long long n = q.bound * hop;
  if (n <= 0) return;
  const unsigned grid = (unsigned)((n + DOC_TILE - 1) / DOC_TILE);
  DocProf ps(s, "doc.join", pcm ? "doc_join_kernel<int16>" : "doc_join_kernel<float>");
  if (pcm)
    hipLaunchKernelGGL(doc_join_kernel<int16_t>, dim3(grid), dim3(256), 0, stream, x, x_bstride, (const int*)q.d_blk, q.B, hop, (const float*)q.d_w, q.fade,
                       vec, pcm_scale, static_cast<int16_t*>(y));
  else
    hipLaunchKernelGGL(doc_join_kernel<float>, dim3(grid), dim3(256), 0, stream, x, x_bstride, (const int*)q.d_blk, q.B, hop, (const float*)q.d_w, q.fade,
                       vec, 1.f, static_cast<float*>(y));
}

// ---- the parity door ---------------------------------------------------------------------------------------------------------
// The join on host buffers (the door, and the multistream family's tail, which crosses the host through the doors' kernels): x [B, N],
// len_frames [B] -> y[0 .. F * hop) of capacity y_cap, *blk = {F, start[B], lo[B], hi[B]}.  What the kernel does not write comes back
// as it went.
static int doc_op(int device, const float* x, const int64_t* len_frames, int32_t B, int64_t N, int32_t hop, DocReq& q, float* y, int64_t y_cap,
                  std::vector<int>* blk) {
  std::vector<int> len32(B);
  std::vector<long long> h_len(B);
  for (int b = 0; b < B; ++b) {
    if (len_frames[b] < 1 || len_frames[b] * hop > N)
      return fail(VITS_ERR_ARG, "document join: %lld frames of segment %d outside [1, N / hop = %lld]", (long long)len_frames[b], b, (long long)(N / hop));
    len32[b] = (int)len_frames[b];
    h_len[b] = len_frames[b] * hop;
  }
  OpDoor d("document join", device);
  if (d.ok()) d.code = doc_prepare(d.bufs, nullptr, q, h_len.data(), hop);
  if (d.ok() && q.bound * hop > y_cap)
    return fail(VITS_ERR_ARG, "document join: the untrimmed bound of %lld samples exceeds y_cap %lld", q.bound * hop, (long long)y_cap);
  const size_t ny = d.ok() ? (size_t)(q.bound * hop) : 0;
  float* dx = d.up(x, (size_t)B * N);
  int* dl = d.up(len32.data(), B);
  float* dy = d.up(y, ny);
  if (d.ok()) doc_join_launch(nullptr, nullptr, dx, N, dl, hop, q, dy, false, 1.f);
  d.finish();
  blk->assign(q.blk_ints(), 0);
  d.down(blk->data(), q.d_blk, blk->size());
  d.down(y, dy, ny);
  return d.rc();
}

int vits_op_document_join(int device, const float* x, const int64_t* len_frames, int32_t B, int64_t N, int32_t hop, const vits_document* doc, float* y,
                          int64_t y_cap, int64_t* out_frames, int32_t* start, int32_t* trim) {
  if (!x || !len_frames || !y || !out_frames || B <= 0 || B > 65535 || N <= 0 || N >= (1LL << 31) || hop <= 0 || y_cap < 0)
    return fail(VITS_ERR_ARG, "document join: bad argument");
  DocReq q;
  TRY(doc_req(doc, B, hop, &q));
  std::vector<int> blk;
  TRY(doc_op(device, x, len_frames, B, N, hop, q, y, y_cap, &blk));
  *out_frames = blk[0];
  for (int b = 0; b < B; ++b) {
    if (start) start[b] = blk[1 + b];
    if (trim) { trim[2 * b] = blk[1 + B + b]; trim[2 * b + 1] = blk[1 + 2 * B + b]; }
  }
  return VITS_OK;
}

// What the host fills once the block {F, start, lo, hi} is back: the segment marks, the trims and the token ends (cum [B, cum_bstride]
// on the host, read only where token ends are asked for).  Returns the document's length in output samples.
static int64_t doc_results(const DocReq& q, const int* blk, const int* cum, long long cum_bstride, const int64_t* lengths, int Tx, int hop, long long L,
                           long long M) {
  const int B = q.B;
  const int *start = blk + 1, *lo = blk + 1 + B, *hi = blk + 1 + 2 * B;
  for (int b = 0; b < B; ++b) {
    const int n = hi[b] - lo[b];
    if (q.out_seg_start) q.out_seg_start[b] = marks_end(start[b], hop, L, M);
    if (q.out_seg_end) q.out_seg_end[b] = marks_end(start[b] + n, hop, L, M);
    if (q.out_trim) { q.out_trim[2 * b] = lo[b]; q.out_trim[2 * b + 1] = hi[b]; }
    if (!q.token_ends) continue;
    long long len = lengths[b] > Tx ? Tx : lengths[b];
    for (int t = 0; t < Tx; ++t) {
      int64_t e = 0;
      if (len > 0) {
        const int c = cum[(size_t)b * cum_bstride + (t < len ? t : len - 1)] - lo[b];
        e = marks_end(start[b] + std::min(std::max(c, 0), n), hop, L, M);
      }
      q.token_ends[(size_t)b * Tx + t] = e;
    }
  }
  return marks_end(blk[0], hop, L, M);
}
