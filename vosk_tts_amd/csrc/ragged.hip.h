// ragged.hip.h -- the object every output-tail stage works on: a padded batch [B, stride] of float audio whose item b holds a number of
// valid samples derived from a device array of counts.  Part of the ONE translation unit engine.hip (included there, ahead of
// resample.hip.h).  The length rule is stated here once; kernels take an Items by value (32 bytes) and the launch functions pass it on.
// A stage in front of the resampler (denoise, pitch, the resampler itself) reads len_in and never pays len_out's 64-bit division; a
// stage behind it (watermark, loudness, limit) reads len_out, and `cap` is also the N of its [B, N] scratch rows.  The window a stream
// slot holds of an item (x_off / x_n of resample and denoise) describes the buffer, not the items: it is not part of this.
#pragma once

// samples at the rate L / M (lowest terms) of x samples at the native rate: the one rounding rule of the resampler, the marks and the lengths
__host__ __device__ __forceinline__ long long n_out(long long x, long long L, long long M) { return (x * L + M - 1) / M; }

struct Items {
  const int* units = nullptr;  // device, [B]; null: every item has `mul` samples
  long long mul = 0;           // samples per unit (hop), or the length itself
  int L = 1, M = 1;            // output rate / native rate in lowest terms
  long long cap = 0;           // samples an item can have as returned (N); the clamp of len_out
  __host__ __device__ __forceinline__ long long len_in(int b) const { return units ? units[b] * mul : mul; }  // the item at the vocoder's rate
  // the item as it is returned: len_in taken to the rate L / M, at most cap
  __host__ __device__ __forceinline__ long long len_out(int b) const {
    const long long l = n_out(len_in(b), L, M);
    return l < 0 ? 0 : (l > cap ? cap : l);
  }
  Items from(int b0) const { return Items{units ? units + b0 : nullptr, mul, L, M, cap}; }  // the same batch from item b0 on (group launches)
};
