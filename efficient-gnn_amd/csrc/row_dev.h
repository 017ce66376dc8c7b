// row_dev.h -- a wave per row of (n, C) logits, C <= 256: lane l owns the columns l, l + 64, l + 128, l + 192.  The
// float64 row reductions that scale.hip (TS / VS / MS / ETS) and watstrain.hip (the WATS head's training epoch) share.
#pragma once

#include <climits>
#include <cmath>

#include <hip/hip_runtime.h>

namespace wg {
namespace {

constexpr int kRowMaxC = 256;       // four columns per lane
constexpr int kNQ = kRowMaxC / 64;

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);   // the same sum on every lane
  return v;
}
__device__ inline double wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// the first index of the row's maximum, a NaN ranking above every number (torch.max, np.argmax)
__device__ inline bool better(double a, int ia, double b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na != nb) return na;
  if (!na && a != b) return a > b;
  return ia < ib;
}
__device__ inline int wave_argmax(const double (&v)[kNQ], int C, int lane) {
  double bv = -INFINITY;
  int bi = INT_MAX;
#pragma unroll
  for (int q = 0; q < kNQ; ++q) {
    const int c = lane + 64 * q;
    if (c < C && better(v[q], c, bv, bi)) bv = v[q], bi = c;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (better(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  return bi;
}

// m and S = sum exp(v - m) over the row's columns; e[q] = exp(v[q] - m).  fmax drops a NaN, the sum brings it back.
__device__ inline void row_exp(const double (&v)[kNQ], int C, int lane, double (&e)[kNQ], double* m, double* S) {
  double mx = -INFINITY;
#pragma unroll
  for (int q = 0; q < kNQ; ++q)
    if (lane + 64 * q < C) mx = fmax(mx, v[q]);
  mx = wave_max(mx);
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < kNQ; ++q) {
    e[q] = lane + 64 * q < C ? exp(v[q] - mx) : 0.0;
    s += e[q];
  }
  *m = mx;
  *S = wave_sum(s);
}

__device__ inline void load_row(double (&z)[kNQ], const float* __restrict__ row, int C, int lane) {
#pragma unroll
  for (int q = 0; q < kNQ; ++q) z[q] = lane + 64 * q < C ? (double)row[lane + 64 * q] : 0.0;
}

}  // namespace
}  // namespace wg
