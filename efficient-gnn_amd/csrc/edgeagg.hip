// edgeagg.hip -- the weighted propagation of the DCGC calibrator (reference calibration/DCGC.py:62-63, :147-148 on
// src/gnn/model.py:43-52): the base model runs on an adjacency whose values are the edge MLP's output, new in every
// epoch.  The pattern is fixed, so the values are an argument instead of part of a planned operator:
//
//     out[i][c] = row_scale[i] * sum over p in [indptr[i], indptr[i + 1]) of
//                     val[map ? map[p] : p] * col_scale[j_p] * x[j_p][c]          j_p = indices[p]
//
// (either scale NULL = 1).  Forward: row_scale = 1 / deg.  Gradient w.r.t. x: the transposed structure, map = the
// transpose map, col_scale = 1 / deg.  The decomposition is symnorm.hip's: a lane owns four adjacent columns, the
// lanes of a row's column quads form a sub-group, rows of at least kAggLong entries are run by a workgroup each from
// the caller's list (a long row that is not listed is still computed by its sub-group, a listed short row skipped
// by the workgroup kernel), both bins in one launch.  Every product and sum is float64 in an order fixed by the row,
// C and the block size; no float atomics: the same input gives the same bits.
//
// wg_edge_pair_inv_distance: DCGC's homophily coefficient (DCGC.py:164-165), 1 / (|Q_r - Q_c|_2 + alpha) per entry,
// as a float64 sum of squared differences (not |a|^2 + |b|^2 - 2 a.b, which cancels where the rows are close: a self
// loop gives exactly 1 / alpha).
#include <climits>
#include <cmath>
#include <cstdint>

#include "internal.h"

namespace wg {
namespace {

constexpr int kAggLong = 128;    // rows of at least this many entries take the workgroup kernel
constexpr int kAggFlight = 8;    // gathers in flight per lane
constexpr int kAggWaves = kBlock / 64;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

struct AggArgs {
  int64_t n, nnz;
  const int64_t* indptr;
  const int32_t* indices;
  const int32_t* long_rows;
  int64_t n_long;
  const float* val;
  const int32_t* map;
  const float* row_scale;
  const float* col_scale;
  int C;
  bool vec;
  const float* x;
  float* out;
};

__device__ inline void agg_axpy4(double (&acc)[4], double s, const float* __restrict__ row, int c0, int C, bool vec) {
  if (vec) {
    const float4 v = *reinterpret_cast<const float4*>(row + c0);
    acc[0] += s * (double)v.x;
    acc[1] += s * (double)v.y;
    acc[2] += s * (double)v.z;
    acc[3] += s * (double)v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < C) acc[k] += s * (double)row[c0 + k];
  }
}

// the weight of entry e and its column: val[map ? map[e] : e] * col_scale[j]
__device__ inline double agg_weight(const AggArgs& a, int64_t e, int64_t& j) {
  WG_DCHECK(e >= 0 && e < a.nnz, "edgeagg: entry %lld of %lld", (long long)e, (long long)a.nnz);
  j = a.indices[e];
  WG_DCHECK(j >= 0 && j < a.n, "edgeagg: entry %lld has column %lld outside [0, %lld)", (long long)e, (long long)j,
            (long long)a.n);
  int64_t q = e;
  if (a.map) {
    q = a.map[e];
    WG_DCHECK(q >= 0 && q < a.nnz, "edgeagg: entry %lld maps to %lld outside [0, %lld)", (long long)e, (long long)q,
              (long long)a.nnz);
  }
  double s = (double)a.val[q];
  if (a.col_scale) s *= (double)a.col_scale[j];
  return s;
}

// acc += sum over e = beg, beg + step, ... < end of weight(e) * x[j_e][c0 .. c0 + 4), in that order
__device__ inline void agg_walk(double (&acc)[4], const AggArgs& a, int64_t beg, int64_t end, int64_t step, int c0) {
  constexpr int U = kAggFlight;
  int64_t e = beg;
  for (; e + (U - 1) * step < end; e += U * step) {
    int64_t j[U];
    double s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) s[u] = agg_weight(a, e + u * step, j[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) agg_axpy4(acc, s[u], a.x + j[u] * a.C, c0, a.C, a.vec);
  }
  for (; e < end; e += step) {
    int64_t j;
    const double s = agg_weight(a, e, j);
    agg_axpy4(acc, s, a.x + j * a.C, c0, a.C, a.vec);
  }
}

__device__ inline bool agg_listed(const int32_t* __restrict__ long_rows, int64_t n_long, int64_t i) {
  int64_t lo = 0, hi = n_long;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (long_rows[mid] < i) lo = mid + 1;
    else hi = mid;
  }
  return lo < n_long && long_rows[lo] == i;
}

// LONG: one listed row per workgroup (list entry `blk`).  Else: one row per sub-group of G lanes.
template <int G, bool LONG>
__device__ inline void agg_rows(int64_t blk, const AggArgs& a) {
  constexpr int NG = kBlock / G;
  constexpr int T = LONG ? NG : 1;
  __shared__ double lds[LONG ? kAggWaves * G * 4 : 1];
  const int sub = threadIdx.x & (G - 1);
  const int team = LONG ? (int)threadIdx.x / G : 0;
  int64_t i;
  if constexpr (LONG) {
    i = a.long_rows[blk];
    WG_DCHECK(i >= 0 && i < a.n, "edgeagg: long row %lld outside [0, %lld)", (long long)i, (long long)a.n);
  } else {
    i = blk * NG + threadIdx.x / G;
  }
  bool active = i >= 0 && i < a.n;
  int64_t beg = 0, end = 0;
  if (active) {
    const int64_t b = a.indptr[i], e = a.indptr[i + 1];
    WG_DCHECK(b >= 0 && b <= e && e <= a.nnz, "edgeagg: row %lld has the range [%lld, %lld) of %lld", (long long)i,
              (long long)b, (long long)e, (long long)a.nnz);
    if (LONG ? (e - b >= kAggLong) : (e - b < kAggLong || !agg_listed(a.long_rows, a.n_long, i))) {
      beg = b;
      end = e;
    } else {
      active = false;
    }
  }
  if (!active) i = 0;
  const double ri = (active && a.row_scale) ? (double)a.row_scale[i] : 1.0;
  const int C = a.C, NQ = (C + 3) >> 2;
  for (int w0 = 0; w0 < NQ; w0 += G) {
    const int w = w0 + sub, c0 = 4 * w;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (w < NQ) agg_walk(acc, a, beg + team, end, T, c0);
    if constexpr (LONG) {
#pragma unroll
      for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
      }
      __syncthreads();
      if ((threadIdx.x & 63) < G) {
#pragma unroll
        for (int k = 0; k < 4; ++k) lds[((threadIdx.x >> 6) * G + sub) * 4 + k] = acc[k];
      }
      __syncthreads();
      if (team == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = lds[sub * 4 + k];
#pragma unroll
        for (int v = 1; v < kAggWaves; ++v) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] += lds[(v * G + sub) * 4 + k];
        }
      }
    }
    if (active && team == 0 && w < NQ) {
      float r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = (float)(ri * acc[k]);
      float* o = a.out + i * C + c0;
      if (a.vec) {
        *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c0 + k < C) o[k] = r[k];
      }
    }
  }
}

template <int G>
__global__ __launch_bounds__(kBlock) void edge_agg_kernel(AggArgs a) {
  if ((int64_t)blockIdx.x < a.n_long) agg_rows<G, true>(blockIdx.x, a);   // uniform over the workgroup
  else agg_rows<G, false>((int64_t)blockIdx.x - a.n_long, a);
}

__global__ __launch_bounds__(kBlock) void pair_inv_distance_kernel(int64_t nnz, const int32_t* __restrict__ rows,
                                                                   const int32_t* __restrict__ cols, int C,
                                                                   int64_t n, const float* __restrict__ Q,
                                                                   double alpha, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= nnz) return;
  const int64_t r = rows[e], c = cols[e];
  WG_DCHECK(r >= 0 && r < n && c >= 0 && c < n, "edgeagg: pair %lld is (%lld, %lld) outside [0, %lld)", (long long)e,
            (long long)r, (long long)c, (long long)n);
  const float* qr = Q + r * C;
  const float* qc = Q + c * C;
  double s = 0.0;
  for (int k = 0; k < C; ++k) {
    const double d = (double)qr[k] - (double)qc[k];
    s = fma(d, d, s);
  }
  out[e] = (float)(1.0 / (sqrt(s) + alpha));
}

int agg_pow2_lanes(int64_t want) {
  int g = 1;
  while (g < 64 && g < want) g <<= 1;
  return g;
}

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_edge_aggregate_long_row(void) { return kAggLong; }

int wg_edge_aggregate(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t n_long,
                      const int32_t* long_rows, const float* val, const int32_t* map, const float* row_scale,
                      const float* col_scale, int64_t C, const float* x, float* out, void* stream_) {
  if (n < 0 || nnz < 0 || C < 0 || n_long < 0)
    return fail(WG_ERR_INVALID, "wg_edge_aggregate: negative size (n=%lld nnz=%lld C=%lld long rows=%lld)",
                (long long)n, (long long)nnz, (long long)C, (long long)n_long);
  if (C > INT32_MAX) return fail(WG_ERR_INVALID, "wg_edge_aggregate: C must be below 2^31 (C=%lld)", (long long)C);
  if (n > INT32_MAX || nnz > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "wg_edge_aggregate: n=%lld / nnz=%lld exceed int32", (long long)n,
                (long long)nnz);
  if (n_long > n)
    return fail(WG_ERR_INVALID, "wg_edge_aggregate: %lld long rows of %lld rows", (long long)n_long, (long long)n);
  if (n == 0 || C == 0) return WG_OK;
  if (!indptr || !x || !out)
    return fail(WG_ERR_INVALID, "wg_edge_aggregate: NULL indptr / x / out with n=%lld C=%lld", (long long)n,
                (long long)C);
  if (nnz > 0 && (!indices || !val))
    return fail(WG_ERR_INVALID, "wg_edge_aggregate: NULL indices / val with nnz=%lld", (long long)nnz);
  if (n_long > 0 && !long_rows)
    return fail(WG_ERR_INVALID, "wg_edge_aggregate: NULL long_rows with %lld long rows", (long long)n_long);
  if (out == x) return fail(WG_ERR_INVALID, "wg_edge_aggregate: out must not alias x");
  hipStream_t stream = as_stream(stream_);
  AggArgs a{n, nnz, indptr, indices, long_rows, n_long, val, map, row_scale, col_scale, (int)C,
            (C % 4 == 0) && aligned16(x) && aligned16(out), x, out};
  const int G = agg_pow2_lanes(ceil_div(C, 4));
  if (n_long + ceil_div(n, kBlock / G) > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "wg_edge_aggregate: n=%lld rows at C=%lld need more than 2^31 workgroups",
                (long long)n, (long long)C);
#define WG_AGG_LAUNCH(g)                                                                                          \
  case g:                                                                                                         \
    hipLaunchKernelGGL((edge_agg_kernel<g>), dim3((unsigned)(n_long + ceil_div(n, kBlock / g))), dim3(kBlock), 0, \
                       stream, a);                                                                                \
    break;
  switch (G) {
    WG_AGG_LAUNCH(1)
    WG_AGG_LAUNCH(2)
    WG_AGG_LAUNCH(4)
    WG_AGG_LAUNCH(8)
    WG_AGG_LAUNCH(16)
    WG_AGG_LAUNCH(32)
    default:
      hipLaunchKernelGGL((edge_agg_kernel<64>), dim3((unsigned)(n_long + ceil_div(n, kBlock / 64))), dim3(kBlock), 0,
                         stream, a);
  }
#undef WG_AGG_LAUNCH
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_edge_pair_inv_distance(int64_t nnz, const int32_t* rows, const int32_t* cols, int64_t C, int64_t n,
                              const float* Q, double alpha, float* out, void* stream_) {
  if (nnz < 0 || C < 0 || n < 0 || C > INT32_MAX)
    return fail(WG_ERR_INVALID, "wg_edge_pair_inv_distance: bad size (nnz=%lld C=%lld n=%lld)", (long long)nnz,
                (long long)C, (long long)n);
  if (nnz == 0) return WG_OK;
  if (!rows || !cols || !out || (C > 0 && !Q))
    return fail(WG_ERR_INVALID, "wg_edge_pair_inv_distance: NULL pointer with nnz=%lld", (long long)nnz);
  if (nnz > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "wg_edge_pair_inv_distance: nnz=%lld exceeds int32", (long long)nnz);
  hipLaunchKernelGGL(pair_inv_distance_kernel, dim3((unsigned)ceil_div(nnz, kBlock)), dim3(kBlock), 0,
                     as_stream(stream_), nnz, rows, cols, (int)C, n, Q, alpha, out);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // extern "C"
