// symnorm.hip -- SURVEY section 8(f): the aggregation of the CaGCN calibrator (reference calibration/CaGCN.py).
// Its scaling model is two PyG GCNConv layers (CaGCN.py:68-70, :104-108): gcn_norm builds one weight per edge of
// the graph with one self loop per node, w_ij = deg_i^-1/2 deg_j^-1/2 with deg the in-degree, and message passing
// materialises one (E, C) tensor of scaled source rows that a scatter adds up per target.  Here the weights are
// never built: with dinv = deg^-1/2 per node,
//
//     out[i][c] = act( dinv[i] * sum over p in [indptr[i], indptr[i + 1]) of dinv[j_p] * x[j_p][c]  +  bias[c] )
//
// is one pull pass over the by-destination CSR that reads an id, one float of dinv and one C-wide row per entry
// (wg_symnorm_aggregate).  The gradient w.r.t. x is the same entry over the transposed structure, no bias, no ReLU.
//
// Decomposition.  A lane owns four adjacent columns of an output row (16 bytes per gather when C % 4 == 0 and x /
// out are 16-byte aligned, dwords otherwise); the G = 1 .. 64 lanes that cover a row's ceil(C / 4) column quads form
// a sub-group (a row wider than 256 columns takes several passes of its sub-group), and the sub-groups of a wave
// work on different rows.  Rows come in two bins.  A row of fewer than kSymLong entries has one sub-group, which
// walks the row's entries in ascending position, kInFlight gathers in flight per lane.  A longer row (a hub; the
// caller lists them) gets a workgroup: its kBlock / G sub-groups deal the entries round-robin, the sub-groups of a
// wave meet in a butterfly and the waves' partials in LDS, added in wave order.  The workgroup kernel skips a listed
// row that is not long, and the sub-group kernel looks a long row up in the list (a binary search, once per long
// row) and walks it itself when it is not there: every row is written, whatever the list holds.  Both bins are one
// launch: the first n_long workgroups take the list, the rest the sub-group rows.
//
// Arithmetic.  Every product and sum is float64 (the product of two float32 is exact there); the epilogue
// dinv_i * acc + bias_c is float64, rounded once to float32, then the ReLU as v < 0 ? 0 : v (a NaN stays a NaN).
// The order of a row's sum is fixed by the row, G and the block size; no float atomics: the same input gives the
// same bits, whatever the order of the edge list the CSR was built from.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see DESIGN.md 4.3; no kernel
// of this file uses scratch.
#include <climits>
#include <cstdint>

#include "internal.h"

namespace wg {
namespace {

constexpr int kSymLong = 128;    // rows of at least this many entries take the workgroup kernel
constexpr int kInFlight = 8;     // gathers in flight per lane
constexpr int kWaves = kBlock / 64;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ inline void axpy4(double (&acc)[4], double s, const float* __restrict__ row, int c0, int C, bool vec) {
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

// acc += sum over the entries e = beg, beg + step, ... < end of dinv[ids[e]] * x[ids[e]][c0 .. c0 + 4), in that
// order.  kInFlight entries at a time: their ids first, then their scales and rows (both depend on the id alone),
// then the adds in order.
__device__ inline void walk(double (&acc)[4], int64_t beg, int64_t end, int64_t step, const int32_t* __restrict__ ids,
                            const float* __restrict__ dinv, const float* __restrict__ x, int C, int c0, bool vec,
                            int64_t n, int64_t nnz) {
  constexpr int U = kInFlight;
  int64_t e = beg;
  for (; e + (U - 1) * step < end; e += U * step) {
    int64_t j[U];
    double s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      WG_DCHECK(e + u * step < nnz, "symnorm: entry %lld of %lld", (long long)(e + u * step), (long long)nnz);
      j[u] = ids[e + u * step];
      WG_DCHECK(j[u] >= 0 && j[u] < n, "symnorm: entry %lld has column %lld outside [0, %lld)",
                (long long)(e + u * step), (long long)j[u], (long long)n);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) s[u] = (double)dinv[j[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) axpy4(acc, s[u], x + j[u] * C, c0, C, vec);
  }
  for (; e < end; e += step) {
    WG_DCHECK(e < nnz, "symnorm: entry %lld of %lld", (long long)e, (long long)nnz);
    const int64_t j = ids[e];
    WG_DCHECK(j >= 0 && j < n, "symnorm: entry %lld has column %lld outside [0, %lld)", (long long)e, (long long)j,
              (long long)n);
    axpy4(acc, (double)dinv[j], x + j * C, c0, C, vec);
  }
}

// row i is in the ascending list (an unsorted list may hide it: the row is then computed by a workgroup and by a
// sub-group, both right to the last rounding, and either's bits may stay)
__device__ inline bool listed(const int32_t* __restrict__ long_rows, int64_t n_long, int64_t i) {
  int64_t lo = 0, hi = n_long;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (long_rows[mid] < i) lo = mid + 1;
    else hi = mid;
  }
  return lo < n_long && long_rows[lo] == i;
}

// LONG: one listed row per workgroup (list entry `blk`).  Else: one row per sub-group of G lanes (rows blk * NG ..).
// A row of the other bin, or past the end, leaves the thread with an empty range (LONG: its workgroup still runs the
// barriers).
template <int G, bool LONG>
__device__ inline void symnorm_rows(int64_t blk, int64_t n, int64_t nnz, const int64_t* __restrict__ indptr,
                                    const int32_t* __restrict__ indices, const int32_t* __restrict__ long_rows,
                                    int64_t n_long, const float* __restrict__ dinv, int C, bool vec,
                                    const float* __restrict__ x, const float* __restrict__ bias, bool relu,
                                    float* __restrict__ out) {
  constexpr int NG = kBlock / G;       // sub-groups per workgroup
  constexpr int T = LONG ? NG : 1;     // sub-groups per row
  __shared__ double lds[LONG ? kWaves * G * 4 : 1];
  const int sub = threadIdx.x & (G - 1);
  const int team = LONG ? (int)threadIdx.x / G : 0;
  int64_t i;
  if constexpr (LONG) {
    i = long_rows[blk];
    WG_DCHECK(i >= 0 && i < n, "symnorm: long row %lld outside [0, %lld)", (long long)i, (long long)n);
  } else {
    i = blk * NG + threadIdx.x / G;
  }
  bool active = i >= 0 && i < n;
  int64_t beg = 0, end = 0;
  if (active) {
    const int64_t b = indptr[i], e = indptr[i + 1];
    WG_DCHECK(b >= 0 && b <= e && e <= nnz, "symnorm: row %lld has the range [%lld, %lld) of %lld", (long long)i,
              (long long)b, (long long)e, (long long)nnz);
    if (LONG ? (e - b >= kSymLong) : (e - b < kSymLong || !listed(long_rows, n_long, i))) {
      beg = b;
      end = e;
    } else {
      active = false;
    }
  }
  if (!active) i = 0;
  const double di = active ? (double)dinv[i] : 0.0;
  const int NQ = (C + 3) >> 2;
  for (int w0 = 0; w0 < NQ; w0 += G) {   // one trip when the row's column quads fit the sub-group
    const int w = w0 + sub, c0 = 4 * w;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (w < NQ) walk(acc, beg + team, end, T, indices, dinv, x, C, c0, vec, n, nnz);
    if constexpr (LONG) {
      // the wave's sub-groups meet in a butterfly over the lanes that own the same columns, the waves in LDS
#pragma unroll
      for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
      }
      __syncthreads();  // the readers of the previous trip are done
      if ((threadIdx.x & 63) < G) {
#pragma unroll
        for (int k = 0; k < 4; ++k) lds[((threadIdx.x >> 6) * G + sub) * 4 + k] = acc[k];
      }
      __syncthreads();
      if (team == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = lds[sub * 4 + k];
#pragma unroll
        for (int v = 1; v < kWaves; ++v) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] += lds[(v * G + sub) * 4 + k];
        }
      }
    }
    if (active && team == 0 && w < NQ) {
      float r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double b = (bias && c0 + k < C) ? (double)bias[c0 + k] : 0.0;
        r[k] = (float)(di * acc[k] + b);
        if (relu) r[k] = r[k] < 0.0f ? 0.0f : r[k];   // keeps a NaN
      }
      float* o = out + i * C + c0;
      if (vec) {
        *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c0 + k < C) o[k] = r[k];
      }
    }
  }
}

// One launch for both bins: the first n_long workgroups take the listed rows (the hubs start first and finish beside
// the short rows instead of after them), the rest the sub-group rows.
template <int G>
__global__ __launch_bounds__(kBlock) void symnorm_kernel(int64_t n, int64_t nnz, const int64_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ indices,
                                                         const int32_t* __restrict__ long_rows, int64_t n_long,
                                                         const float* __restrict__ dinv, int C, bool vec,
                                                         const float* __restrict__ x, const float* __restrict__ bias,
                                                         bool relu, float* __restrict__ out) {
  if ((int64_t)blockIdx.x < n_long)   // uniform over the workgroup
    symnorm_rows<G, true>(blockIdx.x, n, nnz, indptr, indices, long_rows, n_long, dinv, C, vec, x, bias, relu, out);
  else
    symnorm_rows<G, false>((int64_t)blockIdx.x - n_long, n, nnz, indptr, indices, long_rows, n_long, dinv, C, vec, x,
                           bias, relu, out);
}

int pow2_lanes(int64_t want) {
  int g = 1;
  while (g < 64 && g < want) g <<= 1;
  return g;
}

#define WG_SYM_CASES(G_, MACRO) \
  switch (G_) {                 \
    MACRO(1)                    \
    MACRO(2)                    \
    MACRO(4)                    \
    MACRO(8)                    \
    MACRO(16)                   \
    MACRO(32)                   \
    default:                    \
      MACRO(64)                 \
  }

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_symnorm_long_row(void) { return kSymLong; }

int wg_symnorm_aggregate(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t n_long,
                         const int32_t* long_rows, const float* dinv, int64_t C, const float* x, const float* bias,
                         int32_t relu, float* out, void* stream_) {
  if (n < 0 || nnz < 0 || C < 0 || n_long < 0)
    return fail(WG_ERR_INVALID, "wg_symnorm_aggregate: negative size (n=%lld nnz=%lld C=%lld long rows=%lld)",
                (long long)n, (long long)nnz, (long long)C, (long long)n_long);
  if (C > INT32_MAX) return fail(WG_ERR_INVALID, "wg_symnorm_aggregate: C must be below 2^31 (C=%lld)", (long long)C);
  if (n > INT32_MAX || nnz > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "wg_symnorm_aggregate: n=%lld / nnz=%lld exceed int32", (long long)n,
                (long long)nnz);
  if (n_long > n)
    return fail(WG_ERR_INVALID, "wg_symnorm_aggregate: %lld long rows of %lld rows", (long long)n_long, (long long)n);
  if (n == 0 || C == 0) return WG_OK;
  if (!indptr || !dinv || !x || !out)
    return fail(WG_ERR_INVALID, "wg_symnorm_aggregate: NULL indptr / dinv / x / out with n=%lld C=%lld", (long long)n,
                (long long)C);
  if (nnz > 0 && !indices)
    return fail(WG_ERR_INVALID, "wg_symnorm_aggregate: NULL indices with nnz=%lld", (long long)nnz);
  if (n_long > 0 && !long_rows)
    return fail(WG_ERR_INVALID, "wg_symnorm_aggregate: NULL long_rows with %lld long rows", (long long)n_long);
  if (out == x) return fail(WG_ERR_INVALID, "wg_symnorm_aggregate: out must not alias x");
  hipStream_t stream = as_stream(stream_);
  const bool vec = (C % 4 == 0) && aligned16(x) && aligned16(out);
  const int G = pow2_lanes(ceil_div(C, 4));
  if (n_long + ceil_div(n, kBlock / G) > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "wg_symnorm_aggregate: n=%lld rows at C=%lld need more than 2^31 workgroups",
                (long long)n, (long long)C);
#define WG_SYM_LAUNCH(g)                                                                                            \
  case g:                                                                                                           \
    hipLaunchKernelGGL((symnorm_kernel<g>), dim3((unsigned)(n_long + ceil_div(n, kBlock / g))), dim3(kBlock), 0,    \
                       stream, n, nnz, indptr, indices, long_rows, n_long, dinv, (int)C, vec, x, bias, relu != 0,   \
                       out);                                                                                        \
    break;
  WG_SYM_CASES(G, WG_SYM_LAUNCH)
#undef WG_SYM_LAUNCH
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // extern "C"
