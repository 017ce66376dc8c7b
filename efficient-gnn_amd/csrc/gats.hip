// gats.hip -- SURVEY section 8(f): the attention layer of the GATS calibrator (reference calibration/GATS.py).
// CalibAttentionLayer.message (GATS.py:147-167) computes, for every edge j -> i of the graph with one self loop
// per node (GATS.py:102-106),
//     d_ij = sum_c a_i[c] a_j[c]          e_ij = leaky_relu(d_ij, slope)          p_ij = softmax over In(i) of e_ij
// and aggregates  sim_i[h] = sum_j p_ij t_j[h],  dconf_i = sum_j (conf_i - conf_j)  through PyG's message
// passing, which materialises one (E, C) tensor per operand.  Its BFS (shortest_path_length, GATS.py:25-49) is
// a Python loop over nodes that masks all E edges per node.  This file holds both on the device:
//
//   wg_csr_transpose_map   the transposed structure of a canonical CSR and, per transposed entry, the position
//                          of the entry it mirrors (a stable radix sort of the positions by column)
//   wg_bfs_levels          the BFS levels 0 .. max_hop - 1 from a mask, one launch per level
//   wg_gat_forward         the edge softmax and both aggregations, one pass over the by-destination CSR
//   wg_gat_backward        d loss / d a and d loss / d t from d loss / d sim: an edge pass (p and s per edge)
//                          and a node pass (each node's own row and its transposed row)
//
// Decomposition.  Rows come in two bins.  A row of fewer than kGatLong entries gets a sub-group of G lanes
// (G = the mean row length rounded up to a power of two, 4 .. 64), one entry per lane and turn; a longer row
// (a hub; the caller lists them) gets a workgroup, whose wave partials meet in LDS in wave order.  In the
// forward and the edge pass a lane owns an entry: it reads both C-wide rows itself (16 bytes per load when
// C % 4 == 0 and the base is 16-byte aligned, dwords otherwise; the row a_i is the same address over the
// sub-group), so the dot product needs no cross-lane step.  In the node pass a node has a wave: a lane owns four
// columns of the output row, and the wave's sub-groups deal the node's entries round-robin.
//
// Arithmetic.  Every product and sum (d_ij, the row maximum, the softmax denominator, sim, dconf, m_i and the
// gradients) and exp are float64; e_ij, the row maximum, the denominator, p_ij and s_ij are handed from the
// forward to the backward and from the edge pass to the node pass as float64.  The order of every sum is fixed
// by the row, G and the widths: a lane adds its entries in ascending position, lanes meet in a fixed butterfly,
// waves in wave order.  No float atomics: the same input gives the same bits.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "internal.h"

namespace wg {
namespace {

constexpr int kGatLong = 256;      // rows of at least this many entries take the workgroup kernels
constexpr int kGatMaxHeads = 64;   // Hh above this is WG_ERR_INVALID
constexpr int kGatHeadTile = 8;    // heads accumulated per sweep over a row
constexpr int kWaves = kBlock / 64;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---------------------------------------------------------------------------------------------------------
// reductions over the lanes of one row: a butterfly over the sub-group (every lane ends with the same bits:
// both partners of a step add the same two numbers), then, for a workgroup row, the waves' values in wave order
// ---------------------------------------------------------------------------------------------------------
template <int G>
__device__ inline double butterfly_sum(double v) {
#pragma unroll
  for (int off = G >> 1; off >= 1; off >>= 1) v += __shfl_xor(v, off, G);
  return v;
}

template <int G>
__device__ inline double butterfly_max(double v) {
#pragma unroll
  for (int off = G >> 1; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, G));
  return v;
}

// Every thread of the workgroup calls these (LONG: they hold barriers).
template <int G, bool LONG>
__device__ inline double row_sum(double v, double* lds) {
  v = butterfly_sum<LONG ? 64 : G>(v);
  if constexpr (LONG) {
    __syncthreads();  // the readers of the previous reduction are done
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    v = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += lds[w];
  }
  return v;
}

template <int G, bool LONG>
__device__ inline double row_max_of(double v, double* lds) {
  v = butterfly_max<LONG ? 64 : G>(v);
  if constexpr (LONG) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    v = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v = fmax(v, lds[w]);
  }
  return v;
}

// sum_c x[c] y[c] in float64, ascending c (a product of two float32 is exact in float64)
__device__ inline double dot_f64(const float* __restrict__ x, const float* __restrict__ y, int C, bool vec) {
  double acc = 0.0;
  if (vec) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const float4* y4 = reinterpret_cast<const float4*>(y);
    const int nq = C >> 2;
#pragma unroll 4  // the loads of four steps in flight; the sum stays one chain in ascending c
    for (int q = 0; q < nq; ++q) {
      const float4 u = x4[q];
      const float4 v = y4[q];
      acc += (double)u.x * (double)v.x;
      acc += (double)u.y * (double)v.y;
      acc += (double)u.z * (double)v.z;
      acc += (double)u.w * (double)v.w;
    }
  } else {
#pragma unroll 4
    for (int c = 0; c < C; ++c) acc += (double)x[c] * (double)y[c];
  }
  return acc;
}

__device__ inline double leaky(double d, double slope) { return d > 0.0 ? d : slope * d; }

// The row of this thread's sub-group (LONG: of its workgroup, from the list).  A row of the other bin, or past
// the end, is left to the other kernel: the thread keeps running with an empty range (the reductions need it).
template <int G, bool LONG>
__device__ inline bool pick_row(int64_t n, const int64_t* __restrict__ indptr, const int32_t* __restrict__ long_rows,
                                int64_t* row, int64_t* beg, int64_t* end) {
  int64_t i;
  if constexpr (LONG) {
    i = long_rows[blockIdx.x];
    WG_DCHECK(i >= 0 && i < n, "gat: long row %lld outside [0, %lld)", (long long)i, (long long)n);
  } else {
    i = (int64_t)blockIdx.x * (kBlock / G) + threadIdx.x / G;
  }
  bool active = i >= 0 && i < n;
  *row = active ? i : 0;
  *beg = *end = 0;
  if (active) {
    const int64_t b = indptr[i], e = indptr[i + 1];
    WG_DCHECK(b >= 0 && b <= e, "gat: row %lld has the range [%lld, %lld)", (long long)i, (long long)b, (long long)e);
    if ((e - b >= kGatLong) == LONG) {
      *beg = b;
      *end = e;
    } else {
      active = false;
    }
  }
  return active;
}

// ---------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------
template <int G, bool LONG>
__global__ __launch_bounds__(kBlock) void gat_forward_kernel(
    int64_t n, int64_t nnz, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const int32_t* __restrict__ long_rows, int C, int H, bool vec, const float* __restrict__ a,
    const float* __restrict__ t, const float* __restrict__ conf, double slope, float* __restrict__ sim,
    float* __restrict__ dconf, double* e_save, double* __restrict__ row_max, double* __restrict__ row_den) {
  __shared__ double lds[kWaves];
  constexpr int L = LONG ? kBlock : G;  // lanes of one row
  const int sub = LONG ? (int)threadIdx.x : (int)(threadIdx.x & (G - 1));
  int64_t i, beg, end;
  const bool active = pick_row<G, LONG>(n, indptr, long_rows, &i, &beg, &end);
  const float* ai = a + i * C;
  const int64_t first = beg + sub;

  // sweep 1: the logits and their maximum; the lane's first logit stays in a register
  double m = -INFINITY, e0 = 0.0;
  for (int64_t e = first; e < end; e += L) {
    WG_DCHECK(e < nnz, "gat forward: entry %lld of %lld", (long long)e, (long long)nnz);
    const int64_t j = indices[e];
    WG_DCHECK(j >= 0 && j < n, "gat forward: entry %lld has column %lld outside [0, %lld)", (long long)e,
              (long long)j, (long long)n);
    const double ev = leaky(dot_f64(ai, a + j * C, C, vec), slope);
    if (e_save) e_save[e] = ev;
    if (e == first) e0 = ev;
    m = fmax(m, ev);
  }
  const double M = row_max_of<G, LONG>(m, lds);

  // sweep 2 (once per tile of heads): p = exp(e - M), the denominator, dconf and the heads' sums
  const double ci = active ? (double)conf[i] : 0.0;
  double den = 0.0, dc = 0.0;
  for (int h0 = 0; h0 < H; h0 += kGatHeadTile) {
    double acc[kGatHeadTile];
#pragma unroll
    for (int k = 0; k < kGatHeadTile; ++k) acc[k] = 0.0;
    for (int64_t e = first; e < end; e += L) {
      const int64_t j = indices[e];
      double ev;
      if (e == first) ev = e0;
      else if (e_save) ev = e_save[e];  // written by this thread in sweep 1
      else ev = leaky(dot_f64(ai, a + j * C, C, vec), slope);
      const double p = exp(ev - M);
      if (h0 == 0) {
        den += p;
        dc += ci - (double)conf[j];
      }
      const float* tj = t + j * H + h0;
#pragma unroll
      for (int k = 0; k < kGatHeadTile; ++k)
        if (h0 + k < H) acc[k] += p * (double)tj[k];
    }
    if (h0 == 0) {
      den = row_sum<G, LONG>(den, lds);
      dc = row_sum<G, LONG>(dc, lds);
    }
#pragma unroll
    for (int k = 0; k < kGatHeadTile; ++k) {
      if (h0 + k < H) {  // uniform over the workgroup
        const double v = row_sum<G, LONG>(acc[k], lds);
        if (active && sub == 0) sim[i * H + h0 + k] = end > beg ? (float)(v / den) : 0.0f;  // no entries: 0
      }
    }
  }
  if (active && sub == 0) {
    dconf[i] = (float)dc;
    if (row_max) {
      row_max[i] = M;
      row_den[i] = den;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// backward, edge pass: p_ij and s_ij of every entry (work[e] = p, work[nnz + e] = s)
// ---------------------------------------------------------------------------------------------------------
template <int G, bool LONG>
__global__ __launch_bounds__(kBlock) void gat_backward_edge_kernel(
    int64_t n, int64_t nnz, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const int32_t* __restrict__ long_rows, int H, const float* __restrict__ t, const double* __restrict__ e_save,
    const double* __restrict__ row_max, const double* __restrict__ row_den, const float* __restrict__ g_sim,
    double slope, double* __restrict__ work) {
  __shared__ double lds[kWaves];
  constexpr int L = LONG ? kBlock : G;
  const int sub = LONG ? (int)threadIdx.x : (int)(threadIdx.x & (G - 1));
  int64_t i, beg, end;
  const bool active = pick_row<G, LONG>(n, indptr, long_rows, &i, &beg, &end);
  const double M = active ? row_max[i] : 0.0;
  const double den = active ? row_den[i] : 1.0;
  const float* gi = g_sim + i * H;
  const int64_t first = beg + sub;

  auto edge = [&](int64_t e, double* p, double* q) {
    WG_DCHECK(e < nnz, "gat backward: entry %lld of %lld", (long long)e, (long long)nnz);
    const int64_t j = indices[e];
    WG_DCHECK(j >= 0 && j < n, "gat backward: entry %lld has column %lld outside [0, %lld)", (long long)e,
              (long long)j, (long long)n);
    *p = exp(e_save[e] - M) / den;
    *q = dot_f64(gi, t + j * H, H, false);
  };

  // sweep 1: m_i = sum_j p_ij q_ij
  double ms = 0.0, p0 = 0.0, q0 = 0.0;
  for (int64_t e = first; e < end; e += L) {
    double p, q;
    edge(e, &p, &q);
    if (e == first) {
      p0 = p;
      q0 = q;
    }
    ms += p * q;
  }
  ms = row_sum<G, LONG>(ms, lds);
  // sweep 2: r = p (q - m), s = r * leaky_relu'(d); d > 0 exactly when e > 0, and d == 0 takes the slope
  for (int64_t e = first; e < end; e += L) {
    double p = p0, q = q0;
    if (e != first) edge(e, &p, &q);
    work[e] = p;
    work[nnz + e] = p * (q - ms) * (e_save[e] > 0.0 ? 1.0 : slope);
  }
}

// ---------------------------------------------------------------------------------------------------------
// backward, node pass.  Node i owns the output rows grad_a[i] and grad_t[i]; lane `sub` of its sub-group
// owns four columns of one of them (item w: columns [4 w, 4 w + 4) of grad_a for w < NA, of grad_t after):
//   grad_a[i] = sum over row i of the CSR, ascending position,      of s_ij a_j
//             + sum over row i of the transpose, ascending row l,   of s_li a_l
//   grad_t[i] = sum over row i of the transpose, ascending row l,   of p_li g_l
// A node has a wave: its 64 / G sub-groups deal the entries round-robin (a walk is a chain of dependent loads, so
// the lanes go to entries in flight, not to more nodes) and meet in a butterfly.  LONG (a node whose row or
// transposed row is long): the workgroup's kBlock / G sub-groups do, their partials meet in LDS in sub-group order.
// ---------------------------------------------------------------------------------------------------------
__device__ inline void axpy4(double (&acc)[4], double s, const float* __restrict__ row, int c0, int W, bool vec) {
  if (vec) {
    const float4 v = *reinterpret_cast<const float4*>(row + c0);
    acc[0] += s * (double)v.x;
    acc[1] += s * (double)v.y;
    acc[2] += s * (double)v.z;
    acc[3] += s * (double)v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < W) acc[k] += s * (double)row[c0 + k];
  }
}

// acc += sum over the entries e = beg, beg + step, ... < end of scale[e] * x[ids[e]][c0 .. c0 + 4), in that order.
// U entries are in flight at a time: their ids and scales are loaded first, then their rows (a walk is a chain
// of dependent loads: the hub's 5 749 entries one after the other cost a millisecond), then added in order.
template <int U>
__device__ inline void walk_row(double (&acc)[4], int64_t beg, int64_t end, int64_t step,
                                const int32_t* __restrict__ ids, const double* __restrict__ scale,
                                const float* __restrict__ x, int W, int c0, bool vec, int64_t n) {
  int64_t e = beg;
  for (; e + (U - 1) * step < end; e += U * step) {
    int64_t j[U];
    double s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      j[u] = ids[e + u * step];
      s[u] = scale[e + u * step];
      WG_DCHECK(j[u] >= 0 && j[u] < n, "gat backward: entry %lld has column %lld outside [0, %lld)",
                (long long)(e + u * step), (long long)j[u], (long long)n);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) axpy4(acc, s[u], x + j[u] * W, c0, W, vec);
  }
  for (; e < end; e += step) {
    const int64_t j = ids[e];
    WG_DCHECK(j >= 0 && j < n, "gat backward: entry %lld has column %lld outside [0, %lld)", (long long)e,
              (long long)j, (long long)n);
    axpy4(acc, scale[e], x + j * W, c0, W, vec);
  }
}

// the same over transposed entries: the scale of entry e is scale[pos[e]]
template <int U>
__device__ inline void walk_col(double (&acc)[4], int64_t beg, int64_t end, int64_t step,
                                const int32_t* __restrict__ ids, const int32_t* __restrict__ pos,
                                const double* __restrict__ scale, const float* __restrict__ x, int W, int c0, bool vec,
                                int64_t n, int64_t nnz) {
  int64_t e = beg;
  for (; e + (U - 1) * step < end; e += U * step) {
    int64_t l[U], q[U];
    double s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      l[u] = ids[e + u * step];
      q[u] = pos[e + u * step];
      WG_DCHECK(l[u] >= 0 && l[u] < n && q[u] >= 0 && q[u] < nnz,
                "gat backward: transposed entry %lld is (row %lld, position %lld) of n=%lld nnz=%lld",
                (long long)(e + u * step), (long long)l[u], (long long)q[u], (long long)n, (long long)nnz);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) s[u] = scale[q[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) axpy4(acc, s[u], x + l[u] * W, c0, W, vec);
  }
  for (; e < end; e += step) {
    const int64_t l = ids[e], q = pos[e];
    WG_DCHECK(l >= 0 && l < n && q >= 0 && q < nnz,
              "gat backward: transposed entry %lld is (row %lld, position %lld) of n=%lld nnz=%lld", (long long)e,
              (long long)l, (long long)q, (long long)n, (long long)nnz);
    axpy4(acc, scale[q], x + l * W, c0, W, vec);
  }
}

template <int G, bool LONG>
__global__ __launch_bounds__(kBlock) void gat_backward_node_kernel(
    int64_t n, int64_t nnz, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const int64_t* __restrict__ t_indptr, const int32_t* __restrict__ t_indices, const int32_t* __restrict__ t_pos,
    const int32_t* __restrict__ t_long_rows, int C, int H, bool vec_a, bool vec_t, const float* __restrict__ a,
    const float* __restrict__ g_sim, const double* __restrict__ work, float* __restrict__ grad_a,
    float* __restrict__ grad_t) {
  constexpr int NG = kBlock / G;           // sub-groups per workgroup
  constexpr int T = LONG ? NG : 64 / G;    // sub-groups per node: the workgroup's, or the wave's
  constexpr int U = LONG ? 16 : 4;         // entries in flight per lane
  __shared__ double lds[LONG ? kBlock * 4 : 1];
  const int sub = threadIdx.x & (G - 1);
  const int team = (threadIdx.x / G) % T;
  int64_t i;
  if constexpr (LONG) {
    i = t_long_rows[blockIdx.x];
    WG_DCHECK(i >= 0 && i < n, "gat backward: long node %lld outside [0, %lld)", (long long)i, (long long)n);
  } else {
    i = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  }
  bool active = i >= 0 && i < n;
  int64_t rb = 0, re = 0, cb = 0, ce = 0;
  if (active) {
    rb = indptr[i];
    re = indptr[i + 1];
    cb = t_indptr[i];
    ce = t_indptr[i + 1];
    WG_DCHECK(rb >= 0 && rb <= re && re <= nnz && cb >= 0 && cb <= ce && ce <= nnz,
              "gat backward: node %lld has the ranges [%lld, %lld) and [%lld, %lld) of %lld", (long long)i,
              (long long)rb, (long long)re, (long long)cb, (long long)ce, (long long)nnz);
    if (((re - rb >= kGatLong) || (ce - cb >= kGatLong)) != LONG) {
      active = false;
      rb = re = cb = ce = 0;
    }
  }
  if (!active) i = 0;
  const int NA = (C + 3) >> 2, NT = (H + 3) >> 2;
  const int64_t skip = team, step = T;
  const double* P = work;
  const double* S = work + nnz;
  for (int w0 = 0; w0 < NA + NT; w0 += G) {  // one trip when the row's items fit the sub-group
    const int w = w0 + sub;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (w < NA) {
      walk_row<U>(acc, rb + skip, re, step, indices, S, a, C, 4 * w, vec_a, n);
      walk_col<U>(acc, cb + skip, ce, step, t_indices, t_pos, S, a, C, 4 * w, vec_a, n, nnz);
    } else if (w < NA + NT) {
      walk_col<U>(acc, cb + skip, ce, step, t_indices, t_pos, P, g_sim, H, 4 * (w - NA), vec_t, n, nnz);
    }
    if constexpr (LONG) {
      __syncthreads();  // the readers of the previous trip are done
#pragma unroll
      for (int k = 0; k < 4; ++k) lds[threadIdx.x * 4 + k] = acc[k];
      __syncthreads();
      if (team == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = 0.0;
        for (int g = 0; g < NG; ++g) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] += lds[(g * G + sub) * 4 + k];
        }
      }
    } else {
      // the wave's sub-groups meet in a butterfly over the lanes that own the same columns
#pragma unroll
      for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
      }
    }
    if (active && team == 0 && w < NA + NT) {
      const bool is_a = w < NA;
      float* out = is_a ? grad_a + i * C : grad_t + i * H;
      const int c0 = is_a ? 4 * w : 4 * (w - NA), W = is_a ? C : H;
      if (is_a ? vec_a : vec_t) {
        *reinterpret_cast<float4*>(out + c0) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c0 + k < W) out[c0 + k] = (float)acc[k];
      }
    }
  }
}

int pow2_lanes(int64_t want, int lo) {
  int g = lo;
  while (g < 64 && g < want) g <<= 1;
  return g;
}

// the widths pow2_lanes can give: 4 .. 64 for a row's sub-group, 2 .. 64 for the node pass (C >= 1 and Hh >= 1
// make at least two items)
#define WG_GAT_CASES_FROM4(G_, MACRO) \
  switch (G_) {                       \
    MACRO(4)                          \
    MACRO(8)                          \
    MACRO(16)                         \
    MACRO(32)                         \
    default:                          \
      MACRO(64)                       \
  }
#define WG_GAT_CASES_FROM2(G_, MACRO) \
  switch (G_) {                       \
    MACRO(2)                          \
    MACRO(4)                          \
    MACRO(8)                          \
    MACRO(16)                         \
    MACRO(32)                         \
    default:                          \
      MACRO(64)                       \
  }

// ---------------------------------------------------------------------------------------------------------
// transpose map
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void tr_expand_kernel(int64_t n, int64_t nnz, const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices,
                                                           uint32_t* __restrict__ keys, int32_t* __restrict__ pos,
                                                           int32_t* __restrict__ rows) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= nnz) return;
  int64_t lo = 0, hi = n;  // the last row r with indptr[r] <= e
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo + 1) >> 1);
    if (indptr[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  WG_DCHECK(lo < n && indptr[lo] <= e && e < indptr[lo + 1], "transpose: entry %lld is in no row (found %lld)",
            (long long)e, (long long)lo);
  const int32_t c = indices[e];
  WG_DCHECK(c >= 0 && c < n, "transpose: entry %lld has column %d outside [0, %lld)", (long long)e, (int)c,
            (long long)n);
  keys[e] = (uint32_t)c;
  pos[e] = (int32_t)e;
  rows[e] = (int32_t)lo;
}

__global__ __launch_bounds__(kBlock) void tr_rows_kernel(int64_t nnz, const int32_t* __restrict__ t_pos,
                                                         const int32_t* __restrict__ rows,
                                                         int32_t* __restrict__ t_indices) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= nnz) return;
  const int32_t p = t_pos[e];
  WG_DCHECK(p >= 0 && p < nnz, "transpose: position %d of %lld", (int)p, (long long)nnz);
  t_indices[e] = rows[p];
}

// t_indptr[c] = the number of entries with a column < c (the sorted keys ascend)
__global__ __launch_bounds__(kBlock) void tr_indptr_kernel(int64_t n, int64_t nnz, const uint32_t* __restrict__ sorted,
                                                           int64_t* __restrict__ t_indptr) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c > n) return;
  int64_t lo = 0, hi = nnz;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)sorted[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  t_indptr[c] = lo;
}

struct DeviceBlock {
  char* p = nullptr;
  ~DeviceBlock() { (void)hipFree(p); }  // hipFree waits for the work that still uses it
};

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// ---------------------------------------------------------------------------------------------------------
// BFS levels
// ---------------------------------------------------------------------------------------------------------
constexpr int kBfsLanes = 64;  // lanes per frontier node (a hub's row is one walk)

__global__ __launch_bounds__(kBlock) void bfs_init_kernel(int64_t n, const uint8_t* __restrict__ mask, int32_t max_hop,
                                                          int64_t* __restrict__ dist) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) dist[i] = (max_hop > 0 && mask[i]) ? 0 : INT64_MAX;
}

// Nodes at level hop - 1 give level hop to their unreached out-neighbours.  Every writer of a cell writes the
// same value, and no thread acts on a cell that holds hop, so the result does not depend on the order.
__global__ __launch_bounds__(kBlock) void bfs_level_kernel(int64_t n, const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices, int64_t hop,
                                                           int64_t* dist) {
  const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kBfsLanes;
  const int sub = threadIdx.x & (kBfsLanes - 1);
  if (i >= n || dist[i] != hop - 1) return;
  const int64_t end = indptr[i + 1];
  for (int64_t e = indptr[i] + sub; e < end; e += kBfsLanes) {
    const int64_t j = indices[e];
    WG_DCHECK(j >= 0 && j < n, "bfs: entry %lld has column %lld outside [0, %lld)", (long long)e, (long long)j,
              (long long)n);
    if (dist[j] == INT64_MAX) dist[j] = hop;
  }
}

int gat_check_shape(const char* who, int64_t n, int64_t nnz, int64_t n_long, int64_t C, int64_t Hh) {
  if (n < 0 || nnz < 0 || n_long < 0)
    return fail(WG_ERR_INVALID, "%s: negative size (n=%lld nnz=%lld long rows=%lld)", who, (long long)n,
                (long long)nnz, (long long)n_long);
  if (C < 1 || C > INT32_MAX) return fail(WG_ERR_INVALID, "%s: C must be in [1, 2^31) (C=%lld)", who, (long long)C);
  if (Hh < 1 || Hh > kGatMaxHeads)
    return fail(WG_ERR_INVALID, "%s: Hh must be in [1, %d] (Hh=%lld)", who, kGatMaxHeads, (long long)Hh);
  if (n > INT32_MAX || nnz > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld / nnz=%lld exceed int32", who, (long long)n, (long long)nnz);
  if (n_long > n) return fail(WG_ERR_INVALID, "%s: %lld long rows of %lld rows", who, (long long)n_long, (long long)n);
  return WG_OK;
}

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_gat_long_row(void) { return kGatLong; }

int wg_csr_transpose_map(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t* t_indptr,
                         int32_t* t_indices, int32_t* t_pos, void* stream_) {
  if (n < 0 || nnz < 0)
    return fail(WG_ERR_INVALID, "wg_csr_transpose_map: negative size (n=%lld nnz=%lld)", (long long)n, (long long)nnz);
  if (n > INT32_MAX || nnz > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "wg_csr_transpose_map: n=%lld / nnz=%lld exceed int32", (long long)n,
                (long long)nnz);
  if (!indptr || !t_indptr) return fail(WG_ERR_INVALID, "wg_csr_transpose_map: NULL indptr / t_indptr");
  if (nnz > 0 && (!indices || !t_indices || !t_pos))
    return fail(WG_ERR_INVALID, "wg_csr_transpose_map: NULL indices / t_indices / t_pos with nnz=%lld", (long long)nnz);
  if (nnz > 0 && n == 0) return fail(WG_ERR_INVALID, "wg_csr_transpose_map: %lld entries in no rows", (long long)nnz);
  hipStream_t stream = as_stream(stream_);
  const int M = (int)nnz;
  int cbits = 1;
  while ((1ll << cbits) < n) ++cbits;
  uint32_t* unull = nullptr;
  int32_t* inull = nullptr;
  size_t sort_bytes = 0;
  DeviceBlock blk;
  uint32_t* sorted = nullptr;
  if (M > 0) {
    WG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, unull, unull, inull, inull, M, 0, cbits, stream));
    // one block: [keys M | sorted keys M | positions M | rows M | cub]
    const size_t o_sorted = align256(sizeof(uint32_t) * M), o_pos = o_sorted + align256(sizeof(uint32_t) * M),
                 o_rows = o_pos + align256(sizeof(int32_t) * M), o_cub = o_rows + align256(sizeof(int32_t) * M),
                 total = o_cub + align256(sort_bytes);
    WG_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&blk.p), total));
    uint32_t* keys = reinterpret_cast<uint32_t*>(blk.p);
    sorted = reinterpret_cast<uint32_t*>(blk.p + o_sorted);
    int32_t* pos = reinterpret_cast<int32_t*>(blk.p + o_pos);
    int32_t* rows = reinterpret_cast<int32_t*>(blk.p + o_rows);
    const dim3 grid((unsigned)ceil_div(M, kBlock)), block(kBlock);
    hipLaunchKernelGGL(tr_expand_kernel, grid, block, 0, stream, n, nnz, indptr, indices, keys, pos, rows);
    WG_LAUNCH_CHECK();
    // stable: the entries of one column stay in ascending position, that is in ascending row
    WG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(blk.p + o_cub, sort_bytes, keys, sorted, pos, t_pos, M, 0, cbits,
                                                  stream));
    hipLaunchKernelGGL(tr_rows_kernel, grid, block, 0, stream, nnz, t_pos, rows, t_indices);
    WG_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(tr_indptr_kernel, dim3((unsigned)ceil_div(n + 1, kBlock)), dim3(kBlock), 0, stream, n, nnz, sorted,
                     t_indptr);
  WG_LAUNCH_CHECK();
  WG_HIP_TRY(hipStreamSynchronize(stream));
  return WG_OK;
}

int wg_bfs_levels(int64_t n, const int64_t* indptr, const int32_t* indices, const uint8_t* mask, int32_t max_hop,
                  int64_t* dist, void* stream_) {
  if (n < 0) return fail(WG_ERR_INVALID, "wg_bfs_levels: negative size (n=%lld)", (long long)n);
  if (n > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "wg_bfs_levels: n=%lld exceeds int32", (long long)n);
  if (max_hop < 0) return fail(WG_ERR_INVALID, "wg_bfs_levels: max_hop must be >= 0 (max_hop=%d)", (int)max_hop);
  if (n == 0) return WG_OK;
  if (!indptr || !mask || !dist) return fail(WG_ERR_INVALID, "wg_bfs_levels: NULL indptr / mask / dist with n=%lld", (long long)n);
  if (max_hop > 1 && !indices) return fail(WG_ERR_INVALID, "wg_bfs_levels: NULL indices with max_hop=%d", (int)max_hop);
  hipStream_t stream = as_stream(stream_);
  hipLaunchKernelGGL(bfs_init_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, stream, n, mask, max_hop,
                     dist);
  WG_LAUNCH_CHECK();
  // a level past n - 1 is empty: no launch for it
  const int64_t levels = std::min<int64_t>(max_hop, n);
  for (int64_t hop = 1; hop < levels; ++hop) {
    hipLaunchKernelGGL(bfs_level_kernel, dim3((unsigned)ceil_div(n * kBfsLanes, kBlock)), dim3(kBlock), 0, stream, n,
                       indptr, indices, hop, dist);
    WG_LAUNCH_CHECK();
  }
  return WG_OK;
}

int wg_gat_forward(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t n_long,
                   const int32_t* long_rows, int64_t C, int64_t Hh, const float* a, const float* t, const float* conf,
                   double negative_slope, float* sim, float* dconf, double* e_save, double* row_max, double* row_den,
                   void* stream_) {
  if (int rc = gat_check_shape("wg_gat_forward", n, nnz, n_long, C, Hh)) return rc;
  if (n == 0) return WG_OK;
  if (!indptr || !a || !t || !conf || !sim || !dconf)
    return fail(WG_ERR_INVALID, "wg_gat_forward: NULL indptr / a / t / conf / sim / dconf with n=%lld", (long long)n);
  if (nnz > 0 && !indices) return fail(WG_ERR_INVALID, "wg_gat_forward: NULL indices with nnz=%lld", (long long)nnz);
  if (n_long > 0 && !long_rows)
    return fail(WG_ERR_INVALID, "wg_gat_forward: NULL long_rows with %lld long rows", (long long)n_long);
  const int saved = (e_save != nullptr) + (row_max != nullptr) + (row_den != nullptr);
  if (saved != 0 && saved != 3)
    return fail(WG_ERR_INVALID, "wg_gat_forward: e_save / row_max / row_den are given or NULL together");
  hipStream_t stream = as_stream(stream_);
  const bool vec = (C % 4 == 0) && aligned16(a);
  const int G = pow2_lanes(ceil_div(nnz, n), 4);
#define WG_GAT_FWD(g)                                                                                                  \
  case g:                                                                                                              \
    hipLaunchKernelGGL((gat_forward_kernel<g, false>), dim3((unsigned)ceil_div(n, kBlock / g)), dim3(kBlock), 0, stream, \
                       n, nnz, indptr, indices, long_rows, (int)C, (int)Hh, vec, a, t, conf, negative_slope, sim,      \
                       dconf, e_save, row_max, row_den);                                                               \
    break;
  WG_GAT_CASES_FROM4(G, WG_GAT_FWD)
#undef WG_GAT_FWD
  WG_LAUNCH_CHECK();
  if (n_long > 0) {
    hipLaunchKernelGGL((gat_forward_kernel<64, true>), dim3((unsigned)n_long), dim3(kBlock), 0, stream, n, nnz, indptr,
                       indices, long_rows, (int)C, (int)Hh, vec, a, t, conf, negative_slope, sim, dconf, e_save,
                       row_max, row_den);
    WG_LAUNCH_CHECK();
  }
  return WG_OK;
}

int wg_gat_backward(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t n_long,
                    const int32_t* long_rows, const int64_t* t_indptr, const int32_t* t_indices, const int32_t* t_pos,
                    int64_t n_tlong, const int32_t* t_long_rows, int64_t C, int64_t Hh, const float* a, const float* t,
                    const double* e_save, const double* row_max, const double* row_den, const float* g_sim,
                    double negative_slope, float* grad_a, float* grad_t, double* edge_work, void* stream_) {
  if (int rc = gat_check_shape("wg_gat_backward", n, nnz, n_long, C, Hh)) return rc;
  if (n_tlong < 0 || n_tlong > n)
    return fail(WG_ERR_INVALID, "wg_gat_backward: %lld long nodes of %lld nodes", (long long)n_tlong, (long long)n);
  if (n == 0) return WG_OK;
  if (!indptr || !t_indptr || !a || !t || !row_max || !row_den || !g_sim || !grad_a || !grad_t)
    return fail(WG_ERR_INVALID,
                "wg_gat_backward: NULL indptr / t_indptr / a / t / row_max / row_den / g_sim / grad_a / grad_t with n=%lld",
                (long long)n);
  if (nnz > 0 && (!indices || !t_indices || !t_pos || !e_save || !edge_work))
    return fail(WG_ERR_INVALID, "wg_gat_backward: NULL indices / t_indices / t_pos / e_save / edge_work with nnz=%lld",
                (long long)nnz);
  if ((n_long > 0 && !long_rows) || (n_tlong > 0 && !t_long_rows))
    return fail(WG_ERR_INVALID, "wg_gat_backward: NULL long_rows / t_long_rows with %lld / %lld of them",
                (long long)n_long, (long long)n_tlong);
  hipStream_t stream = as_stream(stream_);
  const int G = pow2_lanes(ceil_div(nnz, n), 4);
#define WG_GAT_EDGE(g)                                                                                                 \
  case g:                                                                                                              \
    hipLaunchKernelGGL((gat_backward_edge_kernel<g, false>), dim3((unsigned)ceil_div(n, kBlock / g)), dim3(kBlock), 0, \
                       stream, n, nnz, indptr, indices, long_rows, (int)Hh, t, e_save, row_max, row_den, g_sim,        \
                       negative_slope, edge_work);                                                                     \
    break;
  WG_GAT_CASES_FROM4(G, WG_GAT_EDGE)
#undef WG_GAT_EDGE
  WG_LAUNCH_CHECK();
  if (n_long > 0) {
    hipLaunchKernelGGL((gat_backward_edge_kernel<64, true>), dim3((unsigned)n_long), dim3(kBlock), 0, stream, n, nnz,
                       indptr, indices, long_rows, (int)Hh, t, e_save, row_max, row_den, g_sim, negative_slope,
                       edge_work);
    WG_LAUNCH_CHECK();
  }
  const bool vec_a = (C % 4 == 0) && aligned16(a) && aligned16(grad_a);
  const bool vec_t = (Hh % 4 == 0) && aligned16(g_sim) && aligned16(grad_t);
  const int G2 = pow2_lanes(ceil_div(C, 4) + ceil_div(Hh, 4), 2);
#define WG_GAT_NODE(g)                                                                                               \
  case g:                                                                                                            \
    hipLaunchKernelGGL((gat_backward_node_kernel<g, false>), dim3((unsigned)ceil_div(n, kBlock / 64)), dim3(kBlock), 0, \
                       stream, n, nnz, indptr, indices, t_indptr, t_indices, t_pos, t_long_rows, (int)C, (int)Hh,    \
                       vec_a, vec_t, a, g_sim, edge_work, grad_a, grad_t);                                           \
    if (n_tlong > 0)                                                                                                 \
      hipLaunchKernelGGL((gat_backward_node_kernel<g, true>), dim3((unsigned)n_tlong), dim3(kBlock), 0, stream, n,   \
                         nnz, indptr, indices, t_indptr, t_indices, t_pos, t_long_rows, (int)C, (int)Hh, vec_a,      \
                         vec_t, a, g_sim, edge_work, grad_a, grad_t);                                                \
    break;
  WG_GAT_CASES_FROM2(G2, WG_GAT_NODE)
#undef WG_GAT_NODE
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // extern "C"
