// gatedagg.hip -- SURVEY section 8(f): the mixture of graph experts of the GETS calibrator (reference
// calibration/GETS.py).  Its E experts end in one PyG GCNConv each (GETS.py:60-62, :86-92), a noisy top-k gate picks
// k of them per node (GETS.py:362-388), and forward stacks all E aggregated (N, C) outputs, multiplies them by gates
// that are exact zeros outside the selection and sums (GETS.py:402-417).  The mixture is linear and the gate belongs
// to the destination row, so it commutes with the aggregation.  With z[j, e, :] expert e's last linear map of node
// j, dinv = deg^-1/2 and sel / gate the k selected experts of a row and their weights,
//
//     T_i   = sum over the slots s of gate[i, s] * ( dinv_i * sum over p in [indptr[i], indptr[i + 1]) of
//                                                    dinv[j_p] * z[j_p, sel[i, s], :]  +  bias[sel[i, s]] )
//     out_i = log_softmax( logits_i * softplus(T_i) )
//
// is one pull pass over the by-destination CSR that reads each id and dinv once and only the k selected C-wide
// slices of a neighbour's row (wg_gated_symnorm_forward); no (N, E, C) tensor exists.  A slice that a row did not
// select is never read: a NaN in it does not reach that row (the reference's 0 * NaN would).  The gradient w.r.t. z
// is one pass over the transposed structure that gathers the single row g_T[i] per entry and adds it, scaled, to the
// accumulators of the experts that row i selected (wg_gated_symnorm_transposed); the row-wise part of the backward
// (log_softmax, the product with the logits, softplus, the gate's gradient) is wg_gets_head_backward, no graph.
//
// Decomposition.  As symnorm.hip: a lane owns four adjacent columns (16 bytes per gather when C % 4 == 0 and the
// buffers are 16-byte aligned, dwords otherwise); the G = 1 .. 64 lanes that cover a row's ceil(C / 4) column quads
// form a sub-group (C <= 256: the whole row sits in one sub-group, which the row's softmax needs), the sub-groups of a
// wave work on different rows.  A row of fewer than kGatedLong entries has one sub-group, which walks the entries in
// ascending position, U gathers in flight per lane and slice (ids first, then what depends on the id alone).  A
// longer row (the caller lists them) gets a workgroup: its kBlock / G sub-groups deal the entries round-robin, the
// sub-groups of a wave meet in a butterfly and the waves' partials in LDS, added in wave order.  The workgroup kernel
// skips a listed row that is not long, the sub-group kernel looks a long row up in the list and walks it itself when
// it is not there.  Both bins are one launch: the first n_long workgroups take the list.
//
// Arithmetic.  Every product and sum is float64: acc_s over the entries, O_s = dinv_i acc_s + bias, T = sum_s gate_s
// O_s in ascending s, softplus as T > 20 ? T : log1p(exp(T)) (torch's default threshold), v = logits * sp, the row's
// maximum and sum of exp across the sub-group, out = v - max - log(sum); each output (out, t_save, o_save, g_z,
// g_logits, g_t, g_gate) is rounded once to float32.  g_gate uses the float64 g_t, not its rounded copy.  The order
// of every sum is fixed by the row, G and the block size; no float atomics: the same input gives the same bits.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see DESIGN.md 4.3; accumulators
// are acc[k][4] doubles forward and acc[E][4] backward (at most 32 VGPRs); no kernel of this file uses scratch.
#include <climits>
#include <cstdint>

#include "internal.h"

namespace wg {
namespace {

constexpr int kGatedLong = 128;   // rows of at least this many entries take the workgroup kernel (as kSymLong)
constexpr int kGatedMaxE = 4;     // experts
constexpr int kGatedMaxC = 256;   // columns: one sub-group of at most 64 lanes holds the row
constexpr int kWaves = kBlock / 64;

// gathers in flight per lane: 8 entries of one or two slices, 4 entries of three or four
constexpr int in_flight(int slices) { return slices <= 2 ? 8 : 4; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ inline void load4(float (&r)[4], const float* __restrict__ row, int c0, int C, bool vec) {
  if (vec) {
    const float4 v = *reinterpret_cast<const float4*>(row + c0);
    r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = c0 + k < C ? row[c0 + k] : 0.0f;
  }
}

__device__ inline void store4(float* __restrict__ row, const float (&r)[4], int c0, int C, bool vec) {
  if (vec) {
    *reinterpret_cast<float4*>(row + c0) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < C) row[c0 + k] = r[k];
  }
}

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

__device__ inline int64_t entry_id(const int32_t* __restrict__ ids, int64_t e, int64_t n, int64_t nnz) {
  WG_DCHECK(e >= 0 && e < nnz, "gatedagg: entry %lld of %lld", (long long)e, (long long)nnz);
  const int64_t j = ids[e];
  WG_DCHECK(j >= 0 && j < n, "gatedagg: entry %lld has column %lld outside [0, %lld)", (long long)e, (long long)j,
            (long long)n);
  return j;
}

// forward: acc[s] += sum over the entries e = beg, beg + step, ... < end of dinv[j_e] * z[j_e][eo[s] .. + C) at the
// lane's four columns, in that order; eo[s] = C * the expert of slot s, EC = E * C
template <int K>
__device__ inline void walk_forward(double (&acc)[K][4], int64_t beg, int64_t end, int64_t step,
                                    const int32_t* __restrict__ ids, const float* __restrict__ dinv,
                                    const float* __restrict__ z, int64_t EC, const int (&eo)[K], int C, int c0,
                                    bool vec, int64_t n, int64_t nnz) {
  constexpr int U = in_flight(K);
  int64_t e = beg;
  for (; e + (U - 1) * step < end; e += U * step) {
    int64_t j[U];
    double s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) j[u] = entry_id(ids, e + u * step, n, nnz);
#pragma unroll
    for (int u = 0; u < U; ++u) s[u] = (double)dinv[j[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int q = 0; q < K; ++q) axpy4(acc[q], s[u], z + j[u] * EC + eo[q], c0, C, vec);
    }
  }
  for (; e < end; e += step) {
    const int64_t j = entry_id(ids, e, n, nnz);
    const double s = (double)dinv[j];
#pragma unroll
    for (int q = 0; q < K; ++q) axpy4(acc[q], s, z + j * EC + eo[q], c0, C, vec);
  }
}

// the weight of row i's gradient in each expert's accumulator: hit[e] when a slot of row i holds e (the ids of a
// row are distinct), wt[e] = dinv[i] * that slot's gate, exact in float64
template <int E>
__device__ inline void slot_weights(bool (&hit)[E], double (&wt)[E], int64_t i, int K, const int32_t* __restrict__ sel,
                                    const float* __restrict__ gate, const float* __restrict__ dinv) {
  const double di = (double)dinv[i];
#pragma unroll
  for (int e = 0; e < E; ++e) hit[e] = false, wt[e] = 0.0;
#pragma unroll
  for (int s = 0; s < kGatedMaxE; ++s) {
    if (s < K) {
      const int q = sel[i * K + s];
      WG_DCHECK(q >= 0 && q < E, "gatedagg: row %lld selects expert %d of %d", (long long)i, q, E);
      const double g = di * (double)gate[i * K + s];
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (q == e) hit[e] = true, wt[e] = g;
    }
  }
}

template <int E>
__device__ inline void scatter4(double (&acc)[E][4], const bool (&hit)[E], const double (&wt)[E],
                                const float (&g)[4]) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[e][k] = hit[e] ? acc[e][k] + wt[e] * (double)g[k] : acc[e][k];   // no 0 * NaN
  }
}

// transposed: acc[e] += sum over the entries (the rows i that gather this row) of dinv_i * gate[i, s] * g_t[i] at
// the lane's four columns, for the slot s of row i that holds e, if any
template <int E>
__device__ inline void walk_transposed(double (&acc)[E][4], int64_t beg, int64_t end, int64_t step,
                                       const int32_t* __restrict__ ids, const float* __restrict__ dinv, int K,
                                       const int32_t* __restrict__ sel, const float* __restrict__ gate,
                                       const float* __restrict__ g_t, int C, int c0, bool vec, int64_t n,
                                       int64_t nnz) {
  constexpr int U = in_flight(1);
  int64_t e = beg;
  for (; e + (U - 1) * step < end; e += U * step) {
    int64_t i[U];
    bool hit[U][E];
    double wt[U][E];
    float g[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) i[u] = entry_id(ids, e + u * step, n, nnz);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      slot_weights<E>(hit[u], wt[u], i[u], K, sel, gate, dinv);
      load4(g[u], g_t + i[u] * C, c0, C, vec);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) scatter4<E>(acc, hit[u], wt[u], g[u]);
  }
  for (; e < end; e += step) {
    const int64_t i = entry_id(ids, e, n, nnz);
    bool hit[E];
    double wt[E];
    float g[4];
    slot_weights<E>(hit, wt, i, K, sel, gate, dinv);
    load4(g, g_t + i * C, c0, C, vec);
    scatter4<E>(acc, hit, wt, g);
  }
}

// row i is in the ascending list
__device__ inline bool listed(const int32_t* __restrict__ long_rows, int64_t n_long, int64_t i) {
  int64_t lo = 0, hi = n_long;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (long_rows[mid] < i) lo = mid + 1;
    else hi = mid;
  }
  return lo < n_long && long_rows[lo] == i;
}

// The row of a thread and its range.  LONG: list entry `blk`, all of the workgroup; else row blk * (kBlock / G) +
// the thread's sub-group.  A row of the other bin, or past the end, leaves an empty range and active == false.
template <int G, bool LONG>
__device__ inline bool row_range(int64_t blk, int64_t n, int64_t nnz, const int64_t* __restrict__ indptr,
                                 const int32_t* __restrict__ long_rows, int64_t n_long, int64_t* i, int64_t* beg,
                                 int64_t* end) {
  if constexpr (LONG) {
    *i = long_rows[blk];
    WG_DCHECK(*i >= 0 && *i < n, "gatedagg: long row %lld outside [0, %lld)", (long long)*i, (long long)n);
  } else {
    *i = blk * (kBlock / G) + threadIdx.x / G;
  }
  *beg = *end = 0;
  if (*i >= 0 && *i < n) {
    const int64_t b = indptr[*i], e = indptr[*i + 1];
    WG_DCHECK(b >= 0 && b <= e && e <= nnz, "gatedagg: row %lld has the range [%lld, %lld) of %lld", (long long)*i,
              (long long)b, (long long)e, (long long)nnz);
    if (LONG ? (e - b >= kGatedLong) : (e - b < kGatedLong || !listed(long_rows, n_long, *i))) {
      *beg = b;
      *end = e;
      return true;
    }
  }
  *i = 0;
  return false;
}

// a long row's NA x 4 partial sums of every sub-group of the workgroup, left in the first sub-group: the wave's
// sub-groups meet in a butterfly over the lanes that own the same columns, the waves in LDS, added in wave order
template <int G, int NA>
__device__ inline void workgroup_sum(double (&acc)[NA][4], double* lds) {
  const int sub = threadIdx.x & (G - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = G; off < 64; off <<= 1) {
#pragma unroll
    for (int a = 0; a < NA; ++a) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[a][k] += __shfl_xor(acc[a][k], off, 64);
    }
  }
  if ((threadIdx.x & 63) < G) {
#pragma unroll
    for (int a = 0; a < NA; ++a) {
#pragma unroll
      for (int k = 0; k < 4; ++k) lds[((wave * G + sub) * NA + a) * 4 + k] = acc[a][k];
    }
  }
  __syncthreads();
  if (threadIdx.x < G) {
#pragma unroll
    for (int a = 0; a < NA; ++a) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[a][k] = lds[(sub * NA + a) * 4 + k];
    }
#pragma unroll
    for (int v = 1; v < kWaves; ++v) {
#pragma unroll
      for (int a = 0; a < NA; ++a) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[a][k] += lds[((v * G + sub) * NA + a) * 4 + k];
      }
    }
  }
}

template <int G>
__device__ inline double group_max(double v) {
#pragma unroll
  for (int off = 1; off < G; off <<= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

template <int G>
__device__ inline double group_sum(double v) {
#pragma unroll
  for (int off = 1; off < G; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ inline double softplus20(double t) { return t > 20.0 ? t : log1p(exp(t)); }

struct ForwardArgs {
  int64_t n, nnz;
  const int64_t* indptr;
  const int32_t* indices;
  const int32_t* long_rows;
  int64_t n_long;
  const float* dinv;
  int C, E;
  bool vec;
  const float* z;
  const int32_t* sel;
  const float* gate;
  const float* bias;
  const float* logits;
  float* out;
  float* t_save;
  float* o_save;
};

template <int G, int K, bool LONG>
__device__ inline void forward_rows(int64_t blk, const ForwardArgs& a) {
  __shared__ double lds[LONG ? kWaves * G * K * 4 : 1];
  const int sub = threadIdx.x & (G - 1);
  const int team = LONG ? (int)threadIdx.x / G : 0;
  const int C = a.C, c0 = 4 * sub;
  int64_t i, beg, end;
  const bool active = row_range<G, LONG>(blk, a.n, a.nnz, a.indptr, a.long_rows, a.n_long, &i, &beg, &end);
  int eo[K];
  double gt[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    const int q = active ? a.sel[i * K + s] : 0;
    WG_DCHECK(q >= 0 && q < a.E, "gatedagg: row %lld selects expert %d of %d", (long long)i, q, a.E);
    eo[s] = q * C;
    gt[s] = active ? (double)a.gate[i * K + s] : 0.0;
  }
  double acc[K][4];
#pragma unroll
  for (int s = 0; s < K; ++s) acc[s][0] = acc[s][1] = acc[s][2] = acc[s][3] = 0.0;
  if (c0 < C)
    walk_forward<K>(acc, beg + team, end, LONG ? kBlock / G : 1, a.indices, a.dinv, a.z, (int64_t)a.E * C, eo, C, c0,
                    a.vec, a.n, a.nnz);
  if constexpr (LONG) workgroup_sum<G, K>(acc, lds);
  // the epilogue: every lane of the sub-group takes part in the row's reductions (a lane past the row's columns with
  // neutral values), only the row's own lanes store
  const bool own = active && team == 0 && c0 < C;
  const double di = active ? (double)a.dinv[i] : 0.0;
  double T[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < K; ++s) {
    float b[4] = {0.0f, 0.0f, 0.0f, 0.0f}, o[4];
    if (a.bias && c0 < C) load4(b, a.bias + eo[s], c0, C, a.vec);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double O = di * acc[s][k] + (double)b[k];
      T[k] += gt[s] * O;
      o[k] = (float)O;
    }
    if (own && a.o_save) store4(a.o_save + (i * K + s) * C, o, c0, C, a.vec);
  }
  float lg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (c0 < C) load4(lg, a.logits + i * C, c0, C, a.vec);
  double v[4], m = -INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = (double)lg[k] * softplus20(T[k]);
    if (c0 + k < C) m = fmax(m, v[k]);   // a NaN comes back through the sum
  }
  m = group_max<G>(m);
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c0 + k < C) sum += exp(v[k] - m);
  const double lse = log(group_sum<G>(sum));
  if (own) {
    float r[4], t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = (float)(v[k] - m - lse), t[k] = (float)T[k];
    store4(a.out + i * C, r, c0, C, a.vec);
    if (a.t_save) store4(a.t_save + i * C, t, c0, C, a.vec);
  }
}

// One launch for both bins: the first n_long workgroups take the listed rows, the rest the sub-group rows.
template <int G, int K>
__global__ __launch_bounds__(kBlock) void gated_forward_kernel(const ForwardArgs a) {
  if ((int64_t)blockIdx.x < a.n_long)   // uniform over the workgroup
    forward_rows<G, K, true>(blockIdx.x, a);
  else
    forward_rows<G, K, false>((int64_t)blockIdx.x - a.n_long, a);
}

struct TransposedArgs {
  int64_t n, nnz;
  const int64_t* indptr;
  const int32_t* indices;
  const int32_t* long_rows;
  int64_t n_long;
  const float* dinv;
  int C, K;
  bool vec;
  const int32_t* sel;
  const float* gate;
  const float* g_t;
  float* g_z;
};

template <int G, int E, bool LONG>
__device__ inline void transposed_rows(int64_t blk, const TransposedArgs& a) {
  __shared__ double lds[LONG ? kWaves * G * E * 4 : 1];
  const int sub = threadIdx.x & (G - 1);
  const int team = LONG ? (int)threadIdx.x / G : 0;
  const int C = a.C, c0 = 4 * sub;
  int64_t j, beg, end;
  const bool active = row_range<G, LONG>(blk, a.n, a.nnz, a.indptr, a.long_rows, a.n_long, &j, &beg, &end);
  double acc[E][4];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e][0] = acc[e][1] = acc[e][2] = acc[e][3] = 0.0;
  if (c0 < C)
    walk_transposed<E>(acc, beg + team, end, LONG ? kBlock / G : 1, a.indices, a.dinv, a.K, a.sel, a.gate, a.g_t, C,
                       c0, a.vec, a.n, a.nnz);
  if constexpr (LONG) workgroup_sum<G, E>(acc, lds);
  if (active && team == 0 && c0 < C) {
    const double dj = (double)a.dinv[j];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      float r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = (float)(dj * acc[e][k]);
      store4(a.g_z + (j * E + e) * C, r, c0, C, a.vec);
    }
  }
}

template <int G, int E>
__global__ __launch_bounds__(kBlock) void gated_transposed_kernel(const TransposedArgs a) {
  if ((int64_t)blockIdx.x < a.n_long)
    transposed_rows<G, E, true>(blockIdx.x, a);
  else
    transposed_rows<G, E, false>((int64_t)blockIdx.x - a.n_long, a);
}

// the row-wise backward of the head: one sub-group per row
template <int G>
__global__ __launch_bounds__(kBlock) void gets_head_backward_kernel(int64_t n, int C, int K, bool vec,
                                                                    const float* __restrict__ g_out,
                                                                    const float* __restrict__ out,
                                                                    const float* __restrict__ logits,
                                                                    const float* __restrict__ t_save,
                                                                    const float* __restrict__ o_save,
                                                                    float* __restrict__ g_logits,
                                                                    float* __restrict__ g_t,
                                                                    float* __restrict__ g_gate) {
  const int sub = threadIdx.x & (G - 1), c0 = 4 * sub;
  int64_t i = (int64_t)blockIdx.x * (kBlock / G) + threadIdx.x / G;
  const bool active = i < n;
  if (!active) i = 0;   // its lanes still take part in the shuffles of their wave
  const bool own = active && c0 < C;
  float go[4] = {0.0f, 0.0f, 0.0f, 0.0f}, o[4], lg[4], t[4];
  if (c0 < C) load4(go, g_out + i * C, c0, C, vec);
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c0 + k < C) sum += (double)go[k];
  sum = group_sum<G>(sum);
  double gt[4] = {0.0, 0.0, 0.0, 0.0};
  if (c0 < C) {
    load4(o, out + i * C, c0, C, vec);
    load4(lg, logits + i * C, c0, C, vec);
    load4(t, t_save + i * C, c0, C, vec);
    float gl[4], gr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double T = (double)t[k];
      const double g_cal = (double)go[k] - exp((double)o[k]) * sum;
      gl[k] = (float)(g_cal * softplus20(T));
      gt[k] = c0 + k < C ? g_cal * (double)lg[k] * (T > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-T))) : 0.0;
      gr[k] = (float)gt[k];
    }
    if (own) {
      store4(g_logits + i * C, gl, c0, C, vec);
      store4(g_t + i * C, gr, c0, C, vec);
    }
  }
#pragma unroll
  for (int s = 0; s < kGatedMaxE; ++s) {
    if (s < K) {   // uniform over the launch
      float os[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (c0 < C) load4(os, o_save + (i * K + s) * C, c0, C, vec);
      double d = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + k < C) d += gt[k] * (double)os[k];
      d = group_sum<G>(d);
      if (active && sub == 0) g_gate[i * K + s] = (float)d;
    }
  }
}

int pow2_lanes(int64_t want) {
  int g = 1;
  while (g < 64 && g < want) g <<= 1;
  return g;
}

#define WG_GATED_G_CASES(G_, MACRO, N_) \
  switch (G_) {                         \
    MACRO(1, N_)                        \
    MACRO(2, N_)                        \
    MACRO(4, N_)                        \
    MACRO(8, N_)                        \
    MACRO(16, N_)                       \
    MACRO(32, N_)                       \
    default:                            \
      MACRO(64, N_)                     \
  }

// the checks the two graph entries share; *done: nothing to launch
int check_graph(const char* who, int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                int64_t n_long, const int32_t* long_rows, const float* dinv, int64_t C, int64_t E, int64_t K,
                bool* done) {
  *done = false;
  if (n < 0 || nnz < 0 || n_long < 0)
    return fail(WG_ERR_INVALID, "%s: negative size (n=%lld nnz=%lld long rows=%lld)", who, (long long)n,
                (long long)nnz, (long long)n_long);
  if (C < 1 || E < 1 || K < 1 || K > E)
    return fail(WG_ERR_INVALID, "%s: needs 1 <= k <= E and 1 <= C (C=%lld E=%lld k=%lld)", who, (long long)C,
                (long long)E, (long long)K);
  if (C > kGatedMaxC || E > kGatedMaxE)
    return fail(WG_ERR_UNSUPPORTED, "%s: C=%lld above %d or E=%lld above %d", who, (long long)C, kGatedMaxC,
                (long long)E, kGatedMaxE);
  if (n > INT32_MAX || nnz > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld / nnz=%lld exceed int32", who, (long long)n, (long long)nnz);
  if (n_long > n) return fail(WG_ERR_INVALID, "%s: %lld long rows of %lld rows", who, (long long)n_long, (long long)n);
  if (n == 0) {
    *done = true;
    return WG_OK;
  }
  if (!indptr || !dinv) return fail(WG_ERR_INVALID, "%s: NULL indptr / dinv with n=%lld", who, (long long)n);
  if (nnz > 0 && !indices) return fail(WG_ERR_INVALID, "%s: NULL indices with nnz=%lld", who, (long long)nnz);
  if (n_long > 0 && !long_rows)
    return fail(WG_ERR_INVALID, "%s: NULL long_rows with %lld long rows", who, (long long)n_long);
  return WG_OK;
}

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_gated_symnorm_long_row(void) { return kGatedLong; }

int wg_gated_symnorm_forward(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t n_long,
                             const int32_t* long_rows, const float* dinv, int64_t C, int64_t E, int64_t K,
                             const float* z, const int32_t* sel, const float* gate, const float* bias,
                             const float* logits, float* out, float* t_save, float* o_save, void* stream_) {
  static const char* who = "wg_gated_symnorm_forward";
  bool done;
  if (int rc = check_graph(who, n, nnz, indptr, indices, n_long, long_rows, dinv, C, E, K, &done)) return rc;
  if (done) return WG_OK;
  if (!z || !sel || !gate || !logits || !out)
    return fail(WG_ERR_INVALID, "%s: NULL z / sel / gate / logits / out with n=%lld", who, (long long)n);
  if ((t_save == nullptr) != (o_save == nullptr))
    return fail(WG_ERR_INVALID, "%s: t_save and o_save go together (both, or both NULL)", who);
  if (out == z || out == logits || (t_save && (t_save == z || t_save == out || t_save == logits)) ||
      (o_save && (o_save == z || o_save == out || o_save == logits || o_save == t_save)))
    return fail(WG_ERR_INVALID, "%s: the outputs must not alias z, logits or each other", who);
  const bool vec = (C % 4 == 0) && aligned16(z) && aligned16(logits) && aligned16(out) && aligned16(bias) &&
                   aligned16(t_save) && aligned16(o_save);
  const int G = pow2_lanes(ceil_div(C, 4));
  const ForwardArgs a{n, nnz, indptr, indices, long_rows, n_long, dinv, (int)C, (int)E, vec,
                      z, sel, gate, bias, logits, out, t_save, o_save};
  const dim3 grid((unsigned)(n_long + ceil_div(n, kBlock / G)));
  hipStream_t stream = as_stream(stream_);
#define WG_GATED_FWD(g, k_)                                                                     \
  case g:                                                                                       \
    hipLaunchKernelGGL((gated_forward_kernel<g, k_>), grid, dim3(kBlock), 0, stream, a);        \
    break;
  switch (K) {
    case 1: WG_GATED_G_CASES(G, WG_GATED_FWD, 1) break;
    case 2: WG_GATED_G_CASES(G, WG_GATED_FWD, 2) break;
    case 3: WG_GATED_G_CASES(G, WG_GATED_FWD, 3) break;
    default: WG_GATED_G_CASES(G, WG_GATED_FWD, 4) break;
  }
#undef WG_GATED_FWD
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_gated_symnorm_transposed(int64_t n, int64_t nnz, const int64_t* t_indptr, const int32_t* t_indices,
                                int64_t n_long, const int32_t* long_rows, const float* dinv, int64_t C, int64_t E,
                                int64_t K, const int32_t* sel, const float* gate, const float* g_t, float* g_z,
                                void* stream_) {
  static const char* who = "wg_gated_symnorm_transposed";
  bool done;
  if (int rc = check_graph(who, n, nnz, t_indptr, t_indices, n_long, long_rows, dinv, C, E, K, &done)) return rc;
  if (done) return WG_OK;
  if (!sel || !gate || !g_t || !g_z)
    return fail(WG_ERR_INVALID, "%s: NULL sel / gate / g_t / g_z with n=%lld", who, (long long)n);
  if (g_z == g_t) return fail(WG_ERR_INVALID, "%s: g_z must not alias g_t", who);
  const bool vec = (C % 4 == 0) && aligned16(g_t) && aligned16(g_z);
  const int G = pow2_lanes(ceil_div(C, 4));
  const TransposedArgs a{n, nnz, t_indptr, t_indices, long_rows, n_long, dinv, (int)C, (int)K, vec, sel, gate, g_t,
                         g_z};
  const dim3 grid((unsigned)(n_long + ceil_div(n, kBlock / G)));
  hipStream_t stream = as_stream(stream_);
#define WG_GATED_BWD(g, e_)                                                                     \
  case g:                                                                                       \
    hipLaunchKernelGGL((gated_transposed_kernel<g, e_>), grid, dim3(kBlock), 0, stream, a);     \
    break;
  switch (E) {
    case 1: WG_GATED_G_CASES(G, WG_GATED_BWD, 1) break;
    case 2: WG_GATED_G_CASES(G, WG_GATED_BWD, 2) break;
    case 3: WG_GATED_G_CASES(G, WG_GATED_BWD, 3) break;
    default: WG_GATED_G_CASES(G, WG_GATED_BWD, 4) break;
  }
#undef WG_GATED_BWD
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_gets_head_backward(int64_t n, int64_t C, int64_t K, const float* g_out, const float* out, const float* logits,
                          const float* t_save, const float* o_save, float* g_logits, float* g_t, float* g_gate,
                          void* stream_) {
  static const char* who = "wg_gets_head_backward";
  if (n < 0) return fail(WG_ERR_INVALID, "%s: negative size (n=%lld)", who, (long long)n);
  if (C < 1 || K < 1) return fail(WG_ERR_INVALID, "%s: needs 1 <= k and 1 <= C (C=%lld k=%lld)", who, (long long)C,
                                  (long long)K);
  if (C > kGatedMaxC || K > kGatedMaxE)
    return fail(WG_ERR_UNSUPPORTED, "%s: C=%lld above %d or k=%lld above %d", who, (long long)C, kGatedMaxC,
                (long long)K, kGatedMaxE);
  if (n > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld exceeds int32", who, (long long)n);
  if (n == 0) return WG_OK;
  if (!g_out || !out || !logits || !t_save || !o_save || !g_logits || !g_t || !g_gate)
    return fail(WG_ERR_INVALID, "%s: NULL argument with n=%lld", who, (long long)n);
  const bool vec = (C % 4 == 0) && aligned16(g_out) && aligned16(out) && aligned16(logits) && aligned16(t_save) &&
                   aligned16(o_save) && aligned16(g_logits) && aligned16(g_t);
  const int G = pow2_lanes(ceil_div(C, 4));
  const dim3 grid((unsigned)ceil_div(n, kBlock / G));
  hipStream_t stream = as_stream(stream_);
#define WG_GATED_HEAD(g, unused_)                                                                                  \
  case g:                                                                                                          \
    hipLaunchKernelGGL((gets_head_backward_kernel<g>), grid, dim3(kBlock), 0, stream, n, (int)C, (int)K, vec,      \
                       g_out, out, logits, t_save, o_save, g_logits, g_t, g_gate);                                 \
    break;
  WG_GATED_G_CASES(G, WG_GATED_HEAD, 0)
#undef WG_GATED_HEAD
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // extern "C"
