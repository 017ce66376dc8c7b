// flips.hip -- edge-flip views of the base model's propagation.
// One iteration of the reference attacks scores the candidates, flips one edge of the dense adjacency
//     v = 1 - 2 adj[r, c];  adj[r, c] += v;  adj[c, r] += v        (calib_attack/calib_fga.py:901-904)
// and evaluates the model on the flipped graph (calib_fga.py:905-913).  A flipped graph differs from its
// parent in two rows, so the view keeps the parent's operators and carries the flips as an overlay: P
// positions sorted by (row, column), segmented by touched row, each with a_old (the parent's entry, 0 if
// absent), a_new and base_pos (its index in the parent's indices, or -1).
//
//   flip_resolve_kernel   one wave per touched row: the float64 row sum s_r, and a_old / base_pos of each
//                         position by binary search in the row's ascending columns
//   flip_rows_kernel      forward: y'_r = sum_c float32(a'_rc / deg'_r) x_c of each touched row, one
//                         workgroup per row; every other row of y is the parent's wg_spmm result
//   flip_cols_kernel      backward: gx'_c = gx_c + sum_p ((a_new - a_old) / deg'_r) g_r per overlay column,
//                         after the parent's transposed wg_spmm on g with the touched rows scaled by deg / deg'
//   csr_patch_*           commit: the canonical CSR of the flipped matrix -- new row lengths, one exclusive
//                         scan, one copy pass that shifts the parent's entries and merges the overlay
//
// The sub-group layout is sddmm.hip's: W = clamp(pow2ceil(ceil(F / 4)), 1, 64) lanes per row of x, 16-byte
// loads when F % 4 == 0 and the bases are 16-byte aligned, coalesced dwords otherwise, a loop over column
// tiles of 4 W when F is wider.  Products and sums are float64 in a fixed order (shuffle tree within the
// wave, LDS across waves in wave order); no float atomics: the same input gives the same bits.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "internal.h"

namespace wg {
namespace {

constexpr int kWaves = kBlock / 64;

// the view's overlay and the parent's CSR, as every kernel here reads them
struct FlipView {
  int64_t n = 0;                     // rows = columns of the adjacency
  const int64_t* indptr = nullptr;   // [n + 1]
  const int32_t* indices = nullptr;  // ascending in each row
  const float* values = nullptr;     // NULL = all ones
  int64_t T = 0;                     // touched rows
  const int32_t* t_rows = nullptr;   // [T] ascending
  const int64_t* seg = nullptr;      // [T + 1]: positions [seg[i], seg[i + 1]) lie in row t_rows[i]
  int64_t P = 0;                     // overlay positions
  const int32_t* cols = nullptr;     // [P] ascending within a segment
};

// first index in [lo, hi) with a[index] >= key (a ascending)
__device__ inline int64_t lower_bound32(const int32_t* __restrict__ a, int64_t lo, int64_t hi, int32_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void flip_resolve_kernel(FlipView v, float* __restrict__ a_old,
                                                              int64_t* __restrict__ base_pos,
                                                              double* __restrict__ row_sum) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);  // uniform over the wave
  const bool active = i < v.T;
  int64_t r = 0, s = 0, e = 0, p0 = 0, p1 = 0;
  if (active) {
    r = v.t_rows[i];
    WG_DCHECK(r >= 0 && r < v.n, "flip resolve: touched row %lld outside [0, %lld)", (long long)r, (long long)v.n);
    s = v.indptr[r];
    e = v.indptr[r + 1];
    p0 = v.seg[i];
    p1 = v.seg[i + 1];
    WG_DCHECK(s <= e && p0 >= 0 && p0 <= p1 && p1 <= v.P, "flip resolve: row %lld is [%lld, %lld), segment [%lld, %lld) of %lld",
              (long long)r, (long long)s, (long long)e, (long long)p0, (long long)p1, (long long)v.P);
  }
  double acc = 0.0;
  if (v.values)
    for (int64_t k = s + lane; k < e; k += 64) acc += (double)v.values[k];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (active && lane == 0) row_sum[i] = v.values ? acc : (double)(e - s);
  for (int64_t p = p0 + lane; p < p1; p += 64) {
    const int32_t c = v.cols[p];
    WG_DCHECK(c >= 0 && c < v.n, "flip resolve: position %lld column %d outside [0, %lld)", (long long)p, (int)c,
              (long long)v.n);
    const int64_t k = lower_bound32(v.indices, s, e, c);
    const bool hit = k < e && v.indices[k] == c;
    a_old[p] = hit ? (v.values ? v.values[k] : 1.0f) : 0.0f;
    base_pos[p] = hit ? k : -1;
  }
}

template <int W, bool VEC>
__global__ __launch_bounds__(kBlock) void flip_rows_kernel(FlipView v, const float* __restrict__ a_new,
                                                           const int64_t* __restrict__ base_pos,
                                                           const float* __restrict__ deg_new, int64_t F,
                                                           const float* __restrict__ x, float* __restrict__ y) {
  constexpr int kSub = kBlock / W;  // sub-groups per workgroup
  // entries a sub-group has in flight.  Their loads are unconditional (an index past the row's end reads
  // the row's last entry, a column past F the last column; neither is added), so that the ids and then
  // the rows of x of one batch are issued together, and the batch searches the segment in lock step: behind
  // a branch each load waited for the one before (hub row of 5 748 entries, F = 64: 290 us, now 91)
  constexpr int kBatch = 8;
  __shared__ double red[kWaves][W][4];
  const int sub = threadIdx.x & (W - 1);
  const int slot = threadIdx.x / W;
  const int wave = threadIdx.x >> 6;
  const int64_t ti = blockIdx.x;
  const int64_t r = v.t_rows[ti];
  WG_DCHECK(r >= 0 && r < v.n, "flip rows: touched row %lld outside [0, %lld)", (long long)r, (long long)v.n);
  const int64_t s = v.indptr[r], len = v.indptr[r + 1] - s;
  const int64_t p0 = v.seg[ti], p1 = v.seg[ti + 1];
  WG_DCHECK(len >= 0 && p0 >= 0 && p0 <= p1 && p1 <= v.P, "flip rows: row %lld length %lld, segment [%lld, %lld) of %lld",
            (long long)r, (long long)len, (long long)p0, (long long)p1, (long long)v.P);
  const float deg = deg_new[ti];
  float* yr = y + r * F;
  // one pass per tile of 4 W columns: lane `sub` owns 4 of them (VEC: one float4; else columns sub + j W)
  for (int64_t f0 = 0; f0 < F; f0 += 4 * W) {
    // the lane's columns, clamped into the row (a clamped lane's sums are never written)
    int64_t fo[4];
    if (VEC) {
      fo[0] = std::min<int64_t>((f0 >> 2) + sub, (F >> 2) - 1);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) fo[j] = std::min<int64_t>(f0 + sub + (int64_t)j * W, F - 1);
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    // the parent's row: an entry the overlay overrides takes a_new, and is dropped when that is 0
    for (int64_t i0 = slot; i0 < len; i0 += (int64_t)kSub * kBatch) {
      int32_t c[kBatch];
      float a[kBatch];
      bool on[kBatch];
      float xv[kBatch][4];
#pragma unroll
      for (int b = 0; b < kBatch; ++b) {
        const int64_t i = i0 + (int64_t)b * kSub;
        on[b] = i < len;
        const int64_t k = s + (on[b] ? i : len - 1);
        c[b] = v.indices[k];
        a[b] = v.values ? v.values[k] : 1.0f;
        WG_DCHECK(c[b] >= 0 && c[b] < v.n, "flip rows: row %lld column %d outside [0, %lld)", (long long)r, (int)c[b],
                  (long long)v.n);
      }
#pragma unroll
      for (int b = 0; b < kBatch; ++b) {
        const float* xc = x + (int64_t)c[b] * F;
        if (VEC) {
          const float4 u = reinterpret_cast<const float4*>(xc)[fo[0]];
          xv[b][0] = u.x, xv[b][1] = u.y, xv[b][2] = u.z, xv[b][3] = u.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) xv[b][j] = xc[fo[j]];
        }
      }
      // the batch's columns against the segment in lock step: pos = the last position whose column is <= c
      if (p0 < p1) {
        int64_t pos[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) pos[b] = p0;
        for (int64_t size = p1 - p0; size > 1;) {
          const int64_t half = size >> 1;
#pragma unroll
          for (int b = 0; b < kBatch; ++b) pos[b] += v.cols[pos[b] + half] <= c[b] ? half : 0;
          size -= half;
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
          WG_DCHECK(pos[b] >= p0 && pos[b] < p1, "flip rows: search ended at %lld outside [%lld, %lld)", (long long)pos[b],
                    (long long)p0, (long long)p1);
          const bool hit = v.cols[pos[b]] == c[b];
          const float an = a_new[pos[b]];
          WG_DCHECK(!(hit && on[b]) || base_pos[pos[b]] == s + i0 + (int64_t)b * kSub,
                    "flip rows: position %lld overrides entry %lld, not %lld", (long long)pos[b],
                    (long long)base_pos[pos[b]], (long long)(s + i0 + (int64_t)b * kSub));
          a[b] = hit ? an : a[b];
        }
      }
#pragma unroll
      for (int b = 0; b < kBatch; ++b) {
        const bool use = on[b] && a[b] != 0.0f;
        const double w = (double)(a[b] / deg);  // the division in float32, as gcn_norm_kernel stores a / deg
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += use ? w * (double)xv[b][j] : 0.0;
      }
    }
    // the overlay's new positions, dealt to the sub-groups after the parent's entries
    for (int64_t p = p0 + slot; p < p1; p += kSub) {
      const float a = a_new[p];
      if (base_pos[p] >= 0 || a == 0.0f) continue;
      const int32_t c = v.cols[p];
      WG_DCHECK(c >= 0 && c < v.n, "flip rows: position %lld column %d outside [0, %lld)", (long long)p, (int)c,
                (long long)v.n);
      const float* xc = x + (int64_t)c * F;
      const double w = (double)(a / deg);
      if (VEC) {
        const float4 u = reinterpret_cast<const float4*>(xc)[fo[0]];
        acc[0] += w * (double)u.x;
        acc[1] += w * (double)u.y;
        acc[2] += w * (double)u.z;
        acc[3] += w * (double)u.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += w * (double)xc[fo[j]];
      }
    }
    // sub-groups of one wave, then the waves in wave order
#pragma unroll
    for (int off = 32; off >= W; off >>= 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += __shfl_down(acc[j], off, 64);
    }
    if ((threadIdx.x & 63) < W) {
#pragma unroll
      for (int j = 0; j < 4; ++j) red[wave][sub][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < W) {
      double out[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        out[j] = red[0][sub][j];
#pragma unroll
        for (int k = 1; k < kWaves; ++k) out[j] += red[k][sub][j];
      }
      if (VEC) {
        const int64_t q = (f0 >> 2) + sub;
        if (q < (F >> 2))
          reinterpret_cast<float4*>(yr)[q] = make_float4((float)out[0], (float)out[1], (float)out[2], (float)out[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t f = f0 + sub + (int64_t)j * W;
          if (f < F) yr[f] = (float)out[j];
        }
      }
    }
    __syncthreads();  // red is written again by the next tile
  }
}

// the overlay by column: C distinct columns, positions [cseg[i], cseg[i + 1]) of column c_cols[i] in
// ascending row order, each with its row, a_new, a_old and the row's deg'
struct FlipCols {
  int64_t n = 0, C = 0, P = 0;
  const int32_t* c_cols = nullptr;
  const int64_t* cseg = nullptr;
  const int32_t* rows = nullptr;
  const float* a_new = nullptr;
  const float* a_old = nullptr;
  const float* deg = nullptr;
};

template <int W, bool VEC>
__global__ __launch_bounds__(kBlock) void flip_cols_kernel(FlipCols o, int64_t F, const float* __restrict__ g,
                                                           float* __restrict__ gx) {
  constexpr int kSub = kBlock / W;
  const int sub = threadIdx.x & (W - 1);
  const int64_t i = (int64_t)blockIdx.x * kSub + threadIdx.x / W;
  if (i >= o.C) return;  // no shuffle and no barrier below: every lane owns its columns of gx
  const int64_t c = o.c_cols[i];
  const int64_t p0 = o.cseg[i], p1 = o.cseg[i + 1];
  WG_DCHECK(c >= 0 && c < o.n, "flip cols: column %lld outside [0, %lld)", (long long)c, (long long)o.n);
  WG_DCHECK(p0 >= 0 && p0 <= p1 && p1 <= o.P, "flip cols: column %lld segment [%lld, %lld) of %lld", (long long)c,
            (long long)p0, (long long)p1, (long long)o.P);
  float* out = gx + c * F;
  if (VEC) {
    float4* out4 = reinterpret_cast<float4*>(out);
    for (int64_t q = sub; q < (F >> 2); q += W) {
      const float4 u = out4[q];
      double a0 = u.x, a1 = u.y, a2 = u.z, a3 = u.w;
      for (int64_t p = p0; p < p1; ++p) {
        const int64_t r = o.rows[p];
        WG_DCHECK(r >= 0 && r < o.n, "flip cols: position %lld row %lld outside [0, %lld)", (long long)p,
                  (long long)r, (long long)o.n);
        const double w = ((double)o.a_new[p] - (double)o.a_old[p]) / (double)o.deg[p];
        const float4 gv = reinterpret_cast<const float4*>(g + r * F)[q];
        a0 += w * (double)gv.x;
        a1 += w * (double)gv.y;
        a2 += w * (double)gv.z;
        a3 += w * (double)gv.w;
      }
      out4[q] = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
    }
  } else {
    for (int64_t f = sub; f < F; f += W) {
      double a = out[f];
      for (int64_t p = p0; p < p1; ++p) {
        const int64_t r = o.rows[p];
        WG_DCHECK(r >= 0 && r < o.n, "flip cols: position %lld row %lld outside [0, %lld)", (long long)p,
                  (long long)r, (long long)o.n);
        a += ((double)o.a_new[p] - (double)o.a_old[p]) / (double)o.deg[p] * (double)g[r * F + f];
      }
      out[f] = (float)a;
    }
  }
}

// ---------------------------------------------------------------- the commit
__device__ inline bool is_insert(const float* a_new, const int64_t* base_pos, int64_t p) {
  return base_pos[p] < 0 && a_new[p] != 0.0f;
}
__device__ inline bool is_delete(const float* a_new, const int64_t* base_pos, int64_t p) {
  return base_pos[p] >= 0 && a_new[p] == 0.0f;
}

// index of row r in t_rows (ascending), or -1
__device__ inline int64_t touched_index(const FlipView& v, int64_t r) {
  const int64_t i = lower_bound32(v.t_rows, 0, v.T, (int32_t)r);
  return (i < v.T && v.t_rows[i] == r) ? i : -1;
}

// lens[r] = the row's new length (lens[n] = 0: the scan's last output is the new nnz)
__global__ __launch_bounds__(kBlock) void csr_patch_len_kernel(FlipView v, const float* __restrict__ a_new,
                                                               const int64_t* __restrict__ base_pos,
                                                               int64_t* __restrict__ lens) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r > v.n) return;
  int64_t len = 0;
  if (r < v.n) {
    len = v.indptr[r + 1] - v.indptr[r];
    const int64_t i = touched_index(v, r);
    if (i >= 0) {
      const int64_t p1 = v.seg[i + 1];
      WG_DCHECK(v.seg[i] >= 0 && v.seg[i] <= p1 && p1 <= v.P, "csr patch: row %lld segment [%lld, %lld) of %lld",
                (long long)r, (long long)v.seg[i], (long long)p1, (long long)v.P);
      for (int64_t p = v.seg[i]; p < p1; ++p) len += (int)is_insert(a_new, base_pos, p) - (int)is_delete(a_new, base_pos, p);
    }
    WG_DCHECK(len >= 0, "csr patch: row %lld would have %lld entries", (long long)r, (long long)len);
  }
  lens[r] = len;
}

// thread k < nnz: the parent's entry k, kept unless the overlay sets it to 0; thread nnz + p: overlay
// position p, written if it is new.  An entry goes to out_indptr[row] + its rank among the row's surviving
// columns: the old offset plus the inserts minus the deletes of the row's segment before its column
__global__ __launch_bounds__(kBlock) void csr_patch_copy_kernel(FlipView v, int64_t nnz,
                                                                const float* __restrict__ a_new,
                                                                const int64_t* __restrict__ base_pos,
                                                                const int64_t* __restrict__ out_indptr,
                                                                int32_t* __restrict__ out_indices,
                                                                float* __restrict__ out_values, int64_t capacity) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= nnz + v.P) return;
  int64_t r, rank, p0, p_end;  // the segment's positions [p0, p_end) come before this entry's column
  int32_t c;
  float a;
  if (k < nnz) {
    // the row of entry k: the last r with indptr[r] <= k (rows without entries repeat their successor's start)
    int64_t lo = 0, hi = v.n;
    while (hi - lo > 1) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (v.indptr[mid] <= k) lo = mid;
      else hi = mid;
    }
    r = lo;
    WG_DCHECK(v.indptr[r] <= k && k < v.indptr[r + 1], "csr patch: entry %lld is not in row %lld", (long long)k,
              (long long)r);
    c = v.indices[k];
    a = v.values ? v.values[k] : 1.0f;
    rank = k - v.indptr[r];
    const int64_t i = touched_index(v, r);
    p0 = p_end = 0;
    if (i >= 0) {
      p0 = v.seg[i];
      p_end = lower_bound32(v.cols, p0, v.seg[i + 1], c);
      if (p_end < v.seg[i + 1] && v.cols[p_end] == c) {
        WG_DCHECK(base_pos[p_end] == k, "csr patch: position %lld overrides entry %lld, not %lld", (long long)p_end,
                  (long long)base_pos[p_end], (long long)k);
        a = a_new[p_end];
        if (a == 0.0f) return;
      }
    }
  } else {
    const int64_t p = k - nnz;
    if (!is_insert(a_new, base_pos, p)) return;
    // the segment of position p: the last i with seg[i] <= p
    int64_t lo = 0, hi = v.T;
    while (hi - lo > 1) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (v.seg[mid] <= p) lo = mid;
      else hi = mid;
    }
    WG_DCHECK(v.seg[lo] <= p && p < v.seg[lo + 1], "csr patch: position %lld is not in segment %lld", (long long)p,
              (long long)lo);
    r = v.t_rows[lo];
    WG_DCHECK(r >= 0 && r < v.n, "csr patch: touched row %lld outside [0, %lld)", (long long)r, (long long)v.n);
    c = v.cols[p];
    a = a_new[p];
    rank = lower_bound32(v.indices, v.indptr[r], v.indptr[r + 1], c) - v.indptr[r];
    p0 = v.seg[lo];
    p_end = p;
  }
  for (int64_t p = p0; p < p_end; ++p) rank += (int)is_insert(a_new, base_pos, p) - (int)is_delete(a_new, base_pos, p);
  const int64_t o = out_indptr[r] + rank;
  WG_DCHECK(rank >= 0 && o < out_indptr[r + 1] && o < capacity, "csr patch: row %lld rank %lld to %lld of [%lld, %lld), capacity %lld",
            (long long)r, (long long)rank, (long long)o, (long long)out_indptr[r], (long long)out_indptr[r + 1],
            (long long)capacity);
  out_indices[o] = c;
  out_values[o] = a;
}

struct DeviceBlock {
  char* p = nullptr;
  ~DeviceBlock() { (void)hipFree(p); }  // hipFree waits for the work that still uses it
};

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int sub_group_width(int64_t F) {
  int W = 1;
  while (W < 64 && W < ceil_div(F, 4)) W <<= 1;
  return W;
}

// the checks every entry shares; WG_OK with *empty when there is nothing to do
int check_view(const char* who, const FlipView& v) {
  if (v.n < 0 || v.T < 0 || v.P < 0)
    return fail(WG_ERR_INVALID, "%s: negative size (n=%lld n_touched=%lld n_pos=%lld)", who, (long long)v.n,
                (long long)v.T, (long long)v.P);
  if (v.n > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld exceeds int32", who, (long long)v.n);
  if (v.T > v.P || v.T > v.n)
    return fail(WG_ERR_INVALID, "%s: %lld touched rows for %lld positions in %lld rows", who, (long long)v.T,
                (long long)v.P, (long long)v.n);
  if ((v.T == 0) != (v.P == 0))
    return fail(WG_ERR_INVALID, "%s: %lld touched rows for %lld positions", who, (long long)v.T, (long long)v.P);
  if (v.n > 0 && !v.indptr) return fail(WG_ERR_INVALID, "%s: NULL indptr with n=%lld", who, (long long)v.n);
  if (v.P > 0 && (!v.t_rows || !v.seg || !v.cols))
    return fail(WG_ERR_INVALID, "%s: NULL t_rows / seg / cols with n_pos=%lld", who, (long long)v.P);
  return WG_OK;
}

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_flip_resolve(int64_t n, const int64_t* indptr, const int32_t* indices, const float* values,
                    int64_t n_touched, const int32_t* t_rows, const int64_t* seg, int64_t n_pos,
                    const int32_t* cols, float* a_old, int64_t* base_pos, double* row_sum, void* stream_) {
  FlipView v{n, indptr, indices, values, n_touched, t_rows, seg, n_pos, cols};
  if (int rc = check_view("wg_flip_resolve", v)) return rc;
  if (n_pos == 0) return WG_OK;
  if (!a_old || !base_pos || !row_sum)
    return fail(WG_ERR_INVALID, "wg_flip_resolve: NULL a_old / base_pos / row_sum with n_pos=%lld", (long long)n_pos);
  hipLaunchKernelGGL(flip_resolve_kernel, dim3((unsigned)ceil_div(n_touched, kWaves)), dim3(kBlock), 0,
                     as_stream(stream_), v, a_old, base_pos, row_sum);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_flip_rows(int64_t n, const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_touched,
                 const int32_t* t_rows, const int64_t* seg, int64_t n_pos, const int32_t* cols, const float* a_new,
                 const int64_t* base_pos, const float* deg_new, int64_t F, const float* x, float* y, void* stream_) {
  FlipView v{n, indptr, indices, values, n_touched, t_rows, seg, n_pos, cols};
  if (int rc = check_view("wg_flip_rows", v)) return rc;
  if (F < 1) return fail(WG_ERR_INVALID, "wg_flip_rows: F must be >= 1 (F=%lld)", (long long)F);
  if (n_pos == 0) return WG_OK;
  if (!a_new || !base_pos || !deg_new || !x || !y)
    return fail(WG_ERR_INVALID, "wg_flip_rows: NULL a_new / base_pos / deg_new / x / y with n_pos=%lld",
                (long long)n_pos);
  const int W = sub_group_width(F);
  const bool vec = (F % 4 == 0) && aligned16(x) && aligned16(y);
  const dim3 grid((unsigned)n_touched), block(kBlock);
  hipStream_t stream = as_stream(stream_);
#define WG_FLIP_ROWS_CASE(w)                                                                                     \
  case w:                                                                                                        \
    if (vec)                                                                                                     \
      hipLaunchKernelGGL((flip_rows_kernel<w, true>), grid, block, 0, stream, v, a_new, base_pos, deg_new, F, x, y);  \
    else                                                                                                         \
      hipLaunchKernelGGL((flip_rows_kernel<w, false>), grid, block, 0, stream, v, a_new, base_pos, deg_new, F, x, y); \
    break;
  switch (W) {
    WG_FLIP_ROWS_CASE(1)
    WG_FLIP_ROWS_CASE(2)
    WG_FLIP_ROWS_CASE(4)
    WG_FLIP_ROWS_CASE(8)
    WG_FLIP_ROWS_CASE(16)
    WG_FLIP_ROWS_CASE(32)
    WG_FLIP_ROWS_CASE(64)
  }
#undef WG_FLIP_ROWS_CASE
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_flip_cols(int64_t n, int64_t n_cols, const int32_t* c_cols, const int64_t* cseg, int64_t n_pos,
                 const int32_t* rows, const float* a_new, const float* a_old, const float* deg_new, int64_t F,
                 const float* g, float* gx, void* stream_) {
  if (n < 0 || n_cols < 0 || n_pos < 0)
    return fail(WG_ERR_INVALID, "wg_flip_cols: negative size (n=%lld n_cols=%lld n_pos=%lld)", (long long)n,
                (long long)n_cols, (long long)n_pos);
  if (n > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "wg_flip_cols: n=%lld exceeds int32", (long long)n);
  if (n_cols > n_pos || n_cols > n || (n_cols == 0) != (n_pos == 0))
    return fail(WG_ERR_INVALID, "wg_flip_cols: %lld columns for %lld positions in %lld columns", (long long)n_cols,
                (long long)n_pos, (long long)n);
  if (F < 1) return fail(WG_ERR_INVALID, "wg_flip_cols: F must be >= 1 (F=%lld)", (long long)F);
  if (n_pos == 0) return WG_OK;
  if (!c_cols || !cseg || !rows || !a_new || !a_old || !deg_new || !g || !gx)
    return fail(WG_ERR_INVALID, "wg_flip_cols: NULL c_cols / cseg / rows / a_new / a_old / deg_new / g / gx with n_pos=%lld",
                (long long)n_pos);
  FlipCols o{n, n_cols, n_pos, c_cols, cseg, rows, a_new, a_old, deg_new};
  const int W = sub_group_width(F);
  const bool vec = (F % 4 == 0) && aligned16(g) && aligned16(gx);
  const dim3 grid((unsigned)ceil_div(n_cols, kBlock / W)), block(kBlock);
  hipStream_t stream = as_stream(stream_);
#define WG_FLIP_COLS_CASE(w)                                                                   \
  case w:                                                                                      \
    if (vec)                                                                                   \
      hipLaunchKernelGGL((flip_cols_kernel<w, true>), grid, block, 0, stream, o, F, g, gx);    \
    else                                                                                       \
      hipLaunchKernelGGL((flip_cols_kernel<w, false>), grid, block, 0, stream, o, F, g, gx);   \
    break;
  switch (W) {
    WG_FLIP_COLS_CASE(1)
    WG_FLIP_COLS_CASE(2)
    WG_FLIP_COLS_CASE(4)
    WG_FLIP_COLS_CASE(8)
    WG_FLIP_COLS_CASE(16)
    WG_FLIP_COLS_CASE(32)
    WG_FLIP_COLS_CASE(64)
  }
#undef WG_FLIP_COLS_CASE
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_csr_patch(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, const float* values,
                 int64_t n_touched, const int32_t* t_rows, const int64_t* seg, int64_t n_pos, const int32_t* cols,
                 const float* a_new, const int64_t* base_pos, int64_t* out_indptr, int32_t* out_indices,
                 float* out_values, int64_t capacity, int64_t* nnz_host, void* stream_) {
  FlipView v{n, indptr, indices, values, n_touched, t_rows, seg, n_pos, cols};
  if (int rc = check_view("wg_csr_patch", v)) return rc;
  if (nnz < 0) return fail(WG_ERR_INVALID, "wg_csr_patch: negative size (nnz=%lld)", (long long)nnz);
  if (n == INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "wg_csr_patch: n + 1 = %lld exceeds int32", (long long)n + 1);
  // checked on its own so that the sum below cannot overflow
  if (nnz > INT32_MAX || nnz + n_pos > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "wg_csr_patch: nnz + n_pos = %lld + %lld exceeds int32", (long long)nnz,
                (long long)n_pos);
  if (!indptr || !out_indptr || !nnz_host) return fail(WG_ERR_INVALID, "wg_csr_patch: NULL indptr / out_indptr / nnz_host");
  if (nnz > 0 && !indices) return fail(WG_ERR_INVALID, "wg_csr_patch: NULL indices with nnz=%lld", (long long)nnz);
  if (n_pos > 0 && (!a_new || !base_pos))
    return fail(WG_ERR_INVALID, "wg_csr_patch: NULL a_new / base_pos with n_pos=%lld", (long long)n_pos);
  if (capacity < nnz + n_pos)
    return fail(WG_ERR_INVALID, "wg_csr_patch: capacity %lld below nnz + n_pos = %lld", (long long)capacity,
                (long long)(nnz + n_pos));
  if (nnz + n_pos > 0 && (!out_indices || !out_values))
    return fail(WG_ERR_INVALID, "wg_csr_patch: NULL out_indices / out_values with capacity %lld", (long long)capacity);
  hipStream_t stream = as_stream(stream_);
  const int rows1 = (int)(n + 1);
  int64_t* lnull = nullptr;
  size_t scan_bytes = 0;
  WG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, lnull, lnull, rows1, stream));
  // one block: [lens n + 1 | cub]
  const size_t o_cub = align256(sizeof(int64_t) * rows1), total = o_cub + align256(scan_bytes);
  DeviceBlock blk;
  WG_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&blk.p), total));
  int64_t* lens = reinterpret_cast<int64_t*>(blk.p);
  hipLaunchKernelGGL(csr_patch_len_kernel, dim3((unsigned)ceil_div(n + 1, kBlock)), dim3(kBlock), 0, stream, v, a_new,
                     base_pos, lens);
  WG_LAUNCH_CHECK();
  WG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(blk.p + o_cub, scan_bytes, lens, out_indptr, rows1, stream));
  if (nnz + n_pos > 0) {
    hipLaunchKernelGGL(csr_patch_copy_kernel, dim3((unsigned)ceil_div(nnz + n_pos, kBlock)), dim3(kBlock), 0, stream,
                       v, nnz, a_new, base_pos, out_indptr, out_indices, out_values, capacity);
    WG_LAUNCH_CHECK();
  }
  int64_t nnz_new = 0;
  WG_HIP_TRY(hipMemcpyAsync(&nnz_new, out_indptr + n, sizeof(nnz_new), hipMemcpyDeviceToHost, stream));
  WG_HIP_TRY(hipStreamSynchronize(stream));
  *nnz_host = nnz_new;
  return WG_OK;
}

}  // extern "C"
