// sddmm.hip -- edge-position gradients of the base model's propagation.
// The reference attacks differentiate CompatibleGCN.forward (src/gnn/model.py:43-52) through a
// dense (N,N) adjacency leaf and read row t and column t of the result
// (calib_attack/calib_fga.py:864-881).  For y = adj_norm(A) @ x with upstream gradient g,
//     d loss / d a_ij = ( g_i . x_j  -  g_i . y_i ) / deg_i        at every (i, j), stored or not,
// so the gradient at a LIST of positions is a sampled dense-dense product (SDDMM) plus a per-row
// term:  wg_sddmm(rows, cols, g, x, row_term = wg_rowdot(g, y), row_scale = 1 / deg).
//
// One kernel serves both entry points.  A sub-group of W = clamp(pow2ceil(ceil(F / 4)), 1, 64)
// lanes owns one pair, so a wave works on 64 / W pairs at once.  Each lane reads 16 bytes of both
// rows per trip when F % 4 == 0 and both bases are 16-byte aligned (every row then starts on a
// 16-byte boundary), coalesced dwords otherwise, and loops when the row is longer than one trip.
// Products and sums are float64 (a product of two float32 is exact there), each lane in ascending
// column order, then a fixed shuffle tree over the sub-group: no atomics, bitwise reproducible.
#include <algorithm>
#include <climits>
#include <cstdint>

#include "internal.h"

namespace wg {
namespace {

template <int W, bool VEC, bool IDENT>
__global__ __launch_bounds__(kBlock) void sddmm_kernel(int64_t n_pairs, const int32_t* __restrict__ rows,
                                                       const int32_t* __restrict__ cols, int64_t F,
                                                       const float* __restrict__ A, int64_t n_a,
                                                       const float* __restrict__ B, int64_t n_b,
                                                       const float* __restrict__ row_term,
                                                       const float* __restrict__ row_scale, float* __restrict__ out) {
  constexpr int kPairs = kBlock / W;  // pairs per workgroup
  const int sub = threadIdx.x & (W - 1);
  const int slot = threadIdx.x / W;
  // the trip count is uniform over the workgroup; a sub-group past the end idles with acc = 0
  for (int64_t base = (int64_t)blockIdx.x * kPairs; base < n_pairs; base += (int64_t)gridDim.x * kPairs) {
    const int64_t p = base + slot;
    const bool active = p < n_pairs;
    int64_t r = 0;
    double acc = 0.0;
    if (active) {
      int64_t c;
      if (IDENT) {
        r = c = p;
      } else {
        r = rows[p];
        c = cols[p];
      }
      WG_DCHECK(r >= 0 && r < n_a, "sddmm pair %lld: row %lld outside [0, %lld)", (long long)p, (long long)r,
                (long long)n_a);
      WG_DCHECK(c >= 0 && c < n_b, "sddmm pair %lld: column %lld outside [0, %lld)", (long long)p, (long long)c,
                (long long)n_b);
      const float* a = A + r * F;  // 64-bit: 169 343 rows x 1 433 columns already exceed 2^31 elements
      const float* b = B + c * F;
      if (VEC) {
        const float4* a4 = reinterpret_cast<const float4*>(a);
        const float4* b4 = reinterpret_cast<const float4*>(b);
        const int64_t nq = F >> 2;
        for (int64_t q = sub; q < nq; q += W) {
          const float4 u = a4[q];
          const float4 v = b4[q];
          acc += (double)u.x * (double)v.x;
          acc += (double)u.y * (double)v.y;
          acc += (double)u.z * (double)v.z;
          acc += (double)u.w * (double)v.w;
        }
      } else {
        for (int64_t f = sub; f < F; f += W) acc += (double)a[f] * (double)b[f];
      }
    }
#pragma unroll
    for (int off = W >> 1; off >= 1; off >>= 1) acc += __shfl_down(acc, off, W);
    if (active && sub == 0) {
      if (row_term) acc -= (double)row_term[r];
      if (row_scale) acc *= (double)row_scale[r];
      out[p] = (float)acc;
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <bool IDENT>
int launch_sddmm(int64_t n_pairs, const int32_t* rows, const int32_t* cols, int64_t F, const float* A, int64_t n_a,
                 const float* B, int64_t n_b, const float* row_term, const float* row_scale, float* out,
                 hipStream_t stream) {
  int W = 1;
  while (W < 64 && W < ceil_div(F, 4)) W <<= 1;
  const bool vec = (F % 4 == 0) && aligned16(A) && aligned16(B);
  const int64_t blocks = std::min<int64_t>(ceil_div(n_pairs, kBlock / W), INT32_MAX);
#define WG_SDDMM_CASE(w)                                                                                        \
  case w:                                                                                                       \
    if (vec)                                                                                                    \
      hipLaunchKernelGGL((sddmm_kernel<w, true, IDENT>), dim3((unsigned)blocks), dim3(kBlock), 0, stream,      \
                         n_pairs, rows, cols, F, A, n_a, B, n_b, row_term, row_scale, out);                     \
    else                                                                                                        \
      hipLaunchKernelGGL((sddmm_kernel<w, false, IDENT>), dim3((unsigned)blocks), dim3(kBlock), 0, stream,     \
                         n_pairs, rows, cols, F, A, n_a, B, n_b, row_term, row_scale, out);                     \
    break;
  switch (W) {
    WG_SDDMM_CASE(1)
    WG_SDDMM_CASE(2)
    WG_SDDMM_CASE(4)
    WG_SDDMM_CASE(8)
    WG_SDDMM_CASE(16)
    WG_SDDMM_CASE(32)
    WG_SDDMM_CASE(64)
  }
#undef WG_SDDMM_CASE
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_sddmm(int64_t n_pairs, const int32_t* rows, const int32_t* cols, int64_t F, const float* A, int64_t n_a,
             const float* B, int64_t n_b, const float* row_term, const float* row_scale, float* out, void* stream_) {
  if (n_pairs < 0 || n_a < 0 || n_b < 0)
    return fail(WG_ERR_INVALID, "wg_sddmm: negative size (n_pairs=%lld n_a=%lld n_b=%lld)", (long long)n_pairs,
                (long long)n_a, (long long)n_b);
  if (F < 1) return fail(WG_ERR_INVALID, "wg_sddmm: F must be >= 1 (F=%lld)", (long long)F);
  if (n_pairs == 0) return WG_OK;
  if (!rows || !cols || !A || !B || !out)
    return fail(WG_ERR_INVALID, "wg_sddmm: NULL rows / cols / A / B / out with n_pairs=%lld", (long long)n_pairs);
  if (n_a == 0 || n_b == 0)
    return fail(WG_ERR_INVALID, "wg_sddmm: %lld pairs into an empty operand (n_a=%lld n_b=%lld)", (long long)n_pairs,
                (long long)n_a, (long long)n_b);
  return launch_sddmm<false>(n_pairs, rows, cols, F, A, n_a, B, n_b, row_term, row_scale, out, as_stream(stream_));
}

int wg_rowdot(int64_t n, int64_t F, const float* A, const float* B, float* out, void* stream_) {
  if (n < 0) return fail(WG_ERR_INVALID, "wg_rowdot: negative size (n=%lld)", (long long)n);
  if (F < 1) return fail(WG_ERR_INVALID, "wg_rowdot: F must be >= 1 (F=%lld)", (long long)F);
  if (n == 0) return WG_OK;
  if (!A || !B || !out) return fail(WG_ERR_INVALID, "wg_rowdot: NULL A / B / out with n=%lld", (long long)n);
  return launch_sddmm<true>(n, nullptr, nullptr, F, A, n, B, n, nullptr, nullptr, out, as_stream(stream_));
}

}  // extern "C"
