// simcalib.hip -- the similarity temperature of the SimCalib calibrator (reference calibration/SimCalib.py:49-58,
// :91-105).  The reference normalises the latent rows, multiplies them with the normalised validation bank into an
// (N, N_val) cosine matrix, takes softmax(. / tau) over every row and dots the weights with 1 / (confidence + eps);
// autograd keeps the matrix and its softmax.  With
//
//     a_i = x_i / max(|x_i|, 1e-12)     s_ij = a_i . b_j     w_ij = softmax_j(s_ij / tau)     t_i = sum_j w_ij v_j
//
// this is attention with a value vector of width one, and it is computed here flash-style: no (n, m) buffer exists,
// forward (wg_simcalib_forward) or backward (wg_simcalib_backward).
//
// Decomposition.  A workgroup of four waves owns 128 rows of X, a wave 32 of them.  The wave keeps its normalised
// rows in registers as the operand of v_mfma_f32_32x32x2_f32 (one register per two columns of the row: lane l holds
// a[row l & 31][2 kk + (l >> 5)]); the row norm is taken while they are loaded (float64 sum of squares, one
// rounding to float32), so X is read once and never rewritten.  The workgroup walks the bank in tiles of 32 rows,
// staged in LDS (two buffers up to d = 128, one above) and shared by the four waves.  A tile's similarities are the
// TRANSPOSED product S^T = B_tile . A^T: the accumulator then has the latent row on the lane (l & 31) and 16 bank
// rows in its registers, so the softmax runs per lane with no cross-lane step inside the loop.  Each lane keeps a
// running maximum, denominator and numerator over its half of the bank rows (exp on the VALU in float32, the two sums
// in float64 so that a weight near 1 does not round the small ones away, both rescaled when the maximum moves: right
// for any tau > 0 and for a similarity that rounding lifts above 1); the two lanes of a row meet once at the end,
// lower half first.
//
// Backward.  ga_i = (g_i / tau) sum_j w_ij (v_j - t_i) b_j: the tile's similarities are recomputed (the same
// instructions in the same order as the forward, so exp(s / tau - max) <= 1 holds bitwise), the weights come from
// the saved row maximum and float64 denominator, t_i from the saved float64 quotient, and the accumulator P^T, still with the latent row on the lane, is the A
// operand of the second product ga += P . B_tile as it stands (k-step r takes register r: bank rows
// (r & 3) + 8 (r >> 2) and that + 4 of the tile).  The epilogue applies F.normalize's Jacobian as torch
// differentiates it: gx_i = (ga_i - a_i (a_i . ga_i)) / |x_i| when |x_i| >= 1e-12 (clamp_min passes its gradient at
// equality), else ga_i / 1e-12.  The row dot is float64, met in a butterfly over the 32 lanes of a half wave.
//
// Order.  Every sum has a fixed order (k ascending inside the MFMA chains, bank tiles ascending, registers
// ascending, lane halves lower first); bank rows are never split over workgroups; no float atomics: the same input
// gives the same bits.  A NaN in row i of X stays in t_i and gx_i (the row is a lane of the first product and a row
// of the second).
//
// Limits.  1 <= d <= kSimMaxD = 256 (the row operand and, backward, the d-wide gradient tile live in registers;
// wider is WG_ERR_UNSUPPORTED); d is padded with zero columns to 32, 64, 128 or 256.
#include <climits>
#include <cmath>
#include <cstdint>

#include "internal.h"

namespace wg {
namespace {

constexpr int kSimMaxD = 256;
constexpr int kSimRows = 128;      // rows of X per workgroup: 32 per wave
constexpr int kSimTile = 32;       // bank rows per tile
constexpr float kNormEps = 1e-12f; // F.normalize's eps

using f32x16 = __attribute__((ext_vector_type(16))) float;

template <int DP>
struct SimCfg {
  static constexpr int DK = DP / 2;             // k-steps of the first product = registers of the row operand
  static constexpr int LD = DP + 2;             // LDS row stride in floats: lanes (j, h) hit 64 distinct banks
  static constexpr int NBUF = DP <= 128 ? 2 : 1;
  static constexpr int NC = DP / 32;            // 32-column chunks of the gradient tile
  static constexpr int TILE = kSimTile * LD;    // floats per buffer
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// bank row of register r in lane half h (the C/D map of the 32x32 MFMA shapes)
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Bank rows [j0, j0 + 32) into tile[j * LD + k] (rows >= m and columns >= d as zeros), their v into vt.
template <int DP>
__device__ inline void stage_tile(float* __restrict__ tile, float* __restrict__ vt, const float* __restrict__ B,
                                  const float* __restrict__ v, int64_t j0, int64_t m, int d, bool vec) {
  constexpr int LD = SimCfg<DP>::LD;
  const int tid = threadIdx.x;
  if (vec) {
    constexpr int Q = DP / 4;
    for (int idx = tid; idx < kSimTile * Q; idx += kBlock) {
      const int j = idx / Q, k = (idx - j * Q) * 4;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j0 + j < m && k < d) {
        WG_DCHECK((j0 + j) * d + k + 3 < m * d, "simcalib: bank element %lld of %lld", (long long)((j0 + j) * d + k + 3),
                  (long long)(m * d));
        val = *reinterpret_cast<const float4*>(B + (j0 + j) * d + k);
      }
      WG_DCHECK(j * LD + k + 3 < SimCfg<DP>::TILE, "simcalib: LDS float %d of %d", j * LD + k + 3, SimCfg<DP>::TILE);
      float* o = tile + j * LD + k;
      o[0] = val.x;
      o[1] = val.y;
      o[2] = val.z;
      o[3] = val.w;
    }
  } else {
    for (int idx = tid; idx < kSimTile * DP; idx += kBlock) {
      const int j = idx / DP, k = idx - j * DP;
      float val = 0.f;
      if (j0 + j < m && k < d) {
        WG_DCHECK((j0 + j) * d + k < m * d, "simcalib: bank element %lld of %lld", (long long)((j0 + j) * d + k),
                  (long long)(m * d));
        val = B[(j0 + j) * d + k];
      }
      WG_DCHECK(j * LD + k < SimCfg<DP>::TILE, "simcalib: LDS float %d of %d", j * LD + k, SimCfg<DP>::TILE);
      tile[j * LD + k] = val;
    }
  }
  if (tid < kSimTile) vt[tid] = (j0 + tid < m) ? v[j0 + tid] : 0.f;
}

// The wave's 32 rows as the MFMA operand: xa[kk] = a[row][2 kk + h], and the row's norm (both lanes of a row).
template <int DP>
__device__ inline float load_rows(float (&xa)[SimCfg<DP>::DK], const float* __restrict__ X, int64_t row, int64_t n,
                                  int d, int h) {
  constexpr int DK = SimCfg<DP>::DK;
  const bool valid = row < n;
  double ss = 0.0;
#pragma unroll
  for (int kk = 0; kk < DK; ++kk) {
    const int k = 2 * kk + h;
    float x = 0.f;
    if (valid && k < d) {
      WG_DCHECK(row * d + k < n * d, "simcalib: latent element %lld of %lld", (long long)(row * d + k),
                (long long)(n * d));
      x = X[row * d + k];
    }
    xa[kk] = x;
    ss += (double)x * (double)x;
  }
  const double other = __shfl_xor(ss, 32, 64);
  ss = h == 0 ? ss + other : other + ss;   // lower half first in both lanes
  const float nrm = (float)sqrt(ss);
  const float c = fmaxf(nrm, kNormEps);
#pragma unroll
  for (int kk = 0; kk < DK; ++kk) xa[kk] = xa[kk] / c;
  return nrm;
}

// S^T tile: lane (i = l & 31, h) gets s[i][acc_row(r, h)] in register r
template <int DP>
__device__ __forceinline__ f32x16 sim_tile(const float* __restrict__ tile, const float (&xa)[SimCfg<DP>::DK], int lane) {
  constexpr int LD = SimCfg<DP>::LD;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* brow = tile + (lane & 31) * LD + (lane >> 5);
#pragma unroll
  for (int kk = 0; kk < SimCfg<DP>::DK; ++kk)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(brow[2 * kk], xa[kk], acc, 0, 0, 0);
  return acc;
}

template <int DP>
__global__ __launch_bounds__(kBlock) void simcalib_fwd_kernel(int64_t n, int64_t m, int d, bool vec,
                                                              const float* __restrict__ X, const float* __restrict__ B,
                                                              const float* __restrict__ v, float inv_tau,
                                                              float* __restrict__ t, double* __restrict__ stats) {
  using C = SimCfg<DP>;
  __shared__ float tiles[C::NBUF * C::TILE];
  __shared__ float vts[C::NBUF * kSimTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  const int64_t row = (int64_t)blockIdx.x * kSimRows + wave * 32 + (lane & 31);
  float xa[C::DK];
  load_rows<DP>(xa, X, row, n, d, h);

  float mrun = -INFINITY;
  double den = 0.0, num = 0.0;   // float32 exp, float64 sums: a dominant weight does not round the others away
  const int64_t n_tiles = (m + kSimTile - 1) / kSimTile;
  if (C::NBUF == 2) {
    stage_tile<DP>(tiles, vts, B, v, 0, m, d, vec);
    __syncthreads();
  }
  for (int64_t tix = 0; tix < n_tiles; ++tix) {
    const int64_t j0 = tix * kSimTile;
    int buf = 0;
    if (C::NBUF == 2) {
      buf = (int)(tix & 1);
      if (tix + 1 < n_tiles)
        stage_tile<DP>(tiles + (buf ^ 1) * C::TILE, vts + (buf ^ 1) * kSimTile, B, v, j0 + kSimTile, m, d, vec);
    } else {
      __syncthreads();   // the readers of the previous tile are done
      stage_tile<DP>(tiles, vts, B, v, j0, m, d, vec);
      __syncthreads();
    }
    const float* tile = tiles + buf * C::TILE;
    const float* vt = vts + buf * kSimTile;
    const f32x16 acc = sim_tile<DP>(tile, xa, lane);
    float x[16];
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      x[r] = (j0 + acc_row(r, h) < m) ? acc[r] * inv_tau : -INFINITY;
      mt = fmaxf(mt, x[r]);
    }
    const float mnew = fmaxf(mrun, mt);
    const float ms = mnew == -INFINITY ? 0.f : mnew;   // nothing seen yet by this lane: every term is exp(-inf) = 0
    const float scale = expf(mrun - ms);
    double dt = 0.0, nt = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const double e = (double)expf(x[r] - ms);
      dt += e;
      nt = fma(e, (double)vt[acc_row(r, h)], nt);
    }
    den = fma(den, (double)scale, dt);
    num = fma(num, (double)scale, nt);
    mrun = mnew;
    if (C::NBUF == 2) __syncthreads();   // the next tile is staged, this one is read
  }
  // the two lanes of a row, lower half first
  const float mo = __shfl_xor(mrun, 32, 64);
  const double deno = __shfl_xor(den, 32, 64), numo = __shfl_xor(num, 32, 64);
  const float m0 = h ? mo : mrun, m1 = h ? mrun : mo;
  const double d0 = h ? deno : den, d1 = h ? den : deno;
  const double n0 = h ? numo : num, n1 = h ? num : numo;
  const float mx = fmaxf(m0, m1);
  const float ms = mx == -INFINITY ? 0.f : mx;
  const double e0 = (double)expf(m0 - ms), e1 = (double)expf(m1 - ms);
  const double dd = fma(d1, e1, d0 * e0);
  const double nn = fma(n1, e1, n0 * e0);
  if (h == 0 && row < n) {
    WG_DCHECK(row >= 0 && row < n, "simcalib: row %lld of %lld", (long long)row, (long long)n);
    const double td = nn / dd;
    t[row] = (float)td;
    stats[3 * row] = (double)mx;
    stats[3 * row + 1] = dd;
    stats[3 * row + 2] = td;
  }
}

template <int DP>
__global__ __launch_bounds__(kBlock) void simcalib_bwd_kernel(int64_t n, int64_t m, int d, bool vec,
                                                              const float* __restrict__ X, const float* __restrict__ B,
                                                              const float* __restrict__ v, float inv_tau,
                                                              const double* __restrict__ stats,
                                                              const float* __restrict__ g, float* __restrict__ gx) {
  using C = SimCfg<DP>;
  __shared__ float tiles[C::NBUF * C::TILE];
  __shared__ float vts[C::NBUF * kSimTile];
  __shared__ float nrms[kSimRows];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * kSimRows + wave * 32;
  const int64_t row = row0 + (lane & 31);
  float xa[C::DK];
  const float nrm = load_rows<DP>(xa, X, row, n, d, h);
  if (h == 0) nrms[wave * 32 + (lane & 31)] = nrm;
  // a row past the end: a = 0, so s = 0 and exp(0 - 0) * (v - 0) * 0 = 0
  // t_i as a float32 pair and the denominator in float64: the weights and v_j - t_i then agree with the forward's
  // sums, so sum_j w_ij (v_j - t_i), zero in exact arithmetic, keeps no systematic residue along the bank's mean
  float mi = 0.f, thi = 0.f, tlo = 0.f, coef = 0.f;
  if (row < n) {
    mi = (float)stats[3 * row];
    const double td = stats[3 * row + 2];
    thi = (float)td;
    tlo = (float)(td - (double)thi);
    coef = (float)((double)g[row] * (double)inv_tau / stats[3 * row + 1]);
  }
  f32x16 ga[C::NC];
#pragma unroll
  for (int cc = 0; cc < C::NC; ++cc)
#pragma unroll
    for (int r = 0; r < 16; ++r) ga[cc][r] = 0.f;

  const int64_t n_tiles = (m + kSimTile - 1) / kSimTile;
  if (C::NBUF == 2) stage_tile<DP>(tiles, vts, B, v, 0, m, d, vec);
  __syncthreads();   // nrms too
  for (int64_t tix = 0; tix < n_tiles; ++tix) {
    const int64_t j0 = tix * kSimTile;
    int buf = 0;
    if (C::NBUF == 2) {
      buf = (int)(tix & 1);
      if (tix + 1 < n_tiles)
        stage_tile<DP>(tiles + (buf ^ 1) * C::TILE, vts + (buf ^ 1) * kSimTile, B, v, j0 + kSimTile, m, d, vec);
    } else {
      if (tix > 0) __syncthreads();
      stage_tile<DP>(tiles, vts, B, v, j0, m, d, vec);
      __syncthreads();
    }
    const float* tile = tiles + buf * C::TILE;
    const float* vt = vts + buf * kSimTile;
    f32x16 p = sim_tile<DP>(tile, xa, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jl = acc_row(r, h);
      const float x = (j0 + jl < m) ? p[r] * inv_tau : -INFINITY;
      p[r] = expf(x - mi) * ((vt[jl] - thi) - tlo) * coef;
    }
    // ga += P . B_tile: register r is the k-step over the tile's rows acc_row(r, 0) and acc_row(r, 1)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* brow = tile + acc_row(r, h) * C::LD + (lane & 31);
#pragma unroll
      for (int cc = 0; cc < C::NC; ++cc)
        ga[cc] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[r], brow[cc * 32], ga[cc], 0, 0, 0);
    }
    if (C::NBUF == 2) __syncthreads();
  }
  // ga[cc][r] is row acc_row(r, h) of the wave, column cc * 32 + (lane & 31)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int il = acc_row(r, h);
    const int64_t i = row0 + il;
    WG_DCHECK(wave * 32 + il < kSimRows, "simcalib: norm slot %d of %d", wave * 32 + il, kSimRows);
    const float ni = nrms[wave * 32 + il];
    const float c = fmaxf(ni, kNormEps);
    float av[C::NC];
    double dot = 0.0;
#pragma unroll
    for (int cc = 0; cc < C::NC; ++cc) {
      const int col = cc * 32 + (lane & 31);
      const float xv = (i < n && col < d) ? X[i * d + col] : 0.f;
      av[cc] = xv / c;
      dot += (double)av[cc] * (double)ga[cc][r];
    }
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) dot += __shfl_xor(dot, off, 64);
    const float fd = (float)dot;
#pragma unroll
    for (int cc = 0; cc < C::NC; ++cc) {
      const int col = cc * 32 + (lane & 31);
      if (i < n && col < d) {
        WG_DCHECK(i * d + col < n * d, "simcalib: gradient element %lld of %lld", (long long)(i * d + col),
                  (long long)(n * d));
        gx[i * d + col] = (ni >= kNormEps) ? (ga[cc][r] - av[cc] * fd) / ni : ga[cc][r] / kNormEps;
      }
    }
  }
}

int check_args(const char* who, int64_t n, int64_t m, int64_t d, double tau, bool null_ptr) {
  if (n <= 0 || m <= 0 || d <= 0)
    return fail(WG_ERR_INVALID, "%s: n, m and d must be positive (n=%lld m=%lld d=%lld)", who, (long long)n,
                (long long)m, (long long)d);
  if (!(tau > 0.0) || !std::isfinite(tau))
    return fail(WG_ERR_INVALID, "%s: tau must be positive and finite (tau=%g)", who, tau);
  if (!std::isfinite((float)(1.0 / tau)))
    return fail(WG_ERR_INVALID, "%s: 1 / tau overflows float32 (tau=%g)", who, tau);
  if (null_ptr) return fail(WG_ERR_INVALID, "%s: NULL pointer with n=%lld m=%lld d=%lld", who, (long long)n,
                            (long long)m, (long long)d);
  if (d > kSimMaxD)
    return fail(WG_ERR_UNSUPPORTED, "%s: d=%lld exceeds the %d columns a row tile holds in registers", who,
                (long long)d, kSimMaxD);
  if (n > INT32_MAX || m > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld / m=%lld exceed int32", who, (long long)n, (long long)m);
  return WG_OK;
}

int padded_d(int64_t d) { return d <= 32 ? 32 : d <= 64 ? 64 : d <= 128 ? 128 : 256; }

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_simcalib_max_d(void) { return kSimMaxD; }

int wg_simcalib_forward(int64_t n, int64_t m, int64_t d, const float* x, const float* bank, const float* inv_conf,
                        double tau, float* t, double* stats, void* stream_) {
  if (int rc = check_args("wg_simcalib_forward", n, m, d, tau, !x || !bank || !inv_conf || !t || !stats)) return rc;
  hipStream_t stream = as_stream(stream_);
  const bool vec = (d % 4 == 0) && aligned16(bank);
  const dim3 grid((unsigned)ceil_div(n, kSimRows));
  const float inv_tau = (float)(1.0 / tau);
#define WG_SIM_FWD(DP)                                                                                            \
  case DP:                                                                                                        \
    hipLaunchKernelGGL((simcalib_fwd_kernel<DP>), grid, dim3(kBlock), 0, stream, n, m, (int)d, vec, x, bank,      \
                       inv_conf, inv_tau, t, stats);                                                              \
    break;
  switch (padded_d(d)) {
    WG_SIM_FWD(32)
    WG_SIM_FWD(64)
    WG_SIM_FWD(128)
    default:
      WG_SIM_FWD(256)
  }
#undef WG_SIM_FWD
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_simcalib_backward(int64_t n, int64_t m, int64_t d, const float* x, const float* bank, const float* inv_conf,
                         double tau, const double* stats, const float* g, float* gx, void* stream_) {
  if (int rc = check_args("wg_simcalib_backward", n, m, d, tau, !x || !bank || !inv_conf || !stats || !g || !gx))
    return rc;
  if (gx == x) return fail(WG_ERR_INVALID, "wg_simcalib_backward: gx must not alias x");
  hipStream_t stream = as_stream(stream_);
  const bool vec = (d % 4 == 0) && aligned16(bank);
  const dim3 grid((unsigned)ceil_div(n, kSimRows));
  const float inv_tau = (float)(1.0 / tau);
#define WG_SIM_BWD(DP)                                                                                            \
  case DP:                                                                                                        \
    hipLaunchKernelGGL((simcalib_bwd_kernel<DP>), grid, dim3(kBlock), 0, stream, n, m, (int)d, vec, x, bank,      \
                       inv_conf, inv_tau, stats, g, gx);                                                          \
    break;
  switch (padded_d(d)) {
    WG_SIM_BWD(32)
    WG_SIM_BWD(64)
    WG_SIM_BWD(128)
    default:
      WG_SIM_BWD(256)
  }
#undef WG_SIM_BWD
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // extern "C"
