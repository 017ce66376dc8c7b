// calib.hip -- SURVEY section 8(f): the evaluation the reference's harness runs after every calibrator and every
// attack.  evaluate_calibration / evaluate_calibration_probs (benchmark_calibration_methods.py:87-158) and
// evaluate_model_calibration (ugca_calib_attack.py:78-104) take probs[test_mask] to the host and loop over
// classes and bins there (utils/ece.py:8-89); ece_chart (utils/ece.py:91-133) bins the same columns again for
// sklearn's calibration_curve.  Here one pass over the listed rows of G sets of outputs gives
//
//     table   (G, C + 1, n_bins + 2, 3) uint64: per class and bin the count, the count of rows labelled with the
//             class and sum p in fixed point (quantum 2^-40); slice C is the top-label table (p = the row's maximum,
//             label count = rows whose first maximal column is the label); slot n_bins holds p <= edges[0] (its
//             third word counts the exact zeros), slot n_bins + 1 everything else (p > edges[n_bins], NaN; its third
//             word counts NaN and +inf)
//     scalars (G, 8) float64: rows taken, rows with every p finite, and over those the correct count, sum max p,
//             sum -log p_label, the rows that sum used, sum_c (p_c - [label == c])^2; then the rows refused
//
// and wg_calib_ece turns the table into utils/ece.py:44-60 per class.
//
// Decomposition.  A wave per row, as scale.hip: lane l owns the columns l, l + 64, l + 128, l + 192 (C <= 256).  The
// rows of the list are cut into FIXED chunks of kChunkRows = 256 entries; a workgroup of 16 waves takes whole chunks,
// wave w the entries w, w + 16, ... of a chunk in ascending order (lane k of the wave fetches entry k's row id and
// label once, and a row's values are loaded while the row before it is binned).  The table is integers: a workgroup
// bins into an LDS copy with integer LDS adds and adds its non-zero cells to the global table with integer global
// adds when it is done (tables above kLdsCells words go to the global table directly); integer sums commute, so the
// table's bits depend on the inputs alone.  (Slabs in the workspace added by the second launch measured slower at the
// ogbn-arxiv size, 122 against 100 us per call: DESIGN.md 9, profiles/r24.)  The float64 sums leave one partial
// vector per chunk, the waves' sums added in wave order; a second launch adds the chunk vectors in chunk order (the
// scheme of wg_scale_epoch): the grid never shows.  No float atomics.
//
// Arithmetic.  p is a float32: the input (PROBS), (float)exp((double)x) (EXP: what the harness does to whatever a
// model returns, benchmark_calibration_methods.py:102-103) or the float64 softmax of the row rounded once (LOGITS).
// It is compared as a double with the caller's float64 edges exactly as np.digitize(p, edges, right=True) - 1 does
// (utils/ece.py:39-40): the kernel never recomputes an edge.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "internal.h"

namespace wg {
namespace {

constexpr int kProbs = WG_CALIB_PROBS, kExp = WG_CALIB_EXP, kLogits = WG_CALIB_LOGITS;
constexpr int kMaxC = 256;            // four columns per lane
constexpr int kMaxBins = 64;
constexpr int64_t kMaxRows = 1 << 23; // 2^23 rows of p <= 1 at quantum 2^-40 stay below 2^63
constexpr int kChunkRows = 256;       // listed rows per float64 partial vector (wg_scale_epoch's chunk)
constexpr int kCalibBlock = 1024;    // 16 waves: a chunk is the unit of parallelism, so its rows go to many waves
constexpr int kWaves = kCalibBlock / 64;
constexpr int kRowsPerWave = kChunkRows / kWaves;
constexpr int kNQ = kMaxC / 64;
constexpr int kMaxGrid = 1024;
constexpr int kMaxSets = 4096;
constexpr int kLdsCells = 5120;       // uint64 words of the LDS table (40 KB)
constexpr int kNS = 8;                // scalars per set
constexpr double kQuantum = 1099511627776.0;   // 2^40

enum : int { kSRows = 0, kSFinite, kSCorrect, kSMaxP, kSNll, kSNllRows, kSBrier, kSRefused };

__host__ __device__ inline int64_t table_cells(int64_t C, int64_t n_bins) { return (C + 1) * (n_bins + 2) * 3; }
inline int64_t n_chunks_of(int64_t rows) { return ceil_div(rows, kChunkRows); }

struct BinArgs {
  int64_t n, n_rows, n_chunks;
  int C, n_bins;
  const float* out;        // this launch's G sets, (G, n, C)
  const int64_t* labels;
  const int64_t* rows;
  const double* edges;
  double* partial;         // (G, n_chunks, kNS)
  unsigned long long* table;
};

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
__device__ inline bool better(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na != nb) return na;
  if (!na && a != b) return a > b;
  return ia < ib;
}

// np.digitize(p, edges, right=True) - 1 on the staged edges: the count of edges below p, less one; -1 -> the slot
// n_bins (p <= edges[0]), n_bins and a NaN -> the slot n_bins + 1
__device__ inline int bin_slot(double p, const double* ed, int n_bins) {
  if (p != p) return n_bins + 1;
  int lo = 0, hi = n_bins + 1;           // edges [0, lo) are below p, edges [hi, n_bins] are not
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ed[mid] < p) lo = mid + 1; else hi = mid;
  }
  WG_DCHECK(lo >= 0 && lo <= n_bins + 1, "calib: %d edges of %d below p", lo, n_bins + 1);
  return lo == 0 ? n_bins : lo == n_bins + 1 ? n_bins + 1 : lo - 1;
}

// the third word of a cell: sum p in fixed point in a bin, the exact zeros below, NaN / +inf above
__device__ inline unsigned long long third_word(float p, int slot, int n_bins) {
  if (slot < n_bins) return (unsigned long long)rint((double)p * kQuantum);
  if (slot == n_bins) return p == 0.0f ? 1ull : 0ull;
  return (p != p || p == INFINITY) ? 1ull : 0ull;
}

template <bool LDS>
__device__ inline void cell_add(unsigned long long* lds, unsigned long long* glob, int64_t cell, int64_t cells,
                                bool labelled, unsigned long long third) {
  WG_DCHECK(cell >= 0 && cell + 2 < cells, "calib: table cell %lld of %lld", (long long)cell, (long long)cells);
  unsigned long long* t = (LDS ? lds : glob) + cell;
  atomicAdd(t, 1ull);
  if (labelled) atomicAdd(t + 1, 1ull);
  if (third) atomicAdd(t + 2, third);
}

template <int KIND, bool LDS>
__global__ __launch_bounds__(kCalibBlock) void calib_bins_kernel(BinArgs a) {
  __shared__ unsigned long long tab[LDS ? kLdsCells : 1];
  __shared__ double ed[kMaxBins + 1];
  __shared__ double red[kWaves * kNS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = a.C, nb = a.n_bins;
  const int64_t g = blockIdx.y, cells = table_cells(C, nb);
  const float* out = a.out + g * a.n * C;
  unsigned long long* gtab = a.table + g * cells;
  for (int i = threadIdx.x; i <= nb; i += kCalibBlock) ed[i] = a.edges[i];
  if constexpr (LDS) {
    for (int64_t i = threadIdx.x; i < cells; i += kCalibBlock) tab[i] = 0ull;
  }
  __syncthreads();
  for (int64_t ch = blockIdx.x; ch < a.n_chunks; ch += gridDim.x) {
    double acc[kNS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // wave-uniform
    const int64_t r0 = ch * kChunkRows;
    const int64_t r1 = a.n_rows < r0 + kChunkRows ? a.n_rows : r0 + kChunkRows;
    // the wave's entries r0 + wave + kWaves k: lane k fetches entry k's row id and label once, and the values of
    // entry k + 1 are on their way while entry k is binned (a wave has a row's dependent loads to itself otherwise)
    int64_t my_i = -1, my_y = -1;
    if (lane < kRowsPerWave && r0 + wave + (int64_t)kWaves * lane < r1) {
      const int64_t r = r0 + wave + (int64_t)kWaves * lane;
      my_i = a.rows ? a.rows[r] : r;
      if (my_i >= 0 && my_i < a.n) my_y = a.labels[my_i];
    }
    float nxt[kNQ];
    auto fetch = [&](int k) {
      const int64_t i = __shfl(my_i, k, 64);
#pragma unroll
      for (int q = 0; q < kNQ; ++q) {
        const int c = lane + 64 * q;
        nxt[q] = (c < C && i >= 0 && i < a.n) ? out[i * C + c] : 0.0f;
      }
    };
    fetch(0);
    for (int k = 0; k < kRowsPerWave && r0 + wave + (int64_t)kWaves * k < r1; ++k) {
      const int64_t i = __shfl(my_i, k, 64), y = __shfl(my_y, k, 64);
      float p[kNQ];
      double x[kNQ];
#pragma unroll
      for (int q = 0; q < kNQ; ++q) {
        x[q] = (double)nxt[q];
        p[q] = nxt[q];
      }
      if (k + 1 < kRowsPerWave) fetch(k + 1);   // an entry past the list has the id -1: nothing is read
      if (i < 0 || i >= a.n) {   // in every build: a row outside the outputs is counted, never read
        acc[kSRefused] += 1.0;
        continue;
      }
      double lse_m = 0.0, lse_s = 1.0;
      if constexpr (KIND == kExp) {
#pragma unroll
        for (int q = 0; q < kNQ; ++q) p[q] = (float)exp(x[q]);
      }
      if constexpr (KIND == kLogits) {
        double mx = -INFINITY;
#pragma unroll
        for (int q = 0; q < kNQ; ++q)
          if (lane + 64 * q < C) mx = fmax(mx, x[q]);
        mx = wave_max(mx);
        double e[kNQ], s = 0.0;
#pragma unroll
        for (int q = 0; q < kNQ; ++q) {
          e[q] = lane + 64 * q < C ? exp(x[q] - mx) : 0.0;   // fmax drops a NaN, the sum brings it back
          s += e[q];
        }
        s = wave_sum(s);
#pragma unroll
        for (int q = 0; q < kNQ; ++q) p[q] = (float)(e[q] / s);
        lse_m = mx, lse_s = s;
      }
      // the row's maximum, its first index, whether every p is finite, the label's terms
      float bv = -INFINITY;
      int bi = INT_MAX;
      bool fin = true;
      double brier = 0.0, nll = 0.0, nll_used = 0.0;
#pragma unroll
      for (int q = 0; q < kNQ; ++q) {
        const int c = lane + 64 * q;
        if (c < C) {
          if (better(p[q], c, bv, bi)) bv = p[q], bi = c;
          fin = fin && (p[q] - p[q] == 0.0f);
          const double d = (double)p[q] - (c == y ? 1.0 : 0.0);
          brier += d * d;
          if (c == y && p[q] > 0.0f) {
            nll_used = 1.0;
            nll = KIND == kLogits ? -((x[q] - lse_m) - log(lse_s)) : KIND == kExp ? -x[q] : -log((double)p[q]);
          }
        }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (better(ov, oi, bv, bi)) bv = ov, bi = oi;
      }
      fin = __all(fin);
      // the table: every column of the row, then (lane 0) the top label
#pragma unroll
      for (int q = 0; q < kNQ; ++q) {
        const int c = lane + 64 * q;
        if (c < C) {
          const int slot = bin_slot((double)p[q], ed, nb);
          cell_add<LDS>(tab, gtab, ((int64_t)c * (nb + 2) + slot) * 3, cells, c == y, third_word(p[q], slot, nb));
        }
      }
      if (lane == 0) {
        const int slot = bin_slot((double)bv, ed, nb);
        cell_add<LDS>(tab, gtab, ((int64_t)C * (nb + 2) + slot) * 3, cells, bi == y, third_word(bv, slot, nb));
      }
      acc[kSRows] += 1.0;
      brier = wave_sum(brier), nll = wave_sum(nll), nll_used = wave_sum(nll_used);
      if (fin) {
        acc[kSFinite] += 1.0;
        acc[kSCorrect] += bi == y ? 1.0 : 0.0;
        acc[kSMaxP] += (double)bv;
        acc[kSNll] += nll;
        acc[kSNllRows] += nll_used;
        acc[kSBrier] += brier;
      }
    }
    // the waves' sums in wave order: the chunk's partial vector
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < kNS; ++k) red[wave * kNS + k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < kNS) {
      double s = red[threadIdx.x];
      for (int w = 1; w < kWaves; ++w) s += red[w * kNS + threadIdx.x];
      a.partial[(g * a.n_chunks + ch) * kNS + threadIdx.x] = s;
    }
    __syncthreads();
  }
  if constexpr (LDS) {
    for (int64_t i = threadIdx.x; i < cells; i += kCalibBlock)
      if (tab[i]) atomicAdd(gtab + i, tab[i]);
  }
}

// the chunk vectors of a set, added in chunk order
__global__ void calib_scalars_kernel(int64_t n_chunks, const double* __restrict__ partial, double* scalars) {
  const int64_t g = blockIdx.x;
  const int k = threadIdx.x;
  if (k >= kNS) return;
  double s = 0.0;
  for (int64_t ch = 0; ch < n_chunks; ++ch) s += partial[(g * n_chunks + ch) * kNS + k];
  scalars[g * kNS + k] = s;
}

// utils/ece.py:44-60 on one (set, class) slice of the table per thread, bins ascending
__global__ void calib_ece_kernel(int C, int n_bins, double n_rows, unsigned long long min_count,
                                 const unsigned long long* __restrict__ table, double* ece_class, double* ece_top) {
  const int64_t g = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > C) return;
  const unsigned long long* t = table + (g * (C + 1) + c) * (int64_t)(n_bins + 2) * 3;
  double ece = 0.0;
  for (int b = 0; b < n_bins; ++b) {
    const unsigned long long cnt = t[3 * b];
    if (cnt < min_count || cnt == 0) continue;
    const double conf = ((double)t[3 * b + 2] / kQuantum) / (double)cnt;
    const double acc = (double)t[3 * b + 1] / (double)cnt;
    ece += fabs(conf - acc) * ((double)cnt / n_rows);
  }
  if (c < C) ece_class[g * C + c] = ece; else ece_top[g] = ece;
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

int check_table_shape(const char* who, int64_t G, int64_t C, int64_t n_bins, int64_t n_rows) {
  if (G < 0 || C < 1 || n_bins < 1 || n_rows < 0)
    return fail(WG_ERR_INVALID, "%s: bad shape (G=%lld C=%lld n_bins=%lld rows=%lld)", who, (long long)G, (long long)C,
                (long long)n_bins, (long long)n_rows);
  if (G > kMaxSets || C > kMaxC || n_bins > kMaxBins || n_rows > kMaxRows)
    return fail(WG_ERR_UNSUPPORTED, "%s: G=%lld C=%lld n_bins=%lld rows=%lld above the limits %d / %d / %d / %lld", who,
                (long long)G, (long long)C, (long long)n_bins, (long long)n_rows, kMaxSets, kMaxC, kMaxBins,
                (long long)kMaxRows);
  return WG_OK;
}

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_calib_chunk_rows(void) { return kChunkRows; }
int wg_calib_max_rows(void) { return (int)kMaxRows; }
int wg_calib_max_classes(void) { return kMaxC; }
int wg_calib_max_bins(void) { return kMaxBins; }

int wg_calib_workspace(int64_t G, int64_t C, int64_t n_bins, int64_t n_rows, int64_t* bytes) {
  if (!bytes) return fail(WG_ERR_INVALID, "wg_calib_workspace: bytes is NULL");
  if (int rc = check_table_shape("wg_calib_workspace", G, C, n_bins, n_rows)) return rc;
  *bytes = std::max<int64_t>(1, G * n_chunks_of(n_rows)) * kNS * (int64_t)sizeof(double);
  return WG_OK;
}

int wg_calib_bins(int64_t G, int64_t n, int64_t C, int32_t kind, const float* out, const int64_t* labels,
                  int64_t n_rows, const int64_t* rows, int32_t n_bins, const double* edges, int32_t n_workgroups,
                  void* workspace, uint64_t* table, double* scalars, void* stream_) {
  static const char* who = "wg_calib_bins";
  if (int rc = check_table_shape(who, G, C, n_bins, n_rows)) return rc;
  if (n < 0 || kind < kProbs || kind > kLogits)
    return fail(WG_ERR_INVALID, "%s: n=%lld, kind %d is none of PROBS 0, EXP 1, LOGITS 2", who, (long long)n, kind);
  if (n > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld exceeds int32", who, (long long)n);
  if (!rows && n_rows != n && n_rows != 0)   // an empty list may come as NULL
    return fail(WG_ERR_INVALID, "%s: no row list, but %lld rows of %lld", who, (long long)n_rows, (long long)n);
  if (n_workgroups < 0 || n_workgroups > kMaxGrid)
    return fail(WG_ERR_INVALID, "%s: n_workgroups=%d outside [0, %d]", who, n_workgroups, kMaxGrid);
  if (G == 0) return WG_OK;
  if (!table || !scalars || !aligned8(table) || !aligned8(scalars))
    return fail(WG_ERR_INVALID, "%s: table / scalars NULL or not 8-byte aligned", who);
  if (n_rows > 0 && (!out || !labels || !edges || !workspace || !aligned8(workspace) || !aligned8(edges) ||
                     !aligned8(labels) || (rows && !aligned8(rows))))
    return fail(WG_ERR_INVALID, "%s: a NULL or misaligned pointer with %lld rows", who, (long long)n_rows);
  hipStream_t stream = as_stream(stream_);
  const int64_t cells = table_cells(C, n_bins);
  WG_HIP_TRY(zero_async(table, (size_t)(G * cells) * sizeof(uint64_t), stream));
  if (n_rows == 0) {
    WG_HIP_TRY(zero_async(scalars, (size_t)(G * kNS) * sizeof(double), stream));
    return WG_OK;
  }
  const int64_t n_chunks = n_chunks_of(n_rows);
  const BinArgs a{n, n_rows, n_chunks, (int)C, (int)n_bins, out, labels, rows, edges, static_cast<double*>(workspace),
                  reinterpret_cast<unsigned long long*>(table)};
  const unsigned gx = n_workgroups > 0 ? (unsigned)n_workgroups
                                       : (unsigned)std::max<int64_t>(1, std::min<int64_t>(kMaxGrid, n_chunks));
  const dim3 grid(gx, (unsigned)G);
  const bool lds = cells <= kLdsCells;
#define WG_CALIB_BINS(K)                                                                                  \
  if (lds) hipLaunchKernelGGL((calib_bins_kernel<K, true>), grid, dim3(kCalibBlock), 0, stream, a);            \
  else hipLaunchKernelGGL((calib_bins_kernel<K, false>), grid, dim3(kCalibBlock), 0, stream, a);
  switch (kind) {
    case kProbs: WG_CALIB_BINS(kProbs) break;
    case kExp: WG_CALIB_BINS(kExp) break;
    default: WG_CALIB_BINS(kLogits) break;
  }
#undef WG_CALIB_BINS
  WG_LAUNCH_CHECK();
  hipLaunchKernelGGL(calib_scalars_kernel, dim3((unsigned)G), dim3(64), 0, stream, n_chunks,
                     static_cast<const double*>(workspace), scalars);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_calib_ece(int64_t G, int64_t C, int32_t n_bins, int64_t n_rows, int32_t min_count, const uint64_t* table,
                 double* ece_class, double* ece_top, void* stream_) {
  static const char* who = "wg_calib_ece";
  if (int rc = check_table_shape(who, G, C, n_bins, n_rows)) return rc;
  if (min_count < 0) return fail(WG_ERR_INVALID, "%s: min_count=%d", who, min_count);
  if (G == 0) return WG_OK;
  if (!ece_class || !ece_top || !aligned8(ece_class) || !aligned8(ece_top))
    return fail(WG_ERR_INVALID, "%s: ece_class / ece_top NULL or not 8-byte aligned", who);
  hipStream_t stream = as_stream(stream_);
  if (n_rows == 0) {
    WG_HIP_TRY(zero_async(ece_class, (size_t)(G * C) * sizeof(double), stream));
    WG_HIP_TRY(zero_async(ece_top, (size_t)G * sizeof(double), stream));
    return WG_OK;
  }
  if (!table || !aligned8(table)) return fail(WG_ERR_INVALID, "%s: table NULL or not 8-byte aligned", who);
  hipLaunchKernelGGL(calib_ece_kernel, dim3((unsigned)ceil_div(C + 1, 64), (unsigned)G), dim3(64), 0, stream, (int)C,
                     (int)n_bins, (double)n_rows, (unsigned long long)min_count,
                     reinterpret_cast<const unsigned long long*>(table), ece_class, ece_top);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // extern "C"
