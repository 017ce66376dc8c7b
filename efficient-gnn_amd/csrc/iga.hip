// iga.hip -- the integrated-gradient scores of the calibration attacks (DESIGN.md 4.3 "Integrated-gradient scores").
// calib_attack/calib_iga.py:152-235 moves row t of the dense adjacency along two straight paths and, for every j and
// every path point, runs the model forward and backward to read one entry of the gradient.  On the two-layer base
// model that gradient is  d loss / d w_j = u . h_j + v . z_j + c  with u, v, c depending on the path point only, so the
// n scores of a target are two skinny matrix-vector products.
//
//   iga_path_kernel     one workgroup per target: row t's neighbour sums of z and h gathered once, then every path
//                       point's p, q, deg, w_t (float64 `state`) and its logits W2 q + b2
//   iga_coeff_kernel    one workgroup per (target, path): U = sum_k u_k, V = sum_k v_k, c = sum_k c_k in float64 from
//                       g_logits and the state
//   iga_score_kernel    one pass over j for all targets: a tile of 64 rows of z and h is staged in LDS once and read
//                       by every target's wave; s_j = +-(U . h_j + V . z_j + c), a_tj by binary search in row t, and
//                       each wave's best `topk` per target kept across its tiles, one entry per lane
//   iga_merge_kernel    the workgroups' partial lists merged, one wave per target (a second launch)
//
// Every sum is float64 in an order fixed by the inputs and the launch shape, every output is rounded once, there are
// no float atomics.  Ranking is the total order of attack.hip's flip_select: a NaN above every number, equal scores
// (-0 == +0) by the smaller index.
#include <algorithm>
#include <climits>
#include <cstdint>

#include "internal.h"

namespace wg {
namespace {

constexpr int kWaves = kBlock / 64;
constexpr int kTopMax = 32;        // the largest topk (a list lives in the lanes of one wave)
constexpr int kMaxGroups = 512;    // the most workgroups of one scoring pass
constexpr int kTile = 64;          // rows of z and h per tile: one per lane
constexpr int kChunk = 16;         // columns of a tile staged at a time (the registers of two workgroups per CU)
constexpr int kPass = 32;          // targets per pass over the tiles: kPerWave per wave
constexpr int kPerWave = kPass / kWaves;
constexpr int kMaxSteps = 4096;

struct Cand {
  unsigned long long key;  // 0 = empty
  float score;
};

__device__ inline unsigned long long rank_key(float s, int32_t j) {
  uint32_t b = __float_as_uint(s);
  uint32_t k;
  if (s != s) k = 0xFFFFFFFFu;                         // a NaN ranks above every number
  else {
    if (b == 0x80000000u) b = 0;                       // -0 == +0
    k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
  return ((unsigned long long)k << 32) | (uint32_t)(0x7FFFFFFF - j);   // equal scores: the smaller index wins
}
__device__ inline int32_t key_index(unsigned long long key) { return 0x7FFFFFFF - (int32_t)(uint32_t)key; }

// first index in [lo, hi) with a[index] >= key (a ascending)
__device__ inline int64_t lower_bound(const int32_t* __restrict__ a, int64_t lo, int64_t hi, int32_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ inline unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// A wave's descending list of its best `topk`: lane l holds the l-th entry.  offer() takes one candidate per lane
// (key 0: none) and inserts, best first, those that beat the list's last entry.  Keys are distinct.
__device__ inline void offer(Cand& slot, Cand mine, int topk, int lane) {
  for (;;) {
    const unsigned long long last = __shfl(slot.key, topk - 1, 64);
    const unsigned long long best = wave_max(mine.key > last ? mine.key : 0ull);
    if (best == 0ull) return;
    const int src = __ffsll((long long)__ballot(mine.key == best)) - 1;
    const float best_score = __shfl(mine.score, src, 64);
    if (lane == src) mine.key = 0ull;
    const int pos = __popcll(__ballot(slot.key > best));
    const unsigned long long up_key = __shfl_up(slot.key, 1, 64);
    const float up_score = __shfl_up(slot.score, 1, 64);
    if (lane > pos) slot.key = up_key, slot.score = up_score;
    else if (lane == pos) slot.key = best, slot.score = best_score;
    if (lane >= topk) slot.key = 0ull, slot.score = 0.0f;
  }
}

// ---------------------------------------------------------------- the path points
struct PathArgs {
  int64_t n = 0, Hd = 0, C = 0;
  int steps = 1;
  const int32_t* targets = nullptr;
  const int64_t* indptr = nullptr;
  const int32_t* indices = nullptr;
  const float* z = nullptr;      // (n, Hd)
  const float* h = nullptr;      // (n, Hd)
  const double* zsum = nullptr;  // [Hd]
  const double* hsum = nullptr;  // [Hd]
  const float* b1 = nullptr;
  const float* W2 = nullptr;     // (C, Hd)
  const float* b2 = nullptr;
  float* logits = nullptr;       // (B, P, C)
  double* state = nullptr;       // (B, P, 2 Hd + 2): p, q, deg, w_t
};

__global__ __launch_bounds__(kBlock) void iga_path_kernel(PathArgs a) {
  __shared__ double red_z[kBlock], red_h[kBlock];
  __shared__ double sz[256], sh[256], q_sh[256];
  __shared__ int self_sh;
  const int tid = threadIdx.x;
  const int64_t t = a.targets[blockIdx.x];
  WG_DCHECK(t >= 0 && t < a.n, "iga path: target %lld outside [0, %lld)", (long long)t, (long long)a.n);
  const int64_t s = a.indptr[t], e = a.indptr[t + 1], len = e - s;
  WG_DCHECK(s >= 0 && s <= e, "iga path: row %lld is [%lld, %lld)", (long long)t, (long long)s, (long long)e);
  // thread (g, f): sub-group g of G takes the entries g, g + G, ... of the row at column f
  int W = 1;
  while (W < a.Hd) W <<= 1;
  const int G = kBlock / W, g = tid / W, f = tid % W;
  double az = 0.0, ah = 0.0;
  if (f < a.Hd) {
    for (int64_t i = s + g; i < e; i += G) {
      const int32_t j = a.indices[i];
      WG_DCHECK(j >= 0 && j < a.n, "iga path: row %lld column %d outside [0, %lld)", (long long)t, (int)j, (long long)a.n);
      az += (double)a.z[(int64_t)j * a.Hd + f];
      ah += (double)a.h[(int64_t)j * a.Hd + f];
    }
  }
  red_z[tid] = az, red_h[tid] = ah;
  if (tid == 0) {
    const int64_t k = lower_bound(a.indices, s, e, (int32_t)t);
    self_sh = (k < e && a.indices[k] == (int32_t)t) ? 1 : 0;
  }
  __syncthreads();
  if (tid < a.Hd) {   // the sub-groups' sums in sub-group order
    double tz = red_z[tid], th = red_h[tid];
    for (int gg = 1; gg < G; ++gg) tz += red_z[gg * W + tid], th += red_h[gg * W + tid];
    sz[tid] = tz, sh[tid] = th;
  }
  __syncthreads();
  const double a_t = (double)self_sh;
  const int P = 2 * (a.steps + 1);
  const int64_t stride = 2 * a.Hd + 2;
  for (int i = 0; i < P; ++i) {
    const int path = i / (a.steps + 1), k = i % (a.steps + 1);
    const double lam = (double)k / (double)a.steps;
    double deg, wt;
    if (path == 0) deg = lam * (double)len, wt = lam * a_t;                                    // w = lam a
    else deg = (1.0 - lam) * (double)a.n + lam * (double)len, wt = 1.0 - lam * (1.0 - a_t);    // w = 1 - lam (1 - a)
    const double d = deg != 0.0 ? deg : 1.0;
    double* st = a.state + ((int64_t)blockIdx.x * P + i) * stride;
    if (tid < a.Hd) {
      double pz, qh;
      if (path == 0) pz = lam * sz[tid], qh = lam * sh[tid];
      else pz = (1.0 - lam) * a.zsum[tid] + lam * sz[tid], qh = (1.0 - lam) * a.hsum[tid] + lam * sh[tid];
      const double p = pz / d;
      double hp = p + (double)a.b1[tid];
      hp = hp > 0.0 ? hp : 0.0;
      const double q = ((qh - wt * (double)a.h[t * a.Hd + tid]) + wt * hp) / d;
      st[tid] = p, st[a.Hd + tid] = q;
      q_sh[tid] = q;
    }
    if (tid == 0) st[2 * a.Hd] = deg, st[2 * a.Hd + 1] = wt;
    __syncthreads();
    if (tid < a.C) {   // one thread per class, columns in ascending order
      const float* w = a.W2 + (int64_t)tid * a.Hd;
      double acc = 0.0;
      for (int64_t c = 0; c < a.Hd; ++c) acc += (double)w[c] * q_sh[c];
      a.logits[((int64_t)blockIdx.x * P + i) * a.C + tid] = (float)(acc + (double)a.b2[tid]);
    }
    __syncthreads();   // q_sh is written again by the next path point
  }
}

// ---------------------------------------------------------------- the coefficients
struct ScoreArgs {
  int64_t n = 0, Hd = 0, C = 0, B = 0, HdP = 0;   // HdP: Hd rounded up to kChunk (the workspace's zero-padded rows)
  int steps = 1, topk = 1;
  const int32_t* targets = nullptr;
  const int64_t* indptr = nullptr;
  const int32_t* indices = nullptr;
  const float* z = nullptr;
  const float* h = nullptr;
  const float* b1 = nullptr;
  const float* W2 = nullptr;
  const float* g_logits = nullptr;   // (B, P, C)
  const double* state = nullptr;     // (B, P, 2 Hd + 2)
  double* co = nullptr;              // workspace (B, 2, 2 HdP + 1): U, V (zero-padded), c
  double* coeffs = nullptr;          // (B, 2, 2 Hd + 1), nullable
  float* scores = nullptr;           // (B, n), nullable
  Cand* partial = nullptr;           // workspace (groups, B, topk)
};

__global__ __launch_bounds__(kBlock) void iga_coeff_kernel(ScoreArgs a) {
  __shared__ double red[kBlock];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x >> 1;
  const int path = blockIdx.x & 1;
  const int P = 2 * (a.steps + 1);
  const int64_t stride = 2 * a.Hd + 2;
  double U = 0.0, V = 0.0, cpart = 0.0;
  if (tid < a.Hd) {
    const double bias = (double)a.b1[tid];
    for (int k = 0; k <= a.steps; ++k) {
      const int64_t pt = b * P + (int64_t)path * (a.steps + 1) + k;
      const double* st = a.state + pt * stride;
      const float* g = a.g_logits + pt * a.C;
      double gq = 0.0;
      for (int64_t c = 0; c < a.C; ++c) gq += (double)a.W2[c * a.Hd + tid] * (double)g[c];   // classes ascending
      const double deg = st[2 * a.Hd], wt = st[2 * a.Hd + 1];
      const bool zero = deg == 0.0;          // a zero row: the model divides by 1, a constant (model.py:44)
      const double d = zero ? 1.0 : deg;
      const double p = st[tid], q = st[a.Hd + tid];
      const double u = gq / d;
      const double v = (wt / (d * d)) * ((p + bias > 0.0) ? gq : 0.0);
      U += u, V += v;
      if (!zero) cpart -= u * q + v * p;
    }
  }
  red[tid] = cpart;
  __syncthreads();
  double* co = a.co + (b * 2 + path) * (2 * a.HdP + 1);
  if (tid < a.HdP) co[tid] = U, co[a.HdP + tid] = V;   // the padding: zeros
  if (tid < a.Hd && a.coeffs) {
    double* out = a.coeffs + (b * 2 + path) * (2 * a.Hd + 1);
    out[tid] = U, out[a.Hd + tid] = V;
  }
  if (tid == 0) {   // columns in ascending order
    double c = 0.0;
    for (int64_t f = 0; f < a.Hd; ++f) c += red[f];
    co[2 * a.HdP] = c;
    if (a.coeffs) a.coeffs[(b * 2 + path) * (2 * a.Hd + 1) + 2 * a.Hd] = c;
  }
}

// ---------------------------------------------------------------- the scores and each workgroup's best
__global__ __launch_bounds__(kBlock, 2) void iga_score_kernel(ScoreArgs a) {
  __shared__ float zt[kTile][kChunk + 1], ht[kTile][kChunk + 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t n_tiles = (a.n + kTile - 1) / kTile;
  const int64_t co_stride = 2 * a.HdP + 1;
  for (int64_t b0 = 0; b0 < a.B; b0 += kPass) {
    // this wave's targets: b0 + wave + kWaves * i
    int64_t tt[kPerWave], rs[kPerWave], re[kPerWave];
    Cand list[kPerWave];
#pragma unroll
    for (int i = 0; i < kPerWave; ++i) {
      const int64_t b = b0 + wave + kWaves * i;
      list[i] = Cand{0ull, 0.0f};
      tt[i] = rs[i] = re[i] = 0;
      if (b < a.B) {
        tt[i] = a.targets[b];
        WG_DCHECK(tt[i] >= 0 && tt[i] < a.n, "iga scores: target %lld outside [0, %lld)", (long long)tt[i], (long long)a.n);
        rs[i] = a.indptr[tt[i]], re[i] = a.indptr[tt[i] + 1];
        WG_DCHECK(rs[i] >= 0 && rs[i] <= re[i], "iga scores: row %lld is [%lld, %lld)", (long long)tt[i], (long long)rs[i],
                  (long long)re[i]);
      }
    }
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
      const int64_t j0 = tile * kTile, j = j0 + lane;
      double acc[kPerWave];
#pragma unroll
      for (int i = 0; i < kPerWave; ++i) {
        const int64_t b = b0 + wave + kWaves * i;
        acc[i] = b < a.B ? a.co[(b * 2 + 1) * co_stride + 2 * a.HdP] : 0.0;   // the add path's c
      }
      for (int64_t f0 = 0; f0 < a.Hd; f0 += kChunk) {
        __syncthreads();   // the tile is read by every wave before it is written again
        for (int idx = tid; idx < kTile * kChunk; idx += kBlock) {
          const int r = idx / kChunk, f = idx % kChunk;
          const bool in = j0 + r < a.n && f0 + f < a.Hd;
          const int64_t at = (j0 + r) * a.Hd + f0 + f;
          zt[r][f] = in ? a.z[at] : 0.0f;
          ht[r][f] = in ? a.h[at] : 0.0f;
        }
        __syncthreads();
        float zr[kChunk], hr[kChunk];
#pragma unroll
        for (int f = 0; f < kChunk; ++f) zr[f] = zt[lane][f], hr[f] = ht[lane][f];
#pragma unroll
        for (int i = 0; i < kPerWave; ++i) {
          const int64_t b = b0 + wave + kWaves * i;
          if (b < a.B) {   // uniform over the wave, as are the coefficients' addresses
            const double* U = a.co + (b * 2 + 1) * co_stride + f0;
            const double* V = U + a.HdP;
            double s = acc[i];
#pragma unroll
            for (int f = 0; f < kChunk; ++f) {
              s = fma(U[f], (double)hr[f], s);
              s = fma(V[f], (double)zr[f], s);
            }
            acc[i] = s;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < kPerWave; ++i) {
        const int64_t b = b0 + wave + kWaves * i;
        if (b >= a.B) continue;
        Cand mine{0ull, 0.0f};
        if (j < a.n) {
          double s = acc[i];
          const int64_t k = lower_bound(a.indices, rs[i], re[i], (int32_t)j);
          WG_DCHECK(k == re[i] || (a.indices[k] >= 0 && a.indices[k] < a.n), "iga scores: column %d outside [0, %lld)",
                    (int)a.indices[k], (long long)a.n);
          if (k < re[i] && a.indices[k] == (int32_t)j) {
            // an existing entry: the remove path's coefficients in the same order, and the sign (calib_iga.py:232)
            const double* U = a.co + (b * 2) * co_stride;
            const double* V = U + a.HdP;
            const float* zj = a.z + j * a.Hd;
            const float* hj = a.h + j * a.Hd;
            s = U[2 * a.HdP];
            for (int64_t f = 0; f < a.Hd; ++f) {
              s = fma(U[f], (double)hj[f], s);
              s = fma(V[f], (double)zj[f], s);
            }
            s = -s;
          }
          float sc = (float)s;
          if (j == tt[i]) sc = -10.0f;
          if (a.scores) a.scores[b * a.n + j] = sc;
          mine = Cand{rank_key(sc, (int32_t)j), sc};
        }
        offer(list[i], mine, a.topk, lane);
      }
    }
#pragma unroll
    for (int i = 0; i < kPerWave; ++i) {
      const int64_t b = b0 + wave + kWaves * i;
      if (b < a.B && lane < a.topk) a.partial[((int64_t)blockIdx.x * a.B + b) * a.topk + lane] = list[i];
    }
  }
}

// one wave per target: the groups' lists, 64 candidates at a time
__global__ __launch_bounds__(64) void iga_merge_kernel(const Cand* __restrict__ partial, int groups, int64_t B, int topk,
                                                      int32_t* __restrict__ best_ids, float* __restrict__ best_scores) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  Cand list{0ull, 0.0f};
  const int total = groups * topk;
  for (int i0 = 0; i0 < total; i0 += 64) {
    const int i = i0 + lane;
    Cand mine{0ull, 0.0f};
    if (i < total) mine = partial[((int64_t)(i / topk) * B + b) * topk + (i % topk)];
    offer(list, mine, topk, lane);
  }
  if (lane < topk) {
    best_ids[b * topk + lane] = list.key ? key_index(list.key) : -1;
    best_scores[b * topk + lane] = list.key ? list.score : -INFINITY;
  }
}

inline int64_t padded(int64_t Hd) { return ceil_div(Hd, (int64_t)kChunk) * kChunk; }
inline int64_t co_bytes(int64_t B, int64_t Hd) { return (int64_t)sizeof(double) * B * 2 * (2 * padded(Hd) + 1); }

int check_common(const char* who, int64_t n, int64_t nnz, int64_t Hd, int64_t C, int64_t B, int32_t steps) {
  if (n < 1 || nnz < 0) return fail(WG_ERR_INVALID, "%s: n=%lld nnz=%lld", who, (long long)n, (long long)nnz);
  if (n > INT32_MAX || nnz > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld or nnz=%lld exceeds int32", who, (long long)n, (long long)nnz);
  if (Hd < 1 || C < 1 || B < 1 || steps < 1)
    return fail(WG_ERR_INVALID, "%s: Hd=%lld C=%lld B=%lld steps=%d must be >= 1", who, (long long)Hd, (long long)C,
                (long long)B, (int)steps);
  if (Hd > 256 || C > 256) return fail(WG_ERR_UNSUPPORTED, "%s: Hd=%lld or C=%lld above 256", who, (long long)Hd, (long long)C);
  if (steps > kMaxSteps) return fail(WG_ERR_UNSUPPORTED, "%s: steps=%d above %d", who, (int)steps, kMaxSteps);
  if (B > (1 << 20)) return fail(WG_ERR_UNSUPPORTED, "%s: B=%lld above %d", who, (long long)B, 1 << 20);
  return WG_OK;
}

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_iga_max_topk(void) { return kTopMax; }

int wg_iga_path_logits(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t Hd, const float* z,
                       const float* h, const double* zsum, const double* hsum, const float* b1, const float* W2,
                       const float* b2, int64_t C, int64_t B, const int32_t* targets, int32_t steps, float* logits,
                       double* state, void* stream_) {
  if (int rc = check_common("wg_iga_path_logits", n, nnz, Hd, C, B, steps)) return rc;
  if (!indptr || !z || !h || !zsum || !hsum || !b1 || !W2 || !b2 || !targets || !logits || !state)
    return fail(WG_ERR_INVALID, "wg_iga_path_logits: NULL indptr / z / h / zsum / hsum / b1 / W2 / b2 / targets / logits / state");
  if (nnz > 0 && !indices) return fail(WG_ERR_INVALID, "wg_iga_path_logits: NULL indices with nnz=%lld", (long long)nnz);
  if (reinterpret_cast<uintptr_t>(state) & 7u || reinterpret_cast<uintptr_t>(zsum) & 7u || reinterpret_cast<uintptr_t>(hsum) & 7u)
    return fail(WG_ERR_INVALID, "wg_iga_path_logits: zsum / hsum / state must be 8-byte aligned");
  PathArgs a;
  a.n = n, a.Hd = Hd, a.C = C, a.steps = steps, a.targets = targets, a.indptr = indptr, a.indices = indices;
  a.z = z, a.h = h, a.zsum = zsum, a.hsum = hsum, a.b1 = b1, a.W2 = W2, a.b2 = b2, a.logits = logits, a.state = state;
  hipLaunchKernelGGL(iga_path_kernel, dim3((unsigned)B), dim3(kBlock), 0, as_stream(stream_), a);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_iga_scores_workspace(int64_t B, int64_t Hd, int64_t* bytes) {
  if (!bytes) return fail(WG_ERR_INVALID, "wg_iga_scores_workspace: NULL bytes");
  if (B < 1 || Hd < 1 || Hd > 256 || B > (1 << 20))
    return fail(WG_ERR_INVALID, "wg_iga_scores_workspace: B=%lld Hd=%lld", (long long)B, (long long)Hd);
  *bytes = co_bytes(B, Hd) + (int64_t)sizeof(Cand) * kMaxGroups * B * kTopMax;
  return WG_OK;
}

int wg_iga_scores(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t Hd, const float* z,
                  const float* h, const float* b1, const float* W2, int64_t C, int64_t B, const int32_t* targets,
                  int32_t steps, const float* g_logits, const double* state, int32_t topk, int32_t n_workgroups,
                  void* workspace, double* coeffs, float* scores, int32_t* best_ids, float* best_scores, void* stream_) {
  if (int rc = check_common("wg_iga_scores", n, nnz, Hd, C, B, steps)) return rc;
  if (topk < 1 || topk > kTopMax) return fail(WG_ERR_INVALID, "wg_iga_scores: topk=%d outside [1, %d]", (int)topk, kTopMax);
  if (n_workgroups < 0 || n_workgroups > kMaxGroups)
    return fail(WG_ERR_INVALID, "wg_iga_scores: n_workgroups=%d outside [0, %d]", (int)n_workgroups, kMaxGroups);
  if (!indptr || !z || !h || !b1 || !W2 || !targets || !g_logits || !state || !best_ids || !best_scores)
    return fail(WG_ERR_INVALID, "wg_iga_scores: NULL indptr / z / h / b1 / W2 / targets / g_logits / state / best_ids / best_scores");
  if (nnz > 0 && !indices) return fail(WG_ERR_INVALID, "wg_iga_scores: NULL indices with nnz=%lld", (long long)nnz);
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u))
    return fail(WG_ERR_INVALID, "wg_iga_scores: workspace is NULL or not 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(state) & 7u || reinterpret_cast<uintptr_t>(coeffs) & 7u)
    return fail(WG_ERR_INVALID, "wg_iga_scores: state / coeffs must be 8-byte aligned");
  const int groups = n_workgroups ? n_workgroups : (int)std::min<int64_t>(ceil_div(n, (int64_t)kTile), kMaxGroups);
  ScoreArgs a;
  a.n = n, a.Hd = Hd, a.C = C, a.B = B, a.HdP = padded(Hd), a.steps = steps, a.topk = topk, a.targets = targets;
  a.indptr = indptr, a.indices = indices, a.z = z, a.h = h, a.b1 = b1, a.W2 = W2, a.g_logits = g_logits, a.state = state;
  a.co = static_cast<double*>(workspace);
  a.partial = reinterpret_cast<Cand*>(static_cast<char*>(workspace) + co_bytes(B, Hd));
  a.coeffs = coeffs, a.scores = scores;
  hipStream_t stream = as_stream(stream_);
  hipLaunchKernelGGL(iga_coeff_kernel, dim3((unsigned)(2 * B)), dim3(kBlock), 0, stream, a);
  WG_LAUNCH_CHECK();
  hipLaunchKernelGGL(iga_score_kernel, dim3((unsigned)groups), dim3(kBlock), 0, stream, a);
  WG_LAUNCH_CHECK();
  hipLaunchKernelGGL(iga_merge_kernel, dim3((unsigned)B), dim3(64), 0, stream, a.partial, groups, B, (int)topk, best_ids,
                     best_scores);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // extern "C"
