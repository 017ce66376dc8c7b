// fga.hip -- the flip scores of Calib_FGA for many targets at once (DESIGN.md 4.3 "Batched attack step").
// calib_attack/calib_fga.py:864-898 runs the whole model forward and backward to read row t and column t of the
// adjacency's gradient.  The loss reads out[t] only, so on the two-layer base model those 2n entries are, with
// g = d L / d out_t, q = W2^T g, m_i = q * [y1_i + b1 > 0] and a_tt = [t in N'(t)],
//   d / d A[t, j] = (q . h_j - q . y2) / deg_t + (a_tt / deg_t^2) m_t . (z_j - y1_t)        = U . h_j + V . z_j + c
//   d / d A[i, t] = [i in N'(t)] (1 / (deg_t deg_i)) m_i . (z_t - y1_i)
// on the graph with the target's toggles applied.  Only the rows of N(t) + S_b differ from the base graph's.
//
//   fga_local_kernel    one workgroup per target: the ascending list of its local ids (N(t) + S_b), every local
//                       row's y1_j and h_j gathered from z on the flipped rows (the whole workgroup per row, the
//                       waves' sums added in wave order), U, V, c per gradient row, and the local j's two gradient
//                       entries, each rounded once
//   fga_score_kernel    one pass over j for all targets: a tile of 64 rows of z and h is staged in LDS once and read
//                       by every target's wave; a local j takes the list's values, every other j gets U . h_j + V . z_j
//                       + c and a column entry of +0; then wg_flip_select's float32 score and rerank, and each wave's
//                       best `topk` per target
//   fga_merge_kernel    the workgroups' partial lists merged, one wave per target (a second launch)
//
// Every sum is float64 in an order fixed by the rows, Hd and the launch shape, every gradient entry is rounded once,
// there are no float atomics.  The float32 score is attack.hip's flip_select expression (contraction off).
#include <algorithm>
#include <climits>
#include <cstdint>

#include "internal.h"

#pragma clang fp contract(off)

namespace wg {
namespace {

constexpr int kWaves = kBlock / 64;
constexpr int kTop = 8;            // the largest topk, as wg_flip_select
constexpr int kMaxGroups = 512;    // the most workgroups of one scoring pass
constexpr int kTile = 64;          // rows of z and h per tile: one per lane
constexpr int kChunk = 16;         // columns of a tile staged at a time
constexpr int kPass = 32;          // targets per pass over the tiles: kPerWave per wave
constexpr int kPerWave = kPass / kWaves;
constexpr int kMaxG = 3;

struct Cand {
  unsigned long long key;  // 0 = empty
  float score;
};

struct Meta {      // one target's share of the local lists
  int64_t off;
  int32_t nloc;    // entries that fit under local_cap
  int32_t att;     // t in N'(t)
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
__device__ inline bool contains(const int32_t* __restrict__ a, int64_t len, int32_t key) {
  const int64_t k = lower_bound(a, 0, len, key);
  return k < len && a[k] == key;
}

__device__ inline unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// A wave's descending list of its best `topk`: lane l holds the l-th entry (iga.hip's offer()).
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

struct Args {
  int64_t n = 0, Hd = 0, C = 0, B = 0, HdP = 0, cap = 0;   // HdP: Hd rounded up to kChunk; cap: local_cap
  int G = 1, topk = 1;
  const int64_t* indptr = nullptr;
  const int32_t* indices = nullptr;
  const float* z = nullptr;
  const float* h = nullptr;
  const float* b1 = nullptr;
  const float* W2 = nullptr;
  const int32_t* targets = nullptr;
  const int32_t* tog_ptr = nullptr;
  const int32_t* tog_ids = nullptr;
  const float* g_logits = nullptr;   // (B, G, C)
  const int32_t* rerank = nullptr;   // [B], nullable
  const float* p_top2 = nullptr;     // (B, 2)
  // the workspace
  double* co = nullptr;              // (B, G, 2 HdP + 1): U, V (zero-padded), c
  double* tmp = nullptr;             // (G, cap): U . h_j + V . z_j of the local j before c is known
  Meta* meta = nullptr;              // [B]
  Cand* partial = nullptr;           // (groups, B, topk)
  int32_t* lids = nullptr;           // [cap]: the targets' local ids, each target's share ascending
  int32_t* live = nullptr;           // [cap]: 1 where (t, j) is an entry of the flipped graph
  float* grow = nullptr;             // (G, cap)
  float* gcol = nullptr;             // (G, cap)
  // outputs
  float* grads = nullptr;            // (B, G, 2 n), nullable
  float* scores = nullptr;           // (B, n), nullable
};

// the workgroup's sum over f < Hd of v (thread f holds column f; threads past Hd pass 0): lanes by xor butterfly,
// then the waves that hold columns in wave order.  Every thread returns the total
__device__ inline double block_sum(double v, int n_waves, double* __restrict__ sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();   // sh is read by every thread before it is written again
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double tot = sh[0];
  for (int w = 1; w < n_waves; ++w) tot += sh[w];
  return tot;
}

// sum_{k in N'(j)} z_k at column threadIdx.x (valid below Hd): the base row's entries that T leaves, wave w taking the
// entries w, w + kWaves, ..., then the partners T adds, dealt the same way; the waves' sums in wave order
__device__ inline double row_sum(const Args& a, const int32_t* __restrict__ row, int64_t len,
                                 const int32_t* __restrict__ T, int nT, double (*red)[256]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  // kBatch entries of the wave's share at a time: their ids, then their rows of z, are in flight together (an index
  // past the end reads the row's last entry and is not added)
  constexpr int kBatch = 8;
  for (int64_t i0 = wave; i0 < len; i0 += (int64_t)kWaves * kBatch) {
    int32_t k[kBatch];
    bool on[kBatch];
    float xv[kBatch][4];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int64_t i = i0 + (int64_t)u * kWaves;
      on[u] = i < len;
      k[u] = row[on[u] ? i : len - 1];
      WG_DCHECK(k[u] >= 0 && k[u] < a.n, "fga local: column %d outside [0, %lld)", (int)k[u], (long long)a.n);
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const float* zk = a.z + (int64_t)k[u] * a.Hd;
#pragma unroll
      for (int c = 0; c < 4; ++c) xv[u][c] = lane + 64 * c < a.Hd ? zk[lane + 64 * c] : 0.0f;
    }
    if (nT > 0) {
#pragma unroll
      for (int u = 0; u < kBatch; ++u) on[u] = on[u] && !contains(T, nT, k[u]);
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] += on[u] ? (double)xv[u][c] : 0.0;
    }
  }
  for (int q = wave; q < nT; q += kWaves) {
    const int32_t k = T[q];
    WG_DCHECK(k >= 0 && k < a.n, "fga local: partner %d outside [0, %lld)", (int)k, (long long)a.n);
    if (contains(row, len, k)) continue;
    const float* zk = a.z + (int64_t)k * a.Hd;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (lane + 64 * c < a.Hd) acc[c] += (double)zk[lane + 64 * c];
  }
  __syncthreads();   // red is read by every thread before it is written again
#pragma unroll
  for (int c = 0; c < 4; ++c) red[wave][lane + 64 * c] = acc[c];
  __syncthreads();
  double tot = red[0][threadIdx.x];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) tot += red[w][threadIdx.x];
  return tot;
}

__global__ __launch_bounds__(kBlock) void fga_local_kernel(Args a) {
  __shared__ double red[kWaves][256];
  __shared__ double sum_sh[kWaves];
  __shared__ double c_sh[kMaxG];
  __shared__ unsigned long long off_sh;
  __shared__ int inter_sh;
  __shared__ int32_t t_sh;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int G = a.G;
  const int32_t t = a.targets[b];
  WG_DCHECK(t >= 0 && t < a.n, "fga local: target %d outside [0, %lld)", (int)t, (long long)a.n);
  const int32_t c0 = a.tog_ptr[b], c1 = a.tog_ptr[b + 1];
  WG_DCHECK(c0 >= 0 && c0 <= c1, "fga local: target %d toggles are [%d, %d)", (int)b, (int)c0, (int)c1);
  const int32_t* S = a.tog_ids + c0;
  const int nS = c1 - c0;
  const int64_t st = a.indptr[t], lt = a.indptr[t + 1] - st;
  WG_DCHECK(st >= 0 && lt >= 0, "fga local: row %d is [%lld, +%lld)", (int)t, (long long)st, (long long)lt);
  const int32_t* Nt = a.indices + st;
  if (tid == 0) off_sh = 0ull, inter_sh = 0, t_sh = t;
  __syncthreads();
  // where this target's share of the local lists begins: the rows and toggle sets of the targets before it
  unsigned long long before = 0ull;
  for (int64_t bb = tid; bb < b; bb += kBlock) {
    const int64_t tb = a.targets[bb];
    before += (unsigned long long)(a.indptr[tb + 1] - a.indptr[tb]);
  }
  if (before) atomicAdd(&off_sh, before);
  int hits = 0;
  for (int q = tid; q < nS; q += kBlock) {
    WG_DCHECK(S[q] >= 0 && S[q] < a.n && S[q] != t && (q == 0 || S[q - 1] < S[q]),
              "fga local: target %d partner %d is outside [0, %lld), the target or not ascending", (int)b, (int)S[q],
              (long long)a.n);
    hits += contains(Nt, lt, S[q]) ? 1 : 0;
  }
  if (hits) atomicAdd(&inter_sh, hits);
  __syncthreads();
  const int64_t off = (int64_t)off_sh + (c0 - a.tog_ptr[0]);
  const int64_t inter = inter_sh;
  const int64_t deg_t = lt + nS - 2 * inter;            // |N(t) delta S|
  const int64_t n_all = lt + nS - inter;                // |N(t) + S|
  WG_DCHECK(n_all <= a.cap - off, "fga local: target %d has %lld local entries from %lld on, local_cap=%lld", (int)b,
            (long long)n_all, (long long)off, (long long)a.cap);
  const int64_t nloc = std::max<int64_t>(0, std::min<int64_t>(n_all, a.cap - off));   // never past the workspace
  const bool att = contains(Nt, lt, t);                 // S never holds t
  if (tid == 0) a.meta[b] = Meta{off, (int32_t)nloc, att ? 1 : 0};
  // the local ids in ascending order: a base entry moves up by the added partners below it, an added partner sits
  // after the base entries below it
  for (int64_t i = tid; i < lt + nS; i += kBlock) {
    int32_t j;
    int64_t pos;
    int alive;
    if (i < lt) {
      j = Nt[i];
      const int64_t below = lower_bound(S, 0, nS, j);
      int64_t shared = 0;
      for (int64_t q = 0; q < below; ++q) shared += contains(Nt, lt, S[q]) ? 1 : 0;
      pos = i + below - shared;
      alive = !(below < nS && S[below] == j);
    } else {
      const int64_t q = i - lt;
      j = S[q];
      if (contains(Nt, lt, j)) continue;
      int64_t shared = 0;
      for (int64_t r = 0; r < q; ++r) shared += contains(Nt, lt, S[r]) ? 1 : 0;
      pos = lower_bound(Nt, 0, lt, j) + q - shared;
      alive = 1;
    }
    if (pos < nloc) a.lids[off + pos] = j, a.live[off + pos] = alive;
  }
  // y1_t, then q, U and V of every gradient row at column tid
  const int n_waves = (int)((a.Hd + 63) / 64);
  const bool col = tid < a.Hd;
  const double dt = (double)(deg_t > 0 ? deg_t : 1);
  const double y1t = row_sum(a, Nt, lt, S, nS, red) / dt;
  const double bias = col ? (double)a.b1[tid] : 0.0;
  const double ztf = col ? (double)a.z[(int64_t)t * a.Hd + tid] : 0.0;
  const bool on_t = y1t + bias > 0.0;
  double qv[kMaxG], U[kMaxG], V[kMaxG];
#pragma unroll
  for (int g = 0; g < kMaxG; ++g) {
    qv[g] = U[g] = V[g] = 0.0;
    if (g < G && col) {
      const float* gl = a.g_logits + (b * G + g) * a.C;
      double s = 0.0;
      for (int64_t c = 0; c < a.C; ++c) s += (double)a.W2[c * a.Hd + tid] * (double)gl[c];   // classes ascending
      qv[g] = s;
      U[g] = s / dt;
      V[g] = (att && on_t) ? (1.0 / (dt * dt)) * s : 0.0;
    }
    if (g < G && tid < a.HdP) {
      double* co = a.co + (b * G + g) * (2 * a.HdP + 1);
      co[tid] = U[g], co[a.HdP + tid] = V[g];   // the padding: zeros
    }
  }
  __syncthreads();   // the list written above is read below
  // the local rows in ascending order
  double hs = 0.0;
  for (int64_t p = 0; p < nloc; ++p) {
    const int32_t j = a.lids[off + p];
    const bool alive = a.live[off + p] != 0;
    WG_DCHECK(j >= 0 && j < a.n, "fga local: local id %d outside [0, %lld)", (int)j, (long long)a.n);
    if (j < 0 || j >= a.n) continue;   // uniform over the workgroup: never a row outside the graph
    const int64_t sj = a.indptr[j], lj = a.indptr[j + 1] - sj;
    const int32_t* row = a.indices + sj;
    const int32_t* T = nullptr;
    int nT = 0;
    int64_t deg = lj;
    if (j == t) T = S, nT = nS, deg = deg_t;
    else if (contains(S, nS, j)) {
      T = &t_sh, nT = 1;
      deg = lj + 1 - 2 * (contains(row, lj, t) ? 1 : 0);
    }
    const double dj = (double)(deg > 0 ? deg : 1);
    const double y1 = row_sum(a, row, lj, T, nT, red) / dj;
    const double pre = y1 + bias;
    const bool on = pre > 0.0;
    const double hj = on ? pre : 0.0;
    const double zj = col ? (double)a.z[(int64_t)j * a.Hd + tid] : 0.0;
    if (alive) hs += hj;
    const double inv = 1.0 / (dt * dj);
#pragma unroll
    for (int g = 0; g < kMaxG; ++g) {
      if (g >= G) continue;
      double r = 0.0, k = 0.0;
      if (col) {
        r = U[g] * hj;
        if (att) r += V[g] * zj;
        k = on ? qv[g] * (ztf - y1) : 0.0;
      }
      const double rt = block_sum(r, n_waves, sum_sh);
      const double kt = block_sum(k, n_waves, sum_sh);
      if (tid == 0) {
        a.tmp[(int64_t)g * a.cap + off + p] = rt;
        a.gcol[(int64_t)g * a.cap + off + p] = alive ? (float)(inv * kt) : 0.0f;
      }
    }
  }
  // c = -(U . y2 + V . y1_t), then the row entries of the local j
  const double y2 = hs / dt;
#pragma unroll
  for (int g = 0; g < kMaxG; ++g) {
    if (g >= G) continue;
    double v = 0.0;
    if (col) {
      v = U[g] * y2;
      if (att) v += V[g] * y1t;
    }
    const double tot = block_sum(v, n_waves, sum_sh);
    if (tid == 0) {
      c_sh[g] = -tot;
      a.co[(b * G + g) * (2 * a.HdP + 1) + 2 * a.HdP] = -tot;
    }
  }
  __syncthreads();   // c_sh, and tmp written by thread 0
  for (int64_t p = tid; p < nloc; p += kBlock) {
    for (int g = 0; g < G; ++g)
      a.grow[(int64_t)g * a.cap + off + p] = (float)(a.tmp[(int64_t)g * a.cap + off + p] + c_sh[g]);
  }
}

// ---------------------------------------------------------------- the scores and each workgroup's best
template <int G>
__global__ __launch_bounds__(kBlock, 2) void fga_score_kernel(Args a) {
  __shared__ float zt[kTile][kChunk + 1], ht[kTile][kChunk + 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t n_tiles = (a.n + kTile - 1) / kTile;
  const int64_t co_stride = 2 * a.HdP + 1;
  for (int64_t b0 = 0; b0 < a.B; b0 += kPass) {
    // this wave's targets: b0 + wave + kWaves * i
    int32_t tt[kPerWave], nloc[kPerWave];
    int64_t off[kPerWave];
    bool att[kPerWave], rr[kPerWave];
    float pm[kPerWave], ps[kPerWave];
    Cand list[kPerWave];
#pragma unroll
    for (int i = 0; i < kPerWave; ++i) {
      const int64_t b = b0 + wave + kWaves * i;
      list[i] = Cand{0ull, 0.0f};
      tt[i] = 0, nloc[i] = 0, off[i] = 0, att[i] = rr[i] = false, pm[i] = ps[i] = 0.0f;
      if (b < a.B) {
        const Meta m = a.meta[b];
        tt[i] = a.targets[b], nloc[i] = m.nloc, off[i] = m.off, att[i] = m.att != 0;
        rr[i] = G == 3 && a.rerank && a.rerank[b] != 0;
        if (rr[i]) pm[i] = a.p_top2[2 * b], ps[i] = a.p_top2[2 * b + 1];
      }
    }
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
      const int64_t j0 = tile * kTile, j = j0 + lane;
      double acc[kPerWave][G];
#pragma unroll
      for (int i = 0; i < kPerWave; ++i) {
        const int64_t b = b0 + wave + kWaves * i;
#pragma unroll
        for (int g = 0; g < G; ++g) acc[i][g] = b < a.B ? a.co[(b * G + g) * co_stride + 2 * a.HdP] : 0.0;
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
          if (b >= a.B) continue;   // uniform over the wave, as are the coefficients' addresses
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const double* U = a.co + (b * G + g) * co_stride + f0;
            const double* V = U + a.HdP;
            double s = acc[i][g];
#pragma unroll
            for (int f = 0; f < kChunk; ++f) s = fma(U[f], (double)hr[f], s);
            if (att[i]) {   // without the self loop V is zero: its products are skipped
#pragma unroll
              for (int f = 0; f < kChunk; ++f) s = fma(V[f], (double)zr[f], s);
            }
            acc[i][g] = s;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < kPerWave; ++i) {
        const int64_t b = b0 + wave + kWaves * i;
        if (b >= a.B) continue;
        Cand mine{0ull, 0.0f};
        if (j < a.n) {
          float gr[G], gc[G];
#pragma unroll
          for (int g = 0; g < G; ++g) gr[g] = (float)acc[i][g], gc[g] = 0.0f;
          float aj = 0.0f;
          const int64_t lo = off[i], hi = off[i] + nloc[i];
          const int64_t k = lower_bound(a.lids, lo, hi, (int32_t)j);
          if (k < hi && a.lids[k] == (int32_t)j) {   // a local j: the list's values
            aj = a.live[k] ? 1.0f : 0.0f;
#pragma unroll
            for (int g = 0; g < G; ++g) gr[g] = a.grow[(int64_t)g * a.cap + k], gc[g] = a.gcol[(int64_t)g * a.cap + k];
          }
          if (a.grads) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
              float* out = a.grads + (b * G + g) * 2 * a.n;
              out[j] = gr[g], out[a.n + j] = gc[g];
            }
          }
          // wg_flip_select's expressions (attack.hip), operation for operation
          const float d = 1.0f - 2.0f * aj;
          float sc = (gr[0] + gc[0]) * d;
          if (G == 3 && rr[i]) {   // the row half only
            const float c = ((pm[i] + gr[G - 2] * d) - ps[i]) - gr[G - 1] * d;
            const float flag = c > 0.0f ? 1.0f : -1.0f;   // a NaN condition: -1
            sc = sc * flag;
          }
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
__global__ __launch_bounds__(64) void fga_merge_kernel(const Cand* __restrict__ partial, int groups, int64_t B, int topk,
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
inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }
inline int max_groups(int64_t n) { return (int)std::min<int64_t>(ceil_div(n, (int64_t)kTile), kMaxGroups); }

// the workspace's parts, in order; every part begins on a 16-byte boundary
struct Layout {
  int64_t co, tmp, meta, partial, lids, live, grow, gcol, bytes;
};
Layout layout(int64_t n, int64_t Hd, int64_t B, int G, int64_t cap) {
  Layout L;
  int64_t at = 0;
  auto take = [&](int64_t bytes) {
    const int64_t here = at;
    at += up16(bytes);
    return here;
  };
  L.co = take((int64_t)sizeof(double) * B * G * (2 * padded(Hd) + 1));
  L.tmp = take((int64_t)sizeof(double) * G * cap);
  L.meta = take((int64_t)sizeof(Meta) * B);
  L.partial = take((int64_t)sizeof(Cand) * max_groups(n) * B * kTop);
  L.lids = take((int64_t)sizeof(int32_t) * cap);
  L.live = take((int64_t)sizeof(int32_t) * cap);
  L.grow = take((int64_t)sizeof(float) * G * cap);
  L.gcol = take((int64_t)sizeof(float) * G * cap);
  L.bytes = at;
  return L;
}

int check_sizes(const char* who, int64_t n, int64_t Hd, int64_t B, int32_t G, int64_t cap) {
  if (n < 1) return fail(WG_ERR_INVALID, "%s: n=%lld", who, (long long)n);
  if (n > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld exceeds int32", who, (long long)n);
  if (Hd < 1 || B < 1) return fail(WG_ERR_INVALID, "%s: Hd=%lld B=%lld must be >= 1", who, (long long)Hd, (long long)B);
  if (Hd > 256) return fail(WG_ERR_UNSUPPORTED, "%s: Hd=%lld above 256", who, (long long)Hd);
  if (B > (1 << 20)) return fail(WG_ERR_UNSUPPORTED, "%s: B=%lld above %d", who, (long long)B, 1 << 20);
  if (G != 1 && G != 3) return fail(WG_ERR_INVALID, "%s: G=%d is neither 1 nor 3", who, (int)G);
  if (cap < 0) return fail(WG_ERR_INVALID, "%s: local_cap=%lld is negative", who, (long long)cap);
  if (cap > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "%s: local_cap=%lld exceeds int32", who, (long long)cap);
  return WG_OK;
}

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_fga_scores_workspace(int64_t n, int64_t Hd, int64_t B, int32_t G, int64_t local_cap, int64_t* bytes) {
  if (!bytes) return fail(WG_ERR_INVALID, "wg_fga_scores_workspace: NULL bytes");
  if (int rc = check_sizes("wg_fga_scores_workspace", n, Hd, B, G, local_cap)) return rc;
  *bytes = layout(n, Hd, B, G, local_cap).bytes;
  return WG_OK;
}

int wg_fga_scores(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t Hd, const float* z,
                  const float* h, const float* b1, const float* W2, int64_t C, int64_t B, const int32_t* targets,
                  const int32_t* tog_ptr, const int32_t* tog_ids, int32_t G, const float* g_logits, const int32_t* rerank,
                  const float* p_top2, int32_t topk, int32_t n_workgroups, int64_t local_cap, void* workspace,
                  float* grads, float* scores, int32_t* best_ids, float* best_scores, void* stream_) {
  if (int rc = check_sizes("wg_fga_scores", n, Hd, B, G, local_cap)) return rc;
  if (nnz < 0) return fail(WG_ERR_INVALID, "wg_fga_scores: nnz=%lld", (long long)nnz);
  if (nnz > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "wg_fga_scores: nnz=%lld exceeds int32", (long long)nnz);
  if (C < 1) return fail(WG_ERR_INVALID, "wg_fga_scores: C=%lld must be >= 1", (long long)C);
  if (C > 256) return fail(WG_ERR_UNSUPPORTED, "wg_fga_scores: C=%lld above 256", (long long)C);
  if (topk < 1 || topk > kTop) return fail(WG_ERR_INVALID, "wg_fga_scores: topk=%d outside [1, %d]", (int)topk, kTop);
  if (n_workgroups < 0 || n_workgroups > kMaxGroups)
    return fail(WG_ERR_INVALID, "wg_fga_scores: n_workgroups=%d outside [0, %d]", (int)n_workgroups, kMaxGroups);
  if (!indptr || !z || !h || !b1 || !W2 || !targets || !tog_ptr || !g_logits || !best_ids || !best_scores)
    return fail(WG_ERR_INVALID,
                "wg_fga_scores: NULL indptr / z / h / b1 / W2 / targets / tog_ptr / g_logits / best_ids / best_scores");
  if (nnz > 0 && !indices) return fail(WG_ERR_INVALID, "wg_fga_scores: NULL indices with nnz=%lld", (long long)nnz);
  if (G == 3 && rerank && !p_top2) return fail(WG_ERR_INVALID, "wg_fga_scores: NULL p_top2 with the rerank");
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u))
    return fail(WG_ERR_INVALID, "wg_fga_scores: workspace is NULL or not 16-byte aligned");
  const int groups = std::min(n_workgroups ? (int)n_workgroups : max_groups(n), max_groups(n));
  const Layout L = layout(n, Hd, B, G, local_cap);
  char* ws = static_cast<char*>(workspace);
  Args a;
  a.n = n, a.Hd = Hd, a.C = C, a.B = B, a.HdP = padded(Hd), a.cap = local_cap, a.G = G, a.topk = topk;
  a.indptr = indptr, a.indices = indices, a.z = z, a.h = h, a.b1 = b1, a.W2 = W2, a.targets = targets;
  a.tog_ptr = tog_ptr, a.tog_ids = tog_ids, a.g_logits = g_logits, a.rerank = G == 3 ? rerank : nullptr, a.p_top2 = p_top2;
  a.co = reinterpret_cast<double*>(ws + L.co), a.tmp = reinterpret_cast<double*>(ws + L.tmp);
  a.meta = reinterpret_cast<Meta*>(ws + L.meta), a.partial = reinterpret_cast<Cand*>(ws + L.partial);
  a.lids = reinterpret_cast<int32_t*>(ws + L.lids), a.live = reinterpret_cast<int32_t*>(ws + L.live);
  a.grow = reinterpret_cast<float*>(ws + L.grow), a.gcol = reinterpret_cast<float*>(ws + L.gcol);
  a.grads = grads, a.scores = scores;
  hipStream_t stream = as_stream(stream_);
  hipLaunchKernelGGL(fga_local_kernel, dim3((unsigned)B), dim3(kBlock), 0, stream, a);
  WG_LAUNCH_CHECK();
  if (G == 3) hipLaunchKernelGGL(fga_score_kernel<3>, dim3((unsigned)groups), dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL(fga_score_kernel<1>, dim3((unsigned)groups), dim3(kBlock), 0, stream, a);
  WG_LAUNCH_CHECK();
  hipLaunchKernelGGL(fga_merge_kernel, dim3((unsigned)B), dim3(64), 0, stream, a.partial, groups, B, (int)topk, best_ids,
                     best_scores);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // extern "C"
