// attack.hip -- one step of the calibration attacks on the sparse path (DESIGN.md 4.3 "Attack step").
// calib_attack/calib_fga.py scores the n partners of the target t from the gradient's row and column t,
// flips the argmax (:880-898) and evaluates the model on the flipped graph to read one output row (:907-910).
//
//   flip_select_kernel     the scores of all n partners and the top-k of each workgroup's share, in one
//                          pass: a_j by binary search in row t of the base CSR and in the sorted list of
//                          partners already toggled; every float32 operation is the one torch performs on
//                          the same tensors (contraction off: no fused multiply-add)
//   flip_merge_kernel      the workgroups' partial lists merged by one workgroup (a second launch)
//   target_logits_kernel   the logits of node t under B candidate adjacencies, one workgroup per candidate,
//                          from the 2-hop ball of t alone: float64 sums in a fixed order, rounded once.  The same
//                          kernel evaluates the trials of the random attacks (calib_random.py:127-186,
//                          calib_rnd.py:169-236): a target per candidate, t itself among the partners (its self
//                          loop), and deltas of the target's own feature row carried as dz = W1 delta
//
// Ranking is a total order on (score, index) -- a NaN above every number, equal scores by smaller index,
// -0 == +0 -- packed into one 64-bit key whose maximum is the winner, so the result cannot depend on how
// the partners are dealt to workgroups.
#include <algorithm>
#include <climits>
#include <cstdint>

#include "internal.h"

#pragma clang fp contract(off)

namespace wg {
namespace {

constexpr int kWaves = kBlock / 64;
constexpr int kTop = 8;           // the largest topk
constexpr int kSelGroups = 256;   // the most workgroups of one selection
constexpr int kLongRow = 128;     // target_logits: rows from this length are shared by the workgroup
constexpr int kLongList = 64;     // ... and this many of them are remembered from the first pass (more: a second scan)

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

// a thread's best kTop so far, descending
struct TopList {
  Cand c[kTop];
  __device__ void clear() {
#pragma unroll
    for (int i = 0; i < kTop; ++i) c[i] = Cand{0ull, 0.0f};
  }
  __device__ void insert(Cand v) {
    if (v.key <= c[kTop - 1].key) return;
#pragma unroll
    for (int i = kTop - 1; i >= 0; --i) {
      const bool above = i > 0 && c[i - 1].key < v.key;   // slot i takes its upper neighbour
      const bool here = c[i].key < v.key && !above;
      if (above) c[i] = c[i - 1];
      else if (here) c[i] = v;
    }
  }
  __device__ void pop() {
#pragma unroll
    for (int i = 0; i + 1 < kTop; ++i) c[i] = c[i + 1];
    c[kTop - 1] = Cand{0ull, 0.0f};
  }
};

// the workgroup's best `topk` of its threads' lists, in order, to out[0 .. topk)
__device__ inline void block_topk(TopList& mine, int topk, Cand* __restrict__ out) {
  __shared__ unsigned long long wave_best[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = 0; r < topk; ++r) {
    unsigned long long best = mine.c[0].key;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off, 64);
      best = o > best ? o : best;
    }
    if (lane == 0) wave_best[wave] = best;
    __syncthreads();
    best = wave_best[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) best = wave_best[w] > best ? wave_best[w] : best;
    if (best != 0ull && mine.c[0].key == best) {   // keys are distinct: one thread holds it
      out[r] = mine.c[0];
      mine.pop();
    } else if (best == 0ull && threadIdx.x == 0) {
      out[r] = Cand{0ull, 0.0f};
    }
    __syncthreads();   // wave_best is written again by the next round
  }
}

struct SelectArgs {
  int64_t n = 0, t = 0;
  const float* grad_loss = nullptr;
  const float* grad_pmax = nullptr;    // NULL (with grad_psmax): no rerank
  const float* grad_psmax = nullptr;
  const float* p_top2 = nullptr;
  const int64_t* indptr = nullptr;
  const int32_t* indices = nullptr;
  const float* values = nullptr;
  int64_t n_toggled = 0;
  const int32_t* toggled = nullptr;
  int topk = 1;
  float* scores = nullptr;
};

__device__ inline void write_best(const Cand* __restrict__ list, int topk, int32_t* __restrict__ best_ids,
                                  float* __restrict__ best_scores) {
  if ((int)threadIdx.x < topk) {
    const Cand c = list[threadIdx.x];
    best_ids[threadIdx.x] = c.key ? key_index(c.key) : -1;
    best_scores[threadIdx.x] = c.key ? c.score : -INFINITY;
  }
}

__global__ __launch_bounds__(kBlock) void flip_select_kernel(SelectArgs a, Cand* __restrict__ partial,
                                                             int32_t* __restrict__ best_ids,
                                                             float* __restrict__ best_scores) {
  __shared__ Cand mine_out[kTop];
  const int64_t s = a.indptr[a.t], e = a.indptr[a.t + 1];
  WG_DCHECK(s >= 0 && s <= e, "flip select: row %lld is [%lld, %lld)", (long long)a.t, (long long)s, (long long)e);
  const bool rerank = a.grad_pmax != nullptr;
  float p_max = 0.0f, p_smax = 0.0f;
  if (rerank) p_max = a.p_top2[0], p_smax = a.p_top2[1];
  TopList mine;
  mine.clear();
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.n; j += (int64_t)gridDim.x * kBlock) {
    // a_j: row t of the base, then the toggle v = 1 - 2 a, a += v (calib_fga.py:901-903)
    float aj = 0.0f;
    if (s < e) {
      const int64_t k = lower_bound(a.indices, s, e, (int32_t)j);
      WG_DCHECK(k == e || (a.indices[k] >= 0 && a.indices[k] < a.n), "flip select: column %d outside [0, %lld)",
                (int)a.indices[k], (long long)a.n);
      if (k < e && a.indices[k] == (int32_t)j) aj = a.values ? a.values[k] : 1.0f;
    }
    if (a.n_toggled > 0) {
      const int64_t q = lower_bound(a.toggled, 0, a.n_toggled, (int32_t)j);
      WG_DCHECK(q == a.n_toggled || (a.toggled[q] >= 0 && a.toggled[q] < a.n && (q == 0 || a.toggled[q - 1] < a.toggled[q])),
                "flip select: toggled[%lld] = %d is outside [0, %lld) or not ascending", (long long)q, (int)a.toggled[q],
                (long long)a.n);
      if (q < a.n_toggled && a.toggled[q] == (int32_t)j) {
        const float v = 1.0f - 2.0f * aj;
        aj = aj + v;
      }
    }
    const float d = 1.0f - 2.0f * aj;
    float sc = (a.grad_loss[j] + a.grad_loss[a.n + j]) * d;
    if (rerank) {   // the row half only (div_pmax[target_node], calib_fga.py:893)
      const float c = ((p_max + a.grad_pmax[j] * d) - p_smax) - a.grad_psmax[j] * d;
      const float flag = c > 0.0f ? 1.0f : -1.0f;   // a NaN condition: -1
      sc = sc * flag;
    }
    if (j == a.t) sc = -10.0f;
    if (a.scores) a.scores[j] = sc;
    mine.insert(Cand{rank_key(sc, (int32_t)j), sc});
  }
  if (gridDim.x == 1) {
    block_topk(mine, a.topk, mine_out);
    __syncthreads();
    write_best(mine_out, a.topk, best_ids, best_scores);
  } else {
    block_topk(mine, a.topk, partial + (int64_t)blockIdx.x * a.topk);
  }
}

__global__ __launch_bounds__(kBlock) void flip_merge_kernel(const Cand* __restrict__ partial, int n_partial, int topk,
                                                            int32_t* __restrict__ best_ids,
                                                            float* __restrict__ best_scores) {
  __shared__ Cand merged[kTop];
  TopList mine;
  mine.clear();
  for (int i = threadIdx.x; i < n_partial; i += kBlock) mine.insert(partial[i]);
  block_topk(mine, topk, merged);
  __syncthreads();
  write_best(merged, topk, best_ids, best_scores);
}

// ---------------------------------------------------------------- the candidates' logits
struct LogitArgs {
  int64_t n = 0, Hd = 0, C = 0, t = 0;
  const int64_t* indptr = nullptr;
  const int32_t* indices = nullptr;
  const float* z = nullptr;    // (n, Hd)
  const float* b1 = nullptr;   // [Hd]
  const float* W2 = nullptr;   // (C, Hd)
  const float* b2 = nullptr;   // [C]
  const int32_t* cand_ptr = nullptr;
  const int32_t* cand_ids = nullptr;
  float* out = nullptr;        // (B, C)
  // the trials (wg_trial_logits); all NULL for wg_target_logits
  const int32_t* trial_t = nullptr;     // [B]: candidate b's own target, which may be among its partners
  int64_t nfeat = 0;
  const float* W1 = nullptr;            // (Hd, nfeat)
  const int32_t* feat_ptr = nullptr;    // [B + 1]; NULL: no feature deltas
  const int32_t* feat_ids = nullptr;
  const float* feat_delta = nullptr;
};

__device__ inline bool contains(const int32_t* __restrict__ a, int64_t len, int32_t key) {
  const int64_t k = lower_bound(a, 0, len, key);
  return k < len && a[k] == key;
}

// one j of N'(t): its row under the toggle set T (the partners whose entry in row j differs from the base)
struct Item {
  bool live = false;
  bool has_t = false;   // t is in N'(j): the row gathers z_t, so it carries dz (read with feature deltas only)
  int64_t j = 0, s = 0, len = 0, deg = 0;
  const int32_t* T = nullptr;
  int nT = 0;
};

// acc += the rows z_k of N'(j) that sub-group g of G takes: the base row's entries that T leaves, in the sub-group's
// stride, then the partners T adds.  Loads are unconditional (an index past the end reads the row's last entry and
// is not added) so that a batch's ids, then its rows of z, are in flight together
template <int W, bool VEC>
__device__ inline void row_sum(const LogitArgs& a, const Item& it, int g, int G, const int64_t* fo, double* acc) {
  constexpr int kBatch = 4;
  const int32_t* row = a.indices + it.s;
  for (int64_t i0 = g; i0 < it.len; i0 += (int64_t)G * kBatch) {
    int32_t k[kBatch];
    bool on[kBatch];
    float xv[kBatch][4];
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const int64_t i = i0 + (int64_t)b * G;
      on[b] = i < it.len;
      k[b] = row[on[b] ? i : it.len - 1];
      WG_DCHECK(k[b] >= 0 && k[b] < a.n, "target logits: row %lld column %d outside [0, %lld)", (long long)it.j, (int)k[b],
                (long long)a.n);
    }
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const float* zk = a.z + (int64_t)k[b] * a.Hd;
      if (VEC) {
        const float4 u = reinterpret_cast<const float4*>(zk)[fo[0]];
        xv[b][0] = u.x, xv[b][1] = u.y, xv[b][2] = u.z, xv[b][3] = u.w;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) xv[b][c] = zk[fo[c]];
      }
    }
    if (it.nT > 0) {
#pragma unroll
      for (int b = 0; b < kBatch; ++b) on[b] = on[b] && !contains(it.T, it.nT, k[b]);
    }
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] += on[b] ? (double)xv[b][c] : 0.0;
    }
  }
  for (int q = g; q < it.nT; q += G) {
    const int32_t k = it.T[q];
    WG_DCHECK(k >= 0 && k < a.n, "target logits: partner %d outside [0, %lld)", (int)k, (long long)a.n);
    if (contains(row, it.len, k)) continue;
    const float* zk = a.z + (int64_t)k * a.Hd;
    if (VEC) {
      const float4 u = reinterpret_cast<const float4*>(zk)[fo[0]];
      acc[0] += (double)u.x, acc[1] += (double)u.y, acc[2] += (double)u.z, acc[3] += (double)u.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] += (double)zk[fo[c]];
    }
  }
}

template <int W, bool VEC>
__global__ __launch_bounds__(kBlock) void target_logits_kernel(LogitArgs a) {
  constexpr int kSubWave = 64 / W;   // sub-groups per wave
  __shared__ double red[kWaves][W][4];
  __shared__ double y2[256];
  __shared__ double dz_sh[256];
  __shared__ int32_t t_sh;
  __shared__ int inter_sh, long_sh;
  __shared__ int32_t long_list[kLongList];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (W - 1), slot = lane / W;
  const int32_t c0 = a.cand_ptr[blockIdx.x], c1 = a.cand_ptr[blockIdx.x + 1];
  WG_DCHECK(c0 >= 0 && c0 <= c1, "target logits: candidate %d is [%d, %d)", (int)blockIdx.x, (int)c0, (int)c1);
  const int32_t* S = a.cand_ids + c0;
  const int nS = c1 - c0;
  const bool trial = a.trial_t != nullptr;
  const int64_t t = trial ? (int64_t)a.trial_t[blockIdx.x] : a.t;
  WG_DCHECK(t >= 0 && t < a.n, "target logits: candidate %d target %lld outside [0, %lld)", (int)blockIdx.x, (long long)t,
            (long long)a.n);
  const int64_t st = a.indptr[t], lt = a.indptr[t + 1] - st;
  const int32_t* Nt = a.indices + st;
  if (threadIdx.x == 0) t_sh = (int32_t)t, inter_sh = 0, long_sh = 0;
  // dz = W1 delta of the target's own feature row: one thread per hidden unit, the features in ascending order
  const bool feat = a.feat_ptr != nullptr;
  if (feat && (int64_t)threadIdx.x < a.Hd) {
    const int32_t f0 = a.feat_ptr[blockIdx.x], f1 = a.feat_ptr[blockIdx.x + 1];
    WG_DCHECK(f0 >= 0 && f0 <= f1, "trial logits: trial %d features are [%d, %d)", (int)blockIdx.x, (int)f0, (int)f1);
    const float* w = a.W1 + (int64_t)threadIdx.x * a.nfeat;
    double d = 0.0;
    for (int32_t q = f0; q < f1; ++q) {
      const int32_t f = a.feat_ids[q];
      WG_DCHECK(f >= 0 && f < a.nfeat && (q == f0 || a.feat_ids[q - 1] < f),
                "trial logits: trial %d feature %d is outside [0, %lld) or not ascending", (int)blockIdx.x, (int)f,
                (long long)a.nfeat);
      d += (double)a.feat_delta[q] * (double)w[f];
    }
    dz_sh[threadIdx.x] = d;
  }
  __syncthreads();
  int hits = 0;
  for (int q = threadIdx.x; q < nS; q += kBlock) {
    WG_DCHECK(S[q] >= 0 && S[q] < a.n && (trial || S[q] != t) && (q == 0 || S[q - 1] < S[q]),
              "target logits: candidate %d partner %d is outside [0, %lld), the target or not ascending", (int)blockIdx.x,
              (int)S[q], (long long)a.n);
    hits += contains(Nt, lt, S[q]) ? 1 : 0;
  }
  if (hits) atomicAdd(&inter_sh, hits);
  __syncthreads();
  const int64_t deg_t = lt + nS - 2 * (int64_t)inter_sh;   // |N(t) delta S|
  // the lane's columns, clamped into the row (a clamped lane's sums are never read)
  int64_t fo[4];
  bool valid[4];
  if (VEC) {
    fo[0] = std::min<int64_t>(sub, (a.Hd >> 2) - 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) valid[c] = sub < (a.Hd >> 2);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      valid[c] = sub + (int64_t)c * W < a.Hd;
      fo[c] = std::min<int64_t>(sub + (int64_t)c * W, a.Hd - 1);
    }
  }
  double bias[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bias[c] = (double)a.b1[VEC ? std::min<int64_t>(4 * fo[0] + c, a.Hd - 1) : fo[c]];
  double dz[4] = {0.0, 0.0, 0.0, 0.0};
  if (feat) {
#pragma unroll
    for (int c = 0; c < 4; ++c) dz[c] = dz_sh[VEC ? std::min<int64_t>(4 * fo[0] + c, a.Hd - 1) : fo[c]];
  }

  // item i: the base row's entries, then the candidate's partners; dead when the toggle removes it
  auto item = [&](int64_t i) {
    Item it;
    if (i < lt) {
      it.j = Nt[i];
      WG_DCHECK(it.j >= 0 && it.j < a.n, "target logits: row %lld column %lld outside [0, %lld)", (long long)t,
                (long long)it.j, (long long)a.n);
      it.live = !contains(S, nS, (int32_t)it.j);
    } else {
      it.j = S[i - lt];
      it.live = !contains(Nt, lt, (int32_t)it.j);
    }
    it.s = a.indptr[it.j];
    it.len = a.indptr[it.j + 1] - it.s;
    if (it.j == t) {
      it.T = S, it.nT = nS, it.deg = deg_t;
      it.has_t = true;           // a live item j == t: the self loop is in N'(t)
    } else if (i >= lt) {
      const bool in_base = contains(a.indices + it.s, it.len, (int32_t)t);
      it.T = &t_sh, it.nT = 1;
      it.deg = it.len + 1 - 2 * (in_base ? 1 : 0);
      it.has_t = !in_base;
    } else {
      it.deg = it.len;
      if (feat) it.has_t = contains(a.indices + it.s, it.len, (int32_t)t);   // asked of the row: no symmetry assumed
    }
    return it;
  };
  // h_j = max(y1_j + b1, 0) of the finished row sum, added to hs
  auto add_h = [&](const double* sum, int64_t deg, bool with_dz, double* hs) {
    const double inv = 1.0 / (double)(deg > 0 ? deg : 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double h = inv * (with_dz ? sum[c] + dz[c] : sum[c]) + bias[c];
      hs[c] += h > 0.0 ? h : 0.0;
    }
  };

  const int64_t n_items = lt + nS;
  double hs[4] = {0.0, 0.0, 0.0, 0.0};
  // short rows: wave w takes the items w, w + kWaves, ...
  for (int64_t i = wave; i < n_items; i += kWaves) {
    const Item it = item(i);
    if (!it.live) continue;
    if (it.len >= kLongRow) {
      if (lane == 0) {
        const int p = atomicAdd(&long_sh, 1);
        if (p < kLongList) long_list[p] = (int32_t)i;
      }
      continue;
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    row_sum<W, VEC>(a, it, slot, kSubWave, fo, acc);
#pragma unroll
    for (int off = 32; off >= W; off >>= 1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] += __shfl_down(acc[c], off, 64);
    }
    add_h(acc, it.deg, feat && it.has_t, hs);   // meaningful in the lanes below W
  }
  __syncthreads();
  // long rows in ascending item order: the whole workgroup per row, the waves' sums in wave order, h into wave
  // 0's share.  The remembered items are taken smallest first (their arrival order is not fixed)
  const int n_long = long_sh;
  if (n_long) {
    const bool listed = n_long <= kLongList;
    int64_t last = -1;
    for (int64_t r = 0; r < (listed ? (int64_t)n_long : n_items); ++r) {
      int64_t i = r;
      if (listed) {
        i = INT64_MAX;
        for (int q = 0; q < n_long; ++q) i = (long_list[q] > last && long_list[q] < i) ? long_list[q] : i;
        last = i;
      }
      const Item it = item(i);                      // uniform over the workgroup
      if (!it.live || it.len < kLongRow) continue;
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      row_sum<W, VEC>(a, it, wave * kSubWave + slot, kWaves * kSubWave, fo, acc);
#pragma unroll
      for (int off = 32; off >= W; off >>= 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] += __shfl_down(acc[c], off, 64);
      }
      if (lane < W) {
#pragma unroll
        for (int c = 0; c < 4; ++c) red[wave][sub][c] = acc[c];
      }
      __syncthreads();
      if (threadIdx.x < W) {
        double tot[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          tot[c] = red[0][sub][c];
#pragma unroll
          for (int w = 1; w < kWaves; ++w) tot[c] += red[w][sub][c];
        }
        add_h(tot, it.deg, feat && it.has_t, hs);
      }
      __syncthreads();   // red is written again by the next long row
    }
  }
  // y2 = (1 / deg'_t) sum_j h_j: the waves' shares in wave order
  if (lane < W) {
#pragma unroll
    for (int c = 0; c < 4; ++c) red[wave][sub][c] = hs[c];
  }
  __syncthreads();
  if (threadIdx.x < W) {
    const double inv = 1.0 / (double)(deg_t > 0 ? deg_t : 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double tot = red[0][sub][c];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) tot += red[w][sub][c];
      const int64_t f = VEC ? 4 * (int64_t)sub + c : sub + (int64_t)c * W;
      if (valid[c]) y2[f] = inv * tot;
    }
  }
  __syncthreads();
  // out = W2 y2 + b2, one thread per class, columns in ascending order
  if ((int64_t)threadIdx.x < a.C) {
    const float* w = a.W2 + (int64_t)threadIdx.x * a.Hd;
    double acc = 0.0;
    for (int64_t f = 0; f < a.Hd; ++f) acc += (double)w[f] * y2[f];
    a.out[(int64_t)blockIdx.x * a.C + threadIdx.x] = (float)(acc + (double)a.b2[threadIdx.x]);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// what wg_target_logits and wg_trial_logits check alike, before any device call
int check_sizes(const char* who, int64_t n, int64_t nnz, int64_t Hd, int64_t C, int64_t B) {
  if (n < 1 || nnz < 0) return fail(WG_ERR_INVALID, "%s: n=%lld nnz=%lld", who, (long long)n, (long long)nnz);
  if (n > INT32_MAX || nnz > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld or nnz=%lld exceeds int32", who, (long long)n, (long long)nnz);
  if (Hd < 1 || C < 1 || B < 1)
    return fail(WG_ERR_INVALID, "%s: Hd=%lld C=%lld B=%lld must be >= 1", who, (long long)Hd, (long long)C, (long long)B);
  if (Hd > 256 || C > 256) return fail(WG_ERR_UNSUPPORTED, "%s: Hd=%lld or C=%lld above 256", who, (long long)Hd, (long long)C);
  if (B > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "%s: B=%lld exceeds int32", who, (long long)B);
  return WG_OK;
}

int check_pointers(const char* who, int64_t nnz, const int64_t* indptr, const int32_t* indices, const float* z,
                   const float* b1, const float* W2, const float* b2, const int32_t* cand_ptr, const float* out) {
  if (!indptr || !z || !b1 || !W2 || !b2 || !cand_ptr || !out)
    return fail(WG_ERR_INVALID, "%s: NULL indptr / z / b1 / W2 / b2 / cand_ptr / out", who);
  if (nnz > 0 && !indices) return fail(WG_ERR_INVALID, "%s: NULL indices with nnz=%lld", who, (long long)nnz);
  return WG_OK;
}

int launch_logits(const LogitArgs& a, int64_t B, void* stream_) {
  int W = 1;
  while (W < 64 && W < ceil_div(a.Hd, 4)) W <<= 1;
  const bool vec = (a.Hd % 4 == 0) && aligned16(a.z);
  const dim3 grid((unsigned)B), block(kBlock);
  hipStream_t stream = as_stream(stream_);
#define WG_TARGET_CASE(w)                                                                     \
  case w:                                                                                     \
    if (vec) hipLaunchKernelGGL((target_logits_kernel<w, true>), grid, block, 0, stream, a);  \
    else hipLaunchKernelGGL((target_logits_kernel<w, false>), grid, block, 0, stream, a);     \
    break;
  switch (W) {
    WG_TARGET_CASE(1)
    WG_TARGET_CASE(2)
    WG_TARGET_CASE(4)
    WG_TARGET_CASE(8)
    WG_TARGET_CASE(16)
    WG_TARGET_CASE(32)
    WG_TARGET_CASE(64)
  }
#undef WG_TARGET_CASE
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_target_long_row(void) { return kLongRow; }

int wg_target_logits(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t Hd, const float* z,
                     const float* b1, const float* W2, const float* b2, int64_t C, int64_t t, int64_t B,
                     const int32_t* cand_ptr, const int32_t* cand_ids, float* out, void* stream_) {
  if (const int rc = check_sizes("wg_target_logits", n, nnz, Hd, C, B)) return rc;
  if (t < 0 || t >= n) return fail(WG_ERR_INVALID, "wg_target_logits: target %lld outside [0, %lld)", (long long)t, (long long)n);
  if (const int rc = check_pointers("wg_target_logits", nnz, indptr, indices, z, b1, W2, b2, cand_ptr, out)) return rc;
  LogitArgs a;
  a.n = n, a.Hd = Hd, a.C = C, a.t = t, a.indptr = indptr, a.indices = indices, a.z = z, a.b1 = b1, a.W2 = W2, a.b2 = b2;
  a.cand_ptr = cand_ptr, a.cand_ids = cand_ids, a.out = out;
  return launch_logits(a, B, stream_);
}

int wg_trial_logits(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t Hd, const float* z,
                    const float* b1, const float* W2, const float* b2, int64_t C, int64_t B, const int32_t* trial_t,
                    const int32_t* cand_ptr, const int32_t* cand_ids, int64_t nfeat, const float* W1,
                    const int32_t* feat_ptr, const int32_t* feat_ids, const float* feat_delta, float* out, void* stream_) {
  if (const int rc = check_sizes("wg_trial_logits", n, nnz, Hd, C, B)) return rc;
  if (const int rc = check_pointers("wg_trial_logits", nnz, indptr, indices, z, b1, W2, b2, cand_ptr, out)) return rc;
  if (!trial_t) return fail(WG_ERR_INVALID, "wg_trial_logits: NULL trial_t");
  if (feat_ptr) {
    if (nfeat < 1) return fail(WG_ERR_INVALID, "wg_trial_logits: nfeat=%lld with feature deltas", (long long)nfeat);
    if (nfeat > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "wg_trial_logits: nfeat=%lld exceeds int32", (long long)nfeat);
    if (!W1) return fail(WG_ERR_INVALID, "wg_trial_logits: NULL W1 with feature deltas");
    if ((feat_ids == nullptr) != (feat_delta == nullptr))
      return fail(WG_ERR_INVALID, "wg_trial_logits: feat_ids and feat_delta are both given or both NULL");
  }
  LogitArgs a;
  a.n = n, a.Hd = Hd, a.C = C, a.t = 0, a.indptr = indptr, a.indices = indices, a.z = z, a.b1 = b1, a.W2 = W2, a.b2 = b2;
  a.cand_ptr = cand_ptr, a.cand_ids = cand_ids, a.out = out, a.trial_t = trial_t;
  if (feat_ptr) a.nfeat = nfeat, a.W1 = W1, a.feat_ptr = feat_ptr, a.feat_ids = feat_ids, a.feat_delta = feat_delta;
  return launch_logits(a, B, stream_);
}

int wg_flip_select_workspace(int64_t* bytes) {
  if (!bytes) return fail(WG_ERR_INVALID, "wg_flip_select_workspace: NULL bytes");
  *bytes = (int64_t)sizeof(Cand) * kSelGroups * kTop;
  return WG_OK;
}

int wg_flip_select(int64_t n, int64_t t, const float* grad_loss, const float* grad_pmax, const float* grad_psmax,
                   const float* p_top2, const int64_t* indptr, const int32_t* indices, const float* values,
                   int64_t n_toggled, const int32_t* toggled, int32_t topk, int32_t n_workgroups, void* workspace,
                   float* scores, int32_t* best_ids, float* best_scores, void* stream_) {
  if (n < 0 || n_toggled < 0)
    return fail(WG_ERR_INVALID, "wg_flip_select: negative size (n=%lld n_toggled=%lld)", (long long)n, (long long)n_toggled);
  if (n > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "wg_flip_select: n=%lld exceeds int32", (long long)n);
  if (topk < 1 || topk > kTop) return fail(WG_ERR_INVALID, "wg_flip_select: topk=%d outside [1, %d]", (int)topk, kTop);
  if (n_workgroups < 0 || n_workgroups > kSelGroups)
    return fail(WG_ERR_INVALID, "wg_flip_select: n_workgroups=%d outside [0, %d]", (int)n_workgroups, kSelGroups);
  if (n == 0) return WG_OK;
  if (t < 0 || t >= n) return fail(WG_ERR_INVALID, "wg_flip_select: target %lld outside [0, %lld)", (long long)t, (long long)n);
  if (n_toggled > n) return fail(WG_ERR_INVALID, "wg_flip_select: %lld toggled partners of %lld", (long long)n_toggled, (long long)n);
  if ((grad_pmax == nullptr) != (grad_psmax == nullptr))
    return fail(WG_ERR_INVALID, "wg_flip_select: grad_pmax and grad_psmax are both given or both NULL");
  if (grad_pmax && !p_top2) return fail(WG_ERR_INVALID, "wg_flip_select: NULL p_top2 with the rerank");
  if (!grad_loss || !indptr || !best_ids || !best_scores)
    return fail(WG_ERR_INVALID, "wg_flip_select: NULL grad_loss / indptr / best_ids / best_scores");
  if (n_toggled > 0 && !toggled) return fail(WG_ERR_INVALID, "wg_flip_select: NULL toggled with n_toggled=%lld", (long long)n_toggled);
  const int groups = n_workgroups ? n_workgroups : (int)std::min<int64_t>(ceil_div(n, kBlock), kSelGroups);
  if (groups > 1 && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u)))
    return fail(WG_ERR_INVALID, "wg_flip_select: workspace is NULL or not 8-byte aligned with %d workgroups", groups);
  SelectArgs a;
  a.n = n, a.t = t, a.grad_loss = grad_loss, a.grad_pmax = grad_pmax, a.grad_psmax = grad_psmax, a.p_top2 = p_top2;
  a.indptr = indptr, a.indices = indices, a.values = values, a.n_toggled = n_toggled, a.toggled = toggled;
  a.topk = topk, a.scores = scores;
  hipStream_t stream = as_stream(stream_);
  Cand* partial = static_cast<Cand*>(workspace);
  hipLaunchKernelGGL(flip_select_kernel, dim3((unsigned)groups), dim3(kBlock), 0, stream, a, partial, best_ids, best_scores);
  WG_LAUNCH_CHECK();
  if (groups > 1) {
    hipLaunchKernelGGL(flip_merge_kernel, dim3(1), dim3(kBlock), 0, stream, partial, groups * (int)topk, (int)topk,
                       best_ids, best_scores);
    WG_LAUNCH_CHECK();
  }
  return WG_OK;
}

}  // extern "C"
