// edgemlp.hip -- the edge MLP of the DCGC calibrator (reference calibration/DCGC.py:36-44, :66-79).  The reference
// gathers [emb_r ; emb_c] for every stored entry (r, c) of the adjacency into an (E, 2C) tensor, runs a
// 2C -> 4C -> 2C -> 1 MLP with ReLU and dropout over it and keeps every (E, k) activation for autograd.  Here no
// (E, k) buffer exists: the forward (wg_edge_mlp_forward) keeps an entry's activations in registers, and the
// backward (wg_edge_mlp_backward) recomputes them per tile.
//
//     z1 = W1 [emb_r ; emb_c] + b1    h1 = D1 * relu(z1)    z2 = W2 h1 + b2    h2 = D2 * relu(z2)
//     z3 = w3 . h2 + b3               w_e = relu(z3)
//
// Decomposition.  A wave owns 32 entries, one per lane pair (lanes l and l + 32 hold entry l & 31).  Every product
// is the TRANSPOSED one on v_mfma_f32_32x32x2_f32: the units of a layer are the M side, the entries the N side, so
// an activation tile is "unit acc_row(r, h) of a 32-unit block in register r, entry on the lane" and ReLU, dropout
// and the last layer run per lane.  The k-steps of the next product take that accumulator as it stands: step r of
// block b contracts the units 32 b + acc_row(r, 0) and 32 b + acc_row(r, 1); the weights are packed once per call
// into that operand order (pack_kernel: one coalesced 256-byte read per MFMA, no LDS), so no activation is moved.
// The input operand is gathered straight from emb into registers (2C values per entry, zero padded to 32 NB0).
//
// Backward.  Pass 1 walks the entries in CSR order in tiles of kMlpTile = 1024 (8 turns of 128, tile t on
// workgroup t mod G, G = min(tiles, 256)).  Per turn: recompute, d3 = g (z3 > 0), d2 = d3 w3 D2 (z2 > 0),
// d1 = (W2^T d2) D1 (z1 > 0) and, with g_emb, the first half of W1^T d1.  The weight gradients d2^T h1 and
// d1^T [emb_r ; emb_c] contract over the entries, so the operands are turned through LDS 32 entries at a time and
// every wave owns a quarter of the 32 x 32 output blocks: float32 MFMA chains over the turn's 128 entries in
// ascending order, added to the workgroup's float64 partial at the turn's end (chains over a whole tile measured
// twice the error of torch's blocked float32 product).  Bias and last-layer gradients are float64 sums of the
// staged rows (d3 h2 as a float64 product).  A last kernel adds the workgroups' partials in
// ascending order in float64 and rounds once.
//
// g_emb.  The half that belongs to the row sums over a row's entries, which are contiguous in CSR order; the half
// that belongs to the column is a second recomputing pass (no weight gradients) over the transposed order, with
// dropout and g_w looked up at the entry's CSR position through the transpose map.  In both a turn's 128 x C tile
// goes to LDS and one lane per column walks the entries in ascending order with a float64 sum per node; a node
// whose entries start in an earlier tile hands its part to a carry slot of the tile, and a fix-up kernel adds the
// carries in tile order.  One node's sum is never split over workgroups inside a tile, and a hub that spans tiles
// is added tile by tile.  No float atomics anywhere: the same input gives the same bits.
//
// Dropout: keep_bit() below, a stateless hash of (seed, layer, CSR position, unit); include/wats_hip.h specifies
// it.  p == 0 does no hashing.
//
// Limits.  1 <= C <= kMlpMaxC = 48 (the activations of 32 entries and a quarter of both weight gradients live in a
// wave's registers; wider is WG_ERR_UNSUPPORTED).
#include <climits>
#include <cmath>
#include <cstdint>

#include "internal.h"

namespace wg {
namespace {

constexpr int kMlpMaxC = 48;
constexpr int kTurn = 128;                   // entries per turn: 32 per wave
constexpr int kTurns = 8;
constexpr int kMlpTile = kTurn * kTurns;     // entries per workgroup tile
constexpr int kMlpMaxWG = 256;               // workgroups of a backward pass
constexpr int kLdw = 33;                     // LDS row stride of a staged [unit][32 entries] tile

using f32x16 = __attribute__((ext_vector_type(16))) float;

// The products are fully unrolled (the register tiles need constant indices); without a fence after every 16 MFMAs
// the scheduler hoists hundreds of operand loads to the top of the block and spills the activations to scratch.
#define WG_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

// A pack's base as a value the compiler cannot see through: the operand addresses are loop invariant, and hoisted
// out of the turn loop they would take two registers per MFMA (thousands in the backward).
__device__ __forceinline__ const float* opaque(const float* p) {
  asm volatile("" : "+v"(p));
  return p;
}

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// A product's 32-unit blocks of k are float32 MFMA chains of 32 terms each; the blocks meet in float64 (one
// sequential float32 chain over 4C = 160 terms measured twice the error of torch's blocked float32 product).
struct Acc64 {
  double v[16];
  __device__ __forceinline__ Acc64() {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = 0.0;
  }
  __device__ __forceinline__ void add(const f32x16& p) {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] += (double)p[r];
  }
};

__host__ __device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ uint64_t hash_base(uint64_t seed, int layer, uint64_t e) {
  return (seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)layer)) + e * 0xBF58476D1CE4E5B9ull;
}
__device__ __forceinline__ bool keep_bit(uint64_t base, uint32_t j, uint32_t thr) {
  uint64_t x = base + (uint64_t)j * 0x94D049BB133111EBull;
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (uint32_t)(x >> 32) >= thr;
}

struct MlpShape {
  int C, NB0, NB1, NBH, KH;
  int64_t w1p, w2p, w2tp, w1tp;   // floats of each pack
  int64_t P;                      // parameters
};

MlpShape shape_of(int64_t C) {
  MlpShape s;
  s.C = (int)C;
  s.NB0 = (int)ceil_div(2 * C, 32);
  s.NB1 = (int)ceil_div(4 * C, 32);
  s.NBH = (s.NB0 + 1) / 2;
  s.KH = 16 * s.NB0;
  s.w1p = (int64_t)s.NB1 * s.KH * 64;
  s.w2p = (int64_t)s.NB0 * s.NB1 * 16 * 64;
  s.w2tp = s.w2p;
  s.w1tp = (int64_t)s.NBH * s.NB1 * 16 * 64;
  s.P = 16 * C * C + 8 * C + 1;
  return s;
}

struct MlpWs {
  int32_t* rows;
  int32_t* trows;
  float *w1p, *w2p, *w2tp, *w1ta, *w1tb, *b1p, *b2p, *w3p;
  double *partial, *gacc, *carry;
  int64_t bytes;
};

inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

MlpWs carve(void* base, int64_t n, int64_t nnz, const MlpShape& s) {
  MlpWs w;
  char* p = static_cast<char*>(base);
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* q = p ? p + off : nullptr;
    off += align16(bytes);
    return q;
  };
  const int64_t tiles = ceil_div(nnz, kMlpTile);
  w.partial = reinterpret_cast<double*>(take(8 * s.P * kMlpMaxWG));
  w.gacc = reinterpret_cast<double*>(take(8 * n * s.C));
  w.carry = reinterpret_cast<double*>(take(8 * tiles * s.C));
  w.w1p = reinterpret_cast<float*>(take(4 * s.w1p));
  w.w2p = reinterpret_cast<float*>(take(4 * s.w2p));
  w.w2tp = reinterpret_cast<float*>(take(4 * s.w2tp));
  w.w1ta = reinterpret_cast<float*>(take(4 * s.w1tp));
  w.w1tb = reinterpret_cast<float*>(take(4 * s.w1tp));
  w.b1p = reinterpret_cast<float*>(take(4 * s.NB1 * 16 * 64));
  w.b2p = reinterpret_cast<float*>(take(4 * s.NB0 * 16 * 64));
  w.w3p = reinterpret_cast<float*>(take(4 * s.NB0 * 16 * 64));
  w.rows = reinterpret_cast<int32_t*>(take(4 * nnz));
  w.trows = reinterpret_cast<int32_t*>(take(4 * nnz));
  w.bytes = off;
  return w;
}

// kind 0: W1 as the A operand of layer 1; 1: W2 as the A operand of layer 2 (k in accumulator order);
// 2: W2^T for d1; 3 / 4: the emb_r / emb_c half of W1^T for g_emb; 5: a vector (W1 = the vector, C = its length) in
// accumulator order, out[(b * 16 + r) * 64 + lane] = vec[32 b + acc_row(r, lane >> 5)]
__global__ __launch_bounds__(kBlock) void pack_kernel(int kind, int C, int NB0, int NB1, int64_t count,
                                                      const float* __restrict__ W1, const float* __restrict__ W2,
                                                      float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= count) return;
  const int lane = (int)(idx & 63), m = lane & 31, h = lane >> 5;
  int64_t t = idx >> 6;
  float v = 0.f;
  if (kind == 0) {
    const int KH = 16 * NB0;
    const int kk = (int)(t % KH), b = (int)(t / KH);
    const int u = 32 * b + m, k = 2 * kk + h;
    if (u < 4 * C && k < 2 * C) v = W1[u * 2 * C + k];
  } else if (kind == 1) {
    const int r = (int)(t % 16);
    t /= 16;
    const int b1 = (int)(t % NB1), b2 = (int)(t / NB1);
    const int u2 = 32 * b2 + m, u1 = 32 * b1 + acc_row(r, h);
    if (u2 < 2 * C && u1 < 4 * C) v = W2[u2 * 4 * C + u1];
  } else if (kind == 2) {
    const int r = (int)(t % 16);
    t /= 16;
    const int b2 = (int)(t % NB0), b1 = (int)(t / NB0);
    const int u2 = 32 * b2 + acc_row(r, h), u1 = 32 * b1 + m;
    if (u2 < 2 * C && u1 < 4 * C) v = W2[u2 * 4 * C + u1];
  } else if (kind == 5) {
    const int u = 32 * (int)(t / 16) + acc_row((int)(t % 16), h);
    if (u < C) v = W1[u];
  } else {
    const int r = (int)(t % 16);
    t /= 16;
    const int b1 = (int)(t % NB1), bh = (int)(t / NB1);
    const int u1 = 32 * b1 + acc_row(r, h), f = 32 * bh + m;
    if (u1 < 4 * C && f < C) v = W1[u1 * 2 * C + (kind - 3) * C + f];
  }
  out[idx] = v;
}

// rows[p] = the row whose range [indptr[i], indptr[i + 1]) holds position p
__global__ __launch_bounds__(kBlock) void entry_rows_kernel(int64_t n, int64_t nnz, const int64_t* __restrict__ indptr,
                                                            int32_t* __restrict__ rows) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= nnz) return;
  int64_t lo = 0, hi = n;   // the last i in [0, n) with indptr[i] <= p
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (indptr[mid] <= p) lo = mid;
    else hi = mid;
  }
  rows[p] = (int32_t)lo;
}

struct MlpArgs {
  int64_t n, nnz;
  int C;
  const int32_t* seg;     // node of each position of the pass: rows (CSR order) / trows (transposed order)
  const int32_t* other;   // indices / t_indices
  const int32_t* pos;     // NULL (CSR order) or the transpose map
  const float* emb;
  const float *w1p, *w2p, *w2tp, *w1tp;
  const float *b1p, *b2p, *w3p, *b3;   // b1, b2, w3 in accumulator order
  uint32_t thr;
  float scale;
  uint64_t seed;
  int drop;
  const float* g_w;
  double *partial, *gacc, *carry;
  int64_t P;
};

// the entry of a lane: CSR position e, its row r and column c (valid: the position exists)
struct Entry {
  int64_t e;
  int32_t r, c, seg;
  bool valid;
};

__device__ __forceinline__ Entry load_entry(const MlpArgs& a, int64_t p, int64_t end) {
  Entry t;
  t.valid = p < end;
  t.e = 0;
  t.r = t.c = 0;
  t.seg = -1;
  if (t.valid) {
    WG_DCHECK(p >= 0 && p < a.nnz, "edgemlp: position %lld of %lld", (long long)p, (long long)a.nnz);
    const int32_t s = a.seg[p], o = a.other[p];
    t.seg = s;
    if (a.pos) {
      t.e = a.pos[p];
      t.r = o;
      t.c = s;
    } else {
      t.e = p;
      t.r = s;
      t.c = o;
    }
    WG_DCHECK(t.e >= 0 && t.e < a.nnz, "edgemlp: position %lld maps to entry %lld of %lld", (long long)p,
              (long long)t.e, (long long)a.nnz);
    WG_DCHECK(t.r >= 0 && t.r < a.n && t.c >= 0 && t.c < a.n, "edgemlp: entry %lld is (%d, %d) outside [0, %lld)",
              (long long)t.e, t.r, t.c, (long long)a.n);
  }
  return t;
}

template <int NB0>
__device__ __forceinline__ void load_input(float (&xa)[16 * NB0], const MlpArgs& a, const Entry& t, int h) {
  const int C = a.C;
  const float* er = a.emb + (int64_t)t.r * C;
  const float* ec = a.emb + (int64_t)t.c * C;
#pragma unroll
  for (int kk = 0; kk < 16 * NB0; ++kk) {
    const int k = 2 * kk + h;
    float x = 0.f;
    if (t.valid && k < 2 * C) x = k < C ? er[k] : ec[k - C];
    xa[kk] = x;
  }
}

// h1, h2 in accumulator layout (unit 32 b + acc_row(r, h) in register r of block b) and z3 (both lanes of an entry)
// h2lo (narrow layers only, NB0 == 1): what rounding h2 to float32 dropped, for the last layer's gradient
template <int NB0, int NB1>
__device__ __forceinline__ float mlp_forward(const MlpArgs& a, const float (&xa)[16 * NB0], int64_t e, int lane,
                                             f32x16 (&h1)[NB1], f32x16 (&h2)[NB0], f32x16* h2lo = nullptr) {
  constexpr int KH = 16 * NB0;
  const int h = lane >> 5;
  const uint64_t base1 = hash_base(a.seed, 1, (uint64_t)e), base2 = hash_base(a.seed, 2, (uint64_t)e);
#pragma unroll
  for (int b = 0; b < NB1; ++b) {
    Acc64 acc;
    const float* wp = opaque(a.w1p + (int64_t)b * KH * 64 + lane);
    const float* bp = opaque(a.b1p + b * 16 * 64 + lane);
#pragma unroll
    for (int k0 = 0; k0 < KH; k0 += 16) {
      f32x16 part = zero16();
#pragma unroll
      for (int kk = k0; kk < k0 + 16; ++kk)
        part = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[kk * 64], xa[kk], part, 0, 0, 0);
      acc.add(part);
      WG_SCHED_FENCE();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int u = 32 * b + acc_row(r, h);
      const float z = (float)(acc.v[r] + (double)bp[r * 64]);
      float v = z < 0.f ? 0.f : z;   // keeps a NaN
      if (a.drop) v = v * (keep_bit(base1, (uint32_t)u, a.thr) ? a.scale : 0.f);
      h1[b][r] = v;
    }
  }
#pragma unroll
  for (int b2 = 0; b2 < NB0; ++b2) {
    Acc64 acc;
    const float* wp = opaque(a.w2p + (int64_t)b2 * NB1 * 16 * 64 + lane);
    const float* bp = opaque(a.b2p + b2 * 16 * 64 + lane);
#pragma unroll
    for (int b1 = 0; b1 < NB1; ++b1) {
      f32x16 part = zero16();
#pragma unroll
      for (int r = 0; r < 16; ++r)
        part = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[(b1 * 16 + r) * 64], h1[b1][r], part, 0, 0, 0);
      acc.add(part);
      WG_SCHED_FENCE();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int u = 32 * b2 + acc_row(r, h);
      const double zd = acc.v[r] + (double)bp[r * 64];
      const float z = (float)zd;
      float v = z < 0.f ? 0.f : z;
      float keep = 1.f;
      if (a.drop) {
        keep = keep_bit(base2, (uint32_t)u, a.thr) ? a.scale : 0.f;
        v = v * keep;
      }
      h2[b2][r] = v;
      if (h2lo) h2lo[b2][r] = z > 0.f ? (float)((zd - (double)z) * (double)keep) : 0.f;
    }
  }
  double s = 0.0;
#pragma unroll
  for (int b2 = 0; b2 < NB0; ++b2) {
    const float* vp = opaque(a.w3p + b2 * 16 * 64 + lane);   // zero past 2C
#pragma unroll
    for (int r = 0; r < 16; ++r) s = fma((double)vp[r * 64], (double)h2[b2][r], s);
  }
  const double o = __shfl_xor(s, 32, 64);
  s = h == 0 ? s + o : o + s;   // lower half first in both lanes
  return (float)(s + (double)a.b3[0]);
}

template <int NB0, int NB1>
__global__ __launch_bounds__(kBlock) void edge_mlp_fwd_kernel(MlpArgs a, float* __restrict__ w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = (int64_t)blockIdx.x * kTurn + wave * 32 + (lane & 31);
  const Entry t = load_entry(a, p, a.nnz);
  float xa[16 * NB0];
  load_input<NB0>(xa, a, t, lane >> 5);
  f32x16 h1[NB1], h2[NB0];
  const float z3 = mlp_forward<NB0, NB1>(a, xa, t.e, lane, h1, h2);
  if (t.valid && lane < 32) w[t.e] = z3 < 0.f ? 0.f : z3;
}

// PARAM: the weight, bias and last-layer gradients (CSR pass); GEMB: this pass's half of g_emb
template <int NB0, int NB1, bool PARAM, bool GEMB>
__global__ __launch_bounds__(kBlock) void edge_mlp_bwd_kernel(MlpArgs a, int64_t n_tiles) {
  constexpr int NBH = (NB0 + 1) / 2;
  constexpr int NA = (NB0 * NB1 + 3) / 4;          // output blocks of a wave, either weight gradient
  constexpr int kStage = (NB1 + 2 * NB0 + (NB0 == 1 ? 1 : 0)) * 32 * kLdw + 32;
  constexpr int kCs = 32 * NBH + 1;                // row stride of the g_emb tile
  constexpr int kLds = PARAM ? kStage : (kTurn * kCs);
  __shared__ float lds[kLds > kTurn * kCs ? kLds : kTurn * kCs];
  __shared__ int32_t sseg[kTurn];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, m = lane & 31;
  const int C = a.C;
  const float sc = a.drop ? a.scale : 1.f;

  f32x16 accA[PARAM ? NA : 1], accC[PARAM ? NA : 1];
  double gb1 = 0.0, gb2 = 0.0, gw3 = 0.0, gb3 = 0.0;   // thread tid: unit tid of b1 / b2 / w3; thread 0: b3
  if constexpr (PARAM) {
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) accA[i][r] = accC[i][r] = 0.f;
  }
  float* H1s = lds;                                  // phase A: h1 | d2 | h2 | d3
  float* D2s = lds + NB1 * 32 * kLdw;
  float* P3s = D2s + NB0 * 32 * kLdw;
  float* D3s = P3s + NB0 * 32 * kLdw;
  float* L3s = D3s + 32;                             // NB0 == 1: h2's float32 rounding residue
  float* D1s = lds;                                  // phase C: d1 | input
  float* Fs = lds + NB1 * 32 * kLdw;

  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t p0 = tile * kMlpTile;
    const int64_t end = a.nnz < p0 + kMlpTile ? a.nnz : p0 + kMlpTile;
    const int turns = (int)((end - p0 + kTurn - 1) / kTurn);
    // the node walk of g_emb (threads tid < C): the current node, its sum, and whether the tile's first node began
    // in an earlier tile (its part goes to the tile's carry slot)
    int32_t cur = -1;
    double nsum = 0.0;
    bool lead = false;
    if constexpr (GEMB) lead = p0 > 0 && a.seg[p0 - 1] == a.seg[p0];

    for (int turn = 0; turn < turns; ++turn) {
      const int64_t p = p0 + (int64_t)turn * kTurn + wave * 32 + m;
      const Entry t = load_entry(a, p, end);
      float xa[16 * NB0];
      load_input<NB0>(xa, a, t, h);
      constexpr bool kLo = PARAM && NB0 == 1;
      f32x16 h1[NB1], h2[NB0], d2[NB0], h2lo[kLo ? NB0 : 1];
      const float z3 = mlp_forward<NB0, NB1>(a, xa, t.e, lane, h1, h2, kLo ? h2lo : nullptr);
      const float g = t.valid ? a.g_w[t.e] : 0.f;
      const float d3 = z3 > 0.f ? g : 0.f;
#pragma unroll
      for (int b2 = 0; b2 < NB0; ++b2) {
        const float* vp = opaque(a.w3p + b2 * 16 * 64 + lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) d2[b2][r] = h2[b2][r] > 0.f ? d3 * vp[r * 64] * sc : 0.f;
      }

      if constexpr (PARAM) {
        // phase A: g_W2 += d2^T h1, 32 entries (one wave's) at a time
        for (int w = 0; w < 4; ++w) {
          __syncthreads();   // the readers of the previous staging are done
          if (wave == w) {
#pragma unroll
            for (int b = 0; b < NB1; ++b)
#pragma unroll
              for (int r = 0; r < 16; ++r) H1s[(32 * b + acc_row(r, h)) * kLdw + m] = h1[b][r];
#pragma unroll
            for (int b = 0; b < NB0; ++b)
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                D2s[(32 * b + acc_row(r, h)) * kLdw + m] = d2[b][r];
                P3s[(32 * b + acc_row(r, h)) * kLdw + m] = h2[b][r];
                if constexpr (kLo) L3s[(32 * b + acc_row(r, h)) * kLdw + m] = h2lo[b][r];
              }
            if (h == 0) D3s[m] = d3;
          }
          __syncthreads();
#pragma unroll
          for (int i = 0; i < NA; ++i) {
            const int blk = wave + 4 * i;
            if (blk < NB0 * NB1) {
              const float* ap = D2s + (32 * (blk / NB1) + m) * kLdw + h;
              const float* bp = H1s + (32 * (blk % NB1) + m) * kLdw + h;
#pragma unroll
              for (int kk = 0; kk < 16; ++kk)
                accA[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * kk], bp[2 * kk], accA[i], 0, 0, 0);
              WG_SCHED_FENCE();
            }
          }
          if (tid < 32 * NB0) {
            double s2 = 0.0, s3 = 0.0;
            for (int j = 0; j < 32; ++j) {
              s2 += (double)D2s[tid * kLdw + j];
              double hv = (double)P3s[tid * kLdw + j];   // d3 h2 as a float64 product
              if constexpr (kLo) hv += (double)L3s[tid * kLdw + j];
              s3 = fma((double)D3s[j], hv, s3);
            }
            gb2 += s2;
            gw3 += s3;
          }
          if (tid == kBlock - 1) {
            double s = 0.0;
            for (int j = 0; j < 32; ++j) s += (double)D3s[j];
            gb3 += s;
          }
        }
      }

      // d1 = (W2^T d2) D1 (z1 > 0), over h1
#pragma unroll
      for (int b1 = 0; b1 < NB1; ++b1) {
        Acc64 acc;
        const float* wp = opaque(a.w2tp + (int64_t)b1 * NB0 * 16 * 64 + lane);
#pragma unroll
        for (int b2 = 0; b2 < NB0; ++b2) {
          f32x16 part = zero16();
#pragma unroll
          for (int r = 0; r < 16; ++r)
            part = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[(b2 * 16 + r) * 64], d2[b2][r], part, 0, 0, 0);
          acc.add(part);
          WG_SCHED_FENCE();
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) h1[b1][r] = h1[b1][r] > 0.f ? (float)(acc.v[r] * (double)sc) : 0.f;
      }

      if constexpr (PARAM) {
        // phase C: g_W1 += d1^T [emb_r ; emb_c]
        for (int w = 0; w < 4; ++w) {
          __syncthreads();
          if (wave == w) {
#pragma unroll
            for (int b = 0; b < NB1; ++b)
#pragma unroll
              for (int r = 0; r < 16; ++r) D1s[(32 * b + acc_row(r, h)) * kLdw + m] = h1[b][r];
#pragma unroll
            for (int kk = 0; kk < 16 * NB0; ++kk) Fs[(2 * kk + h) * kLdw + m] = xa[kk];
          }
          __syncthreads();
#pragma unroll
          for (int i = 0; i < NA; ++i) {
            const int blk = wave + 4 * i;
            if (blk < NB0 * NB1) {
              const float* ap = D1s + (32 * (blk / NB0) + m) * kLdw + h;
              const float* bp = Fs + (32 * (blk % NB0) + m) * kLdw + h;
#pragma unroll
              for (int kk = 0; kk < 16; ++kk)
                accC[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * kk], bp[2 * kk], accC[i], 0, 0, 0);
              WG_SCHED_FENCE();
            }
          }
          if (tid < 32 * NB1) {
            double s1 = 0.0;
            for (int j = 0; j < 32; ++j) s1 += (double)D1s[tid * kLdw + j];
            gb1 += s1;
          }
        }
      }

      if constexpr (PARAM) {
        // the turn's float32 chains (128 entries) into the workgroup's float64 partial
        double* part = const_cast<double*>(reinterpret_cast<const double*>(
            opaque(reinterpret_cast<const float*>(a.partial + (int64_t)blockIdx.x * a.P))));
        const int64_t oW1 = 0, oW2 = (int64_t)8 * C * C + 4 * C;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
          const int blk = wave + 4 * i;
          if (blk < NB0 * NB1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int u2 = 32 * (blk / NB1) + acc_row(r, h), u1 = 32 * (blk % NB1) + m;
              if (u2 < 2 * C && u1 < 4 * C) part[oW2 + (int64_t)u2 * 4 * C + u1] += (double)accA[i][r];
              const int v1 = 32 * (blk / NB0) + acc_row(r, h), k = 32 * (blk % NB0) + m;
              if (v1 < 4 * C && k < 2 * C) part[oW1 + (int64_t)v1 * 2 * C + k] += (double)accC[i][r];
              accA[i][r] = accC[i][r] = 0.f;
            }
          }
        }
      }
      if constexpr (GEMB) {
        f32x16 gf[NBH];
#pragma unroll
        for (int bh = 0; bh < NBH; ++bh) {
          Acc64 acc;
          const float* wp = opaque(a.w1tp + (int64_t)bh * NB1 * 16 * 64 + lane);
#pragma unroll
          for (int b1 = 0; b1 < NB1; ++b1) {
            f32x16 part = zero16();
#pragma unroll
            for (int r = 0; r < 16; ++r)
              part = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[(b1 * 16 + r) * 64], h1[b1][r], part, 0, 0, 0);
            acc.add(part);
            WG_SCHED_FENCE();
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) gf[bh][r] = (float)acc.v[r];
        }
        __syncthreads();   // the staging buffer is free
#pragma unroll
        for (int bh = 0; bh < NBH; ++bh)
#pragma unroll
          for (int r = 0; r < 16; ++r) lds[(wave * 32 + m) * kCs + 32 * bh + acc_row(r, h)] = gf[bh][r];
        if (h == 0) sseg[wave * 32 + m] = t.seg;
        __syncthreads();
        if (tid < C) {
#pragma unroll 2
          for (int j = 0; j < kTurn; ++j) {
            const int32_t sg = sseg[j];
            if (sg < 0) break;   // past the tile's end
            if (sg != cur) {
              if (cur >= 0) {
                if (lead) a.carry[tile * C + tid] = nsum;
                else a.gacc[(int64_t)cur * C + tid] += nsum;
                lead = false;
              }
              cur = sg;
              nsum = 0.0;
            }
            nsum += (double)lds[j * kCs + tid];
          }
        }
      }
    }

    if (GEMB && tid < C && cur >= 0) {
      if (lead) a.carry[tile * C + tid] = nsum;
      else a.gacc[(int64_t)cur * C + tid] += nsum;
    }
  }
  if constexpr (PARAM) {
    double* part = a.partial + (int64_t)blockIdx.x * a.P;
    const int64_t ob1 = (int64_t)8 * C * C, ob2 = (int64_t)16 * C * C + 4 * C;
    if (tid < 4 * C) part[ob1 + tid] = gb1;
    if (tid < 2 * C) {
      part[ob2 + tid] = gb2;
      part[ob2 + 2 * C + tid] = gw3;
    }
    if (tid == kBlock - 1) part[ob2 + 4 * C] = gb3;
  }
}

// gacc[node of the tile's first position] += the carries of the tiles that node runs through, in tile order
__global__ __launch_bounds__(kBlock) void carry_kernel(int64_t n_tiles, int C, const int32_t* __restrict__ seg,
                                                       const double* __restrict__ carry, double* __restrict__ gacc) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n_tiles * C) return;
  const int64_t k = idx / C;
  const int c = (int)(idx - k * C);
  if (k == 0) return;
  const int32_t node = seg[k * kMlpTile];
  if (seg[k * kMlpTile - 1] != node) return;                      // the tile starts a node: no carry
  if (seg[(k - 1) * kMlpTile] == node && k - 1 > 0 && seg[(k - 1) * kMlpTile - 1] == node) return;   // not the first carry
  double s = gacc[(int64_t)node * C + c];
  for (int64_t j = k; j < n_tiles && seg[j * kMlpTile] == node; ++j) s += carry[j * C + c];
  gacc[(int64_t)node * C + c] = s;
}

__global__ __launch_bounds__(kBlock) void round_kernel(int64_t count, const double* __restrict__ src,
                                                       float* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < count) dst[i] = (float)src[i];
}

// the workgroups' partials in ascending order, rounded once, into the six arrays
__global__ __launch_bounds__(kBlock) void reduce_kernel(int64_t P, int G, int C, const double* __restrict__ partial,
                                                        float* gW1, float* gb1, float* gW2, float* gb2, float* gw3,
                                                        float* gb3) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= P) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += partial[(int64_t)g * P + i];
  const float v = (float)s;
  const int64_t n1 = (int64_t)8 * C * C;
  int64_t j = i;
  if (j < n1) { gW1[j] = v; return; }
  j -= n1;
  if (j < 4 * C) { gb1[j] = v; return; }
  j -= 4 * C;
  if (j < n1) { gW2[j] = v; return; }
  j -= n1;
  if (j < 2 * C) { gb2[j] = v; return; }
  j -= 2 * C;
  if (j < 2 * C) { gw3[j] = v; return; }
  gb3[0] = v;
}

int check_common(const char* who, int64_t n, int64_t nnz, int64_t C, double p) {
  if (n < 0 || nnz < 0 || C <= 0)
    return fail(WG_ERR_INVALID, "%s: bad size (n=%lld nnz=%lld C=%lld)", who, (long long)n, (long long)nnz,
                (long long)C);
  if (!(p >= 0.0) || !(p < 1.0)) return fail(WG_ERR_INVALID, "%s: p must lie in [0, 1) (p=%g)", who, p);
  if (C > kMlpMaxC)
    return fail(WG_ERR_UNSUPPORTED, "%s: C=%lld exceeds the %d classes whose activations a wave holds in registers",
                who, (long long)C, kMlpMaxC);
  if (n > INT32_MAX || nnz > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld / nnz=%lld exceed int32", who, (long long)n, (long long)nnz);
  return WG_OK;
}

int launch_pack(const MlpShape& s, const MlpWs& ws, const float* W1, const float* W2, const float* b1,
                const float* b2, const float* w3, bool bwd, bool gemb,
                hipStream_t stream) {
  struct Item { int kind; int len; int64_t count; const float* src; float* out; bool on; };
  const Item items[8] = {{0, s.C, s.w1p, W1, ws.w1p, true},     {1, s.C, s.w2p, W1, ws.w2p, true},
                         {2, s.C, s.w2tp, W1, ws.w2tp, bwd},    {3, s.C, s.w1tp, W1, ws.w1ta, gemb},
                         {4, s.C, s.w1tp, W1, ws.w1tb, gemb},   {5, 4 * s.C, (int64_t)s.NB1 * 1024, b1, ws.b1p, true},
                         {5, 2 * s.C, (int64_t)s.NB0 * 1024, b2, ws.b2p, true},
                         {5, 2 * s.C, (int64_t)s.NB0 * 1024, w3, ws.w3p, true}};
  for (const Item& it : items) {
    if (!it.on) continue;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)ceil_div(it.count, kBlock)), dim3(kBlock), 0, stream, it.kind, it.len,
                       s.NB0, s.NB1, it.count, it.src, W2, it.out);
    WG_LAUNCH_CHECK();
  }
  return WG_OK;
}

#define WG_MLP_SHAPES(s, MACRO)                       \
  switch ((s).NB0 * 8 + (s).NB1) {                    \
    case 1 * 8 + 1: MACRO(1, 1) break;                \
    case 1 * 8 + 2: MACRO(1, 2) break;                \
    case 2 * 8 + 3: MACRO(2, 3) break;                \
    case 2 * 8 + 4: MACRO(2, 4) break;                \
    case 3 * 8 + 5: MACRO(3, 5) break;                \
    default: MACRO(3, 6) break;                       \
  }

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_edge_mlp_max_c(void) { return kMlpMaxC; }
int wg_edge_mlp_tile(void) { return kMlpTile; }

int wg_edge_mlp_workspace(int64_t n, int64_t nnz, int64_t C, int64_t* bytes) {
  if (!bytes) return fail(WG_ERR_INVALID, "wg_edge_mlp_workspace: NULL bytes");
  if (int rc = check_common("wg_edge_mlp_workspace", n, nnz, C, 0.0)) return rc;
  *bytes = carve(nullptr, n, nnz, shape_of(C)).bytes;
  return WG_OK;
}

int wg_edge_mlp_forward(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t C,
                        const float* emb, const float* W1, const float* b1, const float* W2, const float* b2,
                        const float* w3, const float* b3, double p, uint64_t seed, void* workspace, float* w,
                        void* stream_) {
  if (int rc = check_common("wg_edge_mlp_forward", n, nnz, C, p)) return rc;
  if (n == 0 || nnz == 0) return WG_OK;
  if (!indptr || !indices || !emb || !W1 || !b1 || !W2 || !b2 || !w3 || !b3 || !workspace || !w)
    return fail(WG_ERR_INVALID, "wg_edge_mlp_forward: NULL pointer with n=%lld nnz=%lld", (long long)n,
                (long long)nnz);
  hipStream_t stream = as_stream(stream_);
  const MlpShape s = shape_of(C);
  const MlpWs ws = carve(workspace, n, nnz, s);
  if (int rc = launch_pack(s, ws, W1, W2, b1, b2, w3, false, false, stream)) return rc;
  hipLaunchKernelGGL(entry_rows_kernel, dim3((unsigned)ceil_div(nnz, kBlock)), dim3(kBlock), 0, stream, n, nnz, indptr,
                     ws.rows);
  WG_LAUNCH_CHECK();
  MlpArgs a{};
  a.n = n; a.nnz = nnz; a.C = (int)C;
  a.seg = ws.rows; a.other = indices; a.pos = nullptr; a.emb = emb;
  a.w1p = ws.w1p; a.w2p = ws.w2p;
  a.b1p = ws.b1p; a.b2p = ws.b2p; a.w3p = ws.w3p; a.b3 = b3;
  a.drop = p > 0.0;
  a.thr = (uint32_t)(p * 4294967296.0);
  a.scale = (float)(1.0 / (1.0 - p));
  a.seed = seed;
  const dim3 grid((unsigned)ceil_div(nnz, kTurn));
#define WG_MLP_FWD(A, B) hipLaunchKernelGGL((edge_mlp_fwd_kernel<A, B>), grid, dim3(kBlock), 0, stream, a, w);
  WG_MLP_SHAPES(s, WG_MLP_FWD)
#undef WG_MLP_FWD
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_edge_mlp_backward(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t C,
                         const float* emb, const float* W1, const float* b1, const float* W2, const float* b2,
                         const float* w3, const float* b3, double p, uint64_t seed, const float* g_w,
                         const int64_t* t_indptr, const int32_t* t_indices, const int32_t* t_pos, float* gW1,
                         float* gb1, float* gW2, float* gb2, float* gw3, float* gb3, float* g_emb, void* workspace,
                         void* stream_) {
  if (int rc = check_common("wg_edge_mlp_backward", n, nnz, C, p)) return rc;
  if (!gW1 || !gb1 || !gW2 || !gb2 || !gw3 || !gb3)
    return fail(WG_ERR_INVALID, "wg_edge_mlp_backward: NULL parameter gradient");
  const bool live = n > 0 && nnz > 0;
  if (live && (!indptr || !indices || !emb || !W1 || !b1 || !W2 || !b2 || !w3 || !b3 || !workspace || !g_w))
    return fail(WG_ERR_INVALID, "wg_edge_mlp_backward: NULL pointer with n=%lld nnz=%lld", (long long)n,
                (long long)nnz);
  if (live && g_emb && (!t_indptr || !t_indices || !t_pos))
    return fail(WG_ERR_INVALID, "wg_edge_mlp_backward: g_emb needs the transposed CSR and its entry map");
  if (g_emb && g_emb == emb) return fail(WG_ERR_INVALID, "wg_edge_mlp_backward: g_emb must not alias emb");
  hipStream_t stream = as_stream(stream_);
  const MlpShape s = shape_of(C);
  if (!live) {   // zero gradients
    WG_HIP_TRY(zero_async(gW1, sizeof(float) * 8 * C * C, stream));
    WG_HIP_TRY(zero_async(gb1, sizeof(float) * 4 * C, stream));
    WG_HIP_TRY(zero_async(gW2, sizeof(float) * 8 * C * C, stream));
    WG_HIP_TRY(zero_async(gb2, sizeof(float) * 2 * C, stream));
    WG_HIP_TRY(zero_async(gw3, sizeof(float) * 2 * C, stream));
    WG_HIP_TRY(zero_async(gb3, sizeof(float), stream));
    if (g_emb && n > 0) WG_HIP_TRY(zero_async(g_emb, sizeof(float) * n * C, stream));
    return WG_OK;
  }
  const MlpWs ws = carve(workspace, n, nnz, s);
  const int64_t n_tiles = ceil_div(nnz, kMlpTile);
  const int G = (int)(n_tiles < kMlpMaxWG ? n_tiles : kMlpMaxWG);
  const bool gemb = g_emb != nullptr;
  if (int rc = launch_pack(s, ws, W1, W2, b1, b2, w3, true, gemb, stream)) return rc;
  hipLaunchKernelGGL(entry_rows_kernel, dim3((unsigned)ceil_div(nnz, kBlock)), dim3(kBlock), 0, stream, n, nnz, indptr,
                     ws.rows);
  WG_LAUNCH_CHECK();
  WG_HIP_TRY(zero_async(ws.partial, sizeof(double) * s.P * G, stream));
  if (gemb) WG_HIP_TRY(zero_async(ws.gacc, sizeof(double) * n * C, stream));
  MlpArgs a{};
  a.n = n; a.nnz = nnz; a.C = (int)C;
  a.seg = ws.rows; a.other = indices; a.pos = nullptr; a.emb = emb;
  a.w1p = ws.w1p; a.w2p = ws.w2p; a.w2tp = ws.w2tp; a.w1tp = ws.w1ta;
  a.b1p = ws.b1p; a.b2p = ws.b2p; a.w3p = ws.w3p; a.b3 = b3;
  a.drop = p > 0.0;
  a.thr = (uint32_t)(p * 4294967296.0);
  a.scale = (float)(1.0 / (1.0 - p));
  a.seed = seed;
  a.g_w = g_w;
  a.partial = ws.partial; a.gacc = ws.gacc; a.carry = ws.carry; a.P = s.P;
  const dim3 grid((unsigned)G);
  const dim3 cgrid((unsigned)ceil_div(n_tiles * C, kBlock));
#define WG_MLP_BWD(A, B)                                                                                        \
  if (gemb) hipLaunchKernelGGL((edge_mlp_bwd_kernel<A, B, true, true>), grid, dim3(kBlock), 0, stream, a, n_tiles); \
  else hipLaunchKernelGGL((edge_mlp_bwd_kernel<A, B, true, false>), grid, dim3(kBlock), 0, stream, a, n_tiles);
  WG_MLP_SHAPES(s, WG_MLP_BWD)
#undef WG_MLP_BWD
  WG_LAUNCH_CHECK();
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)ceil_div(s.P, kBlock)), dim3(kBlock), 0, stream, s.P, G, (int)C,
                     ws.partial, gW1, gb1, gW2, gb2, gw3, gb3);
  WG_LAUNCH_CHECK();
  if (gemb) {
    hipLaunchKernelGGL(carry_kernel, cgrid, dim3(kBlock), 0, stream, n_tiles, (int)C, ws.rows, ws.carry, ws.gacc);
    WG_LAUNCH_CHECK();
    // the column half: the transposed order, dropout and g_w at the entry's CSR position
    hipLaunchKernelGGL(entry_rows_kernel, dim3((unsigned)ceil_div(nnz, kBlock)), dim3(kBlock), 0, stream, n, nnz,
                       t_indptr, ws.trows);
    WG_LAUNCH_CHECK();
    a.seg = ws.trows; a.other = t_indices; a.pos = t_pos; a.w1tp = ws.w1tb;
#define WG_MLP_BWD2(A, B) \
  hipLaunchKernelGGL((edge_mlp_bwd_kernel<A, B, false, true>), grid, dim3(kBlock), 0, stream, a, n_tiles);
    WG_MLP_SHAPES(s, WG_MLP_BWD2)
#undef WG_MLP_BWD2
    WG_LAUNCH_CHECK();
    hipLaunchKernelGGL(carry_kernel, cgrid, dim3(kBlock), 0, stream, n_tiles, (int)C, ws.trows, ws.carry, ws.gacc);
    WG_LAUNCH_CHECK();
    hipLaunchKernelGGL(round_kernel, dim3((unsigned)ceil_div(n * C, kBlock)), dim3(kBlock), 0, stream, n * C, ws.gacc,
                       g_emb);
    WG_LAUNCH_CHECK();
  }
  return WG_OK;
}

}  // extern "C"
