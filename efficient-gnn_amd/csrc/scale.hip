// scale.hip -- SURVEY section 8(f): the four node-wise calibrators of the reference, TS (calibration/TS.py), VS
// (VS.py), MS (MS.py) and ETS (ETS.py).  All four are row-wise maps of the base model's logits z (N, C):
//
//     TS / VS   out = log_softmax(z * s),  s = log(exp(temperature) + 1.1), one s or one per column   (TS.py:39-43)
//     MS        z' = z - z[:, -1:],  out = z' W + b, raw (MS.py:43-57); the normalize flag adds log_softmax
//     ETS       temp = log(exp(tau) + 1.1),  out = log(w1 softmax(z / temp) + w2 softmax(z) + w3 / C)  (ETS.py:22-26)
//
// so one pass over the listed rows gives the output (wg_scale_forward), the gradient w.r.t. the logits and every
// parameter gradient (wg_scale_backward), or a whole training epoch of TS.py:59-83 / VS.py:65-89 / MS.py:64-89
// (wg_scale_epoch): forward, nll loss, parameter gradients, the count of correct argmaxes, then -- in the workgroup
// that arrives last -- MS's L1 term, torch's Adam step with L2 weight decay, the early-stopping state and the
// traces, all in one device state block, so that a training run needs no host round trip.  wg_ets_label_probs is
// the one pass ETS.fit needs (ETS.py:50-76 reads only the label column of its two softmaxes).
//
// Decomposition.  A wave per row, as head.hip: lane l owns the columns l, l + 64, l + 128, l + 192 (C <= 256); MS
// has one lane per column (C <= 64), W in LDS as float64 with rows padded to C + 1 (the forward reads a column, the
// backward a row, both without bank conflicts) and a column of dW in 64 float64 registers per lane -- which is what
// sets MS's limit: 128 VGPRs of accumulators, and W (33 KB) shares the workgroup's LDS with the reduction buffer.
// Rows are cut into FIXED chunks of kChunkRows = 256 listed rows; a workgroup takes whole chunks, wave w the rows
// w, w + 4, ... of the chunk in ascending order, the waves' sums meet in LDS in wave order, and each chunk leaves
// one float64 partial vector.  Chunk partials are added in chunk order (by the last workgroup of wg_scale_epoch, by
// a second launch of wg_scale_backward), so the bits depend on the rows and C only, never on the grid.
//
// The epoch's hand-off is the fence-free one of step.hip: partials are agent-scope (sc1) stores drained with
// s_waitcnt vmcnt(0) in front of a barrier, then ONE relaxed agent-scope fetch_add per workgroup; the workgroup
// whose add completes the count resets it and reads every partial with agent-scope loads.  No workgroup waits on
// another.
//
// Arithmetic.  Everything is float64: the scaled logits, the row maximum, the sum of exp, the log, every gradient
// and the optimiser (float64 master parameters and moments); out, g_logits and the parameter gradients that
// wg_scale_backward returns are rounded to float32 once.  No float atomics.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "internal.h"
#include "row_dev.h"

namespace wg {
namespace {

constexpr int kTS = 0, kVS = 1, kMS = 2, kETS = 3;
constexpr int kScaleMaxC = kRowMaxC;   // four columns per lane (row_dev.h)
constexpr int kScaleMaxCMS = 64;    // one lane per column, a column of dW in registers
constexpr int kChunkRows = 256;     // listed rows per partial vector; 64 measured slower
constexpr int kScaleWaves = kBlock / 64;
constexpr int kMaxGrid = 1024;
constexpr int kRedMax = 2 + kScaleMaxCMS * kScaleMaxCMS + kScaleMaxCMS;   // the longest partial vector (MS)

// the state block of wg_scale_epoch, in 8-byte slots: slot 0 holds the arrival counter (uint32), the rest doubles
enum : int {
  kStTicket = 0, kStStopped, kStEpochs, kStStep, kStPatienceLeft, kStBest, kStLr, kStWd, kStLambda, kStPatience,
  kStMaxEpochs, kStMode, kStC, kStFlags, kStMaxRows, kStReserved, kStHeader
};
constexpr double kBeta1 = 0.9, kBeta2 = 0.999, kAdamEps = 1e-8;

__host__ __device__ inline int64_t n_params(int mode, int64_t C) {
  return mode == kTS ? 1 : mode == kVS ? C : mode == kMS ? C * C + C : 4;
}
// [0] loss, [1] correct, [2 ..) the parameter gradients in state order (MS: W row-major, then b; ETS: tau, w1..w3)
__host__ __device__ inline int64_t partial_len(int mode, int64_t C) { return 2 + n_params(mode, C); }
inline int64_t n_chunks_of(int64_t rows) { return ceil_div(rows, kChunkRows); }

// What a lane keeps of the parameters.  TS / VS: s and ds / d temperature of its columns; ETS: temp, its derivative
// and the weights; MS: its bias (W is in LDS).
struct LaneParams {
  double s[kNQ], ds[kNQ];
  double temp, dtemp, w1, w2, w3, b;
};

template <int MODE, class PT>
__device__ inline void lane_params(LaneParams& L, const PT* p0, const PT* p1, const PT* p2, const PT* p3, int C,
                                   int lane) {
#pragma unroll
  for (int q = 0; q < kNQ; ++q) L.s[q] = 1.0, L.ds[q] = 0.0;
  L.temp = 1.0, L.dtemp = 0.0, L.w1 = L.w2 = L.w3 = 0.0, L.b = 0.0;
  if constexpr (MODE == kTS || MODE == kVS) {
#pragma unroll
    for (int q = 0; q < kNQ; ++q) {
      const int c = lane + 64 * q;
      if (c < C) {
        const double et = exp((double)p0[MODE == kVS ? c : 0]);
        L.s[q] = log(et + 1.1);
        L.ds[q] = et / (et + 1.1);
      }
    }
  } else if constexpr (MODE == kETS) {
    const double et = exp((double)p0[0]);
    L.temp = log(et + 1.1);
    L.dtemp = et / (et + 1.1);
    L.w1 = (double)p1[0], L.w2 = (double)p2[0], L.w3 = (double)p3[0];
  } else {
    if (lane < C) L.b = (double)p1[lane];
  }
}

// MS: W (C, C) into LDS as float64, rows padded to C + 1
template <class PT>
__device__ inline void stage_w(double* sh, const PT* W, int C) {
  for (int i = threadIdx.x; i < C * C; i += kBlock) sh[(i / C) * (C + 1) + (i % C)] = (double)W[i];
}

// The lane-local sums of one wave over its rows of a chunk.
template <int MODE>
struct Acc {
  double loss = 0.0, correct = 0.0;
  double gt[MODE == kVS ? kNQ : 1];                 // TS: the lane's share of g_temperature; VS: its columns
  double ge[MODE == kETS ? 4 : 1];                  // ETS: g_tau, g_w1, g_w2, g_w3 (wave-uniform)
  double gb = 0.0;                                  // MS
  double dW[MODE == kMS ? kScaleMaxCMS : 1];        // MS: column `lane` of dW
  __device__ Acc() {
    for (double& x : gt) x = 0.0;
    for (double& x : ge) x = 0.0;
    for (double& x : dW) x = 0.0;
  }
};

// One row.  z: the lane's logits; out: the float64 output at its columns.  BWD: g holds d loss / d out on entry
// (LABEL >= 0: it is built here as -1 at the label, the nll gradient before the division by the row count) and
// d loss / d z on exit; the parameter gradients go to A.
template <int MODE, bool BWD>
__device__ inline void row_map(const LaneParams& L, const double* shW, int C, int lane, bool normalize,
                               const double (&z)[kNQ], double (&out)[kNQ], double (&g)[kNQ], Acc<MODE>& A) {
  if constexpr (MODE == kTS || MODE == kVS) {
    double v[kNQ], e[kNQ], m, S;
#pragma unroll
    for (int q = 0; q < kNQ; ++q) v[q] = z[q] * L.s[q];
    row_exp(v, C, lane, e, &m, &S);
    const double lse = log(S);
#pragma unroll
    for (int q = 0; q < kNQ; ++q) out[q] = v[q] - m - lse;
    if constexpr (BWD) {
      double gs = 0.0;
#pragma unroll
      for (int q = 0; q < kNQ; ++q) gs += lane + 64 * q < C ? g[q] : 0.0;
      gs = wave_sum(gs);
#pragma unroll
      for (int q = 0; q < kNQ; ++q) {
        if (lane + 64 * q < C) {
          const double gv = g[q] - (e[q] / S) * gs;
          A.gt[MODE == kVS ? q : 0] += gv * z[q] * L.ds[q];
          g[q] = gv * L.s[q];
        }
      }
    }
  } else if constexpr (MODE == kETS) {
    double a[kNQ], e0[kNQ], e1[kNQ], m0, S0, m1, S1, p[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) a[q] = z[q] / L.temp;
    row_exp(a, C, lane, e0, &m0, &S0);
    row_exp(z, C, lane, e1, &m1, &S1);
    const double u = L.w3 / (double)C;
#pragma unroll
    for (int q = 0; q < kNQ; ++q) {
      e0[q] /= S0, e1[q] /= S1;                    // p0, p1
      p[q] = L.w1 * e0[q] + L.w2 * e1[q] + u;
      out[q] = log(p[q]);
    }
    if constexpr (BWD) {
      double gp[kNQ], d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
      for (int q = 0; q < kNQ; ++q) {
        gp[q] = lane + 64 * q < C ? g[q] / p[q] : 0.0;
        d0 += gp[q] * e0[q], d1 += gp[q] * e1[q], d2 += gp[q];
      }
      d0 = wave_sum(d0), d1 = wave_sum(d1), d2 = wave_sum(d2);
      double gtemp = 0.0;
#pragma unroll
      for (int q = 0; q < kNQ; ++q) {
        if (lane + 64 * q < C) {
          const double ga = L.w1 * e0[q] * (gp[q] - d0);        // d / d a
          gtemp -= ga * z[q] / (L.temp * L.temp);
          g[q] = ga / L.temp + L.w2 * e1[q] * (gp[q] - d1);
        }
      }
      A.ge[0] += wave_sum(gtemp) * L.dtemp;
      A.ge[1] += d0, A.ge[2] += d1, A.ge[3] += d2 / (double)C;
    }
  } else {
    const bool own = lane < C;
    const double zl = __shfl(z[0], C - 1, 64);
    const double zp = own ? z[0] - zl : 0.0;
    double o = L.b;
    for (int k = 0; k < C; ++k) {
      const double zk = __shfl(zp, k, 64);
      if (own) o += zk * shW[k * (C + 1) + lane];
    }
    double v[kNQ] = {o, 0.0, 0.0, 0.0}, e[kNQ] = {0.0, 0.0, 0.0, 0.0}, S = 1.0;
    if (normalize) {
      double m;
      row_exp(v, C, lane, e, &m, &S);
      o = o - m - log(S);
    }
    out[0] = o, out[1] = out[2] = out[3] = 0.0;
    if constexpr (BWD) {
      double go = own ? g[0] : 0.0;
      if (normalize) go -= (e[0] / S) * wave_sum(go);
      A.gb += go;
#pragma unroll
      for (int k = 0; k < kScaleMaxCMS; ++k) {
        if (k < C) A.dW[k] += __shfl(zp, k, 64) * go;           // uniform over the wave
      }
      double gz = 0.0;
      for (int c = 0; c < C; ++c) {
        const double gc = __shfl(go, c, 64);
        if (own) gz += shW[lane * (C + 1) + c] * gc;
      }
      const double tot = wave_sum(gz);
      g[0] = lane == C - 1 ? gz - tot : gz;                     // the column shift's gradient
    }
  }
}

struct PassArgs {
  int64_t n_total, n_rows;
  int C;
  bool normalize;
  const float* logits;
  const int32_t* rows;       // nullable
  const int64_t* labels;     // the epoch: by ORIGINAL row id
  const float* g_out;        // the backward: (n_rows, C)
  float* g_logits;           // the backward, nullable: (n_rows, C)
  double* partial;           // [chunks][partial_len], nullable in the backward
};

__device__ inline int64_t source_row(const PassArgs& a, int64_t r) {
  const int64_t i = a.rows ? (int64_t)a.rows[r] : r;
  WG_DCHECK(i >= 0 && i < a.n_total, "scale: listed row %lld is %lld, outside [0, %lld)", (long long)r, (long long)i,
            (long long)a.n_total);
  return i;
}

// One chunk: rows [ch * kChunkRows, ...) of the list.  EPOCH: the gradient of the nll sum, the loss and the correct
// count; else g_out -> g_logits.  Leaves the chunk's partial vector in a.partial (agent-scope stores).  sh: the
// workgroup's kRedMax doubles (MS keeps W there while the rows run).
template <int MODE, bool EPOCH, class PT>
__device__ inline void chunk_pass(const PassArgs& a, int64_t ch, const LaneParams& L, const PT* W, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = a.C;
  if constexpr (MODE == kMS) {
    __syncthreads();   // the previous chunk's partial has left sh
    stage_w(sh, W, C);
    __syncthreads();
  }
  Acc<MODE> A;
  const int64_t r1 = a.n_rows < (ch + 1) * kChunkRows ? a.n_rows : (ch + 1) * kChunkRows;
  for (int64_t r = ch * kChunkRows + wave; r < r1; r += kScaleWaves) {
    const int64_t i = source_row(a, r);
    double z[kNQ], out[kNQ], g[kNQ];
    load_row(z, a.logits + i * C, C, lane);
    if constexpr (EPOCH) {
      const int64_t y = a.labels[i];
      WG_DCHECK(y >= 0 && y < C, "scale: row %lld has the label %lld of %d classes", (long long)i, (long long)y, C);
#pragma unroll
      for (int q = 0; q < kNQ; ++q) g[q] = lane + 64 * q == y ? -1.0 : 0.0;
      row_map<MODE, true>(L, sh, C, lane, a.normalize, z, out, g, A);
      double ly = 0.0;
#pragma unroll
      for (int q = 0; q < kNQ; ++q) ly -= lane + 64 * q == y ? out[q] : 0.0;
      A.loss += wave_sum(ly);
      A.correct += wave_argmax(out, C, lane) == y ? 1.0 : 0.0;
    } else {
#pragma unroll
      for (int q = 0; q < kNQ; ++q) g[q] = lane + 64 * q < C ? (double)a.g_out[r * C + lane + 64 * q] : 0.0;
      row_map<MODE, true>(L, sh, C, lane, a.normalize, z, out, g, A);
      if (a.g_logits) {
#pragma unroll
        for (int q = 0; q < kNQ; ++q)
          if (lane + 64 * q < C) a.g_logits[r * C + lane + 64 * q] = (float)g[q];
      }
    }
  }
  if (!a.partial) return;   // uniform over the launch
  if constexpr (MODE == kTS) A.gt[0] = wave_sum(A.gt[0]);
  if constexpr (MODE == kMS) __syncthreads();   // every wave is done with W
  // the waves' sums, added in wave order
  for (int w = 0; w < kScaleWaves; ++w) {
    if (wave == w) {
      auto put = [&](int idx, double v) { sh[idx] = w == 0 ? v : sh[idx] + v; };
      if (lane == 0) {
        put(0, A.loss), put(1, A.correct);
        if constexpr (MODE == kTS) put(2, A.gt[0]);
        if constexpr (MODE == kETS) {
          for (int k = 0; k < 4; ++k) put(2 + k, A.ge[k]);
        }
      }
      if constexpr (MODE == kVS) {
#pragma unroll
        for (int q = 0; q < kNQ; ++q)
          if (lane + 64 * q < C) put(2 + lane + 64 * q, A.gt[q]);
      }
      if constexpr (MODE == kMS) {
        if (lane < C) {
#pragma unroll
          for (int k = 0; k < kScaleMaxCMS; ++k)
            if (k < C) put(2 + k * C + lane, A.dW[k]);
          put(2 + C * C + lane, A.gb);
        }
      }
    }
    __syncthreads();
  }
  const int64_t Q = partial_len(MODE, C);
  for (int64_t idx = threadIdx.x; idx < Q; idx += kBlock)
    __hip_atomic_store(a.partial + ch * Q + idx, sh[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // sc1
  if constexpr (MODE != kMS) __syncthreads();   // sh is free for the next chunk
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void scale_forward_kernel(PassArgs a, const float* p0, const float* p1,
                                                               const float* p2, const float* p3, float* out_) {
  __shared__ double sh[MODE == kMS ? kScaleMaxCMS * (kScaleMaxCMS + 1) : 1];
  const int lane = threadIdx.x & 63, C = a.C;
  LaneParams L;
  lane_params<MODE>(L, p0, p1, p2, p3, C, lane);
  if constexpr (MODE == kMS) {
    stage_w(sh, p0, C);
    __syncthreads();
  }
  Acc<MODE> A;
  const int64_t waves = (int64_t)gridDim.x * kScaleWaves;
  for (int64_t r = (int64_t)blockIdx.x * kScaleWaves + (threadIdx.x >> 6); r < a.n_rows; r += waves) {
    const int64_t i = source_row(a, r);
    double z[kNQ], out[kNQ], g[kNQ] = {0.0, 0.0, 0.0, 0.0};
    load_row(z, a.logits + i * C, C, lane);
    row_map<MODE, false>(L, sh, C, lane, a.normalize, z, out, g, A);
#pragma unroll
    for (int q = 0; q < kNQ; ++q)
      if (lane + 64 * q < C) out_[r * C + lane + 64 * q] = (float)out[q];
  }
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void scale_backward_kernel(PassArgs a, const float* p0, const float* p1,
                                                                const float* p2, const float* p3, int64_t n_chunks) {
  __shared__ double sh[MODE == kMS ? kRedMax : 2 + kScaleMaxC];
  LaneParams L;
  lane_params<MODE>(L, p0, p1, p2, p3, a.C, threadIdx.x & 63);
  for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) chunk_pass<MODE, false>(a, ch, L, p0, sh);
}

// the chunk partials of wg_scale_backward, added in chunk order and rounded once; g[j] may be NULL
__global__ void scale_reduce_kernel(int mode, int C, int64_t n_chunks, const double* __restrict__ partial, float* g0,
                                    float* g1, float* g2, float* g3) {
  const int64_t P = n_params(mode, C), Q = P + 2;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  double s = 0.0;
  for (int64_t ch = 0; ch < n_chunks; ++ch) s += partial[ch * Q + 2 + i];
  float* dst = g0;
  int64_t at = i;
  if (mode == kMS && i >= (int64_t)C * C) dst = g1, at = i - (int64_t)C * C;
  if (mode == kETS && i > 0) dst = i == 1 ? g1 : i == 2 ? g2 : g3, at = 0;
  if (dst) dst[at] = (float)s;
}

// The last workgroup's part of an epoch: the chunk partials in chunk order, MS's L1 term, Adam, early stopping.
template <int MODE>
__device__ inline void epoch_finish(double* st, int C, int64_t n_rows, int64_t n_chunks, const double* partial,
                                    double* sh) {
  const int64_t P = n_params(MODE, C), Q = P + 2;
  const int tid = threadIdx.x;
  const double lr = st[kStLr], wd = st[kStWd], lam = st[kStLambda];
  const int64_t max_epochs = (int64_t)st[kStMaxEpochs];
  const int64_t epoch = (int64_t)st[kStEpochs];
  const double step = st[kStStep] + 1.0;
  double* theta = st + kStHeader;
  double* m1 = theta + P;
  double* m2 = m1 + P;
  double* trace = m2 + P;
  // MS.py:68-69: Lambda * sum |W - I| of the parameters the forward used, thread shares added in thread order
  double l1 = 0.0;
  if constexpr (MODE == kMS) {
    for (int64_t i = tid; i < (int64_t)C * C; i += kBlock) l1 += fabs(theta[i] - (i / C == i % C ? 1.0 : 0.0));
    sh[tid] = l1;
    __syncthreads();
    l1 = 0.0;
    if (tid == 0)
      for (int t = 0; t < kBlock; ++t) l1 += sh[t];
  }
  const double bc1 = 1.0 - pow(kBeta1, step), bc2s = sqrt(1.0 - pow(kBeta2, step));
  for (int64_t i = tid; i < P; i += kBlock) {
    double g = 0.0;
    for (int64_t ch = 0; ch < n_chunks; ++ch)
      g += __hip_atomic_load(partial + ch * Q + 2 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    g /= (double)n_rows;                                             // nll_loss's mean
    const double th = theta[i];
    if (MODE == kMS && i < (int64_t)C * C) {
      const double d = th - (i / C == i % C ? 1.0 : 0.0);
      g += lam * (d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : d);               // sign(0) = 0, a NaN stays
    }
    g += wd * th;                                                    // torch's Adam: L2, not decoupled
    const double a = kBeta1 * m1[i] + (1.0 - kBeta1) * g;
    const double b = kBeta2 * m2[i] + (1.0 - kBeta2) * g * g;
    m1[i] = a, m2[i] = b;
    theta[i] = th - (lr / bc1) * (a / (sqrt(b) / bc2s + kAdamEps));
  }
  if (tid == 0) {
    double ls = 0.0, correct = 0.0;
    for (int64_t ch = 0; ch < n_chunks; ++ch) {
      ls += __hip_atomic_load(partial + ch * Q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      correct += __hip_atomic_load(partial + ch * Q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const double loss = ls / (double)n_rows + (MODE == kMS ? lam * l1 : 0.0);
    trace[epoch] = loss;
    trace[max_epochs + epoch] = correct / (double)n_rows;
    double left = st[kStPatienceLeft];
    if (loss < st[kStBest]) {                                        // TS.py:75-83; false for a NaN loss
      st[kStBest] = loss;
      left = st[kStPatience];
    } else {
      left -= 1.0;
    }
    st[kStPatienceLeft] = left;
    st[kStStep] = step;
    st[kStEpochs] = (double)(epoch + 1);
    if (left <= 0.0) st[kStStopped] = 1.0;
    else if (epoch + 1 >= max_epochs) st[kStStopped] = 2.0;
  }
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void scale_epoch_kernel(PassArgs a, double* st, int64_t n_chunks,
                                                             int64_t max_epochs, int64_t max_rows) {
  __shared__ double sh[MODE == kMS ? kRedMax : 2 + kScaleMaxC];
  __shared__ int s_last;
  if (st[kStStopped] != 0.0) return;   // set only after every workgroup of its launch arrived: uniform
  WG_DCHECK((int)st[kStMode] == MODE && (int)st[kStC] == a.C && (int64_t)st[kStMaxRows] == max_rows &&
                (int64_t)st[kStMaxEpochs] == max_epochs,
            "scale: the state block was initialised for mode %d C %d rows %lld epochs %lld", (int)st[kStMode],
            (int)st[kStC], (long long)st[kStMaxRows], (long long)st[kStMaxEpochs]);
  const double* theta = st + kStHeader;
  LaneParams L;
  lane_params<MODE>(L, theta, theta + (int64_t)a.C * a.C, theta, theta, a.C, threadIdx.x & 63);
  for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) chunk_pass<MODE, true>(a, ch, L, theta, sh);
  // the hand-off of step.hip: partials drained, one agent-scope arrival per workgroup, the last one finishes
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  uint32_t* ticket = reinterpret_cast<uint32_t*>(st + kStTicket);
  if (threadIdx.x == 0) {
    const uint32_t old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = old + 1u == gridDim.x;
    if (s_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch starts at 0
  }
  __syncthreads();
  if (s_last) epoch_finish<MODE>(st, a.C, a.n_rows, n_chunks, a.partial, sh);
}

__global__ void scale_state_init_kernel(double* st, int mode, int flags, int C, int64_t max_epochs, int64_t max_rows,
                                        int patience, double lr, double wd, double lam, const float* init,
                                        int64_t slots) {
  const int64_t P = n_params(mode, C);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (int64_t)gridDim.x * blockDim.x) {
    double v = 0.0;
    if (i == kStTicket) {
      *reinterpret_cast<uint64_t*>(st) = 0ull;
      continue;
    }
    if (i == kStPatienceLeft || i == kStPatience) v = (double)patience;
    else if (i == kStBest) v = INFINITY;
    else if (i == kStLr) v = lr;
    else if (i == kStWd) v = wd;
    else if (i == kStLambda) v = lam;
    else if (i == kStMaxEpochs) v = (double)max_epochs;
    else if (i == kStMode) v = (double)mode;
    else if (i == kStC) v = (double)C;
    else if (i == kStFlags) v = (double)flags;
    else if (i == kStMaxRows) v = (double)max_rows;
    else if (i >= kStHeader && i < kStHeader + P) v = init ? (double)init[i - kStHeader] : 1.0;   // TS.py:26, MS.py:28-29
    st[i] = v;
  }
}

// info: [0] stopped, [1] epochs run, [2] Adam steps, [3] patience left, [4] best loss, then the loss trace and the
// accuracy trace, max_epochs each
__global__ void scale_state_read_kernel(const double* st, int mode, int C, int64_t max_epochs, float* params,
                                        double* info) {
  const int64_t P = n_params(mode, C);
  const double* theta = st + kStHeader;
  const double* trace = theta + 3 * P;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P + 5 + 2 * max_epochs;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i < P) {
      if (params) params[i] = (float)theta[i];
    } else if (info) {
      const int64_t j = i - P;
      info[j] = j < 5 ? st[kStStopped + j] : trace[j - 5];
    }
  }
}

__global__ __launch_bounds__(kBlock) void ets_label_probs_kernel(PassArgs a, const float* temperature, double* p0y,
                                                                 double* p1y) {
  const int lane = threadIdx.x & 63, C = a.C;
  const double t = (double)temperature[0];   // ETS.py:43, :57: the RAW parameter divides
  const int64_t waves = (int64_t)gridDim.x * kScaleWaves;
  for (int64_t r = (int64_t)blockIdx.x * kScaleWaves + (threadIdx.x >> 6); r < a.n_rows; r += waves) {
    const int64_t i = source_row(a, r);
    const int64_t y = a.labels[i];
    WG_DCHECK(y >= 0 && y < C, "scale: row %lld has the label %lld of %d classes", (long long)i, (long long)y, C);
    double z[kNQ], v[kNQ], e0[kNQ], e1[kNQ], m, S0, S1;
    load_row(z, a.logits + i * C, C, lane);
#pragma unroll
    for (int q = 0; q < kNQ; ++q) v[q] = z[q] / t;
    row_exp(v, C, lane, e0, &m, &S0);
    row_exp(z, C, lane, e1, &m, &S1);
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int q = 0; q < kNQ; ++q)
      if (lane + 64 * q == y) a0 += e0[q], a1 += e1[q];
    a0 = wave_sum(a0), a1 = wave_sum(a1);
    const bool has = y >= 0 && y < C;
    if (lane == 0) {
      p0y[r] = has ? a0 / S0 : NAN;
      p1y[r] = has ? a1 / S1 : NAN;
    }
  }
}

int check_shape(const char* who, int mode, int64_t n_total, int64_t n_rows, int64_t C, const void* logits,
                const int32_t* rows) {
  if (mode < kTS || mode > kETS) return fail(WG_ERR_INVALID, "%s: mode %d is none of TS 0, VS 1, MS 2, ETS 3", who, mode);
  if (n_total < 0 || n_rows < 0 || C < 1)
    return fail(WG_ERR_INVALID, "%s: bad shape (n=%lld rows=%lld C=%lld)", who, (long long)n_total, (long long)n_rows,
                (long long)C);
  const int maxc = mode == kMS ? kScaleMaxCMS : kScaleMaxC;
  if (C > maxc) return fail(WG_ERR_UNSUPPORTED, "%s: C=%lld above %d for mode %d", who, (long long)C, maxc, mode);
  if (n_total > INT32_MAX || n_rows > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld / rows=%lld exceed int32", who, (long long)n_total, (long long)n_rows);
  if (!rows && n_rows != n_total)
    return fail(WG_ERR_INVALID, "%s: no row list, but %lld rows of %lld", who, (long long)n_rows, (long long)n_total);
  if (n_rows > 0 && !logits) return fail(WG_ERR_INVALID, "%s: NULL logits with %lld rows", who, (long long)n_rows);
  return WG_OK;
}

int check_params(const char* who, int mode, const void* p0, const void* p1, const void* p2, const void* p3) {
  const bool ok = mode == kMS ? (p0 && p1) : mode == kETS ? (p0 && p1 && p2 && p3) : p0 != nullptr;
  return ok ? WG_OK : fail(WG_ERR_INVALID, "%s: a NULL parameter of mode %d", who, mode);
}

int64_t state_slots(int mode, int64_t C, int64_t max_epochs, int64_t max_rows) {
  return kStHeader + 3 * n_params(mode, C) + 2 * max_epochs + n_chunks_of(max_rows) * partial_len(mode, C);
}

// One workgroup per chunk: the chunk fixes the bits AND is the unit of parallelism, so 29 799 rows are 117 workgroups
// on 256 CUs.  Smaller chunks fill the GPU but lengthen the last workgroup's serial sum over the chunk vectors, which
// cost more than it gained at 64 rows; a second level of parallelism inside a chunk is not built.
unsigned pick_grid(int64_t n_chunks, int n_workgroups) {
  if (n_workgroups > 0) return (unsigned)n_workgroups;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(kMaxGrid, n_chunks));
}

}  // namespace
}  // namespace wg

using namespace wg;

#define WG_SCALE_MODES(mode_, MACRO) \
  switch (mode_) {                   \
    case kTS: MACRO(kTS) break;      \
    case kVS: MACRO(kVS) break;      \
    case kMS: MACRO(kMS) break;      \
    default: MACRO(kETS) break;      \
  }

extern "C" {

int wg_scale_max_c(int32_t mode) {
  if (mode < kTS || mode > kETS) return fail(WG_ERR_INVALID, "wg_scale_max_c: mode %d", mode);
  return mode == kMS ? kScaleMaxCMS : kScaleMaxC;
}

int wg_scale_chunk_rows(void) { return kChunkRows; }

int wg_scale_forward(int32_t mode, int32_t flags, int64_t n_total, int64_t n_rows, int64_t C, const float* logits,
                     const int32_t* rows, const float* p0, const float* p1, const float* p2, const float* p3,
                     float* out, void* stream_) {
  static const char* who = "wg_scale_forward";
  if (int rc = check_shape(who, mode, n_total, n_rows, C, logits, rows)) return rc;
  if (int rc = check_params(who, mode, p0, p1, p2, p3)) return rc;
  if (n_rows == 0) return WG_OK;
  if (!out || out == logits) return fail(WG_ERR_INVALID, "%s: out is NULL or aliases logits", who);
  const PassArgs a{n_total, n_rows, (int)C, (flags & 1) != 0, logits, rows, nullptr, nullptr, nullptr, nullptr};
  const dim3 grid((unsigned)std::min<int64_t>(4096, ceil_div(n_rows, kScaleWaves)));
#define WG_SCALE_FWD(m) \
  hipLaunchKernelGGL((scale_forward_kernel<m>), grid, dim3(kBlock), 0, as_stream(stream_), a, p0, p1, p2, p3, out);
  WG_SCALE_MODES(mode, WG_SCALE_FWD)
#undef WG_SCALE_FWD
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_scale_backward_workspace(int32_t mode, int64_t n_rows, int64_t C, int64_t* bytes) {
  if (!bytes || mode < kTS || mode > kETS || n_rows < 0 || C < 1)
    return fail(WG_ERR_INVALID, "wg_scale_backward_workspace: bad arguments");
  *bytes = std::max<int64_t>(1, n_chunks_of(n_rows)) * partial_len(mode, C) * (int64_t)sizeof(double);
  return WG_OK;
}

int wg_scale_backward(int32_t mode, int32_t flags, int64_t n_total, int64_t n_rows, int64_t C, const float* logits,
                      const int32_t* rows, const float* p0, const float* p1, const float* p2, const float* p3,
                      const float* g_out, float* g_logits, float* g_p0, float* g_p1, float* g_p2, float* g_p3,
                      void* workspace, void* stream_) {
  static const char* who = "wg_scale_backward";
  if (int rc = check_shape(who, mode, n_total, n_rows, C, logits, rows)) return rc;
  if (int rc = check_params(who, mode, p0, p1, p2, p3)) return rc;
  const bool want = g_p0 || g_p1 || g_p2 || g_p3;
  if (want && !workspace) return fail(WG_ERR_INVALID, "%s: parameter gradients need the workspace", who);
  if (n_rows > 0 && (!g_out || (g_logits && (g_logits == g_out || g_logits == logits))))
    return fail(WG_ERR_INVALID, "%s: g_out is NULL, or g_logits aliases an input", who);
  hipStream_t stream = as_stream(stream_);
  const int64_t n_chunks = n_chunks_of(n_rows);
  double* partial = want ? static_cast<double*>(workspace) : nullptr;
  if (n_rows > 0) {
    const PassArgs a{n_total, n_rows, (int)C, (flags & 1) != 0, logits, rows, nullptr, g_out, g_logits, partial};
    const dim3 grid(pick_grid(n_chunks, 0));
#define WG_SCALE_BWD(m) \
  hipLaunchKernelGGL((scale_backward_kernel<m>), grid, dim3(kBlock), 0, stream, a, p0, p1, p2, p3, n_chunks);
    WG_SCALE_MODES(mode, WG_SCALE_BWD)
#undef WG_SCALE_BWD
    WG_LAUNCH_CHECK();
  }
  if (want) {
    const int64_t P = n_params(mode, C);
    hipLaunchKernelGGL(scale_reduce_kernel, dim3((unsigned)ceil_div(P, 256)), dim3(256), 0, stream, (int)mode, (int)C,
                       n_chunks, partial, g_p0, g_p1, g_p2, g_p3);
    WG_LAUNCH_CHECK();
  }
  return WG_OK;
}

int wg_scale_state_bytes(int32_t mode, int64_t C, int64_t max_epochs, int64_t max_rows, int64_t* bytes) {
  if (!bytes || mode < kTS || mode > kMS || C < 1 || max_epochs < 1 || max_rows < 1)
    return fail(WG_ERR_INVALID, "wg_scale_state_bytes: bad arguments (mode=%d C=%lld epochs=%lld rows=%lld; ETS has no "
                "trained parameters)", mode, (long long)C, (long long)max_epochs, (long long)max_rows);
  if (C > (mode == kMS ? kScaleMaxCMS : kScaleMaxC))
    return fail(WG_ERR_UNSUPPORTED, "wg_scale_state_bytes: C=%lld above the limit of mode %d", (long long)C, mode);
  *bytes = state_slots(mode, C, max_epochs, max_rows) * (int64_t)sizeof(double);
  return WG_OK;
}

int wg_scale_state_init(void* state, int32_t mode, int32_t flags, int64_t C, int64_t max_epochs, int64_t max_rows,
                        int32_t patience, double lr, double weight_decay, double lambda, const float* init_params,
                        void* stream_) {
  int64_t bytes;
  if (int rc = wg_scale_state_bytes(mode, C, max_epochs, max_rows, &bytes)) return rc;
  if (!state || (reinterpret_cast<uintptr_t>(state) & 7u) || patience < 1)
    return fail(WG_ERR_INVALID, "wg_scale_state_init: NULL or unaligned state, or patience %d < 1", patience);
  const int64_t slots = bytes / (int64_t)sizeof(double);
  hipLaunchKernelGGL(scale_state_init_kernel, dim3((unsigned)std::min<int64_t>(1024, ceil_div(slots, 256))), dim3(256),
                     0, as_stream(stream_), static_cast<double*>(state), (int)mode, (int)flags, (int)C, max_epochs,
                     max_rows, (int)patience, lr, weight_decay, lambda, init_params, slots);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_scale_state_read(const void* state, int32_t mode, int64_t C, int64_t max_epochs, float* params, double* info,
                        void* stream_) {
  int64_t bytes;
  if (int rc = wg_scale_state_bytes(mode, C, max_epochs, 1, &bytes)) return rc;
  if (!state) return fail(WG_ERR_INVALID, "wg_scale_state_read: NULL state");
  const int64_t items = n_params(mode, C) + 5 + 2 * max_epochs;
  hipLaunchKernelGGL(scale_state_read_kernel, dim3((unsigned)std::min<int64_t>(1024, ceil_div(items, 256))), dim3(256),
                     0, as_stream(stream_), static_cast<const double*>(state), (int)mode, (int)C, max_epochs, params,
                     info);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_scale_epoch(void* state, int32_t mode, int32_t flags, int64_t C, int64_t max_epochs, int64_t max_rows,
                   int64_t n_total, int64_t n_rows, const float* logits, const int32_t* rows, const int64_t* labels,
                   int32_t n_workgroups, void* stream_) {
  static const char* who = "wg_scale_epoch";
  if (int rc = check_shape(who, mode, n_total, n_rows, C, logits, rows)) return rc;
  if (mode == kETS) return fail(WG_ERR_INVALID, "%s: ETS has no trained parameters (its TS is trained)", who);
  if (!state || !labels || n_rows < 1 || max_epochs < 1)
    return fail(WG_ERR_INVALID, "%s: NULL state / labels, no rows or no epochs", who);
  if (n_rows > max_rows)   // the block holds the chunk partials of max_rows rows
    return fail(WG_ERR_INVALID, "%s: %lld rows, the state block was sized for %lld", who, (long long)n_rows,
                (long long)max_rows);
  if (n_workgroups < 0 || n_workgroups > kMaxGrid)
    return fail(WG_ERR_INVALID, "%s: n_workgroups %d outside [0, %d]", who, n_workgroups, kMaxGrid);
  const int64_t n_chunks = n_chunks_of(n_rows);
  double* st = static_cast<double*>(state);
  double* partial = st + kStHeader + 3 * n_params(mode, C) + 2 * max_epochs;
  const PassArgs a{n_total, n_rows, (int)C, (flags & 1) != 0, logits, rows, labels, nullptr, nullptr, partial};
  const dim3 grid(pick_grid(n_chunks, n_workgroups));
#define WG_SCALE_EPOCH(m) \
  hipLaunchKernelGGL((scale_epoch_kernel<m>), grid, dim3(kBlock), 0, as_stream(stream_), a, st, n_chunks, \
                     max_epochs, max_rows);
  switch (mode) {
    case kTS: WG_SCALE_EPOCH(kTS) break;
    case kVS: WG_SCALE_EPOCH(kVS) break;
    default: WG_SCALE_EPOCH(kMS) break;
  }
#undef WG_SCALE_EPOCH
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_ets_label_probs(int64_t n_total, int64_t n_rows, int64_t C, const float* logits, const int32_t* rows,
                       const int64_t* labels, const float* temperature, double* p0y, double* p1y, void* stream_) {
  static const char* who = "wg_ets_label_probs";
  if (int rc = check_shape(who, kETS, n_total, n_rows, C, logits, rows)) return rc;
  if (n_rows == 0) return WG_OK;
  if (!labels || !temperature || !p0y || !p1y || p0y == p1y)
    return fail(WG_ERR_INVALID, "%s: NULL labels / temperature / output, or one output twice", who);
  const PassArgs a{n_total, n_rows, (int)C, false, logits, rows, labels, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(ets_label_probs_kernel, dim3((unsigned)std::min<int64_t>(4096, ceil_div(n_rows, kScaleWaves))),
                     dim3(kBlock), 0, as_stream(stream_), a, temperature, p0y, p1y);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // extern "C"
