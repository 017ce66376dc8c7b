// watstrain.hip -- SURVEY section 8(f)-3: one epoch of the WATS calibrator's calib_train (reference
// calibration/WATS.py:132-170) over the calibration rows in one launch, the design of wg_scale_epoch (scale.hip):
//
//     pre_j = b1_j + sum_f W1[j][f] H[f],   t = b2 + sum_j W2_j relu(pre_j)        (Linear(F, hid) - ReLU - Linear(hid, 1))
//     T = log(exp(t) + 1.1),   out = log_softmax(z / T),   loss = -mean out[r, y_r]                      (WATS.py:124-130, :150)
//
// then, in the workgroup that arrives last, torch's Adam step with L2 weight decay on all four tensors, the
// early-stopping state and the traces, all in one device state block, so that a training run needs no host round trip.
//
// Decomposition.  A wave per row: the hidden units on lanes 0 .. hid - 1 (hid <= 64) as in head.hip, the columns on all
// lanes as in scale.hip (row_dev.h, C <= 256).  Rows are cut into FIXED chunks of kChunkRows = 256 listed rows; a
// workgroup takes whole chunks, wave w the rows w, w + 4, ... of the chunk in ascending order.  A wave keeps its sums of
// gb1, gW2, gb2, the loss and the correct count in registers and its gW1 [hid][F] in LDS (four waves x P doubles,
// head.hip's bound: P <= 2048); the waves' sums are added in wave order and each chunk leaves one float64 partial
// vector: loss sum, correct count, then gW1, gb1, gW2, gb2.  The last workgroup adds the partials in chunk order, so the
// bits depend on the rows, F, hid and C only, never on the grid.  The hand-off is scale.hip's: partials drained, one
// relaxed agent-scope fetch_add per workgroup, no workgroup waits on another.
//
// Arithmetic.  Everything is float64, from the float64 master parameters and the float32 H / logits widened.  ReLU is
// active iff pre_j > 0 and hands a NaN on; pre_j == 0 is inactive with gradient 0, as torch's.  The constant is
// (double)1.1f, the value the reference's float32 tensor holds and head.hip uses.  No float atomics.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "internal.h"
#include "row_dev.h"

namespace wg {
namespace {

constexpr int kTrainMaxParams = 2048;   // four waves x P doubles of LDS = 64 KB
constexpr int kTrainMaxHid = 64;        // a hidden unit per lane
constexpr int kChunkRows = 256;         // listed rows per partial vector, as scale.hip
constexpr int kTrainWaves = kBlock / 64;
constexpr int kMaxGrid = 1024;
constexpr double kBeta1 = 0.9, kBeta2 = 0.999, kAdamEps = 1e-8;
constexpr double kTempShift = (double)1.1f;

// the state block, in 8-byte slots: slot 0 holds the arrival counter (uint32), the rest doubles; slots 1 .. 5 are what
// wg_wats_train_state_read returns first, in wg_scale_state_read's order
enum : int {
  kStTicket = 0, kStStopped, kStEpochs, kStStep, kStPatienceLeft, kStBest, kStLr, kStWd, kStF, kStPatience,
  kStMaxEpochs, kStHid, kStC, kStParams, kStMaxRows, kStReserved, kStHeader
};

__host__ __device__ inline int64_t n_params(int64_t F, int hid) { return (int64_t)hid * F + 2 * hid + 1; }
inline int64_t n_chunks_of(int64_t rows) { return ceil_div(rows, kChunkRows); }
inline int64_t state_slots(int64_t F, int hid, int64_t max_epochs, int64_t max_rows) {
  const int64_t P = n_params(F, hid);
  return kStHeader + 3 * P + 2 * max_epochs + n_chunks_of(max_rows) * (P + 2);
}

struct TrainArgs {
  int64_t n_total, n_rows, F;
  int C, hid;
  const float* H;            // (n_total, F)
  const float* logits;       // (n_total, C)
  const int32_t* rows;       // nullable
  const int64_t* labels;     // by ORIGINAL row id
  double* partial;           // [chunks][2 + P]
};

__device__ inline void put(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // sc1
}
__device__ inline double get(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One chunk: rows [ch * kChunkRows, ...) of the list.  sh: the workgroup's [4 waves][P] doubles.
__device__ inline void chunk_pass(const TrainArgs& a, int64_t ch, const double* theta, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = a.C, hid = a.hid;
  const int64_t F = a.F, HF = (int64_t)hid * F, P = n_params(F, hid), Q = P + 2;
  const bool unit = lane < hid;
  const double* w1 = theta + (int64_t)(unit ? lane : 0) * F;
  const double w10 = unit ? w1[0] : 0.0, b1 = unit ? theta[HF + lane] : 0.0, w2 = unit ? theta[HF + hid + lane] : 0.0;
  const double b2 = theta[P - 1];
  double* mine = sh + wave * P;
  for (int64_t i = lane; i < HF; i += 64) mine[i] = 0.0;
  __syncthreads();
  double loss = 0.0, correct = 0.0, gb1 = 0.0, gw2 = 0.0, gb2 = 0.0;
  const int64_t r1 = a.n_rows < (ch + 1) * kChunkRows ? a.n_rows : (ch + 1) * kChunkRows;
  for (int64_t r = ch * kChunkRows + wave; r < r1; r += kTrainWaves) {
    const int64_t i = a.rows ? (int64_t)a.rows[r] : r;
    WG_DCHECK(i >= 0 && i < a.n_total, "wats_train: listed row %lld is %lld, outside [0, %lld)", (long long)r,
              (long long)i, (long long)a.n_total);
    const int64_t y = a.labels[i];
    WG_DCHECK(y >= 0 && y < C, "wats_train: row %lld has the label %lld of %d classes", (long long)i, (long long)y, C);
    const float* h = a.H + i * F;
    double z[kNQ];
    load_row(z, a.logits + i * C, C, lane);
    // the head: pre-activations on the lanes, t on every lane
    double pre = 0.0, rl = 0.0;
    if (unit) {
      pre = b1 + w10 * (double)h[0];
      for (int64_t f = 1; f < F; ++f) pre += w1[f] * (double)h[f];
      rl = pre > 0.0 ? pre : (pre == pre ? 0.0 : pre);            // a NaN goes on
    }
    const double t = b2 + wave_sum(w2 * rl);
    const double et = exp(t);
    const double T = log(et + kTempShift);                        // WATS.py:125
    // log_softmax(z / T), the nll's gradient of the SUM (the mean's 1 / n_rows comes with the partials)
    double v[kNQ], e[kNQ], out[kNQ], m, S;
#pragma unroll
    for (int q = 0; q < kNQ; ++q) v[q] = z[q] / T;
    row_exp(v, C, lane, e, &m, &S);
    const double lse = log(S);
    double ly = 0.0, dts = 0.0;
#pragma unroll
    for (int q = 0; q < kNQ; ++q) {
      const bool at = lane + 64 * q == y;
      out[q] = v[q] - m - lse;
      ly -= at ? out[q] : 0.0;
      if (lane + 64 * q < C) dts += (e[q] / S - (at ? 1.0 : 0.0)) * z[q];   // d loss / d (z / T) times z
    }
    loss += wave_sum(ly);
    correct += wave_argmax(out, C, lane) == y ? 1.0 : 0.0;
    const double dT = -wave_sum(dts) / (T * T);
    const double dt = dT * (et / (et + kTempShift));
    gb2 += dt;
    if (unit) {
      gw2 += dt * rl;
      const double dz = pre > 0.0 ? dt * w2 : 0.0;
      gb1 += dz;
      for (int64_t f = 0; f < F; ++f) mine[(int64_t)lane * F + f] += dz * (double)h[f];
    }
  }
  if (unit) mine[HF + lane] = gb1, mine[HF + hid + lane] = gw2;
  if (lane == 0) mine[P - 1] = gb2;
  __syncthreads();
  // the waves' sums, added in wave order
  for (int64_t idx = threadIdx.x; idx < P; idx += kBlock) {
    double s = sh[idx];
    for (int w = 1; w < kTrainWaves; ++w) s += sh[w * P + idx];
    put(a.partial + ch * Q + 2 + idx, s);
  }
  __syncthreads();
  if (lane == 0) sh[2 * wave] = loss, sh[2 * wave + 1] = correct;   // P >= 4: eight doubles fit
  __syncthreads();
  if (threadIdx.x < 2) {
    double s = sh[threadIdx.x];
    for (int w = 1; w < kTrainWaves; ++w) s += sh[2 * w + threadIdx.x];
    put(a.partial + ch * Q + threadIdx.x, s);
  }
  __syncthreads();   // sh is free for the next chunk
}

// The last workgroup's part of an epoch: the chunk partials in chunk order, Adam, early stopping (scale.hip's).
__device__ inline void epoch_finish(double* st, int64_t P, int64_t n_rows, int64_t n_chunks, const double* partial) {
  const int64_t Q = P + 2;
  const int tid = threadIdx.x;
  const double lr = st[kStLr], wd = st[kStWd];
  const int64_t max_epochs = (int64_t)st[kStMaxEpochs];
  const int64_t epoch = (int64_t)st[kStEpochs];
  const double step = st[kStStep] + 1.0;
  double* theta = st + kStHeader;
  double* m1 = theta + P;
  double* m2 = m1 + P;
  double* trace = m2 + P;
  const double bc1 = 1.0 - pow(kBeta1, step), bc2s = sqrt(1.0 - pow(kBeta2, step));
  for (int64_t i = tid; i < P; i += kBlock) {
    double g = 0.0;
    for (int64_t ch = 0; ch < n_chunks; ++ch) g += get(partial + ch * Q + 2 + i);
    g /= (double)n_rows;                                             // nll_loss's mean
    const double th = theta[i];
    g += wd * th;                                                    // torch's Adam: L2, not decoupled
    const double a = kBeta1 * m1[i] + (1.0 - kBeta1) * g;
    const double b = kBeta2 * m2[i] + (1.0 - kBeta2) * g * g;
    m1[i] = a, m2[i] = b;
    theta[i] = th - (lr / bc1) * (a / (sqrt(b) / bc2s + kAdamEps));
  }
  if (tid == 0) {
    double ls = 0.0, correct = 0.0;
    for (int64_t ch = 0; ch < n_chunks; ++ch) {
      ls += get(partial + ch * Q);
      correct += get(partial + ch * Q + 1);
    }
    const double loss = ls / (double)n_rows;
    trace[epoch] = loss;
    trace[max_epochs + epoch] = correct / (double)n_rows;
    double left = st[kStPatienceLeft];
    if (loss < st[kStBest]) {                                        // WATS.py:162-168; false for a NaN loss
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

__global__ __launch_bounds__(kBlock) void wats_train_epoch_kernel(TrainArgs a, double* st, int64_t n_chunks,
                                                                  int64_t max_epochs, int64_t max_rows) {
  extern __shared__ double g_train_red[];   // [4 waves][P]
  if (st[kStStopped] != 0.0) return;   // set only after every workgroup of its launch arrived: uniform
  WG_DCHECK((int64_t)st[kStF] == a.F && (int)st[kStHid] == a.hid && (int)st[kStC] == a.C &&
                (int64_t)st[kStMaxRows] == max_rows && (int64_t)st[kStMaxEpochs] == max_epochs,
            "wats_train: the state block was initialised for F %lld hid %d C %d rows %lld epochs %lld",
            (long long)st[kStF], (int)st[kStHid], (int)st[kStC], (long long)st[kStMaxRows],
            (long long)st[kStMaxEpochs]);
  for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) chunk_pass(a, ch, st + kStHeader, g_train_red);
  // the hand-off of scale.hip: partials drained, one agent-scope arrival per workgroup, the last one finishes
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int* s_last = reinterpret_cast<int*>(g_train_red);
  uint32_t* ticket = reinterpret_cast<uint32_t*>(st + kStTicket);
  if (threadIdx.x == 0) {
    const uint32_t old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = old + 1u == gridDim.x;
    if (*s_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch starts at 0
  }
  __syncthreads();
  if (*s_last) epoch_finish(st, n_params(a.F, a.hid), a.n_rows, n_chunks, a.partial);
}

__global__ void wats_train_state_init_kernel(double* st, int64_t F, int hid, int C, int64_t max_epochs,
                                             int64_t max_rows, int patience, double lr, double wd, const float* W1,
                                             const float* b1, const float* W2, const float* b2, int64_t slots) {
  const int64_t HF = (int64_t)hid * F, P = n_params(F, hid);
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
    else if (i == kStF) v = (double)F;
    else if (i == kStMaxEpochs) v = (double)max_epochs;
    else if (i == kStHid) v = (double)hid;
    else if (i == kStC) v = (double)C;
    else if (i == kStParams) v = (double)P;
    else if (i == kStMaxRows) v = (double)max_rows;
    else if (i >= kStHeader && i < kStHeader + P) {
      const int64_t k = i - kStHeader;
      v = k < HF ? (double)W1[k] : k < HF + hid ? (double)b1[k - HF] : k < P - 1 ? (double)W2[k - HF - hid] : (double)b2[0];
    }
    st[i] = v;
  }
}

// info: [0] stopped, [1] epochs run, [2] Adam steps, [3] patience left, [4] best loss, then the loss trace and the
// accuracy trace, max_epochs each
__global__ void wats_train_state_read_kernel(const double* st, int64_t F, int hid, int64_t max_epochs, float* W1,
                                             float* b1, float* W2, float* b2, double* info) {
  const int64_t HF = (int64_t)hid * F, P = n_params(F, hid);
  const double* theta = st + kStHeader;
  const double* trace = theta + 3 * P;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P + 5 + 2 * max_epochs;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i < P) {
      float* dst = i < HF ? W1 : i < HF + hid ? b1 : i < P - 1 ? W2 : b2;
      const int64_t at = i < HF ? i : i < HF + hid ? i - HF : i < P - 1 ? i - HF - hid : 0;
      if (dst) dst[at] = (float)theta[i];
    } else if (info) {
      const int64_t j = i - P;
      info[j] = j < 5 ? st[kStStopped + j] : trace[j - 5];
    }
  }
}

int check_head(const char* who, int64_t F, int32_t hid, int64_t max_epochs) {
  if (F < 1 || hid < 1 || hid > kTrainMaxHid || max_epochs < 1)
    return fail(WG_ERR_INVALID, "%s: bad shape (F=%lld hid=%d, at most %d; epochs=%lld)", who, (long long)F, hid,
                kTrainMaxHid, (long long)max_epochs);
  if (F > INT32_MAX || max_epochs > INT32_MAX || n_params(F, hid) > kTrainMaxParams)
    return fail(WG_ERR_UNSUPPORTED, "%s: hid * F + 2 hid + 1 = %lld parameters, above %d", who,
                (long long)n_params(F, hid), kTrainMaxParams);
  return WG_OK;
}

int check_classes(const char* who, int64_t C) {
  if (C < 1) return fail(WG_ERR_INVALID, "%s: C=%lld", who, (long long)C);
  if (C > kRowMaxC) return fail(WG_ERR_UNSUPPORTED, "%s: C=%lld above %d", who, (long long)C, kRowMaxC);
  return WG_OK;
}

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_wats_train_max_params(void) { return kTrainMaxParams; }

int wg_wats_train_chunk_rows(void) { return kChunkRows; }

int wg_wats_train_state_bytes(int64_t F, int32_t hid, int64_t max_epochs, int64_t max_rows, int64_t* bytes) {
  static const char* who = "wg_wats_train_state_bytes";
  if (!bytes || max_rows < 1) return fail(WG_ERR_INVALID, "%s: NULL bytes or max_rows %lld < 1", who, (long long)max_rows);
  if (int rc = check_head(who, F, hid, max_epochs)) return rc;
  if (max_rows > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "%s: max_rows=%lld exceeds int32", who, (long long)max_rows);
  *bytes = state_slots(F, hid, max_epochs, max_rows) * (int64_t)sizeof(double);
  return WG_OK;
}

int wg_wats_train_state_init(void* state, int64_t F, int32_t hid, int64_t C, int64_t max_epochs, int64_t max_rows,
                             int32_t patience, double lr, double weight_decay, const float* W1, const float* b1,
                             const float* W2, const float* b2, void* queue) {
  static const char* who = "wg_wats_train_state_init";
  int64_t bytes;
  if (int rc = wg_wats_train_state_bytes(F, hid, max_epochs, max_rows, &bytes)) return rc;
  if (int rc = check_classes(who, C)) return rc;
  if (!state || (reinterpret_cast<uintptr_t>(state) & 7u) || patience < 1 || !W1 || !b1 || !W2 || !b2)
    return fail(WG_ERR_INVALID, "%s: NULL or unaligned state, a NULL parameter, or patience %d < 1", who, patience);
  const int64_t slots = bytes / (int64_t)sizeof(double);
  hipLaunchKernelGGL(wats_train_state_init_kernel, dim3((unsigned)std::min<int64_t>(1024, ceil_div(slots, 256))),
                     dim3(256), 0, as_stream(queue), static_cast<double*>(state), F, (int)hid, (int)C, max_epochs,
                     max_rows, (int)patience, lr, weight_decay, W1, b1, W2, b2, slots);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_wats_train_state_read(const void* state, int64_t F, int32_t hid, int64_t max_epochs, float* W1, float* b1,
                             float* W2, float* b2, double* info, void* queue) {
  static const char* who = "wg_wats_train_state_read";
  if (int rc = check_head(who, F, hid, max_epochs)) return rc;
  if (!state) return fail(WG_ERR_INVALID, "%s: NULL state", who);
  const int64_t items = n_params(F, hid) + 5 + 2 * max_epochs;
  hipLaunchKernelGGL(wats_train_state_read_kernel, dim3((unsigned)std::min<int64_t>(1024, ceil_div(items, 256))),
                     dim3(256), 0, as_stream(queue), static_cast<const double*>(state), F, (int)hid, max_epochs, W1, b1,
                     W2, b2, info);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

int wg_wats_train_epoch(void* state, int64_t F, int32_t hid, int64_t C, int64_t max_epochs, int64_t max_rows,
                        int64_t n_total, int64_t n_rows, const float* H, const float* logits, const int32_t* rows,
                        const int64_t* labels, int32_t n_workgroups, void* queue) {
  static const char* who = "wg_wats_train_epoch";
  if (int rc = check_head(who, F, hid, max_epochs)) return rc;
  if (int rc = check_classes(who, C)) return rc;
  if (n_total < 0 || n_rows < 1 || max_rows < 1)
    return fail(WG_ERR_INVALID, "%s: bad shape (n=%lld rows=%lld max_rows=%lld)", who, (long long)n_total,
                (long long)n_rows, (long long)max_rows);
  if (n_total > INT32_MAX || n_rows > INT32_MAX || max_rows > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld / rows=%lld / max_rows=%lld exceed int32", who, (long long)n_total,
                (long long)n_rows, (long long)max_rows);
  if (!rows && n_rows != n_total)
    return fail(WG_ERR_INVALID, "%s: no row list, but %lld rows of %lld", who, (long long)n_rows, (long long)n_total);
  if (n_rows > max_rows)   // the block holds the chunk partials of max_rows rows
    return fail(WG_ERR_INVALID, "%s: %lld rows, the state block was sized for %lld", who, (long long)n_rows,
                (long long)max_rows);
  if (!state || !H || !logits || !labels) return fail(WG_ERR_INVALID, "%s: NULL state / H / logits / labels", who);
  if (n_workgroups < 0 || n_workgroups > kMaxGrid)
    return fail(WG_ERR_INVALID, "%s: n_workgroups %d outside [0, %d]", who, n_workgroups, kMaxGrid);
  const int64_t n_chunks = n_chunks_of(n_rows), P = n_params(F, hid);
  double* st = static_cast<double*>(state);
  double* partial = st + kStHeader + 3 * P + 2 * max_epochs;
  const TrainArgs a{n_total, n_rows, F, (int)C, (int)hid, H, logits, rows, labels, partial};
  // one workgroup per chunk, as scale.hip's pick_grid
  const unsigned grid = n_workgroups > 0 ? (unsigned)n_workgroups
                                         : (unsigned)std::max<int64_t>(1, std::min<int64_t>(kMaxGrid, n_chunks));
  const size_t lds = (size_t)kTrainWaves * P * sizeof(double);
  hipLaunchKernelGGL(wats_train_epoch_kernel, dim3(grid), dim3(kBlock), lds, as_stream(queue), a, st, n_chunks,
                     max_epochs, max_rows);
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // extern "C"
