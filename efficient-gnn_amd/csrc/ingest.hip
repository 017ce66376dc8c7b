// ingest.hip -- SURVEY section 8(f) rank 1, second half: an edge list (COO) to canonical CSR on the device.
// The reference builds its adjacency from edge_index through a dense (N, N) tensor:
//     adj[src, dst] = 1                                         (calibration/utils.py:19-25 via
//                                                                benchmark_calibration_methods.py:53)
//     adj = clamp(adj + adj.t(), 0, 1); adj.fill_diagonal_(1)   (ugca_calib_attack.py:42-47,
//                                                                exp/ablation/ugca_full_multi_dataset.py:135-140)
// and gives the dense form up above 50 000 nodes (ugca_full_multi_dataset.py:128-133).  wg_coo_to_csr
// computes the CSR of the same matrix without it:
//
//   1. expand: emitted entry p gets the key (row << cbits) | col, cbits = bit width of n - 1.  The forward
//      entry of edge e is p = e, its mirrored entry (WG_COO_SYMMETRIC) p = E + e, the unit diagonal of
//      WG_COO_LOOPS_ONE follows.  An entry that is not kept (an id outside [0, n), which is also counted;
//      an input loop that the loop mode replaces) gets the key 1 << 2 cbits, above every kept key: no
//      later kernel forms an index from it.
//   2. a stable radix sort of the keys over 2 cbits + 1 bits (with WG_COO_SUM the weights ride along), so
//      the entries of one (row, col) stay in emitted order: forward in input order, then mirrored in input
//      order.
//   3. run heads: the first entry of each run of equal kept keys; WG_COO_SUM: the head's thread adds the
//      run's weights in that order in float64 and rounds once.  A head is kept when its value != 0.
//   4. an inclusive scan of the keep flags, a compaction (column, value, row of each kept entry) and the row
//      pointers: indptr[r] = the number of kept entries in rows < r, a binary search over the kept rows.
//
// No float atomics and no order that depends on scheduling: the same input gives the same bits.  Temporary
// memory (one allocation): 16 M bytes of keys + 4 M of flags + the sort's and the scan's workspace, with
// WG_COO_SUM 8 M more for the weights, M = wg_coo_capacity.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "internal.h"

namespace wg {
namespace {

constexpr uint32_t kCooKnown = WG_COO_SYMMETRIC | WG_COO_SUM | WG_COO_LOOPS_REMOVE | WG_COO_LOOPS_ONE;

struct CooShape {
  int64_t n = 0, E = 0, M = 0;
  int cbits = 1;
  bool sym = false, sum = false, drop_loops = false, unit_diag = false;
  __host__ __device__ uint64_t invalid() const { return 1ull << (2 * cbits); }  // the key of an entry that is not kept
};

// the emitted-entry count of (n, E, flags), after the flags and the sizes are checked
int coo_shape(const char* who, int64_t n, int64_t E, uint32_t flags, CooShape* s) {
  if (n < 0 || E < 0)
    return fail(WG_ERR_INVALID, "%s: negative size (n=%lld n_edges=%lld)", who, (long long)n, (long long)E);
  if (flags & ~kCooKnown) return fail(WG_ERR_INVALID, "%s: unknown flag bits 0x%x", who, flags & ~kCooKnown);
  if ((flags & WG_COO_LOOPS_REMOVE) && (flags & WG_COO_LOOPS_ONE))
    return fail(WG_ERR_INVALID, "%s: WG_COO_LOOPS_REMOVE and WG_COO_LOOPS_ONE exclude each other", who);
  s->n = n;
  s->E = E;
  s->sym = (flags & WG_COO_SYMMETRIC) != 0;
  s->sum = (flags & WG_COO_SUM) != 0;
  s->drop_loops = (flags & (WG_COO_LOOPS_REMOVE | WG_COO_LOOPS_ONE)) != 0;
  s->unit_diag = (flags & WG_COO_LOOPS_ONE) != 0;
  if (n > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "%s: n=%lld exceeds int32", who, (long long)n);
  // checked on its own so that the count below cannot overflow
  if (E > INT32_MAX) return fail(WG_ERR_UNSUPPORTED, "%s: n_edges=%lld exceeds int32", who, (long long)E);
  s->M = E * (s->sym ? 2 : 1) + (s->unit_diag ? n : 0);
  if (s->M > INT32_MAX)
    return fail(WG_ERR_UNSUPPORTED, "%s: %lld emitted entries exceed int32 (split the edge list)", who,
                (long long)s->M);
  s->cbits = 1;
  while ((1ll << s->cbits) < n) ++s->cbits;  // n <= 2^31: cbits <= 31, a key has at most 63 bits
  return WG_OK;
}

template <typename IdT>
__global__ __launch_bounds__(kBlock) void coo_expand_kernel(CooShape s, const IdT* __restrict__ src,
                                                            const IdT* __restrict__ dst,
                                                            const float* __restrict__ weights,
                                                            uint64_t* __restrict__ keys, float* __restrict__ w,
                                                            unsigned long long* __restrict__ n_bad) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t invalid = s.invalid();
  if (i < s.E) {
    const int64_t r = (int64_t)src[i];
    const int64_t c = (int64_t)dst[i];
    const int n_out = (r < 0 || r >= s.n) + (c < 0 || c >= s.n);
    const bool bad = n_out != 0;
    if (bad) atomicAdd(n_bad, (unsigned long long)n_out);
    const bool keep = !bad && !(s.drop_loops && r == c);
    WG_DCHECK(i < s.M && (!s.sym || s.E + i < s.M), "coo expand: edge %lld past %lld emitted entries", (long long)i,
              (long long)s.M);
    keys[i] = keep ? ((uint64_t)r << s.cbits) | (uint64_t)c : invalid;
    if (s.sym) keys[s.E + i] = keep ? ((uint64_t)c << s.cbits) | (uint64_t)r : invalid;
    if (w) {
      const float v = weights ? weights[i] : 1.0f;
      w[i] = v;
      if (s.sym) w[s.E + i] = v;
    }
  }
  if (s.unit_diag && i < s.n) {
    const int64_t p = s.M - s.n + i;
    WG_DCHECK(p >= 0 && p < s.M, "coo expand: diagonal entry %lld outside [0, %lld)", (long long)p, (long long)s.M);
    keys[p] = ((uint64_t)i << s.cbits) | (uint64_t)i;
    if (w) w[p] = 1.0f;
  }
}

// keep[p] = 1 at the head of a run of equal kept keys whose value is != 0; WG_COO_SUM (w != NULL): val[p] = the
// run's float64 sum in sorted (= emitted) order, rounded once
__global__ __launch_bounds__(kBlock) void coo_heads_kernel(CooShape s, const uint64_t* __restrict__ keys,
                                                           const float* __restrict__ w, float* __restrict__ val,
                                                           int32_t* __restrict__ keep) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= s.M) return;
  const uint64_t k = keys[p];
  bool head = k < s.invalid() && (p == 0 || keys[p - 1] != k);
  if (head && w) {
    double acc = 0.0;
    for (int64_t q = p; q < s.M && keys[q] == k; ++q) acc += (double)w[q];
    const float v = (float)acc;
    val[p] = v;
    head = v != 0.0f;
  }
  keep[p] = head ? 1 : 0;
}

// inc: the inclusive scan of keep.  Kept entry p goes to position inc[p] - 1; meta[1] = the kept count
__global__ __launch_bounds__(kBlock) void coo_compact_kernel(CooShape s, int64_t capacity,
                                                             const uint64_t* __restrict__ keys,
                                                             const int32_t* __restrict__ inc,
                                                             const float* __restrict__ val,
                                                             int32_t* __restrict__ indices, float* __restrict__ values,
                                                             int32_t* __restrict__ out_row,
                                                             int64_t* __restrict__ meta) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= s.M) return;
  const int32_t c = inc[p];
  if (p == s.M - 1) meta[1] = c;
  if (c == (p ? inc[p - 1] : 0)) return;
  const int64_t o = (int64_t)c - 1;
  const uint64_t k = keys[p];
  const int64_t row = (int64_t)(k >> s.cbits), col = (int64_t)(k & ((1ull << s.cbits) - 1));
  WG_DCHECK(o >= 0 && o < capacity && o <= p, "coo compact: entry %lld to position %lld of %lld", (long long)p,
            (long long)o, (long long)capacity);
  WG_DCHECK(row < s.n && col < s.n, "coo compact: entry %lld is (%lld, %lld) of n=%lld", (long long)p,
            (long long)row, (long long)col, (long long)s.n);
  indices[o] = (int32_t)col;
  if (values) values[o] = val ? val[p] : 1.0f;
  out_row[o] = (int32_t)row;
}

// indptr[r] = the number of kept entries in rows < r (rows ascending in out_row): a row without entries
// gets the position of the next entry
__global__ __launch_bounds__(kBlock) void coo_indptr_kernel(int64_t n, const int32_t* __restrict__ out_row,
                                                            const int64_t* __restrict__ meta,
                                                            int64_t* __restrict__ indptr) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r > n) return;
  int64_t lo = 0, hi = meta[1];
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (out_row[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  indptr[r] = lo;
}

struct DeviceBlock {
  char* p = nullptr;
  ~DeviceBlock() { (void)hipFree(p); }  // hipFree waits for the work that still uses it
};

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

template <typename IdT>
int coo_to_csr(const CooShape& s, const IdT* src, const IdT* dst, const float* weights, int64_t* indptr,
               int32_t* indices, float* values, int64_t capacity, int64_t* nnz_host, hipStream_t stream) {
  const int M = (int)s.M, end_bit = 2 * s.cbits + 1;
  uint64_t* knull = nullptr;
  float* fnull = nullptr;
  int32_t* inull = nullptr;
  size_t sort_bytes = 0, scan_bytes = 0;
  if (s.sum)
    WG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, knull, knull, fnull, fnull, M, 0, end_bit,
                                                  stream));
  else
    WG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, knull, knull, M, 0, end_bit, stream));
  WG_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, inull, inull, M, stream));
  // one block: [meta 2 x int64 | keys M | sorted keys M | keep / inc M | (weights M | sorted weights M) | cub]
  const size_t o_keys = 256, o_sorted = o_keys + align256(sizeof(uint64_t) * M),
               o_keep = o_sorted + align256(sizeof(uint64_t) * M), o_w = o_keep + align256(sizeof(int32_t) * M),
               o_ws = o_w + (s.sum ? align256(sizeof(float) * M) : 0),
               o_cub = o_ws + (s.sum ? align256(sizeof(float) * M) : 0),
               total = o_cub + align256(std::max(sort_bytes, scan_bytes));
  DeviceBlock blk;
  WG_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&blk.p), total));
  int64_t* meta = reinterpret_cast<int64_t*>(blk.p);  // {ids outside [0, n), kept entries}
  uint64_t* keys = reinterpret_cast<uint64_t*>(blk.p + o_keys);
  uint64_t* sorted = reinterpret_cast<uint64_t*>(blk.p + o_sorted);
  int32_t* keep = reinterpret_cast<int32_t*>(blk.p + o_keep);
  float* w = s.sum ? reinterpret_cast<float*>(blk.p + o_w) : nullptr;
  float* w_sorted = s.sum ? reinterpret_cast<float*>(blk.p + o_ws) : nullptr;
  void* cub_tmp = blk.p + o_cub;
  // after the sort the unsorted copies are free: the kept entries' rows and the runs' sums go there
  int32_t* out_row = reinterpret_cast<int32_t*>(keys);
  float* val = w;

  WG_HIP_TRY(hipMemsetAsync(meta, 0, 2 * sizeof(int64_t), stream));
  if (M > 0) {
    const dim3 grid_m((unsigned)ceil_div(M, kBlock)), block(kBlock);
    hipLaunchKernelGGL(coo_expand_kernel<IdT>, dim3((unsigned)ceil_div(std::max(s.E, s.unit_diag ? s.n : 0), kBlock)),
                       block, 0, stream, s, src, dst, weights, keys, w, reinterpret_cast<unsigned long long*>(meta));
    WG_LAUNCH_CHECK();
    if (s.sum)
      WG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(cub_tmp, sort_bytes, keys, sorted, w, w_sorted, M, 0, end_bit,
                                                    stream));
    else
      WG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(cub_tmp, sort_bytes, keys, sorted, M, 0, end_bit, stream));
    hipLaunchKernelGGL(coo_heads_kernel, grid_m, block, 0, stream, s, sorted, w_sorted, val, keep);
    WG_LAUNCH_CHECK();
    WG_HIP_TRY(hipcub::DeviceScan::InclusiveSum(cub_tmp, scan_bytes, keep, keep, M, stream));
    hipLaunchKernelGGL(coo_compact_kernel, grid_m, block, 0, stream, s, capacity, sorted, keep, val, indices, values,
                       out_row, meta);
    WG_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(coo_indptr_kernel, dim3((unsigned)ceil_div(s.n + 1, kBlock)), dim3(kBlock), 0, stream, s.n,
                     out_row, meta, indptr);
  WG_LAUNCH_CHECK();
  int64_t meta_host[2] = {0, 0};
  WG_HIP_TRY(hipMemcpyAsync(meta_host, meta, sizeof(meta_host), hipMemcpyDeviceToHost, stream));
  WG_HIP_TRY(hipStreamSynchronize(stream));
  if (meta_host[0] != 0)
    return fail(WG_ERR_INVALID, "wg_coo_to_csr: %lld ids outside [0, %lld)", (long long)meta_host[0], (long long)s.n);
  *nnz_host = meta_host[1];
  return WG_OK;
}

}  // namespace
}  // namespace wg

using namespace wg;

extern "C" {

int wg_coo_capacity(int64_t n, int64_t n_edges, uint32_t flags, int64_t* capacity_host) {
  if (!capacity_host) return fail(WG_ERR_INVALID, "wg_coo_capacity: capacity_host is NULL");
  CooShape s;
  if (int rc = coo_shape("wg_coo_capacity", n, n_edges, flags, &s)) return rc;
  *capacity_host = s.M;
  return WG_OK;
}

int wg_coo_to_csr(int64_t n, int64_t n_edges, const void* src, const void* dst, int32_t id_bytes, const float* weights,
                  uint32_t flags, int64_t* indptr, int32_t* indices, float* values, int64_t capacity,
                  int64_t* nnz_host, void* stream_) {
  CooShape s;
  if (int rc = coo_shape("wg_coo_to_csr", n, n_edges, flags, &s)) return rc;
  if (id_bytes != 4 && id_bytes != 8)
    return fail(WG_ERR_INVALID, "wg_coo_to_csr: id_bytes must be 4 or 8 (id_bytes=%d)", (int)id_bytes);
  if (!indptr || !nnz_host) return fail(WG_ERR_INVALID, "wg_coo_to_csr: NULL indptr / nnz_host");
  if (n_edges > 0 && (!src || !dst))
    return fail(WG_ERR_INVALID, "wg_coo_to_csr: NULL src / dst with n_edges=%lld", (long long)n_edges);
  if (weights && !s.sum) return fail(WG_ERR_INVALID, "wg_coo_to_csr: weights need WG_COO_SUM");
  if (capacity < s.M)
    return fail(WG_ERR_INVALID, "wg_coo_to_csr: capacity %lld below the %lld entries of wg_coo_capacity",
                (long long)capacity, (long long)s.M);
  if (s.M > 0 && (!indices || (s.sum && !values)))
    return fail(WG_ERR_INVALID, "wg_coo_to_csr: NULL indices%s with capacity %lld", s.sum ? " / values" : "",
                (long long)capacity);
  hipStream_t stream = as_stream(stream_);
  if (id_bytes == 4)
    return coo_to_csr(s, static_cast<const int32_t*>(src), static_cast<const int32_t*>(dst), weights, indptr, indices,
                      values, capacity, nnz_host, stream);
  return coo_to_csr(s, static_cast<const int64_t*>(src), static_cast<const int64_t*>(dst), weights, indptr, indices,
                    values, capacity, nnz_host, stream);
}

}  // extern "C"
