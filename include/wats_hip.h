/*
 * wats_hip.h -- C ABI of the MI355X (gfx950) graph-wavelet feature extractor.
 *
 * Drop-in boundary for the hot path of CaptainCuong/Efficient-GNN
 * `calibration/WATS.py` (the reference is pure Python over scipy.sparse; this
 * header lists the entry points a ctypes / cffi binding of that path binds).
 * Each entry cites the reference function it replaces.
 *
 * Conventions
 *   - Every pointer argument is a DEVICE pointer (hipMalloc / torch CUDA tensor
 *     storage) unless its name ends in `_host`.  Buffers are caller-owned,
 *     row-major, contiguous, F (signal columns) innermost.
 *   - Alignment: a float buffer needs 4-byte alignment only (int32 / int64 / double buffers
 *     that of their element).  Buffers aligned to 16 bytes take the vector kernels (and, in
 *     wg_wavelet_features, the fused finalize and the folded first launch); any other base runs
 *     the 8-byte or scalar forms of the same kernels: same values to the parity tolerance, not
 *     necessarily the same bits as the aligned call.  No entry point rejects a misaligned buffer.
 *   - `stream` is a hipStream_t passed as void* (NULL = legacy default stream).
 *     All work is enqueued on it; no entry point synchronises the device
 *     except the ones documented as "synchronous" (graph creation / dense
 *     ingestion, which size device allocations from device-computed counts).
 *     Entries documented as "may be captured" allocate nothing and read nothing
 *     back, so they may run on a stream that is being captured into a graph and
 *     re-zero whatever they accumulate into on every replay.  tests/stream_cases.py
 *     classifies every entry that takes a stream by these words, and
 *     tests/test_streams.py holds each to them: off the default stream, and from
 *     a replayed graph whose inputs were rewritten.
 *   - Return value: WG_OK (0) or a negative WG_ERR_* code; the message of the
 *     last failure on the calling host thread is wg_last_error().  No entry
 *     point aborts the process.
 *   - A wg_laplacian_t is not thread-safe: one host thread per handle.
 *     Multi-GPU = one process per GPU, one handle per process (row shard).
 */
#ifndef WATS_HIP_H
#define WATS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WG_ABI_VERSION 1

enum wg_status {
  WG_OK = 0,
  WG_ERR_INVALID = -1,   /* bad argument (shape, null pointer, range) */
  WG_ERR_HIP = -2,       /* a HIP runtime call failed */
  WG_ERR_OOM = -3,       /* device allocation failed */
  WG_ERR_UNSUPPORTED = -4,
  WG_ERR_TIMEOUT = -5    /* an in-kernel wait gave up (the one-launch chain): that launch's outputs are NaN */
};

/* creation flags */
#define WG_FLAG_NONE 0u
#define WG_FLAG_NO_REORDER 1u   /* keep the caller's row order (no degree relabelling) */
#define WG_FLAG_TRANSPOSE 2u    /* wg_rownorm_create: build adj_norm^T instead of adj_norm */
#define WG_FLAG_KEEP_COLUMN_ORDER 4u /* keep each row's input entry order (default: ascending
                                        internal column, which shares cache lines between
                                        neighbouring gathers on power-law graphs) */
#define WG_FLAG_CALLER_TIES 8u  /* wg_laplacian_create: rows of equal length keep the caller's
                                   order (default on a whole graph: by their hottest and
                                   second-hottest neighbour, then caller order, so rows that
                                   gather the same hub rows share waves and cache lines) */

typedef struct wg_laplacian_s* wg_laplacian_t;

typedef struct wg_laplacian_info {
  int64_t n_rows;        /* rows owned by this handle (all N on one GPU) */
  int64_t n_cols;        /* column space = n_rows + halo rows (== n_rows on one GPU) */
  int64_t nnz_input;     /* stored entries of the input adjacency rows */
  int64_t nnz;           /* off-diagonal entries of L_hat (self loops removed) */
  int64_t n_isolated;    /* rows with w_i == 0 (L_hat_ii = -1) */
  int64_t max_row_nnz;   /* longest L_hat row */
  int32_t n_segments;    /* row-length bins of the step kernel */
  int32_t reordered;     /* 1 if rows are relabelled by descending degree */
  int64_t n_closed_form; /* purely isolated rows (w_i = 0, empty row and column):
                            T_k = (-1)^k X0 exactly, kept out of the step kernel
                            by wg_wavelet_features */
} wg_laplacian_info;

/* -------------------------------------------------------------------------
 * Library
 * ---------------------------------------------------------------------- */
const char* wg_last_error(void);
int wg_abi_version(void);

/* -------------------------------------------------------------------------
 * a8 / section 8(f)-1: dense adjacency ingestion.
 * Replaces `csr_matrix(adj.cpu().numpy())` (calibration/WATS.py:99) with an
 * on-device compaction.  Two calls: count (writes indptr[n+1], returns nnz in
 * *nnz_host; synchronous), then fill (indices/values sized nnz; async).
 * Entries != 0.0f are kept, in column order, exactly like scipy.
 * ---------------------------------------------------------------------- */
int wg_dense_to_csr_count(const float* adj, int64_t n_rows, int64_t n_cols, int64_t ld,
                          int64_t* indptr, int64_t* nnz_host, void* stream);
int wg_dense_to_csr_fill(const float* adj, int64_t n_rows, int64_t n_cols, int64_t ld,
                         const int64_t* indptr, int32_t* indices, float* values, void* stream);

/* -------------------------------------------------------------------------
 * Degree helpers (used for row shards, where the Laplacian's column degree
 * w_j = colsum_j(A) - A_jj spans every shard and is summed across ranks).
 * wg_column_degree ACCUMULATES (+=) this shard's column sums into
 * colsum_f64[n_cols_global] and its diagonal into diag_f64 (indexed by the
 * global column id `row_offset + i` of local row i).  Column ids are global.
 * scipy semantics: `_laplacian.py:467` (w = m.sum(axis=0) - m.diagonal()).
 * Asynchronous, allocates nothing, may be captured (float64 atomic adds: the
 * order of a column's sum is not fixed).
 * ---------------------------------------------------------------------- */
int wg_column_degree(int64_t n_rows, int64_t row_offset, const int64_t* indptr,
                     const int32_t* indices, const float* values /* NULL = 1 */,
                     double* colsum_f64, double* diag_f64, void* stream);

/* -------------------------------------------------------------------------
 * a1 + a2: compute_normalized_laplacian + rescale.
 * Replaces `csgraph.laplacian(adj, normed=True)` (calibration/WATS.py:24-27,
 * scipy _laplacian.py:467-475) followed by `(2/2.0)*L - identity(N)`
 * (calibration/WATS.py:55).  Builds on the device:
 *     L_hat_ij = -((a_ij / sqrt(w_i)) / sqrt(w_j))   (float32, scipy op order)
 *     for i != j, with w = column sums minus diagonal and sqrt(w)=1 where w==0;
 *     L_hat_ii = -1 for isolated rows (w_i == 0), 0 (dropped) otherwise.
 * Inputs: CSR rows of A (int64 indptr[n_rows+1], int32 indices, float32
 * values or NULL for an unweighted graph); column ids in [0, n_cols) where
 * column i (< n_rows) is local row i (i.e. owned rows first, then halo rows).
 * w_cols (float32[n_cols], nullable): precomputed column degree
 * (colsum - diag) per column id; NULL = compute from this CSR (single GPU).
 * Synchronous.  The handle owns its device copy of L_hat and workspaces.
 * ---------------------------------------------------------------------- */
int wg_laplacian_create(int64_t n_rows, int64_t n_cols, int64_t nnz,
                        const int64_t* indptr, const int32_t* indices, const float* values,
                        const float* w_cols, uint32_t flags, void* stream,
                        wg_laplacian_t* out);
int wg_laplacian_destroy(wg_laplacian_t L);
int wg_laplacian_get_info(wg_laplacian_t L, wg_laplacian_info* info_host);

/* Export L_hat in the CALLER's row/column numbering: the off-diagonal
 * entries as CSR (int64 indptr[n_rows+1], int32 indices / float32 values
 * sized info.nnz; each row in ascending column order, or in the input's
 * order under WG_FLAG_KEEP_COLUMN_ORDER) plus iso[n_rows] (1 where
 * L_hat_ii = -1; nullable).  For bit-exact parity tests against scipy.
 * Synchronous: temporary memory (the scan's scratch and, for a handle whose
 * rows are sorted by internal column, two arrays of info.nnz entries) is
 * allocated and freed inside the call, the work runs on `stream`, which is
 * waited for before the temporaries are freed. */
int wg_laplacian_export(wg_laplacian_t L, int64_t* indptr, int32_t* indices,
                        float* values, uint8_t* iso, void* stream);

/* A literal CSR operator for chebyshev_polynomials(L, k, X0)
 * (calibration/WATS.py:29-37) called with an explicit matrix -- the reference
 * passes `L_rescaled = (2/2.0)*L - identity(N)`, a float64 scipy CSR
 * (WATS.py:55,62).  Every stored entry is kept with its value (float32),
 * diagonal entries included; nothing is normalised and no row is isolated.
 * Square n x n; the handle is a wg_laplacian_t of the same step kernel
 * (wg_cheb_step / wg_permute_rows; freed by wg_laplacian_destroy).
 * Synchronous. */
int wg_operator_create(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                       const float* values, uint32_t flags, void* stream, wg_laplacian_t* out);

/* -------------------------------------------------------------------------
 * a3: input signal.  Replaces `X0 = log1p(adj.sum(axis=1))`
 * (calibration/WATS.py:58-59): row sums INCLUDING self loops, float32 (N,1),
 * in the caller's row order.  One launch on `stream`, no allocation, no wait.
 * Its only input is the handle, so a captured call has nothing a replay
 * could follow: no capture test holds it (tests/stream_cases.py,
 * ASYNC_REASONS) and no promise is made.
 * ---------------------------------------------------------------------- */
int wg_log1p_degree(wg_laplacian_t L, float* x0, void* stream);

/* -------------------------------------------------------------------------
 * a4 (+a5): one Chebyshev step of `chebyshev_polynomials`
 * (calibration/WATS.py:29-37), in the handle's INTERNAL row order (see
 * wg_permute_rows).  k == 1:  T_1 = L_hat T_0;  k >= 2:  T_k = 2 L_hat T_{k-1}
 * - T_{k-2}.  t_km1 has n_cols rows (owned + halo), t_km2 / t_k n_rows rows,
 * all with row stride F.  t_k may alias t_km2 (in-place).  If S != NULL the
 * heat-kernel sum of calibration/WATS.py:65-68 is fused:
 *   k == 1:  S = alpha0 * T_0 + alpha_k * T_1;    k >= 2:  S += alpha_k * T_k.
 * If H != NULL (last step) the row-L1 normalisation of WATS.py:71-72 is fused:
 *   H = S / (sum_f |S| + 1e-8) of the float32 S this call stores (as wg_row_l1_normalize of it, and as
 *   every H that wg_wavelet_features returns): a float64 quotient rounded once.  Row sums accumulate in float64.
 * ---------------------------------------------------------------------- */
int wg_cheb_step(wg_laplacian_t L, int32_t k, int64_t F, const float* t_km1,
                 const float* t_km2, float* t_k, float* S, float* H,
                 double alpha0, double alpha_k, void* stream);

/* F == 1 on an unweighted graph: the column-blocked LDS step kernel
 * (csrc/lds1.hip) gathers u_{k-1} = T_{k-1} * dinv instead of T_{k-1}
 * (dinv_j = 1 / sqrt(w_j), w_j = 0 -> 1), so a row-sharded caller exchanges
 * halo rows of u.  Same recurrence as wg_cheb_step (calibration/WATS.py:32-36,
 * heat sum WATS.py:65-68), internal row order.
 * wg_cheb_u_len: *len = floats a u buffer must hold (n_cols rounded up to whole
 *   column blocks; entries past n_cols are never used), or 0 when this kernel
 *   does not apply (weighted graph, too many column blocks, "lds" tuned off).
 *   Builds the plan (synchronous, once).
 * wg_scale_dinv: u[i] = x[i] * dinv[i] for the handle's own rows i < n_rows.
 * wg_cheb_step_u: u_km1 has wg_cheb_u_len floats (own rows then halo rows,
 *   as t_km1 of wg_cheb_step); t_km1 / t_km2 / t_k are own rows only; u_k
 *   (nullable) receives u_k for the own rows.  WG_ERR_UNSUPPORTED when
 *   wg_cheb_u_len is 0. */
int wg_cheb_u_len(wg_laplacian_t L, int64_t* len_host);
/* Shape of the LDS kernel's plan (for byte accounting), or all zeros when it
 * does not apply: out[0] mode (1 row teams, 2 chunk windows), [1] column
 * blocks, [2] rows, [3] columns, [4] nonzeros, [5] non-empty (row, block)
 * segments, [6] 16-B chunks (padded ids), [7] workgroups.  active_only = 1:
 * the plan wg_wavelet_features uses (rows that enter the chain). */
int wg_lds_plan_info(wg_laplacian_t L, int32_t active_only, int64_t* out8_host);
int wg_scale_dinv(wg_laplacian_t L, const float* x, float* u, void* stream);
int wg_cheb_step_u(wg_laplacian_t L, int32_t k, const float* u_km1, const float* t_km1,
                   const float* t_km2, float* t_k, float* u_k, float* S, double alpha0,
                   double alpha_k, void* stream);

/* One step of the heat sum by Clenshaw's recurrence (WATS.py:32-36 with the
 * sum of :65-68), the step wg_wavelet_features (F > 1) and the row-sharded
 * chain run, on internal rows:
 *   out = ck * x0 + cacc * (L_hat b1) - b2        (b2 NULL = 0)
 * flags: WG_CLEN_UIN  b1 holds u = b * dinv (unweighted handles: the gathers
 *                     read no values; own + halo rows, like t_km1 of wg_cheb_step)
 *        WG_CLEN_UPREV b2 holds u;  WG_CLEN_UOUT out receives u (not with FINAL)
 *        WG_CLEN_FINAL out is the finished sum S
 *        WG_CLEN_ACTIVE only the rows that enter wg_wavelet_features' chain.
 * With WG_CLEN_UIN on a large unweighted graph and F a multiple of 16 (<= 64)
 * this is the hybrid step (dense blocks on the matrix cores). */
#define WG_CLEN_UIN 1
#define WG_CLEN_UPREV 2
#define WG_CLEN_UOUT 4
#define WG_CLEN_FINAL 8
#define WG_CLEN_ACTIVE 16
int wg_clenshaw_step(wg_laplacian_t L, int64_t F, const float* b1, const float* b2, const float* x0,
                     float* out, double ck, double cacc, int32_t flags, void* stream);

/* Row permutation between the caller's order and the internal order:
 * direction 0: dst[i_internal] = src[perm[i]]  (caller -> internal)
 * direction 1: dst[perm[i]] = src[i_internal]  (internal -> caller).
 * Asynchronous, allocates nothing, may be captured. */
int wg_permute_rows(wg_laplacian_t L, int32_t direction, int64_t F, const float* src,
                    float* dst, void* stream);

/* -------------------------------------------------------------------------
 * a7: graph_wavelet_features (calibration/WATS.py:39-74), fused:
 *   T_0 = X0 (N,F) -> K Chebyshev steps -> S = sum_k exp(-s k) T_k ->
 *   H = S / (||S||_1,row + 1e-8).
 * F > 1 or weighted: the sum is evaluated by Clenshaw's recurrence (K SpMM
 * steps, no S stream; tuning key "clenshaw" 0 = forward recurrence).
 * X0, S, H in the caller's row order, row stride F.  S and H nullable (at
 * least one non-NULL).  K >= 0.  Uses the handle's workspace.
 * The FIRST call with a given F (after creation or a wg_laplacian_tune) builds
 * the kernel plans and grows the workspace SYNCHRONOUSLY (host copies, device
 * allocation): on a stream that is being captured it returns
 * WG_ERR_UNSUPPORTED -- call it once uncaptured first; later calls are plain
 * asynchronous launches and may be captured.
 * A chain can be replayed as a hipGraph of the handle's own once the same
 * arguments (pointers, F, K, s) were seen on two calls in a row
 * (tuning key "graph": 0 off = default, the replay measured slower than eager
 * launches on ROCm 7.2; 1 on; -1 only when active nnz x width <= 2^22).
 * ---------------------------------------------------------------------- */
int wg_wavelet_features(wg_laplacian_t L, const float* X0, int64_t F, int32_t K, double s,
                        float* S, float* H, void* stream);
/* F == 1 on a small unweighted graph (<= 2^18 nonzeros, <= 24576 active rows;
 * tuning key "chain": -1 auto, 0 off, 1 on, "chain_wg" workers) with S and H
 * given, wg_wavelet_features runs the whole chain in ONE launch of P
 * cooperating workgroups that hand each step's vector over as tagged granules
 * (csrc/chain.hip).  A wait gives up after 0.5 s instead of
 * hanging; that launch then writes NaN for every S / H row that depends on the
 * missing data and records the failure in host-mapped memory, and the NEXT
 * wg_wavelet_features call on the handle returns WG_ERR_TIMEOUT without
 * launching.  wg_chain_status waits for the handle's last one-launch chain
 * (an event recorded after it, also after a replay of the handle's own
 * captured chain; no device-wide sync -- except after a chain captured into a
 * graph the CALLER replays, which records no event of the handle's, where it
 * synchronises the device) and reports a failure since the last report
 * in *timed_out_host (1 = a chain's results are invalid; tuning key
 * "chain_fault" = j injects one: worker 0 skips publishing phase j).  Either
 * report switches the handle to the multi-launch path (until the next tune)
 * and drops a chain the handle captured with the one-launch kernel, so calling
 * again recomputes the features there (the Python
 * graph_wavelet_features does so by itself).  The plan never asks for more
 * workers than the occupancy query lets be resident (one per CU at most);
 * when the graph would need more, the multi-launch path runs. */
int wg_chain_status(wg_laplacian_t L, int32_t* timed_out_host);

/* Tuning: key "iter" (team-mode nonzeros per lane sub-group; default by
 * shape), "chunk_iter" (chunk-mode nonzeros per sub-group),
 * "clenshaw" (wavelet_features' heat sum, default 1), "tiles" (the hybrid
 * step, DESIGN.md 4.6: -1 auto, 0 off, 1 whenever it applies; with "tile_th",
 * "tile_rows", "tile_max", "tile_rg", "tile_mfma"), "nt" (store hints), and the keys listed in
 * efficient-gnn_amd/csrc/internal.h (struct Tuning).  Plan-shaping keys are
 * synchronous (they drop cached plans); launch-time keys are not.  Timing
 * probes whose results are wrong on purpose ("seg_mask", "probe",
 * "probe_tailwin", "xdelay") exist only in a build
 * with -DWG_TIMING_PROBES; this library rejects them as unknown keys. */
int wg_laplacian_tune(wg_laplacian_t L, const char* key, int64_t value);
/* Row shards: the halo columns [n_rows + offsets[q], n_rows + offsets[q+1])
 * come from peer q (q < n_groups; offsets[0] = 0, offsets[n_groups] = halo
 * size), each group in descending degree.  Lets the F = 1 hub kernel stage
 * the top columns of the own range and of every group in LDS.
 * wg_dist_create sets it from the receive counts; synchronous; drops the F = 1
 * plans built so far.  n_groups = 0 clears it. */
int wg_laplacian_set_halo_groups(wg_laplacian_t L, int32_t n_groups, const int64_t* offsets_host);
/* Human-readable launch plan of the step kernel for an F-column signal
 * (thread-local string, valid until the next call on this thread). */
const char* wg_laplacian_describe(wg_laplacian_t L, int64_t F);

/* Live kernel timing for benchmarks: while enabled, wg_wavelet_features
 * records a HIP event pair on `stream` around every Chebyshev-step launch.
 * wg_profile_collect waits for the recorded events (synchronous), returns
 * the summed step-kernel time (ms), the number of step launches and the
 * longest one since the last collect, and resets the pool. */
int wg_profile_enable(wg_laplacian_t L, int32_t enable);
int wg_profile_collect(wg_laplacian_t L, double* sum_ms_host, int64_t* launches_host,
                       double* max_ms_host);
/* The same events, one duration per launch in launch order (ms_host[i], i < min(cap, *n_host);
 * *n_host = launches recorded): e.g. a folded chain's first launch apart from its K - 1 plain step
 * launches.  Synchronous; resets the record like wg_profile_collect. */
int wg_profile_durations(wg_laplacian_t L, double* ms_host, int64_t cap, int64_t* n_host);

/* a6 standalone: H = S / (||S||_1,row + 1e-8) (calibration/WATS.py:71-72).
 * Asynchronous, allocates nothing, may be captured. */
int wg_row_l1_normalize(const float* S, float* H, int64_t n_rows, int64_t F, void* stream);

/* Row-id mapping between the caller's numbering and the internal one:
 * direction 0: out[i] = internal id of caller row rows[i]; 1: the inverse.
 * Asynchronous, allocates nothing, may be captured. */
int wg_laplacian_map_rows(wg_laplacian_t L, int32_t direction, const int32_t* rows, int64_t n,
                          int32_t* out, void* stream);

/* Multi-GPU halo pack: dst[i] = src[rows[i]] for i < n (row stride F).
 * Asynchronous, allocates nothing, may be captured. */
int wg_gather_rows(const float* src, const int32_t* rows, int64_t n, int64_t F, float* dst,
                   void* stream);

/* -------------------------------------------------------------------------
 * Section 8(e): the row-sharded chain with its halo exchange in native code.
 * One process per GPU.  `L` is this rank's shard (n_rows own rows; columns
 * [own | halo], the halo grouped by owner rank, as wats_hip/dist.py plans
 * it).  Per Chebyshev step (reference calibration/WATS.py:35-36) the own rows
 * peers asked for are packed (send_rows: internal ids, grouped by peer,
 * send_counts[q] for peer q) and exchanged with grouped ncclSend / ncclRecv
 * (RCCL over xGMI) into the halo rows (recv_counts[q] from peer q), then the
 * step kernel runs.  The chain is captured into a hipGraph on its second call
 * with the same arguments and replayed from then on (wg_dist_set_graph(D, 0)
 * keeps it eager; profiling via wg_profile_enable(L) also runs eagerly).
 * Each step exchanges, then computes (the overlap variants measured in round
 * 2 -- two-phase steps, two halo tiers, streamed row blocks -- were slower
 * and are removed).
 * wg_dist_unique_id fills NCCL_UNIQUE_ID_BYTES (128) bytes on one rank; every
 * rank passes the same bytes to wg_dist_create (collective: blocks until all
 * ranks joined); unique_id NULL = no RCCL communicator (IPC exchange below).  X0, S, H: own rows (n_rows, F) in the caller's order.
 * ---------------------------------------------------------------------- */
typedef struct wg_dist_s* wg_dist_t;
int wg_dist_unique_id(void* id_out /* 128 bytes, host */);
int wg_dist_create(wg_laplacian_t L, const void* unique_id, int32_t rank, int32_t world,
                   const int32_t* send_rows, const int64_t* send_counts_host,
                   const int64_t* recv_counts_host, wg_dist_t* out);
int wg_dist_destroy(wg_dist_t D);
int wg_dist_set_graph(wg_dist_t D, int32_t enable);
int wg_dist_wavelet_features(wg_dist_t D, const float* X0, int64_t F, int32_t K, double s, float* S,
                             float* H, void* stream);
/* State of the sharded chain, out8_host: [0] 0 (exchange, then the step),
 * [1] own rows, [2] halo rows, [3] rows sent, [4] world, [5] exchange (1 IPC,
 * 2 RCCL, 0 none), [6] 1 if a captured hipGraph exists, [7] 1 (halo tiers). */
int wg_dist_info(wg_dist_t D, int64_t* out8_host);
/* Total time (ms) and count of the halo exchanges (pack + RCCL, or the IPC
 * pull) recorded while profiling was enabled on the shard's handle; resets. */
int wg_dist_profile_collect(wg_dist_t D, double* exchange_ms_host, int64_t* count_host);

/* One-sided exchange over IPC-mapped peer memory, instead of RCCL (create
 * with unique_id = NULL).  wg_dist_ipc_local allocates this rank's shared
 * region (two slots of the extended vector at up to F_max columns, or of the
 * F = 1 LDS kernel's u, plus `world` int64 phase flags) and writes a 128-byte
 * blob (IPC handle + layout); every rank gathers all blobs (rank order) and
 * calls wg_dist_ipc_connect, with halo_src[h] = the owner's internal row id
 * of halo row h (device int32, n_halo entries).  Per phase a rank waits until
 * every peer completed as many phases as itself (flags written by the peers
 * with system-scope stores), pulls its halo rows with system-scope loads
 * from the owners' slots, runs the step and signals its peers.  A wait gives
 * up after 60 s and sets a flag that wg_dist_status reports (it synchronises
 * the device). */
int wg_dist_ipc_local(wg_dist_t D, int64_t F_max, void* blob_out /* 128 bytes, host */);
int wg_dist_ipc_connect(wg_dist_t D, const void* blobs_host /* world x 128 bytes */,
                        const int32_t* halo_src);
/* Exchange mode "sdma" (after wg_dist_ipc_connect): every phase the owner packs the rows each
 * peer asked for into one of two send buffers in its IPC region (in the peer's halo order) and
 * signals the phase; the receiver waits for the signals on a copy stream and copies each
 * owner's block into its halo rows with hipMemcpyAsync (peer DMA: the transfer takes no CU time
 * on a multi-GPU node), the step waiting on the copies.  peer_send_off[q] = the row of rank q's
 * send buffer where q packed this rank's block (q's send offset for this rank; collective setup,
 * wats_hip.dist).  Replaces the pull exchange of the same handle.
 * (reference: the halo exchange of the row-sharded Chebyshev step, WATS.py:35-36 sharded per
 * SURVEY.md 8(e); no reference interface -- the reference has no multi-GPU path) */
int wg_dist_ipc_sdma(wg_dist_t D, const int64_t* peer_send_off /* world, host */);
int wg_dist_status(wg_dist_t D, int32_t* timed_out_host);

/* -------------------------------------------------------------------------
 * Section 8(f)-2: the base model's propagation.  CompatibleGCN.forward
 * (reference src/gnn/model.py:43-52) computes deg = adj.sum(dim=1),
 * deg[deg == 0] = 1, adj_norm = adj / deg and twice x -> adj_norm @ x with a
 * dense (N,N) torch.mm.  wg_rownorm_create builds adj_norm (every stored
 * entry, self loops included, value a_ij / deg_i in float32) from the CSR
 * rows of adj (square, n x n; values NULL = all ones) as a handle of the same
 * step kernel; WG_FLAG_TRANSPOSE builds adj_norm^T (the backward operator).
 * wg_spmm: y = op @ x for x, y (n, F) row-major in the caller's order, sums in
 * float64.  Handles are freed with wg_laplacian_destroy.  Create is synchronous.
 * wg_spmm: the FIRST call with a given F on a handle built without
 * WG_FLAG_NO_REORDER builds the plan and grows the handle's workspace
 * synchronously (a stream sync, a device allocation); later calls at that width
 * or a narrower one are asynchronous, allocate nothing and may be captured.
 * ---------------------------------------------------------------------- */
int wg_rownorm_create(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                      const float* values, uint32_t flags, void* stream, wg_laplacian_t* out);
int wg_spmm(wg_laplacian_t op, int64_t F, const float* x, float* y, void* stream);

/* -------------------------------------------------------------------------
 * Edge-position gradients of that propagation.  The reference attacks take
 * grad = d loss / d adj through the dense CompatibleGCN.forward (reference
 * src/gnn/model.py:43-52) and read row t and column t of it
 * (calib_attack/calib_fga.py:864-881).  For y = adj_norm(A) @ x with upstream
 * gradient g = d loss / d y and deg as above (0 -> 1),
 *     d loss / d a_ij = ( g_i . x_j  -  g_i . y_i ) / deg_i
 * at every (i, j), stored or not: a sampled dense-dense product at a list of
 * positions plus a per-row term,
 *     wg_sddmm(rows, cols, g, x, row_term = wg_rowdot(g, y), row_scale = 1 / deg).
 * wg_sddmm:
 *   out[p] = row_scale[r] * ( sum_f A[r,f]*B[c,f]  -  row_term[r] ),  r = rows[p], c = cols[p]
 *   row_term / row_scale nullable (0 / 1).  A is (n_a, F), B is (n_b, F), row-major, stride F;
 *   0 <= rows[p] < n_a, 0 <= cols[p] < n_b (checked on the device in the bounds-checked variant only).
 * wg_rowdot:
 *   out[i] = sum_f A[i,f]*B[i,f]   (the row term g_i . y_i)
 * Products and sums in float64 in a fixed order, no atomics: bitwise
 * reproducible.  Asynchronous, no allocation, may be captured.  n_pairs == 0
 * (n == 0) is WG_OK with no launch.
 * ---------------------------------------------------------------------- */
int wg_sddmm(int64_t n_pairs, const int32_t* rows, const int32_t* cols, int64_t F,
             const float* A, int64_t n_a, const float* B, int64_t n_b,
             const float* row_term, const float* row_scale, float* out, void* stream);
int wg_rowdot(int64_t n, int64_t F, const float* A, const float* B, float* out, void* stream);

/* -------------------------------------------------------------------------
 * Edge-flip views of that propagation.  One attack iteration flips an edge of
 * the dense adjacency -- v = 1 - 2 adj[r,c]; adj[r,c] += v; adj[c,r] += v -- and
 * evaluates the model on the flipped graph (calib_attack/calib_fga.py:901-913).
 * The flipped matrix A' differs from A in a few rows, so a view keeps A's
 * operators and an overlay: n_pos positions sorted by (row, column), grouped by
 * touched row -- t_rows [n_touched] ascending, seg [n_touched + 1] with
 * positions [seg[i], seg[i+1]) in row t_rows[i] (none empty), cols [n_pos] --
 * each with a_old (A's entry, 0 if absent), a_new (A''s entry) and base_pos
 * (its index in A's indices, or -1).  A is a canonical CSR: indptr int64
 * [n + 1], indices int32 ascending in each row, values float32 or NULL (ones).
 * wg_flip_resolve: a_old and base_pos of every position (binary search in the
 *   row) and row_sum [n_touched], the float64 sum of each touched row's values
 *   (its length when values is NULL), lanes striding the row, then a fixed
 *   shuffle tree.
 * wg_flip_rows (forward): overwrites the touched rows of y = adj_norm(A) @ x
 *   (wg_spmm of A's handle) with those of adj_norm(A') @ x:
 *     y[r,:] = sum over the entries a'_rc != 0 of row r of float32(a'_rc / deg_new[i]) * x[c,:]
 *   in float64, deg_new [n_touched] the new degrees (0 -> 1).  A row without
 *   entries gives exactly 0.
 * wg_flip_cols (backward): the overlay by column -- c_cols [n_cols] distinct,
 *   cseg [n_cols + 1], and per position in (column, row) order its row, a_new,
 *   a_old and the row's new degree deg_new [n_pos].  After wg_spmm of A's
 *   transposed handle on g with each touched row scaled by deg / deg',
 *     gx[c,:] = float32(gx[c,:] + sum_p ((a_new - a_old) / deg_new) * g[rows[p],:])
 *   in float64 in ascending row order (a removed entry cancels to rounding).
 * wg_csr_patch (commit): the canonical CSR of A' -- columns ascending, no
 *   stored zero -- from A's CSR and the overlay: new row lengths, one exclusive
 *   scan, one copy pass; no row is sorted again.  out_indices / out_values hold
 *   `capacity` >= nnz + n_pos entries, out_indptr n + 1.  Synchronous: one
 *   temporary allocation, freed inside the call; one stream sync returns the
 *   new nnz.  WG_ERR_UNSUPPORTED when n or nnz + n_pos exceeds int32.
 * Ids are trusted (checked on the device in the bounds-checked variant only);
 * every other argument is checked before any device work.  x, y, g, gx are
 * (n, F) row-major.  Float64 sums in a fixed order, no float atomics: bitwise
 * reproducible.  n_pos == 0 is WG_OK with no launch (wg_csr_patch: a copy).
 * The first three are asynchronous, allocate nothing and may be captured.
 * ---------------------------------------------------------------------- */
int wg_flip_resolve(int64_t n, const int64_t* indptr, const int32_t* indices, const float* values,
                    int64_t n_touched, const int32_t* t_rows, const int64_t* seg, int64_t n_pos,
                    const int32_t* cols, float* a_old, int64_t* base_pos, double* row_sum,
                    void* stream);
int wg_flip_rows(int64_t n, const int64_t* indptr, const int32_t* indices, const float* values,
                 int64_t n_touched, const int32_t* t_rows, const int64_t* seg, int64_t n_pos,
                 const int32_t* cols, const float* a_new, const int64_t* base_pos,
                 const float* deg_new, int64_t F, const float* x, float* y, void* stream);
int wg_flip_cols(int64_t n, int64_t n_cols, const int32_t* c_cols, const int64_t* cseg,
                 int64_t n_pos, const int32_t* rows, const float* a_new, const float* a_old,
                 const float* deg_new, int64_t F, const float* g, float* gx, void* stream);
int wg_csr_patch(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                 const float* values, int64_t n_touched, const int32_t* t_rows, const int64_t* seg,
                 int64_t n_pos, const int32_t* cols, const float* a_new, const int64_t* base_pos,
                 int64_t* out_indptr, int32_t* out_indices, float* out_values, int64_t capacity,
                 int64_t* nnz_host, void* stream);

/* -------------------------------------------------------------------------
 * Section 8(f) rank 1, second half: graph ingestion from an edge list.  The
 * reference turns edge_index into a dense (N,N) adjacency --
 *   adj[src, dst] = 1                               (calibration/utils.py:19-25 via
 *                                                    benchmark_calibration_methods.py:53)
 *   adj = clamp(adj + adj.t(), 0, 1); adj.fill_diagonal_(1.0)
 *                                                   (ugca_calib_attack.py:42-47,
 *                                                    exp/ablation/ugca_full_multi_dataset.py:135-140)
 * -- and gives the adjacency up above 50 000 nodes (ugca_full_multi_dataset.py:128-133).
 * wg_coo_to_csr builds the canonical CSR of that matrix from the ids directly.
 * With A0 the duplicates' result, A1 the symmetrised and A2 the final matrix:
 *   duplicates  default: A0[i,j] = 1 if any edge (i,j) is present;
 *               WG_COO_SUM: A0[i,j] = sum of weights (NULL = 1) over the edges (i,j)
 *   WG_COO_SYMMETRIC     default mode: A1 = max(A0, A0^T); WG_COO_SUM: A1 = A0 + A0^T
 *                        (the diagonal doubles, as adj + adj.t() does)
 *   WG_COO_LOOPS_REMOVE  the diagonal becomes 0;  WG_COO_LOOPS_ONE: it becomes 1 on every row
 * Output: the entries of A2 that are != 0 -- indptr int64 [n + 1], indices int32
 * ascending in each row without duplicates, values float32 (may be NULL without
 * WG_COO_SUM: every value is 1).  WG_COO_SUM sums are float64, the forward
 * contributions in input order, then the mirrored ones in input order, rounded
 * once to float32; no float atomics: the same input gives the same bits.
 * src / dst: n_edges ids of id_bytes (4 | 8) each, on the device.  An id outside
 * [0, n) is WG_ERR_INVALID with the count in the message (the outputs are then
 * unspecified; no bad id is ever used as an index).  indices / values hold
 * `capacity` >= wg_coo_capacity entries (host only, no device work:
 * n_edges * (2 if symmetric) + (n if WG_COO_LOOPS_ONE); WG_ERR_UNSUPPORTED when
 * that or n exceeds int32).  Every argument is checked before any device call.
 * Synchronous: temporary memory is allocated and freed inside the call, the work
 * runs on `stream`, one stream sync returns nnz and the bad-id count.
 * ---------------------------------------------------------------------- */
#define WG_COO_SYMMETRIC 1u
#define WG_COO_SUM 2u            /* default: presence ("one") */
#define WG_COO_LOOPS_REMOVE 4u
#define WG_COO_LOOPS_ONE 8u      /* both loop flags: WG_ERR_INVALID */
int wg_coo_capacity(int64_t n, int64_t n_edges, uint32_t flags, int64_t* capacity_host);
int wg_coo_to_csr(int64_t n, int64_t n_edges, const void* src, const void* dst,
                  int32_t id_bytes /* 4 | 8 */,
                  const float* weights /* NULL = 1; must be NULL without WG_COO_SUM */,
                  uint32_t flags, int64_t* indptr, int32_t* indices,
                  float* values /* may be NULL without WG_COO_SUM */, int64_t capacity,
                  int64_t* nnz_host, void* stream);

/* -------------------------------------------------------------------------
 * Section 8(f)-3: the WATS temperature head, fused.  Reference
 * calibration/WATS.py:101-105 (net = Linear(F,16) - ReLU - Linear(16,1)) and
 * :124-130 (T = log(exp(net(H)) + 1.1); out = log_softmax(logits / T)).
 * H (n,F), logits (n,C), out (n,C) row-major; W1 [hid][F], b1 [hid], W2 [hid]
 * (Linear(hid,1).weight), b2 [1] (torch nn.Linear layout); hid <= 64.
 * forward: out, and t_save[n] = net(H) (nullable; speeds up the backward).
 * backward: from grad_out (n,C): grad_logits (nullable) and the parameter
 * gradients gW1 [hid][F], gb1, gW2, gb2 (overwritten, not accumulated), float64
 * sums in a fixed order; `workspace` holds wg_wats_head_workspace bytes.
 * Forward and backward are asynchronous, allocate nothing, zero the workspace
 * they accumulate into and may be captured.
 * ---------------------------------------------------------------------- */
int wg_wats_head_forward(int64_t n, int64_t F, int64_t C, int32_t hid, const float* H,
                         const float* logits, const float* W1, const float* b1, const float* W2,
                         const float* b2, float* out, float* t_save, void* stream);
int wg_wats_head_workspace(int64_t n, int64_t F, int32_t hid, int64_t* bytes_host);
int wg_wats_head_backward(int64_t n, int64_t F, int64_t C, int32_t hid, const float* H,
                          const float* logits, const float* W1, const float* b1, const float* W2,
                          const float* b2, const float* out, const float* t_save,
                          const float* grad_out, float* grad_logits, float* gW1, float* gb1,
                          float* gW2, float* gb2, void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * Section 8(f): the attention layer of the GATS calibrator (reference
 * calibration/GATS.py), the calibrator the harness runs next to WATS
 * (benchmark_calibration_methods.py:317-354).
 *
 * wg_csr_transpose_map: the transposed structure of a canonical CSR (square,
 * n x n, columns ascending in each row): t_indptr int64 [n + 1], t_indices int32
 * [nnz] ascending in each row, and t_pos int32 [nnz], the position in `indices`
 * of the entry that transposed entry e' mirrors.  The layer aggregates over the
 * targets of edge_index = dense_to_sparse(adj) (GATS.py:199, :134-139: row i of
 * the by-destination CSR is column i of adj), and its backward also runs over
 * the sources.  nnz == indptr[n].  Synchronous, temporary memory inside the call.
 *
 * wg_bfs_levels: shortest_path_length (GATS.py:25-49) on the device.  indptr /
 * indices list each node's out-neighbours (the targets of its edges); mask is
 * uint8 [n]; dist int64 [n] gets the level of every node reached at a level in
 * [0, max_hop) and INT64_MAX elsewhere: as in the reference only levels
 * 0 .. max_hop - 1 are ever assigned (bfs_depth = 2: the values are 0, 1 and the
 * maximum), and max_hop == 0 assigns none.  Self loops never change a level.
 * One launch per level; integer stores only, every writer of a cell writes the
 * same value.  Asynchronous, no allocation, may be captured.
 *
 * wg_gat_forward: CalibAttentionLayer.message / aggregation (GATS.py:134-167).
 * indptr / indices: the CSR by destination -- row i lists In(i), the sources j of
 * the edges j -> i, with the self loop of GATS.py:102-106 already in it.  With
 * a (n, C), t (n, Hh), conf (n), row-major float32:
 *   d_ij = sum_c a_i[c] a_j[c];   e_ij = d_ij > 0 ? d_ij : negative_slope * d_ij
 *   p_ij = exp(e_ij - max_l e_il) / sum_l exp(e_il - max_l e_il)     over l in In(i)
 *   sim[i, h] = sum_j p_ij t[j, h];   dconf[i] = sum_j (conf[i] - conf[j])
 * (a row without entries gives 0).  e_save [nnz], row_max [n], row_den [n]
 * (float64: e_ij, the row's maximum and its denominator) are what the backward
 * needs; all three NULL for inference.
 *
 * wg_gat_backward: from g_sim = d loss / d sim (n, Hh), with q_ij = g_i . t_j,
 * m_i = sum_j p_ij q_ij, r_ij = p_ij (q_ij - m_i), s_ij = r_ij * (d_ij > 0 ? 1 :
 * negative_slope) (the slope at d_ij == 0, as torch's leaky_relu backward):
 *   grad_t[j, h] = sum_{i : j in In(i)} p_ij g_sim[i, h]
 *   grad_a[i, c] = sum_{j in In(i)} s_ij a[j, c] + sum_{l : i in In(l)} s_li a[l, c]
 * overwritten, not accumulated; dconf carries no gradient.  edge_work: 2 nnz
 * float64 of scratch (p and s per entry).  t_indptr / t_indices / t_pos: the
 * transpose map of indptr / indices.
 *
 * Rows of at least wg_gat_long_row() entries (256) are run by a workgroup each
 * and must be listed by the caller, ascending: long_rows [n_long] = the rows i
 * with indptr[i + 1] - indptr[i] >= wg_gat_long_row(); t_long_rows [n_tlong] =
 * the nodes for which that holds in indptr or in t_indptr.  A listed row that is
 * not long is harmless; a long row that is not listed is not computed.
 * 1 <= C; 1 <= Hh <= 64.  All sums, products and exp in float64, in an order
 * fixed by the rows and nnz / n; no float atomics: the same input gives the same
 * bits.  Column ids and positions are checked on the device in the
 * bounds-checked variant only; every other argument before any device call.
 * Forward and backward are asynchronous, allocate nothing and may be captured;
 * n == 0 is WG_OK with no launch.
 * ---------------------------------------------------------------------- */
int wg_csr_transpose_map(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                         int64_t* t_indptr, int32_t* t_indices, int32_t* t_pos, void* stream);
int wg_bfs_levels(int64_t n, const int64_t* indptr, const int32_t* indices, const uint8_t* mask,
                  int32_t max_hop, int64_t* dist, void* stream);
int wg_gat_long_row(void);
int wg_gat_forward(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                   int64_t n_long, const int32_t* long_rows, int64_t C, int64_t Hh, const float* a,
                   const float* t, const float* conf, double negative_slope, float* sim,
                   float* dconf, double* e_save, double* row_max, double* row_den, void* stream);
int wg_gat_backward(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                    int64_t n_long, const int32_t* long_rows, const int64_t* t_indptr,
                    const int32_t* t_indices, const int32_t* t_pos, int64_t n_tlong,
                    const int32_t* t_long_rows, int64_t C, int64_t Hh, const float* a,
                    const float* t, const double* e_save, const double* row_max,
                    const double* row_den, const float* g_sim, double negative_slope,
                    float* grad_a, float* grad_t, double* edge_work, void* stream);

/* -------------------------------------------------------------------------
 * Section 8(f): the aggregation of the CaGCN calibrator (reference
 * calibration/CaGCN.py:104-108).  Its scaling model is two PyG GCNConv layers
 * on edge_index = dense_to_sparse(adj); GCNConv calls gcn_norm
 * (add_remaining_self_loops, deg = the in-degree with the loop, one weight
 * deg_i^-1/2 deg_j^-1/2 per edge) and propagates the scaled source rows with
 * aggr='add'.  wg_symnorm_aggregate replaces gcn_norm and that propagation:
 *
 *   out[i][c] = act( dinv[i] * sum_{p in [indptr[i], indptr[i+1])}
 *                                  dinv[indices[p]] * x[indices[p]][c]  +  bias[c] )
 *
 * indptr / indices: the canonical CSR by destination (row i lists the sources
 * of the edges into i, ascending, no duplicates) with one self loop per node
 * already in it; dinv float32 [n] = in-degree^-1/2; x and out row-major (n, C)
 * float32, out must not alias x; bias C floats or NULL; relu != 0: act is
 * v < 0 ? 0 : v (a NaN stays), else the identity.  No edge values are read.
 * The gradient w.r.t. x is the same call on the transposed structure
 * (wg_csr_transpose_map) with bias NULL and relu 0:
 *   grad_x[j] = dinv[j] * sum_{i : j in row i} dinv[i] * g[i].
 *
 * Rows of at least wg_symnorm_long_row() entries (128) are run by a workgroup
 * each, from long_rows [n_long] (ascending).  A listed row that is not long is
 * harmless, and a long row that is not listed is still computed (by one
 * sub-group of lanes: slowly).  Products and sums in float64, the epilogue
 * dinv_i * acc + bias_c in float64 rounded once to float32; the order of a
 * row's sum is fixed by the row, C and the launch shape; no float atomics: the
 * same input gives the same bits.  Any C >= 1; 16-byte loads when C % 4 == 0
 * and x / out are 16-byte aligned, dword loads otherwise.  Column ids, row
 * ranges and listed rows are checked on the device in the bounds-checked
 * variant only; every other argument before any device call: n == 0 or C == 0
 * is WG_OK with no launch; a negative size, a NULL indptr / dinv / x / out
 * (indices with nnz > 0, long_rows with n_long > 0) or out == x is
 * WG_ERR_INVALID.  Asynchronous, allocates nothing, may be captured.
 * ---------------------------------------------------------------------- */
int wg_symnorm_long_row(void);
int wg_symnorm_aggregate(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                         int64_t n_long, const int32_t* long_rows, const float* dinv, int64_t C,
                         const float* x, const float* bias, int32_t relu, float* out,
                         void* stream);

/* -------------------------------------------------------------------------
 * Section 8(f): the gated mixture of graph experts of the GETS calibrator
 * (reference calibration/GETS.py).  Each of its E experts ends in a PyG GCNConv;
 * forward stacks the E aggregated (N, C) outputs, multiplies them by gates that
 * are exact zeros outside a row's top-k selection and sums.  The gate belongs
 * to the destination row, so it commutes with the aggregation, and the three
 * entries below never build an (N, E, C) tensor of aggregated outputs.
 *
 * indptr / indices / dinv / long_rows: exactly what wg_symnorm_aggregate takes
 * (the canonical CSR by destination with one self loop per node, dinv =
 * in-degree^-1/2), with rows of at least wg_gated_symnorm_long_row() entries
 * (128) listed ascending.  A listed row that is not long is harmless, and a
 * long row that is not listed is still computed (by one sub-group: slowly).
 * All row-major: z (n, E, C) float32, each expert's last linear map; sel
 * (n, k) int32, the selected experts of a row, distinct, in [0, E); gate
 * (n, k) float32, their weights; bias (E, C) float32 or NULL; logits (n, C)
 * float32.
 *
 * wg_gated_symnorm_forward replaces the last GCNConv's propagation of every
 * expert (GETS.py:86-92 through :402-407) and GETS.py:410-417.  For row i and
 * slot s, with e = sel[i, s]:
 *   acc_s = sum_{p in [indptr[i], indptr[i+1])} dinv[j_p] * z[j_p, e, :]
 *   O_s   = dinv[i] * acc_s + bias[e]           T = sum_s gate[i, s] * O_s
 *   sp    = T > 20 ? T : log1p(exp(T))          (torch's softplus)
 *   out   = log_softmax(logits[i] * sp)         out (n, C)
 * t_save (n, C) = T and o_save (n, k, C) = O_s are what the backward needs;
 * both NULL for inference.  A slice that a row did not select is never read: a
 * NaN in it does not reach that row (the reference's 0 * NaN would).  A row
 * with an empty range gives T = sum_s gate * bias.
 *
 * wg_gets_head_backward replaces autograd's backward of GETS.py:410-417, row by
 * row without the graph, from g_out = d loss / d out:
 *   g_cal    = g_out - exp(out) * sum_c g_out
 *   g_logits = g_cal * sp(T)
 *   g_t      = g_cal * logits * (T > 20 ? 1 : sigmoid(T))
 *   g_gate[i, s] = sum_c g_t[i, c] * o_save[i, s, c]     (the float64 g_t)
 * with T read from t_save.  None of these reads the gate, so it is no argument.
 *
 * wg_gated_symnorm_transposed replaces the backward of the stacked propagation
 * w.r.t. its inputs, on the transposed structure (wg_csr_transpose_map, with
 * the long rows of t_indptr):
 *   g_z[j, e, :] = dinv[j] * sum_{i : j in row i} dinv[i] *
 *                  (gate[i, s] if sel[i, s] == e for a slot s, else 0) * g_t[i, :]
 * It writes all E slices of every row, exact zeros where no gathering row
 * selected e (a NaN in g_t[i] reaches only the experts that row i selected).
 * The gradient w.r.t. bias is a small (E, n) x (n, C) product left to the
 * caller.
 *
 * Arithmetic: every product, sum, exp and log is float64 (the row's maximum and
 * sum of the log_softmax go across the sub-group in float64), every output is
 * rounded once to float32; the order of every sum is fixed by the row, C and the
 * launch shape; no float atomics: the same input gives the same bits.  16-byte
 * loads when C % 4 == 0 and every float buffer of the call is 16-byte aligned,
 * dword loads otherwise.  Column ids, row ranges, listed rows and the ids in
 * sel are checked on the device in the bounds-checked variant only; every
 * other argument before any device call: a negative size, C < 1, E < 1, k < 1,
 * k > E, n_long > n, a NULL pointer other than those named nullable (indices
 * with nnz > 0, long_rows with n_long > 0), only one of t_save / o_save, an
 * output that aliases an input or another output: WG_ERR_INVALID; C > 256
 * (the row's softmax needs the whole row in one sub-group), E > 4 (k > 4 in
 * wg_gets_head_backward), n or nnz above int32: WG_ERR_UNSUPPORTED.  n == 0 is
 * WG_OK with no launch.  Asynchronous, allocate nothing, may be captured.
 * ---------------------------------------------------------------------- */
int wg_gated_symnorm_long_row(void);
int wg_gated_symnorm_forward(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                             int64_t n_long, const int32_t* long_rows, const float* dinv, int64_t C,
                             int64_t E, int64_t k, const float* z, const int32_t* sel,
                             const float* gate, const float* bias, const float* logits, float* out,
                             float* t_save, float* o_save, void* stream);
int wg_gets_head_backward(int64_t n, int64_t C, int64_t k, const float* g_out, const float* out,
                          const float* logits, const float* t_save, const float* o_save,
                          float* g_logits, float* g_t, float* g_gate, void* stream);
int wg_gated_symnorm_transposed(int64_t n, int64_t nnz, const int64_t* t_indptr,
                                const int32_t* t_indices, int64_t n_long, const int32_t* long_rows,
                                const float* dinv, int64_t C, int64_t E, int64_t k,
                                const int32_t* sel, const float* gate, const float* g_t, float* g_z,
                                void* stream);

/* -------------------------------------------------------------------------
 * Section 8(f): the similarity temperature of the SimCalib calibrator
 * (reference calibration/SimCalib.py:49-58, 91-105).  The reference builds the
 * (N, N_val) cosine matrix of the latent rows against the validation bank, its
 * softmax(. / tau) and the product with 1 / (confidence + eps), and autograd
 * keeps all of them.  These two entries compute the same without any (n, m)
 * buffer.  x (n, d) float32 latent rows, unnormalised; bank (m, d) float32,
 * already L2-normalised; inv_conf (m) float32; all row-major.
 *
 *   a_i = x_i / max(|x_i|, 1e-12)          s_ij = a_i . b_j
 *   w_ij = softmax_j(s_ij / tau)           t_i = sum_j w_ij inv_conf_j
 *
 * wg_simcalib_forward writes t (n), unclamped, and stats (n, 3) float64: each
 * row's maximum of s_ij / tau, the softmax denominator relative to it and t_i
 * before its rounding to float32, which the backward needs (with them its
 * weights sum to one against the same t_i as the forward's, to rounding of
 * single terms).  wg_simcalib_backward takes g = dL/dt (n; the caller has
 * applied the clamp's mask) with the forward's stats and writes
 * gx (n, d) = dL/dx:  ga_i = (g_i / tau) sum_j w_ij (inv_conf_j - t_i) b_j,
 * then F.normalize's Jacobian as torch differentiates it,
 * gx_i = (ga_i - a_i (a_i . ga_i)) / |x_i| for |x_i| >= 1e-12, else
 * ga_i / 1e-12.  There is no gradient w.r.t. bank or inv_conf (the reference
 * detaches both).
 *
 * Both products run on v_mfma_f32_32x32x2_f32 (float32 in, float32 k-ordered
 * fma chains); exp is float32, numerator and denominator are float64 sums
 * with a running maximum, right for any tau > 0; the row norm is a float64
 * sum rounded once.
 * Every sum has a fixed order, bank rows are never split over workgroups and
 * no float atomics are used: the same input gives the same bits.  A NaN in
 * row i of x reaches t_i and gx_i only.
 *
 * Any n >= 1, m >= 1 and 1 <= d <= wg_simcalib_max_d() (256: a row tile and
 * its d-wide gradient live in registers).  Checked before any device call:
 * n, m or d <= 0, a NULL pointer, tau <= 0, non-finite or so small that
 * 1 / tau overflows float32, gx == x: WG_ERR_INVALID; d above the limit or
 * n / m above int32: WG_ERR_UNSUPPORTED.  Asynchronous, allocates nothing, may
 * be captured.
 * ---------------------------------------------------------------------- */
int wg_simcalib_max_d(void);
int wg_simcalib_forward(int64_t n, int64_t m, int64_t d, const float* x, const float* bank,
                        const float* inv_conf, double tau, float* t, double* stats, void* stream);
int wg_simcalib_backward(int64_t n, int64_t m, int64_t d, const float* x, const float* bank,
                         const float* inv_conf, double tau, const double* stats, const float* g,
                         float* gx, void* stream);

/* -------------------------------------------------------------------------
 * Section 8(f): the DCGC calibrator (reference calibration/DCGC.py).
 * Decisive_Edge.get_weight (DCGC.py:66-79) gives every stored entry (r, c) of
 * the adjacency, in the row-major order of dense_to_sparse (= the canonical CSR
 * by row; e numbers its entries), the weight
 *
 *   z1 = W1 [emb_r ; emb_c] + b1   h1 = D1 * relu(z1)     (4C units)
 *   z2 = W2 h1 + b2                h2 = D2 * relu(z2)     (2C units)
 *   z3 = w3 . h2 + b3              w_e = relu(z3)
 *
 * (DCGC.py:36-44, :70-73: `col, row = edge_index` swaps the names, f1 = emb[r],
 * f2 = emb[c], the weight lands at [r, c]; the adjacency's own values are not
 * read).  emb (n, C) float32; W1 (4C, 2C), b1 (4C), W2 (2C, 4C), b2 (2C),
 * w3 (2C), b3 (1): torch Linear layouts, float32.  The reference builds the
 * (E, 2C), (E, 4C) and (E, 2C) tensors and autograd keeps them; these entries
 * keep an entry's activations in registers and the backward recomputes them:
 * no buffer of nnz x k floats with k > 4 exists.  The three products run on
 * v_mfma_f32_32x32x2_f32 (float32 in, float32 k-ordered fma chains); the last
 * layer is a float64 sum per entry.
 *
 * Dropout (D1, D2; DCGC.py:39, :42).  p == 0: all ones, nothing is hashed.
 * Else unit j (0-based) of layer l (1 or 2) of entry e (its CSR position) is
 * kept iff, in unsigned 64-bit arithmetic modulo 2^64,
 *   x  = (seed ^ (0x9E3779B97F4A7C15 * l)) + e * 0xBF58476D1CE4E5B9
 *                                           + j * 0x94D049BB133111EB
 *   x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;
 *   x *= 0x94D049BB133111EB;  x ^= x >> 31
 *   (uint32)(x >> 32) >= (uint32) floor(p * 2^32)
 * and a kept unit is scaled by (float)(1 / (1 - p)).  Examples with seed = 7,
 * l = 1: (e, j) = (0, 0), (1, 0), (0, 1), (123456, 77) give the 32-bit words
 * 0xf75f04cb, 0x73086d4d, 0x5f2f8c48, 0xc768449f; with l = 2: 0xb3466f8a,
 * 0xfe2295de, 0x14959e27, 0x3b9c8399.  The stream is NOT torch's: a run with
 * p > 0 does not reproduce the reference's masks, only their distribution.
 *
 * wg_edge_mlp_forward writes w (nnz).  wg_edge_mlp_backward takes g_w = dL/dw
 * (nnz) and the forward's inputs and overwrites the six parameter gradients
 * (the parameters' shapes) and, unless g_emb is NULL, g_emb (n, C) = dL/demb;
 * g_emb needs the transposed CSR with its entry map (wg_csr_transpose_map);
 * with g_emb NULL those three may be NULL.  workspace: wg_edge_mlp_workspace
 * bytes, 16-byte aligned, scratch (nothing is kept between calls).  It grows
 * with n C, with 256 x the parameter count and with at most 9 bytes per entry.
 *
 * Order.  The backward walks the entries in tiles of wg_edge_mlp_tile() (1024),
 * tile t on workgroup t mod min(tiles, 256), 128 entries at a time.  The weight
 * gradients are float32 MFMA chains over those 128 entries in ascending order;
 * everything across them, and so across tiles, is added in float64 in ascending
 * order, then the workgroups' sums in ascending order.  Bias gradients are
 * float64 sums; a layer's products are float32 chains of 32 terms met in
 * float64.  g_emb is a float64 sum per node over its
 * entries in ascending CSR position (the emb_r half) and ascending transposed
 * position (the emb_c half, a second recomputing pass).  No float atomics: the
 * same input gives the same bits.  A NaN in row i of emb reaches only the
 * weights of the entries in row i or column i.
 *
 * 1 <= C <= wg_edge_mlp_max_c() (48).  Checked before any device call: a
 * negative n / nnz, C <= 0, p outside [0, 1), a NULL pointer that is needed,
 * g_emb == emb: WG_ERR_INVALID; C above the limit, n or nnz above int32:
 * WG_ERR_UNSUPPORTED.  n == 0 or nnz == 0 is WG_OK: the forward writes
 * nothing, the backward writes zero gradients.  Row and column ids and the map
 * are checked on the device in the bounds-checked variant only.  Asynchronous,
 * allocate nothing, may be captured.
 *
 * wg_edge_aggregate: the base model's propagation (src/gnn/model.py:43-52) on
 * an adjacency whose values are an argument:
 *   out[i] = row_scale[i] * sum_{p in [indptr[i], indptr[i+1])}
 *            val[map ? map[p] : p] * col_scale[indices[p]] * x[indices[p]]
 * (either scale NULL = 1).  Forward: row_scale = 1 / deg, deg_i = sum_c w_ic
 * with 0 -> 1 (model.py:43-45).  Gradient w.r.t. x: the transposed structure,
 * map = the transpose map, col_scale = 1 / deg.  The gradient w.r.t. a value
 * is (g_r . x_c - g_r . y_r) / deg_r (wg_sddmm + wg_rowdot).  Rows of at least
 * wg_edge_aggregate_long_row() entries (128) are run by a workgroup each from
 * long_rows (ascending; a long row that is not listed is still computed, a
 * listed short row is harmless).  Products and sums in float64 in a fixed
 * order, rounded once; 16-byte loads when C % 4 == 0 and x / out are 16-byte
 * aligned.  out must not alias x.  n == 0 or C == 0: WG_OK, no launch.
 *
 * wg_edge_pair_inv_distance: DCGC.get_homo_weight's coefficient
 * (DCGC.py:164-165): out[e] = 1 / (sqrt(sum_k (Q[rows[e]][k] - Q[cols[e]][k])^2)
 * + alpha), the sum in float64 over the differences themselves (rows[e] ==
 * cols[e] gives exactly (float)(1 / alpha)).  Q (n, C) float32.
 * wg_edge_aggregate and wg_edge_pair_inv_distance are asynchronous, allocate
 * nothing and may be captured.
 * ---------------------------------------------------------------------- */
int wg_edge_mlp_max_c(void);
int wg_edge_mlp_tile(void);
int wg_edge_mlp_workspace(int64_t n, int64_t nnz, int64_t C, int64_t* bytes);
int wg_edge_mlp_forward(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                        int64_t C, const float* emb, const float* W1, const float* b1,
                        const float* W2, const float* b2, const float* w3, const float* b3,
                        double p, uint64_t seed, void* workspace, float* w, void* stream);
int wg_edge_mlp_backward(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                         int64_t C, const float* emb, const float* W1, const float* b1,
                         const float* W2, const float* b2, const float* w3, const float* b3,
                         double p, uint64_t seed, const float* g_w, const int64_t* t_indptr,
                         const int32_t* t_indices, const int32_t* t_pos, float* gW1, float* gb1,
                         float* gW2, float* gb2, float* gw3, float* gb3, float* g_emb,
                         void* workspace, void* stream);
int wg_edge_aggregate_long_row(void);
int wg_edge_aggregate(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                      int64_t n_long, const int32_t* long_rows, const float* val,
                      const int32_t* map, const float* row_scale, const float* col_scale, int64_t C,
                      const float* x, float* out, void* stream);
int wg_edge_pair_inv_distance(int64_t nnz, const int32_t* rows, const int32_t* cols, int64_t C,
                              int64_t n, const float* Q, double alpha, float* out, void* stream);

/* -------------------------------------------------------------------------
 * One step of the calibration attacks (calib_attack/calib_fga.py) on that path.
 *
 * wg_flip_select: the score of every partner j of the target t and the best
 * topk of them (calib_fga.py:880-898), in one pass over n, all in float32,
 * operation for operation what torch computes on the same tensors (no fused
 * multiply-add):
 *   a_j = the entry (t, j) of the base row (0 if absent; values NULL: 1);
 *         j in toggled: a_j += 1 - 2 a_j
 *   d_j = 1 - 2 a_j
 *   s_j = (grad_loss[j] + grad_loss[n + j]) * d_j
 *   with the rerank: c_j = ((p_top2[0] + grad_pmax[j] * d_j) - p_top2[1]) - grad_psmax[j] * d_j
 *                    s_j *= (c_j > 0 ? 1 : -1)          (a NaN c_j: -1)
 *   s_t = -10
 * grad_loss / grad_pmax / grad_psmax are float32 [2 n] in the layout of the
 * target probe -- d / d a[t, j] for all j, then d / d a[i, t] for all i; only
 * the row half of grad_pmax / grad_psmax is read (div_pmax[target_node],
 * calib_fga.py:893).  Both NULL: no rerank; one NULL: WG_ERR_INVALID.  p_top2:
 * device float32 [2], read only with the rerank.  indptr / indices / values:
 * the base CSR (row t is read); toggled: int32 [n_toggled] ascending, the
 * partners whose entries (t, j) / (j, t) differ from the base (NULL when
 * n_toggled == 0).  Outputs: scores [n] (nullable), best_ids int32 [topk],
 * best_scores [topk], 1 <= topk <= 8, descending by score: a NaN ranks above
 * every number (as torch.argmax has it), equal scores (-0 == +0) go by smaller
 * index, a slot past n entries gets id -1 and score -inf.  The order is total,
 * so the result does not depend on the grid: n_workgroups = 0 picks it
 * (ceil(n / 256), at most 256), 1 .. 256 force it.  More than one workgroup
 * leaves partial lists in workspace (wg_flip_select_workspace(&bytes), 8-byte
 * aligned; may be NULL with one workgroup), merged by a second launch.
 * Asynchronous, no allocation, capturable.  n == 0 is WG_OK with no launch.
 * Ids are checked on the device in the bounds-checked variant only; every
 * other argument before any device call.
 *
 * wg_target_logits: the logits of node t under B candidate adjacencies in one
 * launch, for the two-layer base model (src/gnn/model.py) in eval mode on an
 * unweighted canonical CSR.  z = x @ W1^T (n, Hd) is an argument: the kernel
 * evaluates adj_norm (X W1^T) where the model computes (adj_norm X) W1^T.
 * Candidate b toggles (t, j) and (j, t) for j in S_b = cand_ids[cand_ptr[b] ..
 * cand_ptr[b + 1]) (int32, ascending, no t, no duplicates).  With N'(t) = N(t)
 * delta S_b, N'(j) = N(j) delta {t} for j in S_b, N'(j) = N(j) otherwise and
 * deg' = |N'| (0 -> 1, model.py:43-45):
 *   y1_j = (1 / deg'_j) sum_{k in N'(j)} z_k          for j in N'(t)
 *   h_j  = max(y1_j + b1, 0)
 *   y2   = (1 / deg'_t) sum_{j in N'(t)} h_j
 *   out[b] = W2 y2 + b2                               W2 (C, Hd), out (B, C)
 * One workgroup per candidate; its waves take the j of N'(t) -- the base row's
 * surviving entries in ascending order, then the added partners -- a j whose
 * row has at least wg_target_long_row() (128) entries is shared by the whole
 * workgroup.  Every sum and product is float64 in an order fixed by the rows,
 * Hd and the launch shape; out is rounded once; no float atomics: the same
 * input gives the same bits.  16-byte loads when Hd % 4 == 0 and z is 16-byte
 * aligned.  1 <= Hd, C <= 256, B >= 1; n or nnz above int32:
 * WG_ERR_UNSUPPORTED.  An empty S_b gives the base model's row t.
 * Asynchronous, no allocation, capturable.
 *
 * wg_trial_logits: the logits of B trials of the random attacks in one launch
 * (calib_attack/calib_random.py:127-186, calib_rnd.py:169-236: every trial is a
 * full forward there).  The same kernel and the same sums as wg_target_logits,
 * with three things per trial b:
 *   trial_t[b] (int32)  its own target t; trials of one launch may name
 *                       different targets, and duplicates are allowed
 *   S_b                 as above, but j == t is allowed and toggles the single
 *                       diagonal entry (t, t) (the reference lists t among the
 *                       connected nodes of a row with a self loop): N'(t) =
 *                       N(t) delta S_b, N'(j) = N(j) delta {t} for j != t in S_b
 *   F_b = feat_ids[feat_ptr[b] .. feat_ptr[b + 1]) (int32, ascending, no
 *         duplicates, inside [0, nfeat)) with feat_delta (float32, one per id):
 *         deltas of the target's own feature row.  In float64
 *           dz_b[h] = sum_{f in F_b ascending} (double)feat_delta * (double)W1[h, f]
 *         with W1 (Hd, nfeat), and y1_j = (1 / deg'_j) (sum_{k in N'(j)} z_k + dz_b)
 *         for every j in N'(t) whose row N'(j) holds t (the self loop j == t
 *         included; asked of the row itself, no symmetry is assumed), that is
 *         z_t + dz_b wherever row t of z is gathered.
 * feat_ptr == NULL: no feature trial in the launch; W1, feat_ids, feat_delta
 * and nfeat are then not read.  With every trial_t[b] equal, no t in any S_b
 * and no features, out has wg_target_logits' bits.  trial_t, the ids of S_b
 * and F_b are checked on the device in the bounds-checked variant only; every
 * other argument before any device call (1 <= Hd, C <= 256, B >= 1, nfeat >= 1
 * with features).  Asynchronous, no allocation, capturable.
 * ---------------------------------------------------------------------- */
int wg_flip_select_workspace(int64_t* bytes);
int wg_flip_select(int64_t n, int64_t t, const float* grad_loss, const float* grad_pmax,
                   const float* grad_psmax, const float* p_top2, const int64_t* indptr,
                   const int32_t* indices, const float* values, int64_t n_toggled,
                   const int32_t* toggled, int32_t topk, int32_t n_workgroups, void* workspace,
                   float* scores, int32_t* best_ids, float* best_scores, void* stream);
int wg_target_long_row(void);
int wg_target_logits(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                     int64_t Hd, const float* z, const float* b1, const float* W2, const float* b2,
                     int64_t C, int64_t t, int64_t B, const int32_t* cand_ptr,
                     const int32_t* cand_ids, float* out, void* stream);
int wg_trial_logits(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                    int64_t Hd, const float* z, const float* b1, const float* W2, const float* b2,
                    int64_t C, int64_t B, const int32_t* trial_t, const int32_t* cand_ptr,
                    const int32_t* cand_ids, int64_t nfeat, const float* W1,
                    const int32_t* feat_ptr, const int32_t* feat_ids, const float* feat_delta,
                    float* out, void* stream);

/* ----------------------------------------------------------------------
 * wg_fga_scores (csrc/fga.hip): what calib_fga.py:864-898 reads from one
 * forward and up to three backward passes of the whole graph, for B targets
 * in one call, on the two-layer base model and a unit canonical CSR.  Target b
 * is targets[b] (int32, duplicates allowed) with the toggle set S_b =
 * tog_ids[tog_ptr[b] .. tog_ptr[b + 1]) (ascending, distinct, never t), as
 * wg_target_logits has it: N'(t) = N(t) delta S_b, N'(j) = N(j) delta {t} for
 * j in S_b, deg' = |N'| (0 -> 1, a constant then).  z = x W1^T and
 * h = relu(A_hat z + b1) of the BASE graph are (n, Hd) float32 arguments.
 * g_logits (B, G, C) float32 holds d L / d out_t for G in {1, 3} scalars L per
 * target: row 0 the loss, rows 1 and 2 p_max and p_smax.  Per gradient row,
 * with q = W2^T g, m_i = q * [y1_i + b1 > 0] (strictly) and a_tt = [t in N'(t)]:
 *   grow_j = (q . h_j - q . y2) / deg_t + (a_tt / deg_t^2) m_t . (z_j - y1_t)
 *   gcol_i = [i in N'(t)] (1 / (deg_t deg_i)) m_i . (z_t - y1_i)
 * the entries d / d A[t, j] and d / d A[i, t] of the target probe's layout.
 * For the local j (N(t) + S_b) y1_j, h_j, deg_j, y2 and y1_t are summed in
 * float64 from z on the flipped rows, every row by the whole workgroup (wave w
 * takes the entries w, w + 4, ..., the waves' sums are added in wave order,
 * which is how wg_target_logits shares its long rows); every other j reads
 * the float32 h_j and has gcol_j = +0.  Every sum and product is float64 in an
 * order fixed by the rows, Hd and the launch shape; grow_j and gcol_j are each
 * rounded once to float32.  The entry (t, t) is one variable: its score is -10
 * and its two gradient slots are not defined.
 * From those rounded values, in float32 and operation for operation,
 * wg_flip_select's score: a_j from the base row and S_b, s_j = (grow_j +
 * gcol_j) d_j, the rerank (row half only) for the targets with rerank[b] != 0
 * (int32 [B], nullable, read only with G == 3; p_top2 (B, 2) float32 then),
 * s_t = -10, and the best topk (1 .. 8) per target under wg_flip_select's total
 * order.  Outputs: best_ids (B, topk) int32, best_scores (B, topk); optional
 * (NULL: none) grads (B, G, 2 n) and scores (B, n).  n_workgroups = 0 picks the
 * grid of the pass over j (ceil(n / 64), at most 512), 1 .. 512 force it; the
 * result does not depend on it.  local_cap: the capacity of the local lists,
 * at least the sum over the targets of |N(t)| + |S_b| (an entry past it is
 * dropped, never written: that target's scores are then wrong and the call
 * still returns WG_OK, as nothing on the host knows the rows' lengths; the
 * bounds-checked variant traps with the target and the shortfall).  workspace: wg_fga_scores_workspace(n, Hd, B, G,
 * local_cap, &bytes), 16-byte aligned: the coefficients, the local lists and
 * the partial top-k lists.  No float atomics: the same input gives the same
 * bits.  Asynchronous, no allocation, capturable.  1 <= Hd, C <= 256; n,
 * nnz or local_cap above int32, or B above 2^20: WG_ERR_UNSUPPORTED.  Every argument is checked before any
 * device call, ids on the device in the bounds-checked variant only.
 * ---------------------------------------------------------------------- */
int wg_fga_scores_workspace(int64_t n, int64_t Hd, int64_t B, int32_t G, int64_t local_cap,
                            int64_t* bytes);
int wg_fga_scores(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t Hd,
                  const float* z, const float* h, const float* b1, const float* W2, int64_t C,
                  int64_t B, const int32_t* targets, const int32_t* tog_ptr, const int32_t* tog_ids,
                  int32_t G, const float* g_logits, const int32_t* rerank, const float* p_top2,
                  int32_t topk, int32_t n_workgroups, int64_t local_cap, void* workspace,
                  float* grads, float* scores, int32_t* best_ids, float* best_scores, void* stream);

/* ----------------------------------------------------------------------
 * The integrated-gradient scores of calib_attack/calib_iga.py on the sparse
 * path (csrc/iga.hip), for the two-layer base model (src/gnn/model.py:37-53,
 * eval mode) on a unit (value-free) canonical CSR.  z = x W1^T and
 * h = relu(A_hat z + b1) are (n, Hd) float32 arguments, zsum / hsum their
 * float64 column sums [Hd].
 *
 * The reference moves row t of the dense adjacency (the whole row, entry
 * (t, t) included; column t stays) along two paths with lam = k / steps,
 * k = 0 .. steps (calib_iga.py:185-206): the remove path w = lam a for the j
 * with an entry, the add path w = 1 - lam (1 - a) for the j without one.  Per
 * path point, with deg = sum_j w_j (0 -> 1, a constant then: model.py:44):
 *   p = (sum_j w_j z_j) / deg          h_t' = relu(p + b1)
 *   q = (sum_{j != t} w_j h_j + w_t h_t') / deg
 *   out = W2 q + b2
 * and the sums over all j follow from row t's neighbour sums and zsum / hsum.
 *
 * wg_iga_path_logits (replaces the forward passes of calib_iga.py:201-211):
 * for B targets (int32 [B], duplicates allowed) the logits (B, P, C) float32
 * of the P = 2 (steps + 1) path points, remove path first, k ascending, and
 * the float64 state (B, P, 2 Hd + 2): p [Hd], q [Hd], deg (the sum as
 * summed: 0 for a zero row), w_t.  One workgroup per target; row t is
 * gathered once, by 256 / W sub-groups (W: Hd rounded up to a power of two)
 * whose sums are added in sub-group order.  A row of 0 entries gives the zero
 * row with deg = 1 at every remove point; a full row the all-ones row at every
 * add point.  1 <= steps <= 4096.
 *
 * wg_iga_scores (replaces the backward passes and calib_iga.py:217-233): from
 * g_logits (B, P, C) float32 = d loss / d logits at every path point, per
 * (target, path) in float64
 *   g_q = W2^T g_out    u = g_q / deg    v = (w_t / deg^2) (g_q * [p + b1 > 0])
 *   c = -(u . q + v . p)                  (0 at a zero row)
 *   U = sum_k u, V = sum_k v, cbar = sum_k c       (no division by steps + 1:
 *                                                   :223 takes the mean of a scalar)
 * then in one pass over j for all B targets (a tile of 64 rows of z and h is
 * staged once and read by every target; targets are taken 32 at a time)
 *   s_j = -(U . h_j + V . z_j + cbar) of the remove path if (t, j) is an entry
 *         (binary search in row t), +(...) of the add path if not;  s_t = -10
 * summed in float64 as cbar, then U_f h_jf, V_f z_jf for f ascending, rounded
 * once.  best_ids (B, topk) int32 / best_scores (B, topk): the best topk per
 * target under wg_flip_select's total order (a NaN above every number, equal
 * scores and -0 == +0 by the smaller index, a slot past n entries: id -1,
 * score -inf); s_t takes part.  1 <= topk <= wg_iga_max_topk() (32).
 * n_workgroups = 0 picks the grid (ceil(n / 64), at most 512), 1 .. 512 force
 * it; the result does not depend on it.  workspace: wg_iga_scores_workspace
 * (B, Hd, &bytes), 8-byte aligned, holds the coefficients and the workgroups'
 * partial lists, merged by a further launch.  Optional outputs (NULL: none):
 * coeffs (B, 2, 2 Hd + 1) float64 = U, V, cbar per path; scores (B, n).
 *
 * Both: float64 sums in an order fixed by the inputs and the launch shape,
 * outputs rounded once, no float atomics (the same input gives the same
 * bits); asynchronous, no allocation, capturable; every argument is checked
 * before any device call, ids on the device in the bounds-checked variant
 * only.  1 <= Hd, C <= 256; n or nnz above int32: WG_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------- */
int wg_iga_max_topk(void);
int wg_iga_path_logits(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                       int64_t Hd, const float* z, const float* h, const double* zsum,
                       const double* hsum, const float* b1, const float* W2, const float* b2,
                       int64_t C, int64_t B, const int32_t* targets, int32_t steps, float* logits,
                       double* state, void* stream);
int wg_iga_scores_workspace(int64_t B, int64_t Hd, int64_t* bytes);
int wg_iga_scores(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, int64_t Hd,
                  const float* z, const float* h, const float* b1, const float* W2, int64_t C,
                  int64_t B, const int32_t* targets, int32_t steps, const float* g_logits,
                  const double* state, int32_t topk, int32_t n_workgroups, void* workspace,
                  double* coeffs, float* scores, int32_t* best_ids, float* best_scores, void* stream);

/* -------------------------------------------------------------------------
 * Section 8(f): the four node-wise calibrators (reference calibration/TS.py,
 * VS.py, MS.py, ETS.py).  Each is a row-wise map of the base model's logits
 * z (n_total, C) float32, row-major.  mode: 0 TS, 1 VS, 2 MS, 3 ETS.  The
 * parameters p0 .. p3 are device float32 arrays (unused ones NULL):
 *   TS   p0 temperature (1)     s = log(exp(temperature) + 1.1)
 *        out = log_softmax(z * s)                          (TS.py:26, :39-43)
 *   VS   p0 temperature (C)     the same, s_c per column   (VS.py:33, :45-49)
 *   MS   p0 W (C, C), p1 b (C)  z' = z - z[:, C - 1],  out = z' W + b, raw
 *        (MS.py:43-57); flags bit 0 ("normalize"): out = log_softmax(z' W + b)
 *   ETS  p0 tau (1), p1 w1, p2 w2, p3 w3 (1 each)   temp = log(exp(tau) + 1.1)
 *        out = log(w1 softmax(z / temp) + w2 softmax(z) + w3 / C)
 *                                                          (ETS.py:22-26)
 * rows: an int32 list of n_rows row ids in [0, n_total), any order, repeats
 * allowed; NULL means all rows (then n_rows == n_total).  Outputs and g_out
 * are compact: (n_rows, C), entry r belongs to row rows[r].
 *
 * wg_scale_forward writes out.  wg_scale_backward replaces autograd's
 * backward of the same lines: from g_out = d loss / d out it writes g_logits
 * (nullable; MS's column shift and ETS's mixture included) and, for every
 * non-NULL g_p0 .. g_p3, the gradient of the matching parameter (ETS: tau,
 * w1, w2, w3), which needs workspace of wg_scale_backward_workspace bytes
 * (8-byte aligned).
 *
 * wg_scale_epoch is one epoch of calib_train (TS.py:59-83, VS.py:65-89,
 * MS.py:64-89; modes 0 .. 2) in one launch over the listed rows, labels
 * int64 (n_total) read at the listed ids: the forward, loss =
 * -mean(out[r, y_r]) (MS: + Lambda sum |W - I|, gradient Lambda sign(W - I)
 * with sign(0) = 0), every parameter gradient and the count of rows whose
 * first maximal column is the label.  Rows are cut into fixed chunks of
 * wg_scale_chunk_rows() (256) listed rows; each leaves one float64 partial
 * vector.  The workgroup that arrives last (one relaxed agent-scope
 * fetch_add per workgroup after its partials are drained; no workgroup waits
 * on another) adds the partials in chunk order, takes torch's Adam step (lr,
 * L2 weight decay g += wd * theta, betas 0.9 / 0.999, eps 1e-8,
 * bias-corrected), updates best_loss and the patience counter as TS.py:75-83
 * (a NaN loss counts down), and appends the loss and the accuracy to the
 * traces.  n_workgroups = 0 picks the grid (one workgroup per chunk, at most
 * 1024), 1 .. 1024 force it; the state's bits do not depend on it.  The
 * state is one device block of wg_scale_state_bytes bytes, 8-byte aligned:
 * float64 master parameters and Adam moments, the step count, best_loss, the
 * patience counter, the stopped flag (1: patience ran out, 2: max_epochs
 * reached), the epochs run, both traces and the chunk partials.  A launch
 * that finds stopped set returns without touching anything, so max_epochs
 * launches may be enqueued back to back.  mode, flags, C, max_epochs and
 * max_rows of every wg_scale_epoch must be those the block was initialised
 * with (n_rows <= max_rows is checked on the host, the rest on the device in
 * the bounds-checked variant).  wg_scale_state_init fills it
 * (init_params NULL: the reference's ones; else n float32 in state order, MS:
 * W then b); wg_scale_state_read copies the float32-rounded parameters out
 * (params, nullable) and info (nullable) float64 [5 + 2 max_epochs]:
 * stopped, epochs run, Adam steps, patience left, best loss, then the loss
 * trace and the accuracy trace.
 *
 * wg_ets_label_probs: the one pass ETS.fit needs (ETS.py:50-76): p0y[r] =
 * softmax(z / tau)[y] and p1y[r] = softmax(z)[y] of row rows[r], float64,
 * with the RAW tau as the divisor (ETS.py:43, :57).  A label outside [0, C)
 * gives NaN.
 *
 * Arithmetic: a wave per row; the scaled logits, the row maximum, the sum of
 * exp, the log and every gradient are float64; out, g_logits and
 * wg_scale_backward's parameter gradients are rounded to float32 once; every
 * sum's order is fixed by the rows and C; no float atomics: the same input
 * gives the same bits.  A NaN in a row stays in that row's out / g_logits
 * (and reaches the loss and the parameter gradients).
 *
 * wg_scale_max_c(mode): 256 for TS, VS and ETS (four columns per lane); 64
 * for MS, where a lane owns one column and keeps that column of dW in 64
 * float64 registers (128 VGPRs) while W sits in LDS (33 KB, shared with the
 * workgroup's reduction buffer).  Checked before any device call: a bad
 * mode, a negative size, C < 1, a NULL pointer not named nullable, rows NULL
 * with n_rows != n_total, an output that aliases an input: WG_ERR_INVALID; C
 * above the limit, sizes above int32: WG_ERR_UNSUPPORTED.  Row ids, labels
 * and the state's header are checked on the device in the bounds-checked
 * variant only.  n_rows == 0 is WG_OK with no launch (wg_scale_epoch:
 * WG_ERR_INVALID).  Asynchronous, allocate nothing, may be captured: a replay
 * of wg_scale_epoch is one more epoch on the state block (the last workgroup
 * puts the arrival counter back), of wg_scale_state_init a fresh block.
 * ---------------------------------------------------------------------- */
int wg_scale_max_c(int32_t mode);
int wg_scale_chunk_rows(void);
int wg_scale_forward(int32_t mode, int32_t flags, int64_t n_total, int64_t n_rows, int64_t C,
                     const float* logits, const int32_t* rows, const float* p0, const float* p1,
                     const float* p2, const float* p3, float* out, void* stream);
int wg_scale_backward_workspace(int32_t mode, int64_t n_rows, int64_t C, int64_t* bytes);
int wg_scale_backward(int32_t mode, int32_t flags, int64_t n_total, int64_t n_rows, int64_t C,
                      const float* logits, const int32_t* rows, const float* p0, const float* p1,
                      const float* p2, const float* p3, const float* g_out, float* g_logits,
                      float* g_p0, float* g_p1, float* g_p2, float* g_p3, void* workspace,
                      void* stream);
int wg_scale_state_bytes(int32_t mode, int64_t C, int64_t max_epochs, int64_t max_rows,
                         int64_t* bytes);
int wg_scale_state_init(void* state, int32_t mode, int32_t flags, int64_t C, int64_t max_epochs,
                        int64_t max_rows, int32_t patience, double lr, double weight_decay,
                        double lambda, const float* init_params, void* stream);
int wg_scale_state_read(const void* state, int32_t mode, int64_t C, int64_t max_epochs,
                        float* params, double* info, void* stream);
int wg_scale_epoch(void* state, int32_t mode, int32_t flags, int64_t C, int64_t max_epochs,
                   int64_t max_rows, int64_t n_total, int64_t n_rows, const float* logits,
                   const int32_t* rows, const int64_t* labels, int32_t n_workgroups, void* stream);
int wg_ets_label_probs(int64_t n_total, int64_t n_rows, int64_t C, const float* logits,
                       const int32_t* rows, const int64_t* labels, const float* temperature,
                       double* p0y, double* p1y, void* stream);

/* -------------------------------------------------------------------------
 * Section 8(f)-3: the WATS calibrator's calib_train (reference
 * calibration/WATS.py:132-170) on the device (csrc/watstrain.hip), the design
 * of wg_scale_epoch above.  The head is net = Linear(F, hid) - ReLU -
 * Linear(hid, 1) on the wavelet features H (n_total, F) float32, row-major:
 *   pre_j = b1_j + sum_f W1[j][f] H[f]     relu active iff pre_j > 0 (it hands
 *   t = b2 + sum_j W2_j relu(pre_j)        a NaN on; pre_j == 0: gradient 0)
 *   T = log(exp(t) + 1.1f),  out = log_softmax(z / T)      (WATS.py:124-130)
 * with z = logits (n_total, C) float32.  W1 is (hid, F) row-major, b1 (hid),
 * W2 (hid), b2 (1): P = hid * F + 2 hid + 1 parameters.
 *
 * wg_wats_train_epoch is one epoch in one launch over the listed rows (rows:
 * int32 ids in [0, n_total), any order, repeats allowed; NULL means all rows,
 * then n_rows == n_total), labels int64 (n_total) read at the listed ids: the
 * forward, loss = -mean(out[r, y_r]), the gradients of all four tensors and
 * the count of rows whose first maximal column is the label.  Rows are cut
 * into fixed chunks of wg_wats_train_chunk_rows() (256) listed rows; each
 * leaves one float64 partial vector: loss sum, correct count, then the P
 * gradient sums (gW1 [hid][F], gb1, gW2, gb2).  The workgroup that arrives
 * last (one relaxed agent-scope fetch_add per workgroup after its partials
 * are drained; no workgroup waits on another) adds the partials in chunk
 * order, divides by n_rows, takes torch's Adam step on all four tensors (lr,
 * L2 weight decay g += wd * theta, betas 0.9 / 0.999, eps 1e-8,
 * bias-corrected), updates best_loss, the patience counter and the stopped
 * flag (1: patience ran out, 2: max_epochs reached; a NaN loss counts
 * patience down), appends the loss and the accuracy to the traces and puts
 * the arrival counter back.  A launch that finds stopped set returns without
 * touching anything, so max_epochs launches may be enqueued back to back.
 * n_workgroups = 0 picks the grid (one workgroup per chunk, at most 1024),
 * 1 .. 1024 force it; the state's bits do not depend on it.
 *
 * The state is one device block of wg_wats_train_state_bytes bytes, 8-byte
 * aligned: float64 master parameters and Adam moments, the step count,
 * best_loss, the patience counter, the stopped flag, the epochs run, both
 * traces and the chunk partials.  F, hid, C, max_epochs and max_rows of every
 * wg_wats_train_epoch must be those the block was initialised with (n_rows <=
 * max_rows is checked on the host, the rest on the device in the
 * bounds-checked variant).  wg_wats_train_state_init fills it from the four
 * float32 tensors; wg_wats_train_state_read copies the float32 rounding of
 * the master parameters out (W1, b1, W2, b2: each nullable) and info
 * (nullable) float64 [5 + 2 max_epochs] as wg_scale_state_read: stopped,
 * epochs run, Adam steps, patience left, best loss, then the loss trace and
 * the accuracy trace.
 *
 * Arithmetic: a wave per row, the hidden units on lanes; everything is
 * float64, from the float64 master parameters and the float32 H / logits
 * widened; the constant is (double)1.1f, the value the reference's float32
 * tensor holds; every sum's order is fixed by the rows, F, hid and C; no
 * float atomics: the same input gives the same bits on every grid.
 *
 * Checked before any device call: 1 <= hid <= 64, F >= 1, max_epochs >= 1, a
 * NULL pointer not named nullable, n_rows == 0, n_rows > max_rows, rows NULL
 * with n_rows != n_total, n_workgroups outside [0, 1024], patience < 1:
 * WG_ERR_INVALID; P above wg_wats_train_max_params() (2048: four waves x P
 * doubles of LDS, the bound of wg_wats_head_backward), C above
 * wg_scale_max_c(0) (256), sizes above int32: WG_ERR_UNSUPPORTED.  Row ids,
 * labels and the state's header are checked on the device in the
 * bounds-checked variant only.
 *
 * queue is a HIP stream (NULL: the default stream), with the promise of the
 * wg_scale_* section: the three device entry points are asynchronous,
 * allocate nothing and may be captured: a replay of wg_wats_train_epoch is
 * one more epoch on the state block (the last workgroup puts the arrival
 * counter back), of wg_wats_train_state_init a fresh block.  These entries
 * are held to that promise by tests/test_wats_train.py until a later change
 * classifies them in the registry of tests/stream_cases.py and renames the
 * parameter.
 * ---------------------------------------------------------------------- */
int wg_wats_train_max_params(void);
int wg_wats_train_chunk_rows(void);
int wg_wats_train_state_bytes(int64_t F, int32_t hid, int64_t max_epochs, int64_t max_rows,
                              int64_t* bytes);
int wg_wats_train_state_init(void* state, int64_t F, int32_t hid, int64_t C, int64_t max_epochs,
                             int64_t max_rows, int32_t patience, double lr, double weight_decay,
                             const float* W1, const float* b1, const float* W2, const float* b2,
                             void* queue);
int wg_wats_train_state_read(const void* state, int64_t F, int32_t hid, int64_t max_epochs,
                             float* W1, float* b1, float* W2, float* b2, double* info,
                             void* queue);
int wg_wats_train_epoch(void* state, int64_t F, int32_t hid, int64_t C, int64_t max_epochs,
                        int64_t max_rows, int64_t n_total, int64_t n_rows, const float* H,
                        const float* logits, const int32_t* rows, const int64_t* labels,
                        int32_t n_workgroups, void* queue);

/* -------------------------------------------------------------------------
 * Section 8(f): the evaluation the harness runs after every calibrator and
 * every attack (csrc/calib.hip).  Replaces the host loops of
 * evaluate_calibration / evaluate_calibration_probs
 * (benchmark_calibration_methods.py:87-158), evaluate_model_calibration
 * (ugca_calib_attack.py:78-104), calculate_ece / calculate_average_ece
 * (utils/ece.py:8-89) and the binning of sklearn's calibration_curve that
 * ece_chart / draw_multiple_ece_charts plot (utils/ece.py:109-115, :191-197,
 * :249-251).
 *
 * wg_calib_bins: G sets of outputs out (G, n, C) float32 share labels
 * (n) int64 and the row list rows (n_rows) int64, any order, a row listed
 * twice counts twice (probs[idx]); NULL means all rows in order (then n_rows
 * == n).  A row id outside [0, n) is never read: it is counted in scalars[7]
 * (in every build).  kind says what out holds, per element:
 *   WG_CALIB_PROBS   p = the float32 as given
 *   WG_CALIB_EXP     p = (float)exp((double)x), not normalised: what the
 *                    harness does to whatever a model returns
 *                    (benchmark_calibration_methods.py:102-103), so p may
 *                    exceed 1
 *   WG_CALIB_LOGITS  p = the float64 softmax of the row, rounded once
 * (double)p is compared with edges (n_bins + 1) float64, ascending, on the
 * device, exactly as np.digitize(p, edges, right=True) - 1 (utils/ece.py:
 * 39-40): bin b holds edges[b] < p <= edges[b + 1].  The caller passes
 * np.linspace(0, 1, n_bins + 1); the kernel never recomputes an edge.
 *
 * table (G, C + 1, n_bins + 2, 3) uint64.  Cell (g, c, b) of a bin b <
 * n_bins: the count, the count of those rows whose label is c, and sum p in
 * fixed point, p added as (uint64)rint((double)p * 2^40) (exact for a float32
 * p >= 2^-17, else within 2^-41; 2^23 rows stay below 2^63).  Slot n_bins
 * holds p <= edges[0] (third word: the count of exact zeros), slot n_bins + 1
 * everything else (p > edges[n_bins], NaN; third word: the count of NaN and
 * +inf).  Slice c == C is the top-label table: p is the row's maximum (a NaN
 * above every number), its label count the rows whose first maximal column
 * is the label.  A label outside [0, C) belongs to no class.  sklearn's
 * calibration_curve rule, searchsorted(edges[1:-1], p), differs on [0, 1]
 * only in putting p == 0 into bin 0, so the same table serves it.  Integer
 * sums commute: the table has the same bits for every grid and every run.
 *
 * scalars (G, 8) float64: [0] rows taken, [1] rows whose p are all finite,
 * and over those [2] rows whose first maximal column is the label, [3] sum
 * max p, [4] sum -log p_label (LOGITS: the float64 log-softmax, EXP:
 * -x_label, PROBS: -log p; rows with 0 <= label < C and p_label > 0 only),
 * [5] the rows [4] used, [6] sum_c (p_c - [label == c])^2; [7] row ids
 * refused.  The sums are taken per chunk of wg_calib_chunk_rows() (256)
 * consecutive entries of the row list, a chunk's partial a function of that
 * chunk alone, the partials added in ascending chunk order (wg_scale_epoch's
 * scheme): the same bits for every grid.  n_workgroups = 0 picks the grid
 * (one workgroup per chunk, at most 1024), 1 .. 1024 force it.  workspace:
 * wg_calib_workspace bytes, 8-byte aligned (the chunk partials).  A table
 * of at most 5120 words is kept in LDS by each workgroup and added to the
 * zeroed table with integer global adds at the end; a larger one is added to
 * in place.
 *
 * wg_calib_ece (utils/ece.py:44-60 on every slice): bins with count <
 * min_count (the reference: 4) are skipped, |sum p / cnt - sum y / cnt| *
 * (cnt / n_rows) is added in ascending bin order in float64; ece_class
 * (G, C), ece_top (G) the same sum on slice C.
 *
 * Limits: C <= wg_calib_max_classes() (256), n_bins <= wg_calib_max_bins()
 * (64), n_rows <= wg_calib_max_rows() (2^23), G <= 4096: above them
 * WG_ERR_UNSUPPORTED; a bad kind or shape, a NULL or misaligned pointer:
 * WG_ERR_INVALID, all before any device call.  Both entries are asynchronous,
 * allocate nothing, use no float atomics and may be captured: each call, and
 * so each replay, zeroes what it accumulates into.  n_rows == 0 or G == 0 is
 * WG_OK with zeroed outputs.  The bounds-checked variant checks the bin index
 * and the table cell on the device.
 * ---------------------------------------------------------------------- */
#define WG_CALIB_PROBS 0
#define WG_CALIB_EXP 1
#define WG_CALIB_LOGITS 2
int wg_calib_chunk_rows(void);
int wg_calib_max_rows(void);
int wg_calib_max_classes(void);
int wg_calib_max_bins(void);
int wg_calib_workspace(int64_t G, int64_t C, int64_t n_bins, int64_t n_rows, int64_t* bytes);
int wg_calib_bins(int64_t G, int64_t n, int64_t C, int32_t kind, const float* out,
                  const int64_t* labels, int64_t n_rows, const int64_t* rows, int32_t n_bins,
                  const double* edges, int32_t n_workgroups, void* workspace, uint64_t* table,
                  double* scalars, void* stream);
int wg_calib_ece(int64_t G, int64_t C, int32_t n_bins, int64_t n_rows, int32_t min_count,
                 const uint64_t* table, double* ece_class, double* ece_top, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WATS_HIP_H */
