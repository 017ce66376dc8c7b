"""numpy restatement of the edge-list ingestion semantics (a helper, not a test).

``ingest_ref(src, dst, n, weights, duplicates=, symmetric=, self_loops=)``
returns the canonical CSR ``(indptr int64, indices int32, values float32)`` of

1. A0: ``"one"``: 1 where any edge (i, j) is present; ``"sum"``: the sum of the
   weights (1 when absent) over the edges (i, j);
2. A1: ``symmetric``: ``max(A0, A0.T)`` (one) or ``A0 + A0.T`` (sum);
3. A2: the diagonal kept, zeroed (``"remove"``) or set to 1 (``"one"``);
4. the entries of A2 that are != 0 after one rounding to float32.

Sums are float64, sequential: the forward contributions in input order, then
the mirrored contributions in input order.  ``ingest_ref_terms`` also returns,
per kept entry, the number of terms and the sum of their magnitudes (for the
reordering bound of a parallel sum).

``dense_pipeline`` is the other yardstick: the reference's way through a dense
(n, n) float32 tensor, written out in torch.
"""
import numpy as np
import torch


def ingest_ref_terms(src, dst, n, weights=None, duplicates="one", symmetric=False, self_loops="keep"):
    assert duplicates in ("one", "sum") and self_loops in ("keep", "remove", "one")
    assert weights is None or duplicates == "sum"
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    assert src.shape == dst.shape and src.ndim == 1
    assert src.size == 0 or (min(src.min(), dst.min()) >= 0 and max(src.max(), dst.max()) < n)
    w = np.ones(src.size, np.float32) if weights is None else np.asarray(weights, dtype=np.float32)
    # contributions in summation order: forward in input order, then mirrored in input order
    rows, cols, ws = src, dst, w
    if symmetric:
        rows, cols, ws = np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([w, w])
    if self_loops != "keep":
        off = rows != cols
        rows, cols, ws = rows[off], cols[off], ws[off]
    acc = {}    # (i, j) -> [float64 sum, terms, sum of magnitudes]
    for i, j, v in zip(rows.tolist(), cols.tolist(), ws.astype(np.float64).tolist()):
        a = acc.setdefault((i, j), [0.0, 0, 0.0])
        a[0] += v
        a[1] += 1
        a[2] += abs(v)
    if duplicates == "one":
        acc = {k: [1.0, 1, 1.0] for k in acc}
    if self_loops == "one":
        for i in range(n):
            acc[(i, i)] = [1.0, 1, 1.0]
    kept = sorted(k for k, a in acc.items() if np.float32(a[0]) != 0)
    indptr = np.zeros(n + 1, np.int64)
    for i, _ in kept:
        indptr[i + 1] += 1
    indptr = np.cumsum(indptr).astype(np.int64)
    indices = np.array([j for _, j in kept], dtype=np.int32)
    values = np.array([acc[k][0] for k in kept], dtype=np.float64).astype(np.float32)
    terms = np.array([acc[k][1] for k in kept], dtype=np.int64)
    mags = np.array([acc[k][2] for k in kept], dtype=np.float64)
    return indptr, indices, values, terms, mags


def ingest_ref(src, dst, n, weights=None, duplicates="one", symmetric=False, self_loops="keep"):
    return ingest_ref_terms(src, dst, n, weights, duplicates, symmetric, self_loops)[:3]


def dense_pipeline(src, dst, n, weights, duplicates, symmetric, self_loops, device="cpu"):
    """zeros -> index assign / index_put_(accumulate) -> + .t() -> clamp -> fill_diagonal_ (float32 dense)."""
    src = torch.as_tensor(src, dtype=torch.int64, device=device)
    dst = torch.as_tensor(dst, dtype=torch.int64, device=device)
    adj = torch.zeros(n, n, dtype=torch.float32, device=device)
    if duplicates == "one":
        adj[src, dst] = 1.0
    else:
        w = torch.ones(src.numel(), device=device) if weights is None else torch.as_tensor(weights, device=device)
        adj.index_put_((src, dst), w.to(torch.float32), accumulate=True)
    if symmetric:
        adj = adj + adj.t()
        if duplicates == "one":
            adj = torch.clamp(adj, 0, 1)
    if self_loops == "remove":
        adj.fill_diagonal_(0.0)
    elif self_loops == "one":
        adj.fill_diagonal_(1.0)
    return adj
