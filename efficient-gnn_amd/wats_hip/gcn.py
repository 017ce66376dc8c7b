"""Sparse propagation for the base model WATS wraps.

The reference base model ``CompatibleGCN`` (``src/gnn/model.py:7-53``) builds
``adj_norm = adj / deg`` with ``deg = adj.sum(dim=1)``, ``deg[deg == 0] = 1``
(``model.py:43-45``) and propagates twice with a dense ``torch.mm(adj_norm,
x)`` (``model.py:47,51``).  That is an O(N^2) dense product per call, paid
every epoch of ``WATS.calib_train`` (``calibration/WATS.py:149`` ->
``WATS.forward`` -> ``base_model(x, adj)``, ``WATS.py:128``).

Here ``adj_norm`` becomes a CSR operator on the HIP library's step kernel
(``wg_rownorm_create`` / ``wg_spmm``, ``csrc/gcn.hip``): y = adj_norm @ x with
float64 row sums.  :class:`RowNormalizedAdjacency` holds the operator, its
transpose, the CSR it was built from and ``deg``; :func:`propagate` is
differentiable w.r.t. ``x`` (backward: ``adj_norm^T @ grad``).
:class:`SparseCompatibleGCN` is ``CompatibleGCN`` with that propagation.  It
has the same constructor, parameter names (``gc1``/``gc2``) and state dict, so
weights move between the two.

Edge gradients.  The calibration attacks take ``d loss / d adj`` through a
dense leaf and read row ``t`` and column ``t`` of it
(``calib_attack/calib_fga.py:864-881``).  For ``y = adj_norm(A) @ x`` with
upstream gradient ``g``::

    d loss / d a_ij = (g_i . x_j  -  g_i . y_i) / deg_i

at every position, stored or not, so the gradient at a list of positions is a
sampled dense-dense product plus a per-row term (``wg_sddmm`` / ``wg_rowdot``,
``csrc/sddmm.hip``).  :class:`EdgeProbe` names the positions and collects the
gradient (``propagate(op, x, probe)``, ``SparseCompatibleGCN.forward(x, adj,
probe=...)``); :func:`target_flip_scores` is the score the attack ranks
(``calib_fga.py:880-881``), :func:`toggle_edges` /
:meth:`RowNormalizedAdjacency.flipped` apply the chosen flip
(``calib_fga.py:901-904``).  A dense ``adj`` leaf that requires grad still
raises: its gradient is the N x N matrix this path exists to avoid.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._lib import check, ptr
from .laplacian import dense_to_csr, require_gpu, stream_handle


class _Op:
    """One wg handle (adj_norm or its transpose), destroyed with the object."""

    def __init__(self, n, indptr, indices, values, transpose: bool, reorder: bool, device):
        lib = _lib.load()
        h = ctypes.c_void_p()
        flags = (_lib.WG_FLAG_TRANSPOSE if transpose else 0) | (0 if reorder else _lib.WG_FLAG_NO_REORDER)
        nnz = int(indices.numel())
        with torch.cuda.device(device):
            check(lib.wg_rownorm_create(n, nnz, ptr(indptr), ptr(indices) if nnz else None,
                                        ptr(values) if (nnz and values is not None) else None, flags,
                                        stream_handle(device), ctypes.byref(h)), "rownorm_create")
        self.h = h
        self.n = n
        self.device = device

    def apply(self, x: torch.Tensor) -> torch.Tensor:
        x = x.to(self.device, torch.float32).contiguous()
        if x.dim() != 2 or x.shape[0] != self.n:
            raise ValueError(f"expected ({self.n}, F) features, got {tuple(x.shape)}")
        y = torch.empty_like(x)
        if x.shape[1] == 0 or self.n == 0:
            return y
        with torch.cuda.device(self.device):
            check(_lib.load().wg_spmm(self.h, x.shape[1], ptr(x), ptr(y), stream_handle(self.device)), "spmm")
        return y

    def __del__(self):
        h = getattr(self, "h", None)
        try:
            if h is not None and _lib._lib is not None:
                _lib._lib.wg_laplacian_destroy(h)
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass
        self.h = None


def sddmm(rows: torch.Tensor, cols: torch.Tensor, A: torch.Tensor, B: torch.Tensor,
          row_term: torch.Tensor | None = None, row_scale: torch.Tensor | None = None,
          validate: bool = True) -> torch.Tensor:
    """``out[p] = row_scale[r] * (A[r] . B[c] - row_term[r])`` with ``r = rows[p]``, ``c = cols[p]``
    (``wg_sddmm``): float64 sums in a fixed order, bitwise reproducible.  ``A`` (n_a, F) and ``B``
    (n_b, F) are float32 device tensors; ``rows`` / ``cols`` int32 with ``rows < n_a``, ``cols < n_b``,
    which ``validate`` checks first (a device reduction and a synchronisation; the kernel itself
    checks ids only in the bounds-checked build)."""
    device = require_gpu(A.device if A.is_cuda else None)
    A = A.to(device, torch.float32).contiguous()
    B = B.to(device, torch.float32).contiguous()
    rows = rows.to(device, torch.int32).contiguous()
    cols = cols.to(device, torch.int32).contiguous()
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[1]:
        raise ValueError(f"expected (n_a, F) and (n_b, F), got {tuple(A.shape)} and {tuple(B.shape)}")
    if rows.dim() != 1 or rows.shape != cols.shape:
        raise ValueError("rows and cols must be 1-D and of equal length")
    for name, t in (("row_term", row_term), ("row_scale", row_scale)):
        if t is not None and (t.dim() != 1 or t.shape[0] != A.shape[0]):
            raise ValueError(f"{name} must have one entry per row of A")
    if row_term is not None:
        row_term = row_term.to(device, torch.float32).contiguous()
    if row_scale is not None:
        row_scale = row_scale.to(device, torch.float32).contiguous()
    out = torch.empty(rows.shape[0], dtype=torch.float32, device=device)
    if rows.shape[0] == 0:
        return out
    if A.shape[1] == 0:
        raise ValueError("sddmm needs at least one column")
    if validate:
        lo = int(torch.minimum(rows.min(), cols.min()))
        if lo < 0 or int(rows.max()) >= A.shape[0] or int(cols.max()) >= B.shape[0]:
            raise ValueError(f"sddmm: a pair lies outside ({A.shape[0]}, {B.shape[0]})")
    with torch.cuda.device(device):
        check(_lib.load().wg_sddmm(rows.shape[0], ptr(rows), ptr(cols), A.shape[1], ptr(A), A.shape[0], ptr(B),
                                   B.shape[0], ptr(row_term), ptr(row_scale), ptr(out), stream_handle(device)),
              "sddmm")
    return out


def rowdot(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """``out[i] = A[i] . B[i]`` (``wg_rowdot``), float64 sums in a fixed order."""
    device = require_gpu(A.device if A.is_cuda else None)
    A = A.to(device, torch.float32).contiguous()
    B = B.to(device, torch.float32).contiguous()
    if A.dim() != 2 or A.shape != B.shape:
        raise ValueError(f"expected two (n, F) tensors, got {tuple(A.shape)} and {tuple(B.shape)}")
    out = torch.empty(A.shape[0], dtype=torch.float32, device=device)
    if A.shape[0] == 0:
        return out
    if A.shape[1] == 0:
        raise ValueError("rowdot needs at least one column")
    with torch.cuda.device(device):
        check(_lib.load().wg_rowdot(A.shape[0], A.shape[1], ptr(A), ptr(B), ptr(out), stream_handle(device)),
              "rowdot")
    return out


def toggle_edges(n: int, indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor | None,
                 rows, cols, symmetric: bool = True):
    """The reference's edge flip (``calib_fga.py:901-904``) on a CSR adjacency, in
    float32 as the reference's dense update: for each pair ``v = 1 - 2 a[r, c]``,
    ``a[r, c] += v`` and, if ``symmetric``, ``a[c, r] += v``.  Pure torch, on the
    device of ``indptr``.  Returns a new ``(indptr int64, indices int32, values
    float32)`` with ascending columns in every row and no stored zero (an entry
    that becomes exactly 0 is dropped, as in the dense matrix).  The input rows
    hold each column at most once.  ``r == c`` or a repeated unordered pair
    raises ``ValueError``: the reference flips one off-diagonal edge at a time."""
    device = indptr.device
    n = int(n)
    indptr = indptr.to(torch.int64)
    if indptr.numel() != n + 1:
        raise ValueError("indptr must have n + 1 entries")
    r = torch.as_tensor(rows, device=device).to(torch.int64).reshape(-1)
    c = torch.as_tensor(cols, device=device).to(torch.int64).reshape(-1)
    if r.shape != c.shape:
        raise ValueError("rows and cols must have the same length")
    if r.numel() and (int(torch.minimum(r.min(), c.min())) < 0 or int(torch.maximum(r.max(), c.max())) >= n):
        raise ValueError(f"pair outside [0, {n})")
    if bool((r == c).any()):
        raise ValueError("toggle_edges: r == c (the attack never flips a self loop, calib_fga.py:897)")
    unordered = torch.minimum(r, c) * n + torch.maximum(r, c)
    if torch.unique(unordered).numel() != unordered.numel():
        raise ValueError("toggle_edges: a pair is repeated")
    row_of = torch.repeat_interleave(torch.arange(n, device=device), indptr[1:] - indptr[:-1])
    keys = row_of * n + indices.to(device=device, dtype=torch.int64)
    vals = (torch.ones(keys.numel(), dtype=torch.float32, device=device) if values is None
            else values.to(device=device, dtype=torch.float32))
    # entries sorted by (row, column), closed by a sentinel (key n * n, value 0) that every miss lands on or before
    sentinel = torch.full((1,), n * n, dtype=torch.int64, device=device)
    keys, order = torch.sort(torch.cat([keys, sentinel]), stable=True)
    vals = torch.cat([vals, torch.zeros(1, dtype=torch.float32, device=device)])[order]

    def lookup(k):
        pos = torch.searchsorted(keys, k)
        return pos, keys[pos] == k

    pos, hit = lookup(r * n + c)
    v = 1 - 2 * torch.where(hit, vals[pos], torch.zeros_like(vals[pos]))    # calib_fga.py:901
    upd_keys, upd_v = r * n + c, v
    if symmetric:
        upd_keys, upd_v = torch.cat([upd_keys, c * n + r]), torch.cat([v, v])
    pos, hit = lookup(upd_keys)                                     # the update keys are distinct
    vals[pos[hit]] += upd_v[hit]                                    # calib_fga.py:903-904
    keys = torch.cat([keys, upd_keys[~hit]])
    vals = torch.cat([vals, upd_v[~hit]])                           # an absent entry is 0: 0 + v
    keep = (vals != 0) & (keys < n * n)
    keys, vals = keys[keep], vals[keep]
    keys, order = torch.sort(keys)
    vals = vals[order]
    new_rows = torch.div(keys, n, rounding_mode="floor") if n else keys
    new_indptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
    new_indptr[1:] = torch.cumsum(torch.bincount(new_rows, minlength=n), 0)
    return new_indptr, (keys - new_rows * n).to(torch.int32), vals


class RowNormalizedAdjacency:
    """``adj_norm = adj / deg`` of ``CompatibleGCN.forward`` (model.py:43-45)
    as a device CSR operator plus its transpose.  Keeps the CSR of ``adj`` it
    was built from (``indptr``, ``indices``, ``values``; ``values`` None = all
    ones) and ``deg`` (float32; float64 row sums, 0 -> 1) for the edge
    gradients and :meth:`flipped`."""

    def __init__(self, n: int, indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor | None = None,
                 reorder: bool = True, device=None):
        device = require_gpu(device if device is not None else (indptr.device if indptr.is_cuda else None))
        self.device = device
        indptr = indptr.to(device=device, dtype=torch.int64).contiguous()
        indices = indices.to(device=device, dtype=torch.int32).contiguous()
        if values is not None:
            values = values.to(device=device, dtype=torch.float32).contiguous()
        if indptr.numel() != n + 1:
            raise ValueError("indptr must have n + 1 entries")
        self.n = int(n)
        self.nnz = int(indices.numel())
        self.reorder = bool(reorder)
        self.indptr, self.indices, self.values = indptr, indices, values
        if values is None:
            deg = (indptr[1:] - indptr[:-1]).to(torch.float32)
        else:   # one sequential float64 sum per row: the same on every run
            deg = torch.segment_reduce(values.to(torch.float64), "sum", offsets=indptr).to(torch.float32)
        self.deg = torch.where(deg == 0, torch.ones_like(deg), deg)
        self.inv_deg = 1.0 / self.deg
        self.fwd = _Op(self.n, indptr, indices, values, False, reorder, device)
        self.bwd = _Op(self.n, indptr, indices, values, True, reorder, device)

    def flipped(self, rows, cols, symmetric: bool = True) -> "RowNormalizedAdjacency":
        """A new operator for the adjacency after :func:`toggle_edges` (``calib_fga.py:901-904``)."""
        indptr, indices, values = toggle_edges(self.n, self.indptr, self.indices, self.values, rows, cols, symmetric)
        return RowNormalizedAdjacency(self.n, indptr, indices, values, reorder=self.reorder, device=self.device)

    def with_flips(self, rows, cols, symmetric: bool = True, self_loops: bool = False):
        """The same flip as a view (``wats_hip.flips.FlippedAdjacency``): this operator's handles plus an
        overlay of the flipped positions, for a candidate that is propagated once or twice
        (``calib_fga.py:901-913``).  ``view.materialize()`` builds the real operator.  ``self_loops=True``
        admits pairs ``r == c``, refused otherwise."""
        require_gpu(getattr(self, "device", None))
        from .flips import FlippedAdjacency
        return FlippedAdjacency.compose(self, None, rows, cols, symmetric, self_loops)

    def dense_row(self, t: int) -> torch.Tensor:
        """Row ``t`` of ``adj`` as a dense float32 vector of length n."""
        s, e = (int(v) for v in self.indptr[t:t + 2])
        row = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        row[self.indices[s:e].long()] = 1.0 if self.values is None else self.values[s:e]
        return row

    @classmethod
    def from_dense(cls, adj: torch.Tensor, **kw):
        """From the dense (N, N) adjacency the reference model receives
        (on-device compaction, entries != 0 kept)."""
        if adj.dim() != 2 or adj.shape[0] != adj.shape[1]:
            raise ValueError("adjacency must be square")
        indptr, indices, values = dense_to_csr(adj)
        return cls(adj.shape[0], indptr, indices, values, device=indptr.device, **kw)

    @classmethod
    def from_scipy(cls, A, **kw):
        import numpy as np
        import scipy.sparse as sp
        A = sp.csr_matrix(A)
        return cls(A.shape[0], torch.from_numpy(A.indptr.astype(np.int64)),
                   torch.from_numpy(A.indices.astype(np.int32)), torch.from_numpy(A.data.astype(np.float32)), **kw)

    @classmethod
    def from_graph(cls, g, **kw):
        """From a ``wats_hip.graphgen.CSRGraph`` or a ``wats_hip.ingest.DeviceCSR``."""
        import numpy as np
        to_t = lambda a, dt: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=dt))
        return cls(g.n, to_t(g.indptr, np.int64), to_t(g.indices, np.int32),
                   None if g.values is None else to_t(g.values, np.float32), **kw)

    @classmethod
    def from_edge_index(cls, edge_index, num_nodes: int | None = None, weights=None, *, duplicates: str = "one",
                        symmetric: bool = False, self_loops: str = "keep", convention: str | None = None, **kw):
        """From a (2, E) ``edge_index``, ingested on the device (``wats_hip.ingest.edge_index_to_csr``)."""
        from .ingest import edge_index_to_csr
        g = edge_index_to_csr(edge_index, num_nodes, weights, duplicates=duplicates, symmetric=symmetric,
                              self_loops=self_loops, convention=convention, device=kw.get("device"))
        return cls.from_graph(g, **kw)

    def __matmul__(self, x: torch.Tensor) -> torch.Tensor:
        return propagate(self, x)


class _Propagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, op):
        ctx.op = op
        return op.fwd.apply(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.op.bwd.apply(g), None


class EdgeProbe:
    """Positions ``(rows[p], cols[p])`` of the adjacency, present or absent in the
    graph, at which a gradient is wanted.  The probe stands for
    ``A + sum_p delta_p e_r e_c^T`` at ``delta = 0``: ``delta`` is a float32 zero
    leaf of length P, and every propagation that is given the probe adds
    ``d loss / d a[rows[p], cols[p]]`` to ``delta.grad`` through autograd
    (``loss.backward()`` or ``torch.autograd.grad(loss, probe.delta)``).
    ``rows`` / ``cols`` are in the caller's numbering; a position may repeat."""

    def __init__(self, rows, cols, device=None):
        device = require_gpu(device)
        self.device = device
        self.rows = torch.as_tensor(rows).to(device=device, dtype=torch.int32).reshape(-1).contiguous()
        self.cols = torch.as_tensor(cols).to(device=device, dtype=torch.int32).reshape(-1).contiguous()
        if self.rows.shape != self.cols.shape:
            raise ValueError("rows and cols must have the same length")
        self.delta = torch.zeros(self.rows.shape[0], dtype=torch.float32, device=device, requires_grad=True)
        self.target = None      # (n, t) of for_target
        self._checked_n = None

    @classmethod
    def for_target(cls, n: int, t: int, device=None) -> "EdgeProbe":
        """The 2n positions the attack reads (``calib_fga.py:881``): ``(t, j)`` for
        ``j = 0..n-1`` (row ``t`` of the gradient), then ``(i, t)`` for ``i = 0..n-1`` (column ``t``)."""
        n, t = int(n), int(t)
        if not 0 <= t < n:
            raise ValueError(f"target {t} outside [0, {n})")
        ids = torch.arange(n, dtype=torch.int32)
        tt = torch.full((n,), t, dtype=torch.int32)
        probe = cls(torch.cat([tt, ids]), torch.cat([ids, tt]), device=device)
        probe.target = (n, t)
        return probe

    def __len__(self) -> int:
        return self.rows.shape[0]

    @property
    def grad(self):
        return self.delta.grad

    def zero_grad(self) -> None:
        self.delta.grad = None

    def check(self, n: int) -> None:
        """Every position lies inside an (n, n) adjacency (one device reduction, cached per n)."""
        if self._checked_n == n or len(self) == 0:
            return
        lo = int(torch.minimum(self.rows.min(), self.cols.min()))
        hi = int(torch.maximum(self.rows.max(), self.cols.max()))
        if lo < 0 or hi >= n:
            raise ValueError(f"EdgeProbe position outside [0, {n})")
        self._checked_n = n


class _ProbePropagate(torch.autograd.Function):
    """The same SpMM as :class:`_Propagate`, and in the backward the gradient at the probe's
    positions: ``(g_r . x_c - g_r . y_r) / deg_r``, with ``g . y`` per row from ``wg_rowdot``."""

    @staticmethod
    def forward(ctx, x, delta, op, probe):
        ctx.op, ctx.probe = op, probe
        y = op.fwd.apply(x)
        ctx.save_for_backward(x.to(op.device, torch.float32), y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        op, probe = ctx.op, ctx.probe
        x, y = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        gx = op.bwd.apply(g) if ctx.needs_input_grad[0] else None
        gd = None
        if ctx.needs_input_grad[1]:
            if g.shape[1] == 0:
                gd = torch.zeros(len(probe), dtype=torch.float32, device=op.device)
            else:
                gd = sddmm(probe.rows, probe.cols, g, x, row_term=rowdot(g, y), row_scale=op.inv_deg,
                           validate=False)    # propagate() checked the probe against op.n
        return gx, gd, None, None


def propagate(op: RowNormalizedAdjacency, x: torch.Tensor, probe: EdgeProbe | None = None) -> torch.Tensor:
    """``adj_norm @ x`` (model.py:47, 51), differentiable w.r.t. ``x`` and, with a
    ``probe``, w.r.t. the adjacency at the probe's positions."""
    if probe is None:
        return _Propagate.apply(x, op)
    if probe.device != op.device:
        raise ValueError(f"probe on {probe.device}, operator on {op.device}")
    probe.check(op.n)
    return _ProbePropagate.apply(x, probe.delta, op, probe)


def target_flip_scores(probe: EdgeProbe, op: RowNormalizedAdjacency, t: int) -> torch.Tensor:
    """``(grad[t, :] + grad[:, t]) * (1 - 2 A[t, :])`` (``calib_fga.py:880-881``), length n,
    from the gradient collected by ``EdgeProbe.for_target(n, t)``: the attack flips its argmax."""
    if probe.target != (op.n, int(t)):
        raise ValueError(f"target_flip_scores needs EdgeProbe.for_target({op.n}, {int(t)})")
    if probe.grad is None:
        raise ValueError("the probe has no gradient yet: run backward() through a model given probe=")
    return target_scores_from_grad(probe.grad, op, t)


def target_scores_from_grad(grad: torch.Tensor, op: RowNormalizedAdjacency, t: int) -> torch.Tensor:
    """The same score from a ``for_target`` gradient vector held elsewhere, e.g. the result of
    ``torch.autograd.grad(loss, probe.delta, retain_graph=True)`` (``calib_fga.py:877-890``)."""
    n = op.n
    if grad.shape != (2 * n,):
        raise ValueError(f"expected a gradient of length {2 * n}")
    return (grad[:n] + grad[n:]) * (1 - 2 * op.dense_row(int(t)))


class SparseCompatibleGCN(nn.Module):
    """``CompatibleGCN`` (reference ``src/gnn/model.py:7-53``) with the two
    propagations on the HIP SpMM.  Same constructor, parameters and state dict.

    ``forward(x, adj)`` accepts the dense adjacency the reference takes (the
    CSR operator is built once and cached while ``adj`` is unchanged) or a
    :class:`RowNormalizedAdjacency`.  ``probe`` (an :class:`EdgeProbe`) is
    given to both propagations, which accumulate the gradient w.r.t. the
    adjacency at its positions into ``probe.grad``."""

    DATASET_CLASSES = {
        'cora': 7, 'citeseer': 6, 'pubmed': 3, 'reddit': 41, 'amazon-computers': 10, 'amazon-photo': 8,
        'coauthor-cs': 15, 'coauthor-physics': 5, 'dblp': 4, 'ogbn-arxiv': 40,
    }

    def __init__(self, nfeat: int, dataset_name: str = None, nclass: int = None, nhid: int = 64,
                 dropout: float = 0.5):
        super().__init__()
        if dataset_name and dataset_name.lower() in self.DATASET_CLASSES:
            nclass = self.DATASET_CLASSES[dataset_name.lower()]
        elif nclass is None:
            raise ValueError("Either dataset_name or nclass must be provided")
        self.gc1 = nn.Linear(nfeat, nhid)
        self.gc2 = nn.Linear(nhid, nclass)
        self.dropout = nn.Dropout(dropout)
        self._op_key = None
        self._op = None

    def operator(self, adj) -> RowNormalizedAdjacency:
        if isinstance(adj, RowNormalizedAdjacency):
            return adj
        if adj.requires_grad:
            raise NotImplementedError("SparseCompatibleGCN has no gradient w.r.t. a dense adj leaf (N x N); pass "
                                      "probe=EdgeProbe(rows, cols) for the gradient at edge positions, or use "
                                      "the dense CompatibleGCN")
        key = (adj.data_ptr(), tuple(adj.shape), adj._version, str(adj.device))
        if self._op is None or self._op_key != key:
            device = next(self.parameters()).device
            self._op = RowNormalizedAdjacency.from_dense(adj.to(device))
            self._op_key = key
        return self._op

    def forward(self, x: torch.Tensor, adj, probe: EdgeProbe | None = None) -> torch.Tensor:
        device = next(self.parameters()).device
        x = x.to(device)
        op = self.operator(adj)
        x = propagate(op, x, probe)         # model.py:47
        x = F.relu(self.gc1(x))             # model.py:48
        x = self.dropout(x)                 # model.py:49
        x = propagate(op, x, probe)         # model.py:51
        return self.gc2(x)                  # model.py:52
