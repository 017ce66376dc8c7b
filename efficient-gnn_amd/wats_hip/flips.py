"""Edge-flip views of the base model's propagation.

One iteration of the reference attacks scores the candidate edges, flips one
(``calib_attack/calib_fga.py:901-904``: ``v = 1 - 2 adj[r, c]``, ``adj[r, c] +=
v``, ``adj[c, r] += v``) and evaluates the model on the flipped graph
(``calib_fga.py:905-913``).  The flipped adjacency A' differs from its parent A
in two rows, so :class:`FlippedAdjacency` keeps the parent
:class:`~wats_hip.gcn.RowNormalizedAdjacency` -- its two operators and its CSR
-- and carries the flips as an overlay: the distinct positions where A' != A
bitwise, sorted by (row, column), each with ``a_old`` (A's entry, 0 if absent),
``a_new`` and ``base_pos`` (its index in A's ``indices``, or -1).

* forward ``adj_norm(A') @ x``: the parent's ``wg_spmm``, then the touched rows
  recomputed from the parent's row and the overlay (``wg_flip_rows``);
* backward ``adj_norm(A')^T @ g``: the parent's transposed ``wg_spmm`` on ``g``
  with each touched row scaled by ``deg / deg'``, then per overlay column
  ``+ sum ((a_new - a_old) / deg') g_r`` (``wg_flip_cols``); a removed entry
  cancels to rounding, not to an exact zero;
* ``deg' = float32(s + sum(double(a_new) - double(a_old)))`` with ``s`` the
  float64 sum of the parent's row (``wg_flip_resolve``), 0 -> 1;
* :meth:`FlippedAdjacency.csr` commits the overlay to the canonical CSR of A'
  in one streaming pass (``wg_csr_patch``), bit for bit what
  :func:`~wats_hip.gcn.toggle_edges` returns for the same calls.

A view is a ``RowNormalizedAdjacency`` to everything that takes one
(``propagate``, ``SparseCompatibleGCN``, ``EdgeProbe`` gradients,
``target_flip_scores``, ``WATS.forward``).  The kernels are in
``csrc/flips.hip``; the overlay's bookkeeping (at most a few positions per
flip) is host torch.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import check, ptr
from .gcn import RowNormalizedAdjacency
from .ingest import DeviceCSR
from .laplacian import require_gpu, stream_handle


def _nbytes(t: torch.Tensor) -> int:
    return (t.numel() * t.element_size() + 15) // 16 * 16


def _upload(device, arrays: dict) -> dict:
    """The 1-D host tensors as views of one device buffer (one copy), each 16-byte aligned."""
    offs, total = {}, 0
    for k, t in arrays.items():
        offs[k] = total
        total += _nbytes(t)
    host = torch.zeros(max(total, 16), dtype=torch.uint8)
    for k, t in arrays.items():
        nb = t.numel() * t.element_size()
        if nb:
            host[offs[k]:offs[k] + nb] = t.contiguous().view(torch.uint8)
    dev = host.to(device)
    return {k: dev[offs[k]:offs[k] + t.numel() * t.element_size()].view(t.dtype) for k, t in arrays.items()}


def _pairs(n: int, rows, cols, self_loops: bool = False):
    """The pairs of one flip call as host int64 tensors, validated as ``toggle_edges`` validates them
    (``self_loops``: a pair ``r == c`` is taken and flips the one diagonal entry)."""
    r = torch.as_tensor(rows).detach().cpu().to(torch.int64).reshape(-1)
    c = torch.as_tensor(cols).detach().cpu().to(torch.int64).reshape(-1)
    if r.shape != c.shape:
        raise ValueError("rows and cols must have the same length")
    if r.numel() and (int(torch.minimum(r.min(), c.min())) < 0 or int(torch.maximum(r.max(), c.max())) >= n):
        raise ValueError(f"pair outside [0, {n})")
    if not self_loops and bool((r == c).any()):
        raise ValueError("with_flips: r == c (the attack never flips a self loop, calib_fga.py:897)")
    unordered = torch.minimum(r, c) * n + torch.maximum(r, c)
    if torch.unique(unordered).numel() != unordered.numel():
        raise ValueError("with_flips: a pair is repeated")
    return r, c


def _segments(ids: torch.Tensor):
    """(distinct values, offsets [k + 1], segment of each element) of a sorted host id vector."""
    uniq, counts = torch.unique_consecutive(ids, return_counts=True)
    seg = torch.zeros(uniq.numel() + 1, dtype=torch.int64)
    seg[1:] = torch.cumsum(counts, 0)
    return uniq, seg, torch.repeat_interleave(torch.arange(uniq.numel()), counts)


class _FlipOp:
    """``adj_norm(A')`` or its transpose: the parent's handle, then the fix-up kernel."""

    def __init__(self, view: "FlippedAdjacency", transpose: bool):
        self.view, self.transpose = view, transpose
        self.n, self.device = view.n, view.device

    def apply(self, x: torch.Tensor) -> torch.Tensor:
        v = self.view
        x = x.to(self.device, torch.float32).contiguous()
        if x.dim() != 2 or x.shape[0] != self.n:
            raise ValueError(f"expected ({self.n}, F) features, got {tuple(x.shape)}")
        F = int(x.shape[1])
        if v.n_positions == 0 or F == 0:
            return (v.base.bwd if self.transpose else v.base.fwd).apply(x)
        lib, d = _lib.load(), v._dev
        if not self.transpose:
            y = v.base.fwd.apply(x)
            with torch.cuda.device(self.device):
                check(lib.wg_flip_rows(v.n, ptr(v.base.indptr), ptr(v.base.indices) if v.base.nnz else None,
                                       ptr(v.base.values), v.n_touched, ptr(d["t_rows"]), ptr(d["seg"]),
                                       v.n_positions, ptr(d["cols"]), ptr(d["a_new"]), ptr(d["base_pos"]),
                                       ptr(d["deg_new"]), F, ptr(x), ptr(y), stream_handle(self.device)), "flip_rows")
            return y
        # every parent entry of a touched row becomes a / deg'
        g = x.clone()
        g[d["t_rows64"]] = (x[d["t_rows64"]].double() * v._scale.unsqueeze(1)).to(torch.float32)
        gx = v.base.bwd.apply(g)
        with torch.cuda.device(self.device):
            check(lib.wg_flip_cols(v.n, int(d["c_cols"].numel()), ptr(d["c_cols"]), ptr(d["cseg"]), v.n_positions,
                                   ptr(d["c_rows"]), ptr(d["c_a_new"]), ptr(d["c_a_old"]), ptr(d["c_deg"]), F, ptr(x),
                                   ptr(gx), stream_handle(self.device)), "flip_cols")
        return gx


class FlippedAdjacency(RowNormalizedAdjacency):
    """``adj_norm`` of a :class:`RowNormalizedAdjacency` after edge flips, as a view: no handle is
    built.  Made by :meth:`RowNormalizedAdjacency.with_flips`; ``with_flips`` on a view composes
    onto the same parent.

    ``base`` is the parent (shared, kept alive); ``ov_rows`` / ``ov_cols`` (int32), ``a_old`` /
    ``a_new`` (float32) and ``base_pos`` (int64) are the overlay, sorted by (row, column);
    ``n_positions`` its length.  Memory: the overlay, and two n-float vectors once ``deg`` /
    ``inv_deg`` are read."""

    def __init__(self, base: RowNormalizedAdjacency, keys, a_old, a_new, base_pos, row_sum):
        """Host tensors of one overlay (already reduced to the positions where a_new != a_old bitwise):
        keys = row * n + col ascending, row_sum = the parent's float64 row sum at each position's row."""
        self.base = base
        self.n, self.device, self.reorder = base.n, base.device, base.reorder
        n = self.n
        self._keys, self._a_old, self._a_new, self._base_pos, self._row_sum = keys, a_old, a_new, base_pos, row_sum
        rows = torch.div(keys, n, rounding_mode="floor") if n else keys
        cols = keys - rows * n
        self._rows, self._cols = rows, cols
        self.n_positions = int(keys.numel())
        inserts = int(((base_pos < 0) & (a_new != 0)).sum())
        deletes = int(((base_pos >= 0) & (a_new == 0)).sum())
        self.nnz = base.nnz + inserts - deletes
        self._csr = None
        self._deg = self._inv_deg = None
        self.fwd, self.bwd = _FlipOp(self, False), _FlipOp(self, True)
        t_rows, seg, seg_of = _segments(rows)
        self.n_touched = int(t_rows.numel())
        if self.n_positions == 0:
            empty = lambda dt: torch.empty(0, dtype=dt, device=self.device)
            self._dev = dict(t_rows64=empty(torch.int64), deg_new=empty(torch.float32))
            self.ov_rows, self.ov_cols = empty(torch.int32), empty(torch.int32)
            self.a_old, self.a_new, self.base_pos = empty(torch.float32), empty(torch.float32), empty(torch.int64)
            return
        # deg' = float32(s + sum(double(a_new) - double(a_old))), one sequential sum per row
        diff = torch.segment_reduce(a_new.double() - a_old.double(), "sum", offsets=seg)
        deg_new = (row_sum[seg[:-1]] + diff).to(torch.float32)
        deg_new[deg_new == 0] = 1.0
        # the same positions by (column, row) for the backward
        order = torch.argsort(cols * n + rows)
        c_cols, cseg, _ = _segments(cols[order])
        self._dev = _upload(self.device, dict(
            t_rows=t_rows.to(torch.int32), seg=seg, rows=rows.to(torch.int32), cols=cols.to(torch.int32), a_new=a_new,
            a_old=a_old, base_pos=base_pos, deg_new=deg_new, t_rows64=t_rows, c_cols=c_cols.to(torch.int32), cseg=cseg,
            c_rows=rows[order].to(torch.int32), c_a_new=a_new[order], c_a_old=a_old[order],
            c_deg=deg_new[seg_of][order]))
        d = self._dev
        self.ov_rows, self.ov_cols = d["rows"], d["cols"]
        self.a_old, self.a_new, self.base_pos = d["a_old"], d["a_new"], d["base_pos"]
        self._scale = base.deg[d["t_rows64"]].double() / d["deg_new"].double()

    # ------------------------------------------------------------------ construction
    @classmethod
    def compose(cls, base: RowNormalizedAdjacency, prev: "FlippedAdjacency | None", rows, cols,
                symmetric: bool = True, self_loops: bool = False) -> "FlippedAdjacency":
        """``prev`` (a view of ``base``, or None for ``base`` itself) after one more flip call.  ``self_loops``
        admits pairs ``r == c`` (the random attacks remove a target's self loop, ``calib_random.py:386-390``): the
        two positions of such a pair are one, flipped once."""
        device = require_gpu(base.device)
        n = base.n
        r, c = _pairs(n, rows, cols, self_loops)
        k_rc, k_cr = r * n + c, c * n + r
        old_keys = prev._keys if prev is not None else torch.empty(0, dtype=torch.int64)
        keys = torch.unique(torch.cat([old_keys, k_rc, k_cr] if symmetric else [old_keys, k_rc]))  # ascending
        P = int(keys.numel())
        if P == 0:
            z = lambda dt: torch.empty(0, dtype=dt)
            return cls(base, keys, z(torch.float32), z(torch.float32), z(torch.int64), z(torch.float64))
        # the parent's entry, its index and the parent's row sums at every position (wg_flip_resolve)
        u_rows = torch.div(keys, n, rounding_mode="floor")
        t_rows, seg, seg_of = _segments(u_rows)
        T = int(t_rows.numel())
        d = _upload(device, dict(t_rows=t_rows.to(torch.int32), seg=seg, cols=(keys - u_rows * n).to(torch.int32)))
        out = torch.empty(16 * P + 8 * T, dtype=torch.uint8, device=device)
        base_pos, row_sum, a_old = out[:8 * P].view(torch.int64), out[8 * P:8 * (P + T)].view(torch.float64), \
            out[8 * (P + T):8 * (P + T) + 4 * P].view(torch.float32)
        with torch.cuda.device(device):
            check(_lib.load().wg_flip_resolve(n, ptr(base.indptr), ptr(base.indices) if base.nnz else None,
                                              ptr(base.values), T, ptr(d["t_rows"]), ptr(d["seg"]), P, ptr(d["cols"]),
                                              ptr(a_old), ptr(base_pos), ptr(row_sum), stream_handle(device)),
                  "flip_resolve")
        host = out.cpu()
        base_pos, row_sum, a_old = host[:8 * P].view(torch.int64), host[8 * P:8 * (P + T)].view(torch.float64), \
            host[8 * (P + T):8 * (P + T) + 4 * P].view(torch.float32)
        # A_cur: the parent read through the previous overlay
        a_cur = a_old.clone()
        if prev is not None and prev.n_positions:
            a_cur[torch.searchsorted(keys, prev._keys)] = prev._a_new
        a_new = a_cur.clone()
        if r.numel():
            i_rc = torch.searchsorted(keys, k_rc)
            v = 1 - 2 * a_cur[i_rc]                                 # calib_fga.py:901
            a_new[i_rc] = a_cur[i_rc] + v                           # calib_fga.py:903 (the positions are distinct)
            if symmetric:
                i_cr = torch.searchsorted(keys, k_cr)
                a_new[i_cr] = a_cur[i_cr] + v                       # calib_fga.py:904
        keep = a_new.view(torch.int32) != a_old.view(torch.int32)   # a position back at the parent's bits leaves
        return cls(base, keys[keep], a_old[keep].contiguous(), a_new[keep].contiguous(), base_pos[keep].contiguous(),
                   row_sum[seg_of][keep].contiguous())

    def with_flips(self, rows, cols, symmetric: bool = True, self_loops: bool = False) -> "FlippedAdjacency":
        """This view after one more flip call (``calib_fga.py:901-904``), on the same parent."""
        return FlippedAdjacency.compose(self.base, self, rows, cols, symmetric, self_loops)

    def flipped(self, rows, cols, symmetric: bool = True) -> RowNormalizedAdjacency:
        return self.with_flips(rows, cols, symmetric).materialize()

    # ------------------------------------------------------------------ what an operator carries
    @property
    def deg(self) -> torch.Tensor:
        if self._deg is None:
            self._deg = self.base.deg.clone()
            self._deg[self._dev["t_rows64"]] = self._dev["deg_new"]
        return self._deg

    @property
    def inv_deg(self) -> torch.Tensor:
        if self._inv_deg is None:
            self._inv_deg = 1.0 / self.deg
        return self._inv_deg

    def dense_row(self, t: int) -> torch.Tensor:
        """Row ``t`` of the flipped ``adj`` as a dense float32 vector of length n."""
        row = self.base.dense_row(t)
        sel = self._rows == int(t)
        if bool(sel.any()):
            row[self._cols[sel].to(self.device)] = self._a_new[sel].to(self.device)
        return row

    def csr(self):
        """``(indptr int64, indices int32, values float32)`` of the flipped adjacency: columns ascending, no
        stored zero, bit for bit the chained :func:`toggle_edges` result (``wg_csr_patch``; cached)."""
        if self._csr is not None:
            return self._csr
        base, device = self.base, self.device
        if self.n_positions == 0:
            ones = torch.ones(base.nnz, dtype=torch.float32, device=device)
            self._csr = (base.indptr, base.indices, base.values if base.values is not None else ones)
            return self._csr
        d, capacity = self._dev, base.nnz + self.n_positions
        indptr = torch.empty(self.n + 1, dtype=torch.int64, device=device)
        indices = torch.empty(capacity, dtype=torch.int32, device=device)
        values = torch.empty(capacity, dtype=torch.float32, device=device)
        nnz = ctypes.c_int64(0)
        with torch.cuda.device(device):
            check(_lib.load().wg_csr_patch(self.n, base.nnz, ptr(base.indptr), ptr(base.indices) if base.nnz else None,
                                           ptr(base.values), self.n_touched, ptr(d["t_rows"]), ptr(d["seg"]),
                                           self.n_positions, ptr(d["cols"]), ptr(d["a_new"]), ptr(d["base_pos"]),
                                           ptr(indptr), ptr(indices), ptr(values), capacity, ctypes.byref(nnz),
                                           stream_handle(device)), "csr_patch")
        if nnz.value != self.nnz:
            raise _lib.WaveletError(f"wats_hip csr_patch: {nnz.value} entries, the overlay says {self.nnz}")
        self._csr = (indptr, indices[:nnz.value], values[:nnz.value])
        return self._csr

    indptr = property(lambda self: self.csr()[0])
    indices = property(lambda self: self.csr()[1])
    values = property(lambda self: self.csr()[2])

    def to_graph(self) -> DeviceCSR:
        """The flipped adjacency as a :class:`DeviceCSR`; ``values`` is None when the parent had none and
        every flipped entry is 0 or 1 (a Laplacian built from it stays on the value-free kernels)."""
        indptr, indices, values = self.csr()
        unit = self.base.values is None and bool(((self._a_new == 0) | (self._a_new == 1)).all())
        return DeviceCSR(self.n, indptr, indices, None if unit else values)

    def materialize(self) -> RowNormalizedAdjacency:
        """A real operator of :meth:`csr` (for an adjacency that will be propagated many times)."""
        indptr, indices, values = self.csr()
        return RowNormalizedAdjacency(self.n, indptr, indices, values, reorder=self.reorder, device=self.device)
