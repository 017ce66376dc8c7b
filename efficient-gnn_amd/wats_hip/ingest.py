"""Device-side graph ingestion: ``edge_index`` (COO) -> canonical CSR.

The reference turns ``edge_index`` into a dense (N, N) adjacency --
``adj[src, dst] = 1`` (``calibration/utils.py:19-25`` via
``benchmark_calibration_methods.py:53``) or ``clamp(adj + adj.t(), 0, 1)`` with
``fill_diagonal_(1.0)`` (``ugca_calib_attack.py:42-47``) -- and gives it up
above 50 000 nodes (``exp/ablation/ugca_full_multi_dataset.py:128-133``).
:func:`edge_index_to_csr` builds the CSR of the same matrix from the ids on
the GPU (``csrc/ingest.hip``): no dense tensor, no host scipy.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .laplacian import require_gpu, stream_handle

# convention -> (duplicates, symmetric, self_loops)
CONVENTIONS = {
    "harness": ("one", False, "keep"),   # calibration/utils.py:19-25
    "attack": ("one", True, "one"),      # ugca_calib_attack.py:42-47
}
_LOOP_FLAGS = {"keep": 0, "remove": _lib.WG_COO_LOOPS_REMOVE, "one": _lib.WG_COO_LOOPS_ONE}


class DeviceCSR:
    """A canonical CSR adjacency on the GPU: ``indptr`` int64 (n + 1,),
    ``indices`` int32 ascending in each row, ``values`` float32 or None (all
    ones).  Carries the attribute names of ``graphgen.CSRGraph``, so
    ``graph_wavelet_features(g)``, ``WATS(..., graph=g)`` and the operators'
    ``from_graph`` accept it as it is."""

    def __init__(self, n: int, indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor | None = None):
        self.n = int(n)
        self.indptr, self.indices, self.values = indptr, indices, values
        self.nnz = int(indices.numel())

    @property
    def device(self) -> torch.device:
        return self.indptr.device

    def to_scipy(self):
        import scipy.sparse as sp
        vals = np.ones(self.nnz, np.float32) if self.values is None else self.values.cpu().numpy()
        return sp.csr_matrix((vals, self.indices.cpu().numpy(), self.indptr.cpu().numpy()), shape=(self.n, self.n))

    def to_dense(self) -> torch.Tensor:
        """The (n, n) float32 adjacency on the device (small graphs only)."""
        rows = torch.repeat_interleave(torch.arange(self.n, device=self.device), self.indptr[1:] - self.indptr[:-1])
        out = torch.zeros(self.n, self.n, dtype=torch.float32, device=self.device)
        out[rows, self.indices.long()] = 1.0 if self.values is None else self.values
        return out

    def __repr__(self):
        return (f"DeviceCSR(n={self.n}, nnz={self.nnz}, "
                f"values={'None' if self.values is None else 'float32'}, device={self.device})")


def edge_index_to_csr(edge_index, num_nodes: int | None = None, weights=None, *, duplicates: str = "one",
                      symmetric: bool = False, self_loops: str = "keep", convention: str | None = None,
                      device=None) -> DeviceCSR:
    """The CSR of the adjacency that ``edge_index`` (2, E) describes, defined by its dense equivalent:

    1. ``duplicates="one"``: ``A[i, j] = 1`` if any edge (i, j) is present;
       ``"sum"``: the sum of ``weights`` (1 when absent) over the edges (i, j).
    2. ``symmetric``: ``max(A, A.T)`` (= ``clamp(adj + adj.t(), 0, 1)``) in mode
       ``"one"``, ``A + A.T`` in mode ``"sum"`` (the diagonal doubles).
    3. ``self_loops``: ``"keep"``, ``"remove"`` (diagonal 0) or ``"one"``
       (``fill_diagonal_(1.0)``).
    4. the entries != 0, columns ascending in each row; ``values`` is None in
       mode ``"one"``.

    ``convention="harness"`` is one / not symmetric / keep, ``"attack"`` one /
    symmetric / one.  Sums are float64 -- forward contributions in input order,
    then the mirrored ones in input order -- rounded once to float32: the same
    input gives the same bits.  ``edge_index`` is an int32 or int64 tensor (CPU
    or GPU, any strides) or numpy array; ``num_nodes=None`` means max id + 1.
    """
    if convention is not None:
        if convention not in CONVENTIONS:
            raise ValueError(f"convention must be one of {sorted(CONVENTIONS)}, not {convention!r}")
        duplicates, symmetric, self_loops = CONVENTIONS[convention]
    if duplicates not in ("one", "sum"):
        raise ValueError(f"duplicates must be 'one' or 'sum', not {duplicates!r}")
    if self_loops not in _LOOP_FLAGS:
        raise ValueError(f"self_loops must be 'keep', 'remove' or 'one', not {self_loops!r}")
    if weights is not None and duplicates == "one":
        raise ValueError("weights need duplicates='sum'")
    if isinstance(edge_index, np.ndarray):
        edge_index = torch.from_numpy(edge_index)
    if not isinstance(edge_index, torch.Tensor):
        raise ValueError("edge_index must be a torch tensor or a numpy array")
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must have shape (2, E), not {tuple(edge_index.shape)}")
    if edge_index.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"edge_index must be int32 or int64, not {edge_index.dtype}")
    device = require_gpu(device if device is not None else (edge_index.device if edge_index.is_cuda else None))
    n_edges = int(edge_index.shape[1])
    src = edge_index[0].to(device).contiguous()
    dst = edge_index[1].to(device).contiguous()
    if weights is not None:
        if isinstance(weights, np.ndarray):
            weights = torch.from_numpy(weights)
        if weights.dim() != 1 or weights.numel() != n_edges:
            raise ValueError(f"weights must have shape ({n_edges},), not {tuple(weights.shape)}")
        weights = weights.to(device=device, dtype=torch.float32).contiguous()
    if num_nodes is None:
        num_nodes = int(torch.maximum(src.max(), dst.max())) + 1 if n_edges else 0
    n = int(num_nodes)
    if n < 0:
        raise ValueError(f"num_nodes must be >= 0, not {n}")
    flags = _LOOP_FLAGS[self_loops] | (_lib.WG_COO_SYMMETRIC if symmetric else 0)
    flags |= _lib.WG_COO_SUM if duplicates == "sum" else 0
    lib = _lib.load()
    cap = ctypes.c_int64(0)
    check(lib.wg_coo_capacity(n, n_edges, flags, ctypes.byref(cap)), "coo_capacity")
    capacity = cap.value
    indptr = torch.empty(n + 1, dtype=torch.int64, device=device)
    indices = torch.empty(max(capacity, 1), dtype=torch.int32, device=device)
    values = torch.empty(max(capacity, 1), dtype=torch.float32, device=device) if duplicates == "sum" else None
    nnz = ctypes.c_int64(0)
    with torch.cuda.device(device):
        rc = lib.wg_coo_to_csr(n, n_edges, ptr(src) if n_edges else None, ptr(dst) if n_edges else None,
                               src.element_size(), ptr(weights), flags, ptr(indptr), ptr(indices), ptr(values),
                               capacity, ctypes.byref(nnz), stream_handle(device))
    if rc == -1:   # every other argument was checked above: ids outside [0, n)
        raise ValueError(lib.wg_last_error().decode())
    check(rc, "coo_to_csr")
    # duplicates and dropped entries leave the buffers larger than the result: give the rest back
    trim = (lambda t: t[: nnz.value].clone()) if 2 * nnz.value <= capacity else (lambda t: t[: nnz.value])
    return DeviceCSR(n, indptr, trim(indices), None if values is None else trim(values))
