"""CaGCN calibrator whose graph convolutions run on the HIP path (reference ``calibration/CaGCN.py``).

The reference's scaling model is two PyG ``GCNConv(n_classes, n_classes)`` layers (CaGCN.py:68-70, :104-108):
``D^-1/2 (A + I) D^-1/2 (X W^T) + b`` with ``D`` the in-degree with the self loop (PyG ``gcn_norm``).  Here:

* ``SymNormGraph``: the by-destination CSR with one self loop per node, its transpose and the hub-row lists (an
  ``AttentionGraph``, which GATS and CaGCN may share) plus ``dinv = in_degree^-1/2``;
* ``sym_norm_aggregate(graph, x, bias, relu)``: the propagation, ``csrc/symnorm.hip`` (no per-edge weight and no
  (E, C) tensor is built), differentiable w.r.t. ``x`` and ``bias``;
* ``GCNConv(in_channels, out_channels, graph, bias=True)`` with PyG's parameter names ``lin.weight`` / ``bias``;
* ``calibration_loss`` (CaGCN.py:9-42) and ``CaGCN(base_model, x, y, adj, val_idx)`` (CaGCN.py:45-157), which
  trains in the constructor; ``forward(x, adj, **kwargs)``, ``base_predict`` and ``calib_train(patience, alpha)``
  as there.

Edges keep the reference's direction: ``dense_to_sparse(adj)`` makes every ``adj[r, c] != 0`` an edge r -> c,
node c aggregates over column c of ``adj``, and ``add_remaining_self_loops`` leaves one loop per node.  Edge
values are not used (CaGCN passes ``edge_index`` only).

Differences: ``scaling_model`` is an ``nn.ModuleList`` (the reference keeps a plain list, so its ``state_dict()``
omits the scaling model's parameters; ours has ``scaling_model.0.lin.weight`` ... ``scaling_model.1.bias``); the
graph may be sparse (``CaGCN(graph=)``: whatever ``AttentionGraph`` takes, or a ``SymNormGraph``), no (N, N)
tensor is needed; ``dropout``, ``epochs`` and ``verbose`` are constructor keywords; there is no CPU path.  The
logits are NOT detached: the gradient w.r.t. the adjacency flows through the base model's logits into both the
product and the scaling model (an ``EdgeProbe`` on a ``SparseCompatibleGCN`` receives it); the path through the
normalisation itself is cut, as the reference's ``dense_to_sparse`` cuts it.
"""
from __future__ import annotations

import time

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import check, ptr
from .gats import AttentionGraph
from .laplacian import require_gpu, stream_handle
from .WATS import accuracy


def symnorm_long_row_threshold() -> int:
    """Rows of at least this many entries are run by a workgroup each (``wg_symnorm_long_row``)."""
    return int(_lib.load().wg_symnorm_long_row())


class SymNormGraph:
    """What ``wg_symnorm_aggregate`` needs of a graph, built once.  ``graph``: anything ``AttentionGraph`` takes,
    or a prebuilt ``AttentionGraph`` with self loops (read, never changed).  Adds ``dinv`` (PyG's
    ``deg.pow_(-0.5)`` in float32; every row holds its self loop, so no infinity arises) and the exact long-row
    lists of both directions."""

    def __init__(self, graph, num_nodes: int | None = None, device=None):
        if isinstance(graph, SymNormGraph):
            graph = graph.ag
        if isinstance(graph, AttentionGraph):
            ag = graph
            if num_nodes is not None and int(num_nodes) != ag.n:
                raise ValueError(f"num_nodes={num_nodes} but the graph has {ag.n} nodes")
            src, dst = ag.edge_list()
            if int((src == dst).sum()) != ag.n:
                raise ValueError("SymNormGraph needs an AttentionGraph built with self_loops=True")
        else:
            ag = AttentionGraph(graph, num_nodes, True, require_gpu(device))
        self.ag = ag
        self.device, self.n, self.nnz = ag.device, ag.n, ag.nnz
        self.indptr, self.indices = ag.indptr, ag.indices
        self.t_indptr, self.t_indices = ag.t_indptr, ag.t_indices
        in_len = self.indptr[1:] - self.indptr[:-1]
        out_len = self.t_indptr[1:] - self.t_indptr[:-1]
        self.dinv = in_len.to(torch.float32).pow(-0.5).contiguous()
        th = symnorm_long_row_threshold()
        self.long_rows = torch.nonzero(in_len >= th).flatten().to(torch.int32)
        self.t_long_rows = torch.nonzero(out_len >= th).flatten().to(torch.int32)

    def describe(self) -> str:
        return (f"symnorm: n={self.n} nnz={self.nnz} long rows={int(self.long_rows.numel())} "
                f"long transposed rows={int(self.t_long_rows.numel())} "
                f"(rows >= {symnorm_long_row_threshold()} entries: one workgroup each)")

    def edge_list(self):
        """(src, dst) int64 of the edges, self loops included, in CSR order."""
        return self.ag.edge_list()

    def _launch(self, indptr, indices, long_rows, x, bias, relu):
        out = torch.empty_like(x)
        with torch.cuda.device(self.device):
            check(_lib.load().wg_symnorm_aggregate(self.n, self.nnz, ptr(indptr), ptr(indices),
                                                   int(long_rows.numel()), ptr(long_rows), ptr(self.dinv),
                                                   int(x.shape[1]), ptr(x), ptr(bias), int(bool(relu)), ptr(out),
                                                   stream_handle(self.device)), "symnorm_aggregate")
        return out

    def aggregate(self, x, bias=None, relu: bool = False):
        """``act(D^-1/2 (A + I) D^-1/2 x + bias)`` by destination; x (n, C) float32 contiguous on the device."""
        return self._launch(self.indptr, self.indices, self.long_rows, x, bias, relu)

    def aggregate_transposed(self, g):
        """The gradient w.r.t. x: the same entry over the transposed structure."""
        return self._launch(self.t_indptr, self.t_indices, self.t_long_rows, g, None, False)


class _SymNormAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, graph, relu):
        out = graph.aggregate(x, bias, relu)
        ctx.graph, ctx.relu = graph, relu
        if relu:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = g.to(torch.float32).contiguous()
        if ctx.relu:
            (out,) = ctx.saved_tensors
            g = g * (out > 0)     # one elementwise pass; gathering the mask would double the gather traffic
        grad_x = ctx.graph.aggregate_transposed(g) if ctx.needs_input_grad[0] else None
        grad_bias = g.sum(0) if ctx.needs_input_grad[1] else None
        return grad_x, grad_bias, None, None


def sym_norm_aggregate(graph: SymNormGraph, x: torch.Tensor, bias: torch.Tensor | None = None,
                       relu: bool = False) -> torch.Tensor:
    """``act(D^-1/2 (A + I) D^-1/2 x + bias)`` on ``graph`` (``wg_symnorm_aggregate``): PyG's ``gcn_norm`` and
    ``propagate`` of ``GCNConv`` without the linear map.  Differentiable w.r.t. ``x`` and ``bias`` (first order);
    with ``relu`` the incoming gradient is masked by ``out > 0``."""
    if not isinstance(graph, SymNormGraph):
        raise ValueError("graph must be a SymNormGraph")
    if x.dim() != 2 or x.shape[0] != graph.n:
        raise ValueError(f"x must be ({graph.n}, C), not {tuple(x.shape)}")
    x = x.to(device=graph.device, dtype=torch.float32).contiguous()
    if bias is not None:
        bias = bias.to(device=graph.device, dtype=torch.float32).contiguous()
        if tuple(bias.shape) != (x.shape[1],):
            raise ValueError(f"bias must have shape ({x.shape[1]},), not {tuple(bias.shape)}")
    return _SymNormAggregate.apply(x, bias, graph, bool(relu))


class GCNConv(nn.Module):
    """PyG ``GCNConv(in_channels, out_channels)`` with its defaults (``add_self_loops``, ``normalize``, no edge
    weights) on a fixed graph: ``lin.weight`` (out, in) with Glorot initialisation, a zero ``bias`` (out,)."""

    def __init__(self, in_channels: int, out_channels: int, graph, bias: bool = True):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.graph = graph if isinstance(graph, SymNormGraph) else SymNormGraph(graph)
        self.lin = nn.Linear(self.in_channels, self.out_channels, bias=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(self.out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()
        self.to(self.graph.device)

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.lin.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x: torch.Tensor, relu: bool = False, graph: SymNormGraph | None = None) -> torch.Tensor:
        """``act(A_hat (x W^T) + b)``; ``graph``: another graph for this call (``CaGCN.forward`` with a new adj)."""
        return sym_norm_aggregate(self.graph if graph is None else graph, self.lin(x), self.bias, relu)


def calibration_loss(output: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """CaGCN.py:9-42: the mean of ``1 - p1 + p2`` over the correctly classified rows and ``p1 - p2`` over the
    others, ``p1 >= p2`` the two largest softmax probabilities of a row."""
    output = torch.softmax(output, dim=1)
    pred_max_index = torch.max(output, 1)[1]
    correct_i = torch.where(pred_max_index == labels)
    incorrect_i = torch.where(pred_max_index != labels)
    output = torch.sort(output, dim=1, descending=True)
    pred, sub_pred = output[0][:, 0], output[0][:, 1]
    return (torch.sum(1 - pred[correct_i] + sub_pred[correct_i])
            + torch.sum(pred[incorrect_i] - sub_pred[incorrect_i])) / labels.size()[0]


def _adj_key(adj):
    return (adj.data_ptr(), tuple(adj.shape), adj._version, str(adj.device))


class CaGCN(nn.Module):
    """CaGCN.py:45-157.  ``graph``: a sparse graph for the scaling model instead of the dense ``adj`` (as
    ``GATSCalibrator(graph=)``); ``adj`` then only goes to the base model and may be that model's own operator.
    Without ``graph=`` the scaling model runs on the graph of the construction ``adj``; a ``forward`` with another
    dense ``adj`` tensor (or the same one changed in place) builds that tensor's graph, as the reference rebuilds
    ``edge_index`` on every call, and keeps it while the tensor is unchanged."""

    def __init__(self, base_model, x, y, adj, val_idx, *, graph=None, dropout: float = 0.5, verbose: bool = True,
                 epochs: int = 100):
        super().__init__()
        self.device = require_gpu()
        self.base_model = base_model.to(self.device)
        self.n_classes = int(y.max().item()) + 1
        self.x = x.to(self.device)
        self.y = y.to(self.device)
        self.adj = adj.to(self.device) if torch.is_tensor(adj) else adj
        self.val_idx = val_idx.to(self.device)
        self.verbose, self.epochs = verbose, int(epochs)
        n = self.x.size(0)
        self._fixed_graph = graph is not None
        self._graph_key = set()
        if graph is None:
            if not torch.is_tensor(adj):
                raise ValueError("CaGCN: pass graph= when adj is not a dense tensor")
            self._check_square(adj)
            self._graph_key = {_adj_key(adj), _adj_key(self.adj)}   # the caller's tensor and its device copy
            graph = self.adj
        self.graph = graph if isinstance(graph, SymNormGraph) else SymNormGraph(graph, n, self.device)
        if self.graph.n != n:
            raise ValueError(f"x has {n} rows but the graph has {self.graph.n} nodes")
        self._other_key, self._other_graph = None, None
        self.scaling_model = nn.ModuleList([GCNConv(self.n_classes, self.n_classes, self.graph),
                                            GCNConv(self.n_classes, self.n_classes, self.graph)])
        self.dropout = nn.Dropout(p=dropout)
        for para in self.base_model.parameters():   # CaGCN.py:78-79
            para.requires_grad = False
        self.history = []
        self.calib_train()

    @staticmethod
    def _check_square(adj):
        if adj.dim() != 2 or adj.shape[0] != adj.shape[1]:   # CaGCN.py:99-100
            raise ValueError("The adjacency matrix must be a square matrix.")

    def graph_for(self, adj) -> SymNormGraph:
        """The graph ``forward(x, adj)`` aggregates over."""
        if self._fixed_graph:
            return self.graph
        if not torch.is_tensor(adj):
            raise ValueError("CaGCN: this adj is not a dense tensor; construct the calibrator with graph=")
        self._check_square(adj)
        key = _adj_key(adj)
        if key in self._graph_key:
            return self.graph
        if key != self._other_key:
            self._other_graph = SymNormGraph(adj.detach().to(self.device), self.x.size(0), self.device)
            self._other_key = key
        return self._other_graph

    def forward(self, x, adj, **kwargs):
        graph = self.graph_for(adj)
        x = x.to(self.device)
        if torch.is_tensor(adj):
            adj = adj.to(self.device)
        logits = self.base_model(x, adj, **kwargs)            # CaGCN.py:103
        t = self.scaling_model[0](logits, relu=True, graph=graph)   # :105-106
        t = self.dropout(t)                                   # :107
        t = self.scaling_model[1](t, graph=graph)             # :108
        t = torch.log(torch.exp(t) + 1.1)                     # :109
        return F.log_softmax(logits * t, dim=1)               # :110-112

    def base_predict(self, x, adj):
        return self.base_model(x.to(self.device), adj.to(self.device) if torch.is_tensor(adj) else adj)

    def calib_train(self, patience: int = 10, alpha: float = 0.5):
        """CaGCN.py:118-157: Adam (lr 0.01, weight decay 5e-4) on the scaling model only, NLL plus ``alpha`` times
        the calibration loss on the calibration nodes, early stop after ``patience`` non-improving epochs.
        ``self.history`` gets the loss of every epoch."""
        t0 = time.time()
        best_loss = float("inf")
        patience_counter = patience
        optimizer = torch.optim.Adam(self.scaling_model.parameters(), lr=0.01, weight_decay=5e-4)
        self.history = []
        for epoch in range(self.epochs):
            self.train()
            optimizer.zero_grad()
            output = self(self.x, self.adj)
            loss = F.nll_loss(output[self.val_idx], self.y[self.val_idx]) + \
                alpha * calibration_loss(output[self.val_idx], self.y[self.val_idx])
            loss.backward()
            optimizer.step()
            value = loss.item()
            self.history.append(value)
            with torch.no_grad():
                self.eval()
                if self.verbose:
                    acc = accuracy(output[self.val_idx], self.y[self.val_idx])
                    print(f"epoch: {epoch}", f"loss_calibration: {value:.4f}", f"acc_calibration: {acc:.4f}",
                          f"time: {time.time() - t0:.4f}s")
            if value < best_loss:
                best_loss = value
                patience_counter = patience
            else:
                patience_counter -= 1
            if patience_counter <= 0:
                if self.verbose:
                    print(f"Early stopping at epoch {epoch}, best loss: {best_loss:.4f}")
                break
        return self

    fit = calib_train
