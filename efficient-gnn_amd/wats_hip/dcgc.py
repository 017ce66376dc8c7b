"""DCGC calibrator whose edge MLP and weighted propagation run on the HIP path (reference
``calibration/DCGC.py``).

``Decisive_Edge.get_weight`` (DCGC.py:66-79) gathers ``[emb_r ; emb_c]`` for every stored entry of the adjacency,
runs a ``2C -> 4C -> 2C -> 1`` MLP with ReLU and dropout over the (E, 2C) tensor, scatters the weights into a dense
(N, N) matrix and runs the base model on that matrix; ``DCGC.forward`` (DCGC.py:143-150) multiplies the weights by a
homophily coefficient per edge first.  Here:

* ``EdgeWeightGraph``: the pattern, built once: the canonical CSR by row (``dense_to_sparse``'s row-major order: entry
  ``e`` is the ``e``-th stored entry), its transpose with the entry map, the long-row lists of both and the
  ``(rows, cols)`` lists;
* ``edge_mlp_weights(graph, emb, extractor, p, seed)``: DCGC.py:70-73 and the ``relu`` of :78 as one fused pass per
  direction (``wg_edge_mlp_forward`` / ``wg_edge_mlp_backward``, ``csrc/edgemlp.hip``), no (E, k) tensor;
  differentiable w.r.t. the extractor's parameters and ``emb`` (first order);
* ``weighted_propagate(graph, w, x)``: ``adj_norm @ x`` of ``src/gnn/model.py:43-47`` with the values ``w`` an
  argument (``wg_edge_aggregate``, ``csrc/edgeagg.hip``), differentiable w.r.t. ``w`` and ``x``;
* ``homophily_weights(graph, out, alpha, beta)``: DCGC.py:152-165 per entry (``wg_edge_pair_inv_distance``);
* ``DecisiveEdge`` / ``DCGC`` with the reference's surface and parameter names (``model.extractor.0.weight`` ...).

Differences.  Dropout inside the edge MLP is a stateless hash of (seed, layer, entry, unit) (``include/wats_hip.h``),
not torch's stream: training with ``dropout > 0`` does not reproduce the reference's masks, only their distribution;
the seed of every training step is drawn from torch's generator, so ``torch.manual_seed`` makes a run reproducible.
``DCGC.forward`` computes the edge weights once in eval mode (the reference computes them twice with the same result)
and takes ``probe=`` (an ``EdgeProbe``), which is handed to the ``emb`` pass of a ``SparseCompatibleGCN``: the
gradient w.r.t. the adjacency reaches the output only through ``emb`` (``dense_to_sparse`` cuts every other path).
``out_channels`` is ``gc2.out_features``.  The base model must have the ``gc1`` / ``gc2`` / ``dropout`` layout of
``CompatibleGCN``; anything else raises ``NotImplementedError``.  ``graph=`` gives the pattern without a dense (N, N)
tensor; ``epochs`` and ``verbose`` are constructor keywords; there is no CPU path.  Not built: second-order
gradients, row shards, more than ``max_classes()`` classes.
"""
from __future__ import annotations

import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import WaveletError, check, ptr
from .gats import csr_transpose_map
from .gcn import EdgeProbe, RowNormalizedAdjacency, SparseCompatibleGCN, rowdot, sddmm
from .laplacian import dense_to_csr, stream_handle
from .laplacian import require_gpu as _require_gpu
from .WATS import accuracy


def require_gpu(device=None):
    """``laplacian.require_gpu`` raising the package's error: there is no CPU path."""
    try:
        return _require_gpu(device)
    except WaveletError:
        raise
    except RuntimeError as e:
        raise WaveletError(str(e)) from None


def max_classes() -> int:
    """The widest ``emb`` the edge MLP takes (``wg_edge_mlp_max_c``)."""
    return int(_lib.load().wg_edge_mlp_max_c())


def edge_mlp_tile() -> int:
    """Entries per workgroup tile of the edge MLP's backward (``wg_edge_mlp_tile``)."""
    return int(_lib.load().wg_edge_mlp_tile())


def edge_mlp_workspace(n: int, nnz: int, C: int) -> int:
    """Bytes of scratch the edge MLP needs (``wg_edge_mlp_workspace``)."""
    b = _lib.c_i64()
    check(_lib.load().wg_edge_mlp_workspace(int(n), int(nnz), int(C), b), "edge_mlp_workspace")
    return int(b.value)


class EdgeWeightGraph:
    """The fixed pattern the edge weights live on.  ``graph``: a dense (N, N) adjacency (entries != 0), a
    ``RowNormalizedAdjacency``, a ``DeviceCSR`` / ``CSRGraph`` (anything with ``n``, ``indptr``, ``indices``), a
    (2, E) ``edge_index`` (row ``edge_index[0]``, column ``edge_index[1]``; duplicates merged) or another
    ``EdgeWeightGraph``.  Values are never read."""

    def __init__(self, graph, num_nodes: int | None = None, device=None):
        if isinstance(graph, EdgeWeightGraph):
            self.__dict__.update(graph.__dict__)
            return
        if torch.is_tensor(graph) and graph.dim() == 2 and graph.shape[0] == 2 and not graph.is_floating_point():
            from .ingest import edge_index_to_csr
            graph = edge_index_to_csr(graph, num_nodes, device=device)
        if torch.is_tensor(graph):
            if graph.dim() != 2 or graph.shape[0] != graph.shape[1]:
                raise ValueError("The adjacency matrix must be a square matrix.")
            device = require_gpu(device if device is not None else (graph.device if graph.is_cuda else None))
            indptr, indices, _ = dense_to_csr(graph.detach().to(device))
            n = int(graph.shape[0])
        else:
            device = require_gpu(device if device is not None else getattr(graph, "device", None))
            as_t = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(
                device=device, dtype=dt)
            n, indptr, indices = int(graph.n), as_t(graph.indptr, torch.int64), as_t(graph.indices, torch.int32)
        if num_nodes is not None and int(num_nodes) != n:
            raise ValueError(f"num_nodes={num_nodes} but the graph has {n} nodes")
        self.device, self.n = device, n
        self.indptr, self.indices = indptr.contiguous(), indices.contiguous()
        self.nnz = int(self.indices.numel())
        lens = self.indptr[1:] - self.indptr[:-1]
        self.rows = torch.repeat_interleave(torch.arange(n, device=device, dtype=torch.int32), lens).contiguous()
        self.cols = self.indices
        if self.nnz:
            self.t_indptr, self.t_indices, self.t_pos = csr_transpose_map(self.indptr, self.indices)
        else:
            self.t_indptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
            self.t_indices = torch.zeros(0, dtype=torch.int32, device=device)
            self.t_pos = torch.zeros(0, dtype=torch.int32, device=device)
        th = int(_lib.load().wg_edge_aggregate_long_row())
        t_lens = self.t_indptr[1:] - self.t_indptr[:-1]
        self.long_rows = torch.nonzero(lens >= th).flatten().to(torch.int32)
        self.t_long_rows = torch.nonzero(t_lens >= th).flatten().to(torch.int32)

    def describe(self) -> str:
        return (f"edge weights: n={self.n} nnz={self.nnz} long rows={int(self.long_rows.numel())} "
                f"long columns={int(self.t_long_rows.numel())}")

    def degree(self, w: torch.Tensor) -> torch.Tensor:
        """``deg_r = sum_c w_rc`` with 0 -> 1 (model.py:43-44): one sequential float64 sum per row, float32."""
        if self.nnz == 0:
            return torch.ones(self.n, dtype=torch.float32, device=self.device)
        deg = torch.segment_reduce(w.to(torch.float64), "sum", offsets=self.indptr).to(torch.float32)
        return torch.where(deg == 0, torch.ones_like(deg), deg)

    def _aggregate(self, transposed: bool, w, row_scale, col_scale, x):
        out = torch.empty_like(x)
        if self.n == 0 or x.shape[1] == 0:
            return out
        indptr, indices, long_rows, pos = ((self.t_indptr, self.t_indices, self.t_long_rows, self.t_pos) if transposed
                                           else (self.indptr, self.indices, self.long_rows, None))
        with torch.cuda.device(self.device):
            check(_lib.load().wg_edge_aggregate(self.n, self.nnz, ptr(indptr), ptr(indices), int(long_rows.numel()),
                                                ptr(long_rows), ptr(w), ptr(pos), ptr(row_scale), ptr(col_scale),
                                                int(x.shape[1]), ptr(x), ptr(out), stream_handle(self.device)),
                  "edge_aggregate")
        return out

    def aggregate(self, w, x, row_scale=None):
        """``out[r] = row_scale[r] * sum_c w_rc x[c]``."""
        return self._aggregate(False, w, row_scale, None, x)

    def aggregate_transposed(self, w, g, col_scale=None):
        """``out[c] = sum_r w_rc col_scale[r] g[r]``."""
        return self._aggregate(True, w, None, col_scale, g)


def _extractor_params(extractor):
    """The six arrays of DCGC.py:36-44 (W1, b1, W2, b2, w3, b3) from the ``nn.Sequential`` or a 6-tuple."""
    if isinstance(extractor, nn.Module):
        lin = [m for m in extractor if isinstance(m, nn.Linear)]
        if len(lin) != 3:
            raise ValueError("the extractor must hold three Linear layers (DCGC.py:36-44)")
        extractor = (lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight, lin[2].bias)
    params = tuple(extractor)
    if len(params) != 6:
        raise ValueError("expected (W1, b1, W2, b2, w3, b3)")
    return params


class _EdgeMlp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, W1, b1, W2, b2, W3, b3, graph, p, seed):
        params = (W1, b1, W2, b2, W3, b3)
        w = torch.zeros(graph.nnz, dtype=torch.float32, device=graph.device)
        if graph.nnz:
            check(_lib.load().wg_edge_mlp_forward(
                graph.n, graph.nnz, ptr(graph.indptr), ptr(graph.indices), emb.shape[1], ptr(emb),
                *(ptr(t) for t in params), float(p), int(seed),
                ptr(_workspace(graph, emb.shape[1])), ptr(w), stream_handle(graph.device)), "edge_mlp_forward")
        ctx.save_for_backward(emb, *params)
        ctx.graph, ctx.p, ctx.seed = graph, p, seed
        return w

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        emb, *params = ctx.saved_tensors
        graph = ctx.graph
        g = g.to(torch.float32).contiguous()
        grads = [torch.empty_like(t) for t in params]
        g_emb = torch.empty_like(emb) if ctx.needs_input_grad[0] else None
        with torch.cuda.device(graph.device):
            check(_lib.load().wg_edge_mlp_backward(
                graph.n, graph.nnz, ptr(graph.indptr), ptr(graph.indices), emb.shape[1], ptr(emb),
                *(ptr(t) for t in params), float(ctx.p), int(ctx.seed), ptr(g), ptr(graph.t_indptr),
                ptr(graph.t_indices), ptr(graph.t_pos), *(ptr(t) for t in grads), ptr(g_emb),
                ptr(_workspace(graph, emb.shape[1])), stream_handle(graph.device)), "edge_mlp_backward")
        return (g_emb, *grads, None, None, None)


def _workspace(graph, C):
    return torch.empty(max(edge_mlp_workspace(graph.n, graph.nnz, C), 16), dtype=torch.uint8, device=graph.device)


def edge_mlp_weights(graph: EdgeWeightGraph, emb: torch.Tensor, extractor, p: float = 0.0, seed: int = 0):
    """``relu(extractor([emb_r ; emb_c]))`` for every entry (r, c) of ``graph`` in CSR order (DCGC.py:70-78), (nnz,)
    float32.  ``extractor``: the ``nn.Sequential`` of DCGC.py:36-44 or its six arrays.  ``p``: the dropout
    probability of both hidden layers (0 = eval mode), ``seed``: of the hashed masks.  Differentiable w.r.t. the six
    arrays and ``emb``."""
    require_gpu()
    if not isinstance(graph, EdgeWeightGraph):
        raise ValueError("graph must be an EdgeWeightGraph")
    if emb.dim() != 2 or emb.shape[0] != graph.n:
        raise ValueError(f"emb must be ({graph.n}, C), not {tuple(emb.shape)}")
    C = int(emb.shape[1])
    if C < 1:
        raise ValueError("emb needs at least one column")
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f"p must lie in [0, 1), not {p}")
    params = _extractor_params(extractor)
    shapes = ((4 * C, 2 * C), (4 * C,), (2 * C, 4 * C), (2 * C,), (1, 2 * C), (1,))
    for t, s in zip(params, shapes):
        if tuple(t.shape) != s:
            raise ValueError(f"extractor shapes for C={C} must be {shapes}, got {tuple(t.shape)} for {s}")
    emb = emb.to(device=graph.device, dtype=torch.float32).contiguous()
    params = tuple(t.to(device=graph.device, dtype=torch.float32).contiguous() for t in params)
    with torch.cuda.device(graph.device):
        return _EdgeMlp.apply(emb, *params, graph, float(p), int(seed) & (2 ** 64 - 1))


class _WeightedPropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, x, graph):
        inv = 1.0 / graph.degree(w)
        y = graph.aggregate(w, x, inv)
        ctx.save_for_backward(w, x, y, inv)
        ctx.graph = graph
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        w, x, y, inv = ctx.saved_tensors
        graph = ctx.graph
        g = g.to(torch.float32).contiguous()
        gw = gx = None
        if ctx.needs_input_grad[1]:
            gx = graph.aggregate_transposed(w, g, inv)
        if ctx.needs_input_grad[0]:
            if graph.nnz == 0 or g.shape[1] == 0:
                gw = torch.zeros_like(w)
            else:   # (g_r . x_c - g_r . y_r) / deg_r, the formula of gcn.py
                gw = sddmm(graph.rows, graph.cols, g, x, row_term=rowdot(g, y), row_scale=inv, validate=False)
        return gw, gx, None


def weighted_propagate(graph: EdgeWeightGraph, w: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """``y_r = (sum_c w_rc x_c) / deg_r`` with ``deg_r = sum_c w_rc``, 0 -> 1 (model.py:43-47), ``w`` (nnz,) in the
    graph's CSR order.  Differentiable w.r.t. ``w`` and ``x`` (first order)."""
    require_gpu()
    if not isinstance(graph, EdgeWeightGraph):
        raise ValueError("graph must be an EdgeWeightGraph")
    if x.dim() != 2 or x.shape[0] != graph.n:
        raise ValueError(f"x must be ({graph.n}, F), not {tuple(x.shape)}")
    if tuple(w.shape) != (graph.nnz,):
        raise ValueError(f"w must have one value per entry ({graph.nnz}), not {tuple(w.shape)}")
    w = w.to(device=graph.device, dtype=torch.float32).contiguous()
    x = x.to(device=graph.device, dtype=torch.float32).contiguous()
    return _WeightedPropagate.apply(w, x, graph)


def pair_inv_distance(graph: EdgeWeightGraph, q: torch.Tensor, alpha: float) -> torch.Tensor:
    """``1 / (|q_r - q_c|_2 + alpha)`` per entry (``wg_edge_pair_inv_distance``), no gradient."""
    q = q.detach().to(device=graph.device, dtype=torch.float32).contiguous()
    if q.dim() != 2 or q.shape[0] != graph.n:
        raise ValueError(f"q must be ({graph.n}, C), not {tuple(q.shape)}")
    out = torch.empty(graph.nnz, dtype=torch.float32, device=graph.device)
    with torch.cuda.device(graph.device):
        check(_lib.load().wg_edge_pair_inv_distance(graph.nnz, ptr(graph.rows), ptr(graph.cols), int(q.shape[1]),
                                                    graph.n, ptr(q), float(alpha), ptr(out),
                                                    stream_handle(graph.device)), "edge_pair_inv_distance")
    return out


def homophily_weights(graph: EdgeWeightGraph, out: torch.Tensor, alpha: float = 0.5, beta: float = 10) -> torch.Tensor:
    """DCGC.py:158-165 per entry: ``q = softmax(beta * softmax(out))``, ``1 / (|q_r - q_c|_2 + alpha)``."""
    require_gpu()
    if not isinstance(graph, EdgeWeightGraph):
        raise ValueError("graph must be an EdgeWeightGraph")
    with torch.no_grad():
        pred = F.softmax(out.detach().to(graph.device, torch.float32), dim=1)
        q = F.softmax(beta * pred, dim=1)
        return pair_inv_distance(graph, q, alpha)


def _check_base(base_model):
    ok = (isinstance(getattr(base_model, "gc1", None), nn.Linear) and isinstance(getattr(base_model, "gc2", None), nn.Linear)
          and isinstance(getattr(base_model, "dropout", None), nn.Dropout))
    if not ok:
        raise NotImplementedError("DCGC runs the base model on the edge weights itself and needs the gc1 / gc2 / "
                                  "dropout layout of CompatibleGCN (SparseCompatibleGCN or the dense model)")


class DecisiveEdge(nn.Module):
    """``Decisive_Edge`` (DCGC.py:8-119): the edge-weight MLP on the base model's logits, trained in the constructor
    (Adam, lr 0.01, weight decay 5e-4, cross entropy on the calibration nodes, patience 10)."""

    def __init__(self, out_channels, base_model, x, y, adj, val_idx, dropout: float = 0.5, *, graph=None,
                 epochs: int = 250, verbose: bool = False):
        super().__init__()
        _check_base(base_model)
        self.device = require_gpu()
        self.base_model = base_model.to(self.device)
        self.x, self.y = x.to(self.device), y.to(self.device)
        self.adj = adj.to(self.device) if torch.is_tensor(adj) else adj
        self.val_idx = val_idx.to(self.device) if torch.is_tensor(val_idx) else val_idx
        self.p, self.epochs, self.verbose = float(dropout), int(epochs), verbose
        C = int(out_channels)
        self.extractor = nn.Sequential(                       # DCGC.py:36-44
            nn.Linear(C * 2, C * 4), nn.ReLU(), nn.Dropout(dropout),
            nn.Linear(C * 4, C * 2), nn.ReLU(), nn.Dropout(dropout),
            nn.Linear(C * 2, 1)).to(self.device)
        n = self.x.size(0)
        self._fixed_graph = graph is not None
        self._dense = []      # [(tensor, its version, graph)], newest first: see _pattern_of
        if graph is None:
            graph = self._pattern_of(self.adj)
            if torch.is_tensor(adj) and adj is not self.adj:      # the caller's tensor names the same pattern
                self._remember(adj, graph)
        self._adj_version = self.adj._version if torch.is_tensor(self.adj) else None
        self.graph = graph if isinstance(graph, EdgeWeightGraph) else EdgeWeightGraph(graph, n, self.device)
        if self.graph.n != n:
            raise ValueError(f"x has {n} rows but the graph has {self.graph.n} nodes")
        for para in self.base_model.parameters():             # DCGC.py:46-47
            para.requires_grad = False
        self.history = []
        self.weight_train()

    DENSE_SLOTS = 2     # dense adjacencies whose pattern is kept (each keeps its (N, N) tensor alive)

    def _remember(self, adj, graph):
        self._dense.insert(0, (adj, adj._version, graph))
        del self._dense[self.DENSE_SLOTS:]

    def _pattern_of(self, adj) -> EdgeWeightGraph:
        """The pattern of ``adj``, built once per adjacency.  No key outlives what it names: an operator (a
        ``RowNormalizedAdjacency`` or a ``with_flips`` view) carries its pattern itself, so the pattern goes when the
        operator goes and a new operator never meets an old one's; a dense tensor is recognised by identity and
        version while it sits in one of ``DENSE_SLOTS`` slots, which hold a reference to it."""
        if isinstance(adj, EdgeWeightGraph):
            return adj
        if isinstance(adj, RowNormalizedAdjacency):
            graph = adj.__dict__.get("_edge_weight_graph")
            if graph is None:
                graph = adj._edge_weight_graph = EdgeWeightGraph(adj, None, self.device)
            return graph
        if torch.is_tensor(adj):
            for i, (t, version, graph) in enumerate(self._dense):
                if t is adj and version == adj._version:
                    self._dense.insert(0, self._dense.pop(i))
                    return graph
            graph = EdgeWeightGraph(adj.detach(), None, self.device)
            self._remember(adj, graph)
            return graph
        return EdgeWeightGraph(adj, None, self.device)

    def graph_for(self, adj) -> EdgeWeightGraph:
        """The pattern ``forward(x, adj)`` puts its weights on."""
        if self._fixed_graph:
            return self.graph
        if adj is self.adj and (self._adj_version is None or self._adj_version == adj._version):
            return self.graph
        return self._pattern_of(adj)

    def embeddings(self, x, adj, probe: EdgeProbe | None = None):
        """``emb = base_model(x, adj)`` (DCGC.py:68): the only path from the adjacency to the edge weights."""
        x = x.to(self.device)
        if torch.is_tensor(adj):
            if adj.requires_grad:
                raise NotImplementedError("DCGC has no gradient w.r.t. a dense adj leaf (N x N); use a "
                                          "SparseCompatibleGCN base model and probe=EdgeProbe(rows, cols)")
            adj = adj.to(self.device)
        if isinstance(self.base_model, SparseCompatibleGCN):
            return self.base_model(x, adj, probe=probe)
        if probe is not None:
            raise NotImplementedError("probe= needs a SparseCompatibleGCN base model")
        return self.base_model(x, adj)

    def weighted_base(self, graph: EdgeWeightGraph, w, x):
        """The base model on the adjacency whose stored entries are ``w`` (model.py:43-52)."""
        b = self.base_model
        h = weighted_propagate(graph, w, x.to(self.device))
        h = b.dropout(F.relu(b.gc1(h)))
        return b.gc2(weighted_propagate(graph, w, h))

    def get_weight(self, x, adj, probe: EdgeProbe | None = None, graph: EdgeWeightGraph | None = None):
        """DCGC.py:66-79 at the stored entries: (nnz,) in the graph's CSR order."""
        graph = self.graph_for(adj) if graph is None else graph
        emb = self.embeddings(x, adj, probe)
        if self.training and self.p > 0:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())     # torch.manual_seed makes a run reproducible
            return edge_mlp_weights(graph, emb, self.extractor, self.p, seed)
        return edge_mlp_weights(graph, emb, self.extractor, 0.0, 0)

    def forward(self, x, adj, **kwargs):
        graph = self.graph_for(adj)
        w = self.get_weight(x, adj, kwargs.get("probe"), graph)
        return self.weighted_base(graph, w, x)

    def weight_train(self, patience: int = 10):
        """DCGC.py:81-119."""
        t0 = time.time()
        best_loss = float("inf")
        patience_counter = patience
        optimizer = torch.optim.Adam(self.extractor.parameters(), lr=0.01, weight_decay=5e-4)
        self.history = []
        for epoch in range(self.epochs):
            self.train()
            optimizer.zero_grad()
            output = self(self.x, self.adj)
            loss = F.cross_entropy(output[self.val_idx], self.y[self.val_idx])
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
        self.eval()
        return self


class DCGC(nn.Module):
    """DCGC.py:121-173 with the reference's positional surface.  ``adj``: the dense (N, N) adjacency on any device
    or a ``RowNormalizedAdjacency``; ``graph``: the pattern for the edge weights instead of ``adj``'s (whatever
    ``EdgeWeightGraph`` takes), e.g. for a dense ``CompatibleGCN`` base model."""

    def __init__(self, base_model, features, labels, adj, val_mask, dropout: float = 0.5, alpha: float = 0.5,
                 beta: float = 10, *, graph=None, epochs: int = 250, verbose: bool = False):
        super().__init__()
        _check_base(base_model)
        self.device = require_gpu()
        out_channels = base_model.gc2.out_features
        self.model = DecisiveEdge(out_channels, base_model, features, labels, adj, val_mask, dropout, graph=graph,
                                  epochs=epochs, verbose=verbose)
        self.x, self.y = features.to(self.device), labels.to(self.device)
        self.adj = self.model.adj
        self.val_idx = val_mask.to(self.device)
        self.alpha, self.beta = alpha, beta
        for para in self.model.parameters():                  # DCGC.py:140-141
            para.requires_grad = False

    @property
    def graph(self) -> EdgeWeightGraph:
        return self.model.graph

    def get_homo_weight(self, x, adj, alpha: float = 0.5, beta: float = 10, w=None):
        """DCGC.py:152-173 at the stored entries; ``w``: the eval-mode edge weights if already computed."""
        graph = self.model.graph_for(adj)
        with torch.no_grad():
            self.model.eval()
            if w is None:
                w = self.model.get_weight(x, adj, graph=graph)
            out = self.model.weighted_base(graph, w.detach(), x)
        return homophily_weights(graph, out, alpha, beta)

    def forward(self, x, adj, probe: EdgeProbe | None = None, **kwargs):
        """Other keywords are accepted and ignored, as the reference's ``forward(x, adj, **kwargs)`` ignores them."""
        self.model.eval()
        graph = self.model.graph_for(adj)
        w = self.model.get_weight(x, adj, probe, graph)                     # DCGC.py:144
        homo = self.get_homo_weight(x, adj, self.alpha, self.beta, w=w)     # :145
        return self.model.weighted_base(graph, w * homo, x)                 # :147-148
