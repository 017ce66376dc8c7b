"""GATS calibrator whose attention runs on the HIP path (reference ``calibration/GATS.py``).

Same class names, constructor order, parameter / buffer names and ``forward`` contract as the reference:

* ``shortest_path_length(edge_index, mask, max_hop)`` (GATS.py:25-49), one kernel launch per level instead of a
  Python loop over nodes;
* ``CalibAttentionLayer`` (GATS.py:52-167): ``temp_lin.weight`` (heads, in_channels), ``conf_coef`` [],
  ``bias`` [1], ``train_a`` [1], ``dist1_a`` [1] and the buffer ``dist_to_train``, so a state dict moves
  between the two.  The per-destination softmax over edges and both aggregations (``message`` + ``aggr='add'``,
  GATS.py:134-167) are ``csrc/gats.hip``; the rest of ``forward`` is the reference's torch code;
* ``GATSCalibrator(base_model, features, labels, adj, val_mask, heads, bias, bfs_depth)`` (GATS.py:170-278)
  trains in the constructor; ``calibrate_with_gats`` and ``GATS`` as there.

Edges keep the reference's direction: ``dense_to_sparse(adj)`` makes every ``adj[r, c] != 0`` an edge with
source r and target c, messages flow source -> target and the softmax groups by target, so node i
aggregates over column i of ``adj``.  Edge values are not used.

Differences: the graph may be sparse (a ``DeviceCSR``, an ``(indptr, indices)`` pair or a (2, E)
``edge_index``; ``GATSCalibrator(graph=)``), no (N, N) tensor is needed; the layer takes its logits as
constants (``x`` is detached: the base model is frozen, GATS.py:201-203); there is no CPU path.
"""
from __future__ import annotations

import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import check, ptr
from .ingest import edge_index_to_csr
from .laplacian import dense_to_csr, require_gpu, stream_handle
from .WATS import accuracy

MAX_HEADS = 64   # csrc/gats.hip kGatMaxHeads
DIST_UNREACHED = torch.iinfo(torch.long).max

# name -> shape of the reference layer's state (GATS.py:86-98); `heads` / `in_channels` / `num_nodes` by name
STATE_LAYOUT = {
    "temp_lin.weight": ("heads", "in_channels"),
    "conf_coef": (),
    "bias": (1,),
    "train_a": (1,),
    "dist1_a": (1,),
    "dist_to_train": ("num_nodes",),
}


def long_row_threshold() -> int:
    """Rows of at least this many entries are run by a workgroup each (``wg_gat_long_row``)."""
    return int(_lib.load().wg_gat_long_row())


def _edge_pairs(graph, num_nodes, device):
    """(src, dst, n) of a graph in the reference's convention: entry (r, c) is the edge r -> c."""
    if isinstance(graph, np.ndarray):
        graph = torch.from_numpy(graph)
    if torch.is_tensor(graph):
        if graph.dim() != 2:
            raise ValueError(f"a graph tensor is a dense (N, N) adjacency or a (2, E) edge_index, not {tuple(graph.shape)}")
        if graph.dtype in (torch.int32, torch.int64) and graph.shape[0] == 2:
            ei = graph.to(device)
            n = int(num_nodes) if num_nodes is not None else (int(ei.max()) + 1 if ei.numel() else 0)
            return ei[0], ei[1], n
        if graph.shape[0] != graph.shape[1]:
            raise ValueError(f"a dense adjacency must be square, not {tuple(graph.shape)}")
        indptr, indices, _ = dense_to_csr(graph.to(device))
        n = int(graph.shape[0])
    elif isinstance(graph, (tuple, list)) and len(graph) == 2:
        indptr, indices = (torch.as_tensor(t).to(device) for t in graph)
        n = int(indptr.numel()) - 1
    elif hasattr(graph, "indptr") and hasattr(graph, "indices"):
        indptr, indices = (torch.as_tensor(t).to(device) for t in (graph.indptr, graph.indices))
        n = int(indptr.numel()) - 1
    else:
        raise ValueError("graph must be a DeviceCSR, an (indptr, indices) pair, a dense adjacency or a (2, E) edge_index")
    if num_nodes is not None and int(num_nodes) != n:
        raise ValueError(f"num_nodes={num_nodes} but the graph has {n} rows")
    counts = (indptr[1:] - indptr[:-1]).long()
    src = torch.repeat_interleave(torch.arange(n, device=device, dtype=torch.int64), counts)
    return src, indices.to(torch.int64), n


def csr_transpose_map(indptr: torch.Tensor, indices: torch.Tensor):
    """(t_indptr int64, t_indices int32, t_pos int32) of a canonical device CSR (``wg_csr_transpose_map``)."""
    device = require_gpu(indptr.device if indptr.is_cuda else None)
    indptr = indptr.to(device=device, dtype=torch.int64).contiguous()
    indices = indices.to(device=device, dtype=torch.int32).contiguous()
    n, nnz = int(indptr.numel()) - 1, int(indices.numel())
    t_indptr = torch.empty(n + 1, dtype=torch.int64, device=device)
    t_indices = torch.empty(max(nnz, 1), dtype=torch.int32, device=device)[:nnz]
    t_pos = torch.empty(max(nnz, 1), dtype=torch.int32, device=device)[:nnz]
    with torch.cuda.device(device):
        check(_lib.load().wg_csr_transpose_map(n, nnz, ptr(indptr), ptr(indices), ptr(t_indptr), ptr(t_indices),
                                               ptr(t_pos), stream_handle(device)), "csr_transpose_map")
    return t_indptr, t_indices, t_pos


def _bfs(indptr, indices, mask, max_hop, device):
    n = int(indptr.numel()) - 1
    mask = torch.as_tensor(mask).to(device)
    if mask.dtype != torch.bool:   # an index list, as `train_mask[val_idx] = True` takes (GATS.py:211-212)
        m = torch.zeros(n, dtype=torch.bool, device=device)
        m[mask.long()] = True
        mask = m
    if mask.numel() != n:
        raise ValueError(f"mask has {mask.numel()} entries for {n} nodes")
    mask_u8 = mask.to(torch.uint8).contiguous()
    dist = torch.empty(n, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        check(_lib.load().wg_bfs_levels(n, ptr(indptr), ptr(indices), ptr(mask_u8), int(max_hop), ptr(dist),
                                        stream_handle(device)), "bfs_levels")
    return dist


def shortest_path_length(graph_or_edge_index, mask, max_hop: int, device=None) -> torch.Tensor:
    """GATS.py:25-49 on the device: the hop count from ``mask`` along the edges' direction for every node reached
    within ``max_hop - 1`` hops, ``torch.iinfo(torch.long).max`` elsewhere (with ``max_hop = 2``: 0, 1 or the
    maximum, as in the reference, whose loop assigns levels ``0 .. max_hop - 1`` only)."""
    device = require_gpu(device)
    mask = torch.as_tensor(mask)
    # a boolean mask has one entry per node: an edge_index need not name the last nodes
    src, dst, n = _edge_pairs(graph_or_edge_index, int(mask.numel()) if mask.dtype == torch.bool else None, device)
    g = edge_index_to_csr(torch.stack([src, dst]), n, device=device)   # by source: a row lists the out-neighbours
    return _bfs(g.indptr, g.indices, mask, max_hop, device)


class AttentionGraph:
    """What the attention kernels need of a graph, built once: the CSR by destination (row i lists the sources
    of the edges into i; self loops removed, then one added per node, GATS.py:102-106), its transpose map (the
    backward also runs over the sources), the rows the workgroup kernels take, and 1 / out-degree."""

    def __init__(self, graph, num_nodes: int | None = None, self_loops: bool = True, device=None):
        device = require_gpu(device)
        src, dst, n = _edge_pairs(graph, num_nodes, device)
        self.device, self.n = device, n
        # row = target, column = source; canonical (columns ascending, no duplicates): the order of the input
        # edges does not reach the kernels
        csr = edge_index_to_csr(torch.stack([dst, src]), n, self_loops="one" if self_loops else "keep", device=device)
        self.indptr, self.indices, self.nnz = csr.indptr, csr.indices.contiguous(), csr.nnz
        self.t_indptr, self.t_indices, self.t_pos = csr_transpose_map(self.indptr, self.indices)
        in_len = self.indptr[1:] - self.indptr[:-1]
        out_len = self.t_indptr[1:] - self.t_indptr[:-1]
        th = long_row_threshold()
        self.long_rows = torch.nonzero(in_len >= th).flatten().to(torch.int32)
        self.t_long_rows = torch.nonzero((in_len >= th) | (out_len >= th)).flatten().to(torch.int32)
        # degree(edge_index[0]) (GATS.py:129-131): the edges whose source is the node, after the self-loop step
        deg = out_len.to(torch.float32)
        self.deg_inv = torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))

    def describe(self) -> str:
        return (f"gat: n={self.n} nnz={self.nnz} long rows={int(self.long_rows.numel())} "
                f"long nodes={int(self.t_long_rows.numel())} (rows >= {long_row_threshold()} entries: one workgroup each)")

    def bfs(self, mask, max_hop: int) -> torch.Tensor:
        """Levels along the edges' direction: the transposed rows list each node's out-neighbours (its own
        self loop among them, which never changes a level)."""
        return _bfs(self.t_indptr, self.t_indices, mask, max_hop, self.device)

    def edge_list(self):
        """(src, dst) int64 of the edges the kernels run over, self loops included, in CSR order."""
        dst = torch.repeat_interleave(torch.arange(self.n, device=self.device), self.indptr[1:] - self.indptr[:-1])
        return self.indices.long(), dst

    # -- the two kernels ----------------------------------------------------------------------------------
    def forward(self, a, t, conf, negative_slope: float = 0.2, save: bool = False):
        n, C, H = self.n, int(a.shape[1]), int(t.shape[1])
        dev = self.device
        sim = torch.empty(n, H, dtype=torch.float32, device=dev)
        dconf = torch.empty(n, dtype=torch.float32, device=dev)
        saved = None
        if save:
            saved = (torch.empty(max(self.nnz, 1), dtype=torch.float64, device=dev),
                     torch.empty(max(n, 1), dtype=torch.float64, device=dev),
                     torch.empty(max(n, 1), dtype=torch.float64, device=dev))
        e, m, d = saved if save else (None, None, None)
        with torch.cuda.device(dev):
            check(_lib.load().wg_gat_forward(n, self.nnz, ptr(self.indptr), ptr(self.indices),
                                             int(self.long_rows.numel()), ptr(self.long_rows), C, H, ptr(a), ptr(t),
                                             ptr(conf), float(negative_slope), ptr(sim), ptr(dconf), ptr(e), ptr(m),
                                             ptr(d), stream_handle(dev)), "gat_forward")
        return sim, dconf, saved

    def backward(self, a, t, saved, g_sim, negative_slope: float = 0.2):
        n, C, H = self.n, int(a.shape[1]), int(t.shape[1])
        dev = self.device
        grad_a = torch.empty(n, C, dtype=torch.float32, device=dev)
        grad_t = torch.empty(n, H, dtype=torch.float32, device=dev)
        work = torch.empty(max(2 * self.nnz, 1), dtype=torch.float64, device=dev)
        e, m, d = saved
        with torch.cuda.device(dev):
            check(_lib.load().wg_gat_backward(n, self.nnz, ptr(self.indptr), ptr(self.indices),
                                              int(self.long_rows.numel()), ptr(self.long_rows), ptr(self.t_indptr),
                                              ptr(self.t_indices), ptr(self.t_pos), int(self.t_long_rows.numel()),
                                              ptr(self.t_long_rows), C, H, ptr(a), ptr(t), ptr(e), ptr(m), ptr(d),
                                              ptr(g_sim), float(negative_slope), ptr(grad_a), ptr(grad_t), ptr(work),
                                              stream_handle(dev)), "gat_backward")
        return grad_a, grad_t


def _f32(x, device, shape, what):
    x = x.to(device=device, dtype=torch.float32).contiguous()
    if tuple(x.shape) != shape:
        raise ValueError(f"{what} must have shape {shape}, not {tuple(x.shape)}")
    return x


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, t, conf, graph, negative_slope):
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        sim, dconf, saved = graph.forward(a, t, conf, negative_slope, save=need)
        if need:
            ctx.save_for_backward(a, t, *saved)
        ctx.graph, ctx.slope = graph, negative_slope
        ctx.mark_non_differentiable(dconf)
        return sim, dconf

    @staticmethod
    @once_differentiable
    def backward(ctx, g_sim, _g_dconf):
        a, t, e, m, d = ctx.saved_tensors
        g_sim = g_sim.to(torch.float32).contiguous()
        grad_a, grad_t = ctx.graph.backward(a, t, (e, m, d), g_sim, ctx.slope)
        return grad_a, grad_t, None, None, None


def edge_softmax_attention(graph: AttentionGraph, a: torch.Tensor, t: torch.Tensor, conf: torch.Tensor,
                           negative_slope: float = 0.2):
    """``(sim, dconf)`` of GATS.py:134-167 on ``graph``: with ``p_ij`` the softmax over the sources j of node i
    of ``leaky_relu(a_i . a_j)``, ``sim[i] = sum_j p_ij t[j]`` (N, H) and ``dconf[i] = sum_j (conf[i] -
    conf[j])`` (N,).  Differentiable w.r.t. ``a`` and ``t`` (first order); ``dconf`` carries no gradient."""
    if not isinstance(graph, AttentionGraph):
        raise ValueError("graph must be an AttentionGraph")
    if a.dim() != 2 or t.dim() != 2 or a.shape[1] < 1 or not 1 <= t.shape[1] <= MAX_HEADS:
        raise ValueError(f"a must be (N, C >= 1) and t (N, 1 <= H <= {MAX_HEADS}), not {tuple(a.shape)} / {tuple(t.shape)}")
    n = graph.n
    a = _f32(a, graph.device, (n, a.shape[1]), "a")
    t = _f32(t, graph.device, (n, t.shape[1]), "t")
    conf = _f32(conf.detach(), graph.device, (n,), "conf")
    return _EdgeSoftmax.apply(a, t, conf, graph, float(negative_slope))


class CalibAttentionLayer(nn.Module):
    """GATS.py:52-167.  ``graph``: a ``DeviceCSR``, an ``(indptr, indices)`` pair, a dense adjacency, a (2, E)
    ``edge_index`` or a prebuilt ``AttentionGraph``."""

    def __init__(self, in_channels: int, out_channels: int, graph, num_nodes: int, train_mask,
                 dist_to_train: torch.Tensor | None = None, heads: int = 8, negative_slope: float = 0.2,
                 bias: float = 1.0, self_loops: bool = True, bfs_depth: int = 2, device=None):
        super().__init__()
        if not 1 <= int(heads) <= MAX_HEADS:
            raise ValueError(f"heads must be in [1, {MAX_HEADS}], not {heads}")
        device = require_gpu(device)   # no CPU path: raises without a GPU or the library
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.heads, self.negative_slope = int(heads), float(negative_slope)
        self.num_nodes = int(num_nodes)
        self.graph = graph if isinstance(graph, AttentionGraph) else AttentionGraph(graph, num_nodes, self_loops, device)
        if self.graph.n != self.num_nodes:
            raise ValueError(f"num_nodes={num_nodes} but the graph has {self.graph.n} nodes")
        self.temp_lin = nn.Linear(self.in_channels, self.heads, bias=False)
        self.conf_coef = nn.Parameter(torch.zeros([]))
        self.bias = nn.Parameter(torch.ones(1) * bias)
        self.train_a = nn.Parameter(torch.ones(1))
        self.dist1_a = nn.Parameter(torch.ones(1))
        if dist_to_train is None:
            dist_to_train = self.graph.bfs(train_mask, bfs_depth)
        self.register_buffer("dist_to_train", torch.as_tensor(dist_to_train).to(device=device, dtype=torch.long))
        self.reset_parameters()
        self.to(device)

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.temp_lin.weight)   # PyG Linear(weight_initializer='glorot'), GATS.py:86

    def attention_inputs(self, x: torch.Tensor):
        """GATS.py:114-128, :136-138: ``(a, t, conf)`` = (alpha, temp, conf) as ``propagate`` receives them."""
        nx = x - torch.min(x, 1, keepdim=True)[0]
        nx = nx / (torch.max(x, 1, keepdim=True)[0] - torch.min(x, 1, keepdim=True)[0] + 1e-8)
        temp = self.temp_lin(torch.sort(nx, -1)[0])
        one = torch.ones(1, dtype=torch.float32, device=x.device)
        a_cluster = torch.where(self.dist_to_train == 0, self.train_a,
                                torch.where(self.dist_to_train == 1, self.dist1_a, one))
        conf = F.softmax(x, dim=1).amax(-1)
        return x / a_cluster.unsqueeze(-1), temp * a_cluster.unsqueeze(-1), conf

    def temperature(self, sim: torch.Tensor, dconf: torch.Tensor) -> torch.Tensor:
        """GATS.py:141-145."""
        out = F.softplus(sim + self.conf_coef * dconf.unsqueeze(-1) * self.graph.deg_inv.unsqueeze(-1))
        return (out.mean(dim=1) + self.bias).unsqueeze(1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x.detach().to(device=self.graph.device, dtype=torch.float32)
        if tuple(x.shape) != (self.num_nodes, self.in_channels):
            raise ValueError(f"x must have shape {(self.num_nodes, self.in_channels)}, not {tuple(x.shape)}")
        a, t, conf = self.attention_inputs(x)
        sim, dconf = edge_softmax_attention(self.graph, a, t, conf, self.negative_slope)
        return self.temperature(sim, dconf)


class GATSCalibrator(nn.Module):
    """GATS.py:170-278.  ``graph``: a sparse graph for the attention layer instead of the dense ``adj`` (as
    ``WATS(graph=)``); ``adj`` then only goes to the base model and may be that model's own operator
    (``RowNormalizedAdjacency`` of ``SparseCompatibleGCN``); ``epochs``: of the constructor's ``calib_train``."""

    def __init__(self, base_model, features, labels, adj, val_mask, heads: int = 8, bias: float = 1.0,
                 bfs_depth: int = 2, *, graph=None, verbose: bool = True, epochs: int = 250):
        super().__init__()
        self.device = require_gpu()
        self.base_model = base_model.to(self.device)
        self.x = features.to(self.device)
        self.y = labels.to(self.device)
        self.adj = adj.to(self.device) if torch.is_tensor(adj) else adj
        self.val_idx = val_mask.to(self.device)
        self.verbose = verbose
        for param in self.base_model.parameters():   # GATS.py:201-203
            param.requires_grad = False
        with torch.no_grad():
            num_classes = self.base_model(self.x, self.adj).shape[1]
        n = self.x.size(0)
        train_mask = torch.zeros(n, dtype=torch.bool, device=self.device)
        train_mask[self.val_idx] = True
        if graph is None:
            if not torch.is_tensor(self.adj):
                raise ValueError("GATSCalibrator: pass graph= when adj is not a dense tensor")
            graph = self.adj
        self.calib_attention = CalibAttentionLayer(in_channels=num_classes, out_channels=1, graph=graph, num_nodes=n,
                                                   train_mask=train_mask, heads=heads, bias=bias, bfs_depth=bfs_depth,
                                                   device=self.device)
        self.calib_train(epochs=epochs)

    def forward(self, x, adj, **kwargs):
        x = x.to(self.device)
        if torch.is_tensor(adj):
            adj = adj.to(self.device)
        logits = self.base_model(x, adj, **kwargs)
        temperature = self.graph_temperature_scale(logits)
        return F.log_softmax(logits / temperature, dim=1)

    def graph_temperature_scale(self, logits):
        temperature = self.calib_attention(logits).view(self.x.size(0), -1)
        return temperature.expand(self.x.size(0), logits.size(1))

    def calib_train(self, patience: int = 10, epochs: int = 250, lr: float = 0.01, weight_decay: float = 5e-4):
        """GATS.py:240-278: Adam on the attention layer only, NLL on the calibration nodes, early stop after
        ``patience`` non-improving epochs."""
        t = time.time()
        best_loss = float("inf")
        patience_counter = patience
        optimizer = torch.optim.Adam(self.calib_attention.parameters(), lr=lr, weight_decay=weight_decay)
        for epoch in range(epochs):
            self.train()
            optimizer.zero_grad()
            output = self(self.x, self.adj)
            loss = F.nll_loss(output[self.val_idx], self.y[self.val_idx])
            loss.backward()
            optimizer.step()
            with torch.no_grad():
                self.eval()
                acc = accuracy(output[self.val_idx], self.y[self.val_idx])
                if self.verbose:
                    print(f"epoch: {epoch}", f"loss_calibration: {loss.item():.4f}", f"acc_calibration: {acc:.4f}",
                          f"time: {time.time() - t:.4f}s")
            if loss < best_loss:
                best_loss = loss
                patience_counter = patience
            else:
                patience_counter -= 1
            if patience_counter <= 0:
                if self.verbose:
                    print(f"Early stopping at epoch {epoch}, best loss: {best_loss:.4f}")
                break
        return self

    fit = calib_train


def calibrate_with_gats(base_model, features, labels, adj, val_mask, **kwargs):
    """GATS.py:281-296."""
    return GATSCalibrator(base_model, features, labels, adj, val_mask, **kwargs)


GATS = GATSCalibrator
