"""GETS calibrator whose mixture of graph experts runs on the HIP path (reference
``calibration/GETS.py``).

The reference keeps E experts, each ending in a PyG ``GCNConv`` to the classes, and a noisy top-k gate per node.  Its
``forward`` stacks the E aggregated (N, C) outputs, multiplies them by gates that are exact zeros outside the
selection and sums (GETS.py:402-410), then ``log_softmax(logits * softplus(T))``.  The gate belongs to the
destination row, so it commutes with the aggregation.  Here:

* ``gated_sym_norm_head(graph, z, sel, gate, bias, logits)``: the last propagation of all experts, the mixture and the
  head in one pass over a ``SymNormGraph`` (``csrc/gatedagg.hip``), differentiable to first order w.r.t. ``z``,
  ``gate``, ``bias`` and ``logits``.  ``z`` (n, E, C) holds each expert's last linear map, ``sel`` / ``gate`` (n, k)
  the selected experts and their weights.  No (N, E, C) tensor of aggregated outputs is built.  A slice that a row did
  not select is never read: a NaN in it does not reach that row (the reference's ``0 * NaN`` would).
* ``GCNExpert``: ``GCN_Expert`` (GETS.py:24-92) on this package's ``GCNConv``, with the reference's parameter names
  ``proj_feature``, ``convs.N.lin.weight`` / ``.bias`` and ``degree_embedder.weight``.  ``last_linear`` gives the (n, C)
  product that enters the fused head; ``forward`` is the expert's own, unfused output.
* ``GETSCalibrator``: GETS.py:242-536 with the reference's constructor keywords and defaults plus ``graph=``,
  ``verbose=`` and ``train_degree_embedding=``; ``calibrate_with_gets`` builds and fits one.

Three behaviours of the reference are kept on purpose:

1. The experts' graph is the one ``fit`` saw.  ``forward``'s ``adj`` only reaches the base model (GETS.py:405 passes
   ``self.edge_index``), so the gradient w.r.t. the adjacency flows through the logits alone.  The logits are NOT
   detached: an ``EdgeProbe`` on a ``SparseCompatibleGCN`` receives that gradient.
2. The reference creates each ``degree_embedder`` inside the first forward (GETS.py:74-80), after ``calib_train`` has
   built its optimiser, so Adam never updates the embeddings.  Here they are created in ``_build_networks`` with
   ``requires_grad=True`` and left out of the optimiser unless ``train_degree_embedding=True``.
3. Ties in ``topk`` are whatever torch does; the fused head takes the selection as given.

``degrees`` of a node is its out-degree plus its in-degree over the entries of ``adj`` itself, before any self loop is
added; a diagonal entry counts in both terms (GETS.py:77).  With ``graph=`` and no dense ``adj`` the count is taken
over the graph's edges without their self loops.

Not built: ``backbone='gat'`` (PyG's multi-head ``GATConv`` is not the ``CalibAttentionLayer`` of this package) and
``backbone='gin'`` (GIN's MLP comes after the neighbour sum, so the gate does not commute with it) raise
``NotImplementedError``; row shards, second-order gradients, more than 256 classes, more than 4 experts; there is no
CPU path.  The gate (its (n, E) logits, top-k softmax, ``importance``, ``load`` and ``cv_squared``) is computed in
float64 from the float32 gating input and handed on in float32: ``aux_loss`` is a quotient of a variance of E sums
that nearly cancel, which float32 holds to several ulps only.  ``gating_noise``: a tensor to use instead of ``randn_like`` in the next training-mode forwards (tests).
"""
from __future__ import annotations

import time

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable
from torch.distributions.normal import Normal

from . import _lib
from ._lib import check, ptr
from .cagcn import GCNConv, SymNormGraph, sym_norm_aggregate
from .laplacian import require_gpu, stream_handle
from .WATS import accuracy

EXPERT_CONFIGS = (("logits", "features"), ("logits", "degrees"), ("features", "degrees"),
                  ("logits", "features", "degrees"))   # GETS.py:300-305
MAX_EXPERTS = 4
MAX_CLASSES = 256


def gated_long_row_threshold() -> int:
    """Rows of at least this many entries are run by a workgroup each (``wg_gated_symnorm_long_row``)."""
    return int(_lib.load().wg_gated_symnorm_long_row())


def _long_rows(graph: SymNormGraph):
    """(long_rows, t_long_rows) of the gated kernels' own threshold, built once per graph."""
    cached = getattr(graph, "_gated_long_rows", None)
    if cached is None:
        th = gated_long_row_threshold()
        in_len = graph.indptr[1:] - graph.indptr[:-1]
        out_len = graph.t_indptr[1:] - graph.t_indptr[:-1]
        cached = (torch.nonzero(in_len >= th).flatten().to(torch.int32),
                  torch.nonzero(out_len >= th).flatten().to(torch.int32))
        graph._gated_long_rows = cached
    return cached


def gated_forward(graph: SymNormGraph, z, sel, gate, bias, logits, save: bool, long_rows=None):
    """``wg_gated_symnorm_forward`` on checked device tensors: (out, t_save, o_save), the last two None unless
    ``save``.  ``long_rows``: another ascending list than the graph's own (tests)."""
    n, E, C = z.shape
    k = sel.shape[1]
    long_rows = _long_rows(graph)[0] if long_rows is None else long_rows
    out = torch.empty_like(logits)
    t_save = torch.empty_like(logits) if save else None
    o_save = torch.empty((n, k, C), dtype=torch.float32, device=z.device) if save else None
    with torch.cuda.device(graph.device):
        check(_lib.load().wg_gated_symnorm_forward(
            graph.n, graph.nnz, ptr(graph.indptr), ptr(graph.indices), int(long_rows.numel()), ptr(long_rows),
            ptr(graph.dinv), C, E, k, ptr(z), ptr(sel), ptr(gate), ptr(bias), ptr(logits), ptr(out), ptr(t_save),
            ptr(o_save), stream_handle(graph.device)), "gated_symnorm_forward")
    return out, t_save, o_save


def gets_head_backward(g_out, out, logits, t_save, o_save):
    """``wg_gets_head_backward``: (g_logits, g_t, g_gate)."""
    n, k, C = o_save.shape
    g_logits, g_t = torch.empty_like(logits), torch.empty_like(logits)
    g_gate = torch.empty((n, k), dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        check(_lib.load().wg_gets_head_backward(n, C, k, ptr(g_out), ptr(out), ptr(logits), ptr(t_save), ptr(o_save),
                                                ptr(g_logits), ptr(g_t), ptr(g_gate), stream_handle(logits.device)),
              "gets_head_backward")
    return g_logits, g_t, g_gate


def gated_transposed(graph: SymNormGraph, sel, gate, g_t, E: int, t_long_rows=None):
    """``wg_gated_symnorm_transposed``: g_z (n, E, C)."""
    n, C = g_t.shape
    k = sel.shape[1]
    t_long_rows = _long_rows(graph)[1] if t_long_rows is None else t_long_rows
    g_z = torch.empty((n, E, C), dtype=torch.float32, device=g_t.device)
    with torch.cuda.device(graph.device):
        check(_lib.load().wg_gated_symnorm_transposed(
            graph.n, graph.nnz, ptr(graph.t_indptr), ptr(graph.t_indices), int(t_long_rows.numel()),
            ptr(t_long_rows), ptr(graph.dinv), C, E, k, ptr(sel), ptr(gate), ptr(g_t), ptr(g_z),
            stream_handle(graph.device)), "gated_symnorm_transposed")
    return g_z


BIAS_BLOCK = 1024


def gate_bias_gradient(sel, gate, g_t, E: int):
    """``G^T g_t`` (E, C) with the dense (n, E) gates ``G``, in torch.  As one (E, n) x (n, C) product the inner
    dimension is n and the GEMM library runs it on a few workgroups; the rows are taken in blocks of ``BIAS_BLOCK`` as
    one batched product whose results are added, the remainder as a plain product."""
    n, C = g_t.shape
    dense = torch.zeros((n, E), dtype=torch.float32, device=gate.device).scatter_(1, sel.long(), gate)
    blocks = n // BIAS_BLOCK
    main = blocks * BIAS_BLOCK
    out = dense[main:].t() @ g_t[main:]
    if blocks:
        out = out + torch.bmm(dense[:main].view(blocks, BIAS_BLOCK, E).transpose(1, 2),
                              g_t[:main].view(blocks, BIAS_BLOCK, C)).sum(0)
    return out


class _GatedSymNormHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, gate, bias, logits, sel, graph):
        save = any(ctx.needs_input_grad[:4])
        out, t_save, o_save = gated_forward(graph, z, sel, gate, bias, logits, save)
        if save:
            ctx.graph, ctx.E = graph, z.shape[1]
            ctx.save_for_backward(out, logits, t_save, o_save, gate, sel)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        out, logits, t_save, o_save, gate, sel = ctx.saved_tensors
        g_out = g_out.to(torch.float32).contiguous()
        g_logits, g_t, g_gate = gets_head_backward(g_out, out, logits, t_save, o_save)
        need = ctx.needs_input_grad
        g_z = gated_transposed(ctx.graph, sel, gate, g_t, ctx.E) if need[0] else None
        g_bias = gate_bias_gradient(sel, gate, g_t, ctx.E) if need[2] else None
        return g_z, g_gate if need[1] else None, g_bias, g_logits if need[3] else None, None, None


def gated_sym_norm_head(graph: SymNormGraph, z: torch.Tensor, sel: torch.Tensor, gate: torch.Tensor,
                        bias: torch.Tensor | None, logits: torch.Tensor, check_selection: bool = True) -> torch.Tensor:
    """``log_softmax(logits * softplus(T))`` with ``T_i = sum_s gate[i, s] (A_hat z[:, sel[i, s], :] + bias[sel[i,
    s]])_i`` on ``graph`` (``wg_gated_symnorm_forward``).  z (n, E, C); sel (n, k) integer, a row's ids distinct and
    in [0, E); gate (n, k); bias (E, C) or None; logits (n, C).  1 <= k <= E <= 4, C <= 256.  Differentiable w.r.t.
    ``z``, ``gate``, ``bias`` and ``logits`` (first order).  ``check_selection=False`` skips the check of ``sel``'s
    values, which waits for the device (a caller whose ids come from ``topk`` has nothing to check, and a stream
    being captured cannot wait)."""
    if not isinstance(graph, SymNormGraph):
        raise ValueError("graph must be a SymNormGraph")
    if z.dim() != 3 or z.shape[0] != graph.n:
        raise ValueError(f"z must be ({graph.n}, E, C), not {tuple(z.shape)}")
    n, E, C = (int(v) for v in z.shape)
    if not 1 <= E <= MAX_EXPERTS or not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"z has E={E} experts and C={C} columns; 1 <= E <= {MAX_EXPERTS} and 1 <= C <= {MAX_CLASSES}")
    if sel.dim() != 2 or sel.shape[0] != n or not 1 <= sel.shape[1] <= E:
        raise ValueError(f"sel must be ({n}, k) with 1 <= k <= {E}, not {tuple(sel.shape)}")
    if sel.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"sel must hold int32 or int64 ids, not {sel.dtype}")
    if tuple(gate.shape) != tuple(sel.shape):
        raise ValueError(f"gate must have sel's shape {tuple(sel.shape)}, not {tuple(gate.shape)}")
    if tuple(logits.shape) != (n, C):
        raise ValueError(f"logits must be ({n}, {C}), not {tuple(logits.shape)}")
    if bias is not None and tuple(bias.shape) != (E, C):
        raise ValueError(f"bias must be ({E}, {C}), not {tuple(bias.shape)}")
    for name, t in (("z", z), ("gate", gate), ("bias", bias), ("logits", logits)):
        if t is not None and not t.is_floating_point():
            raise ValueError(f"{name} must be a floating-point tensor, not {t.dtype}")
    sel = sel.to(device=graph.device, dtype=torch.int32).contiguous()
    if check_selection and n:
        if int(sel.min()) < 0 or int(sel.max()) >= E:
            raise ValueError(f"sel holds ids outside [0, {E})")
        srt = torch.sort(sel, dim=1).values
        if bool((srt[:, 1:] == srt[:, :-1]).any()):
            raise ValueError("sel names an expert twice in one row")
    f32 = dict(device=graph.device, dtype=torch.float32)
    return _GatedSymNormHead.apply(z.to(**f32).contiguous(), gate.to(**f32).contiguous(),
                                   None if bias is None else bias.to(**f32).contiguous(),
                                   logits.to(**f32).contiguous(), sel, graph)


class GCNExpert(nn.Module):
    """GETS.py:24-92 on ``GCNConv``.  ``graph``: the ``SymNormGraph`` all layers run on; ``degrees``: (n,) integer,
    needed when ``"degrees"`` is in ``expert_config`` (the embedding has ``degrees.max() + 1`` rows, GETS.py:78-79)."""

    def __init__(self, num_classes: int, hidden_dim: int, dropout_rate: float, num_layers: int, device,
                 expert_config, feature_dim: int, feature_hidden_dim: int, degree_hidden_dim: int, *,
                 graph: SymNormGraph, degrees: torch.Tensor | None = None):
        super().__init__()
        self.dropout_rate, self.expert_config, self.device = dropout_rate, list(expert_config), device
        in_channels = 0
        if "logits" in self.expert_config:
            in_channels += num_classes
        if "features" in self.expert_config:
            self.proj_feature = nn.Linear(feature_dim, feature_hidden_dim)
            in_channels += feature_hidden_dim
        if "degrees" in self.expert_config:
            if degrees is None:
                raise ValueError("an expert with 'degrees' needs the nodes' degrees")
            in_channels += degree_hidden_dim
            self.register_buffer("degrees", degrees.long(), persistent=False)
            self.degree_embedder = nn.Embedding(int(degrees.max().item()) + 1 if degrees.numel() else 1,
                                                degree_hidden_dim)
        widths = [in_channels] + [hidden_dim] * (num_layers - 2) + [num_classes]
        self.graph = graph
        self.convs = nn.ModuleList(GCNConv(widths[i], widths[i + 1], graph) for i in range(len(widths) - 1))
        self.degree_dim = degree_hidden_dim
        self.to(device)

    def _hidden(self, logits, features):
        inputs = []
        if "logits" in self.expert_config:
            inputs.append(logits)
        if "features" in self.expert_config:
            inputs.append(self.proj_feature(features))
        if "degrees" in self.expert_config:
            inputs.append(self.degree_embedder(self.degrees))
        x = torch.cat(inputs, dim=-1)
        for conv in self.convs[:-1]:
            x = conv(x, relu=True)
            x = F.dropout(x, self.dropout_rate, training=self.training)
        return x

    def last_linear(self, logits, features):
        """(n, C): the last layer's linear map, before its propagation and bias (what the fused head gathers)."""
        return self.convs[-1].lin(self._hidden(logits, features))

    def forward(self, logits, features):
        """The expert's own output, one ``sym_norm_aggregate`` (the unfused path)."""
        return sym_norm_aggregate(self.graph, self.last_linear(logits, features), self.convs[-1].bias)


class GETSCalibrator(nn.Module):
    """GETS.py:242-536.  ``graph``: a sparse graph for the experts instead of the dense ``adj`` given to ``fit``
    (whatever ``SymNormGraph`` takes); ``adj`` then only goes to the base model."""

    def __init__(self, base_model, num_classes, device=None, conf=None, x=None, y=None, adj=None, val_idx=None,
                 num_experts: int = 3, expert_select: int = 2, hidden_dim: int = 64, dropout_rate: float = 0.1,
                 num_layers: int = 2, feature_hidden_dim: int = 32, degree_hidden_dim: int = 16,
                 noisy_gating: bool = True, loss_coef: float = 1e-2, backbone: str = "gcn", *, graph=None,
                 verbose: bool = False, train_degree_embedding: bool = False):
        super().__init__()
        if backbone == "gat":
            raise NotImplementedError("GETS backbone 'gat': PyG's multi-head GATConv is not the CalibAttentionLayer "
                                      "built here, and its attention does not commute with the gate")
        if backbone == "gin":
            raise NotImplementedError("GETS backbone 'gin': GIN applies its MLP after the neighbour sum, so the gate "
                                      "does not commute with the aggregation and the fused head does not apply")
        if backbone != "gcn":
            raise NotImplementedError(f"Backbone {backbone} not implemented")
        if not 1 <= expert_select <= num_experts <= MAX_EXPERTS:
            raise ValueError(f"needs 1 <= expert_select <= num_experts <= {MAX_EXPERTS}, not {expert_select} of "
                             f"{num_experts}")
        if num_classes > MAX_CLASSES:
            raise ValueError(f"num_classes={num_classes} above {MAX_CLASSES}")
        self.device = require_gpu(device)
        self.base_model = base_model.to(self.device)
        self.conf, self.num_classes = conf, int(num_classes)
        self.x = self.y = self.adj = self.val_idx = self.feature_dim = None
        for param in self.base_model.parameters():   # GETS.py:286-287
            param.requires_grad = False
        self.noisy_gating, self.num_experts, self.k = noisy_gating, int(num_experts), int(expert_select)
        self.loss_coef, self.backbone = loss_coef, backbone
        self.hidden_dim, self.dropout_rate, self.num_layers = hidden_dim, dropout_rate, num_layers
        self.feature_hidden_dim, self.degree_hidden_dim = feature_hidden_dim, degree_hidden_dim
        self.expert_configs = [list(c) for c in EXPERT_CONFIGS[:self.num_experts]]
        self.verbose, self.train_degree_embedding = verbose, train_degree_embedding
        self._graph_arg, self.graph = graph, None
        self.experts = self.proj_feature = self.w_gate = self.w_noise = None
        self.softplus, self.softmax = nn.Softplus(), nn.Softmax(1)
        self.gating_noise = None
        self.history = []

    # -- the gate (GETS.py:333-388) ------------------------------------------------------------------------
    def cv_squared(self, x):
        eps = 1e-10
        if x.shape[0] == 1:
            return torch.tensor([0], device=x.device, dtype=x.dtype)
        x = x.double()      # a variance of E sums that nearly cancel: float32 loses several ulps of the quotient
        return x.var() / (x.mean() ** 2 + eps)

    def _gates_to_load(self, gates):
        return (gates > 0).sum(0)

    def _prob_in_top_k(self, clean_values, noisy_values, noise_stddev, noisy_top_values):
        batch, m = clean_values.size(0), noisy_top_values.size(1)
        flat = noisy_top_values.flatten()
        pos_in = torch.arange(batch, device=clean_values.device) * m + self.k
        threshold_if_in = flat.gather(0, pos_in).unsqueeze(1)
        is_in = noisy_values > threshold_if_in
        threshold_if_out = flat.gather(0, pos_in - 1).unsqueeze(1)
        normal = Normal(self.mean.to(clean_values.dtype), self.std.to(clean_values.dtype))
        prob_if_in = normal.cdf((clean_values - threshold_if_in) / noise_stddev)
        prob_if_out = normal.cdf((clean_values - threshold_if_out) / noise_stddev)
        return torch.where(is_in, prob_if_in, prob_if_out)

    def _gating(self, x, train, noise_epsilon=1e-2):
        """(gates (n, E), load, top-k ids (n, k), top-k gates (n, k)) of GETS.py:362-388, in float64 from the float32
        gating input: (n, E) work, whose sums feed ``cv_squared``."""
        x = x.double()
        clean_logits = x @ self.w_gate.double()
        if self.noisy_gating and train:
            noise_stddev = self.softplus(x @ self.w_noise.double()) + noise_epsilon
            noise = torch.randn_like(clean_logits, dtype=torch.float32) if self.gating_noise is None else \
                self.gating_noise
            noisy_logits = clean_logits + noise.to(clean_logits) * noise_stddev
            logits = noisy_logits
        else:
            logits = clean_logits
        top_logits, top_indices = logits.topk(min(self.k + 1, self.num_experts), dim=1)
        top_k_indices = top_indices[:, :self.k]
        top_k_gates = self.softmax(top_logits[:, :self.k])
        gates = torch.zeros_like(logits).scatter(1, top_k_indices, top_k_gates)
        if self.noisy_gating and self.k < self.num_experts and train:
            load = self._prob_in_top_k(clean_logits, noisy_logits, noise_stddev, top_logits).sum(0)
        else:
            load = self._gates_to_load(gates)
        return gates, load, top_k_indices, top_k_gates

    def noisy_top_k_gating(self, x, train, noise_epsilon=1e-2):
        gates, load = self._gating(x, train, noise_epsilon)[:2]
        return gates.to(x.dtype), load

    # -- forward (GETS.py:390-417) -------------------------------------------------------------------------
    def gating_input(self, x, logits):
        return torch.cat([self.proj_feature(x), logits], dim=1)

    def forward(self, x, adj, **kwargs):
        if self.experts is None:
            raise RuntimeError("GETSCalibrator: call fit() first (it builds the networks)")
        x = x.to(self.device)
        if torch.is_tensor(adj):
            adj = adj.to(self.device)
        logits = self.base_model(x, adj, **kwargs)
        gates, load, sel, top_gates = self._gating(self.gating_input(x, logits), self.training)
        self.last_gates, self.last_selection = gates, sel
        importance = gates.sum(0)
        z = torch.stack([expert.last_linear(logits, x) for expert in self.experts], dim=1)
        bias = torch.stack([expert.convs[-1].bias for expert in self.experts])
        self.aux_loss = ((self.cv_squared(importance) + self.cv_squared(load)) * self.loss_coef).float()
        # the selection comes from topk: distinct and in range, nothing to check
        return gated_sym_norm_head(self.graph, z, sel, top_gates, bias, logits, check_selection=False)

    # -- fit / training (GETS.py:419-536) ------------------------------------------------------------------
    def fit(self, adj, features, labels, masks, train: bool = True):
        """GETS.py:419-437: keep the data, build the networks on ``adj``'s graph (or ``graph=``), train.  ``masks[1]``
        is the validation mask.  ``train=False`` stops before ``calib_train`` (to load a ``state_dict``)."""
        self.x = features.to(self.device)
        self.y = labels.to(self.device)
        self.adj = adj.to(self.device) if torch.is_tensor(adj) else adj
        self.val_idx = masks[1].to(self.device)
        self.feature_dim = features.shape[1]
        n = self.x.shape[0]
        graph = self._graph_arg
        if graph is None:
            if not torch.is_tensor(adj):
                raise ValueError("GETSCalibrator: pass graph= when adj is not a dense tensor")
            if adj.dim() != 2 or adj.shape[0] != adj.shape[1]:
                raise ValueError("The adjacency matrix must be a square matrix.")
            graph = self.adj
        self.graph = graph if isinstance(graph, SymNormGraph) else SymNormGraph(graph, n, self.device)
        if self.graph.n != n:
            raise ValueError(f"features has {n} rows but the graph has {self.graph.n} nodes")
        if torch.is_tensor(self.adj) and self.adj.dim() == 2 and not self.adj.is_sparse:
            present = self.adj != 0
            self.degrees = (present.sum(1) + present.sum(0)).long()
        else:
            src, dst = self.graph.edge_list()
            keep = src != dst
            self.degrees = (torch.bincount(src[keep], minlength=n) + torch.bincount(dst[keep], minlength=n)).long()
        self._build_networks()
        if train:
            self.calib_train()
        return self

    def _build_networks(self):
        self.experts = nn.ModuleList(
            GCNExpert(self.num_classes, self.hidden_dim, self.dropout_rate, self.num_layers, self.device, config,
                      self.feature_dim, self.feature_hidden_dim, self.degree_hidden_dim, graph=self.graph,
                      degrees=self.degrees) for config in self.expert_configs)
        self.proj_feature = nn.Linear(self.feature_dim, self.feature_hidden_dim).to(self.device)
        gate_in = self.feature_hidden_dim + self.num_classes
        self.w_gate = nn.Parameter(torch.zeros(gate_in, self.num_experts, device=self.device))
        self.w_noise = nn.Parameter(torch.zeros(gate_in, self.num_experts, device=self.device))
        nn.init.normal_(self.w_gate, mean=0.0, std=0.02)
        nn.init.normal_(self.w_noise, mean=0.0, std=0.02)
        self.register_buffer("mean", torch.tensor([0.0], device=self.device))
        self.register_buffer("std", torch.tensor([1.0], device=self.device))

    def optimizer_parameters(self):
        """What Adam updates: every parameter that requires a gradient, the degree embeddings only with
        ``train_degree_embedding`` (the reference's optimiser never sees them)."""
        return [p for name, p in self.named_parameters()
                if p.requires_grad and (self.train_degree_embedding or "degree_embedder" not in name)]

    def calib_train(self, patience: int = 10, epochs: int = 250, lr: float = 0.01, weight_decay: float = 5e-4):
        t0 = time.time()
        best_loss, patience_counter = float("inf"), patience
        optimizer = torch.optim.Adam(self.optimizer_parameters(), lr=lr, weight_decay=weight_decay)
        self.history = []
        for epoch in range(epochs):
            self.train()
            optimizer.zero_grad()
            output = self(self.x, self.adj)
            loss = F.nll_loss(output[self.val_idx], self.y[self.val_idx]) + self.aux_loss.sum()
            loss.backward()
            optimizer.step()
            value = loss.item()
            self.history.append(value)
            self.eval()
            if self.verbose:
                with torch.no_grad():
                    acc = accuracy(output[self.val_idx], self.y[self.val_idx])
                print(f"epoch: {epoch}", f"loss_calibration: {value:.4f}", f"acc_calibration: {acc:.4f}",
                      f"time: {time.time() - t0:.4f}s")
            if value < best_loss:
                best_loss, patience_counter = value, patience
            else:
                patience_counter -= 1
            if patience_counter <= 0:
                if self.verbose:
                    print(f"Early stopping at epoch {epoch}, best loss: {best_loss:.4f}")
                break
        return self


def calibrate_with_gets(base_model, x, y, adj, val_idx, edge_index=None, **kwargs):
    """GETS.py:539-555: a fitted ``GETSCalibrator``.  ``edge_index``: the experts' graph when it is not ``adj``'s
    (``graph=``).  Keywords: the constructor's."""
    if edge_index is not None:
        kwargs.setdefault("graph", edge_index)
    num_classes = kwargs.pop("num_classes", int(y.max().item()) + 1)
    cal = GETSCalibrator(base_model, num_classes, kwargs.pop("device", None), kwargs.pop("conf", None), **kwargs)
    return cal.fit(adj, x, y, (None, val_idx, None))
