"""SimCalib calibrator whose similarity temperature runs on the HIP path (reference
``calibration/SimCalib.py``).

In ``SimCalib.forward`` (SimCalib.py:78-111) every node gets a temperature from a softmax over its cosine similarity
to every validation node: the reference materialises the (N, N_val) similarity matrix and its softmax, and autograd
keeps both.  Here:

* ``SimilarityBank(features_val, val_confidence, epsilon)``: the L2-normalised validation rows and
  ``1 / (confidence + epsilon)``, built once with torch (SimCalib.py:52-53, :102);
* ``similarity_temperature(latent, bank, inv_conf, tau, t_min, t_max)``: SimCalib.py:49-58, :91-106 as one fused pass
  per direction (``wg_simcalib_forward`` / ``wg_simcalib_backward``, ``csrc/simcalib.hip``), with no (N, N_val)
  buffer; differentiable w.r.t. ``latent`` only (first order), the clamp and its gradient mask included;
* ``SimCalib(base_model, features, labels, adj, val_mask, k=10, epsilon=1e-8, *, tau=0.1)`` with the reference's
  surface: ``forward(x, adj, **kwargs)``, ``latent_feature_1``, ``compute_similarity_matrix`` (dense, for small
  inputs only) and ``calib_train`` / ``fit`` (post-hoc: nothing to train).

Differences: an empty validation set raises ``ValueError`` (the reference's softmax over zero columns sums to 0 and
the clamp turns it into 0.1 for every node, silently); ``tau`` is a constructor keyword (the reference hard-codes
0.1, SimCalib.py:95); ``adj`` may be a ``RowNormalizedAdjacency``; with a ``SparseCompatibleGCN`` base model the
hidden layer is computed once and used both as the latent features and on the way to the logits (the base model is in
``eval()``, SimCalib.py:82, so dropout is the identity and this equals the reference's two evaluations), and
``probe=`` (an ``EdgeProbe``) receives the gradient w.r.t. the adjacency through the logits AND the temperatures;
there is no CPU path.  Not built: gradients w.r.t. the bank or the confidences (the reference detaches both), second
order gradients, row shards, a hard top-``k`` (``k`` is stored and unused, as in the reference), latent widths above
``max_latent_width()``.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import check, ptr
from .gcn import EdgeProbe, RowNormalizedAdjacency, SparseCompatibleGCN, propagate
from .laplacian import require_gpu, stream_handle


def max_latent_width() -> int:
    """The widest latent row the kernels take (``wg_simcalib_max_d``)."""
    return int(_lib.load().wg_simcalib_max_d())


class SimilarityBank:
    """The validation side of the similarity temperature, built once: ``bank`` = ``F.normalize(features_val)``
    (m, d) and ``inv_conf`` = ``1 / (val_confidence + epsilon)`` (m), float32 on the device, detached."""

    def __init__(self, features_val: torch.Tensor, val_confidence: torch.Tensor, epsilon: float = 1e-8, device=None):
        device = require_gpu(device if device is not None else (features_val.device if features_val.is_cuda else None))
        if features_val.dim() != 2:
            raise ValueError(f"features_val must be (m, d), not {tuple(features_val.shape)}")
        if features_val.shape[0] == 0:
            raise ValueError("SimCalib needs at least one validation node (the reference would give every node the "
                             "temperature 0.1)")
        if tuple(val_confidence.shape) != (features_val.shape[0],):
            raise ValueError("val_confidence must have one entry per validation row")
        self.device = device
        fv = features_val.detach().to(device=device, dtype=torch.float32)
        self.bank = F.normalize(fv, p=2, dim=1).contiguous()                       # SimCalib.py:53
        self.inv_conf = (1.0 / (val_confidence.detach().to(device=device, dtype=torch.float32)
                                + epsilon)).contiguous()                           # SimCalib.py:102
        self.m, self.d = (int(s) for s in self.bank.shape)


def _forward(latent, bank, inv_conf, tau):
    n, d = latent.shape
    t = torch.empty(n, dtype=torch.float32, device=latent.device)
    stats = torch.empty(n, 3, dtype=torch.float64, device=latent.device)
    with torch.cuda.device(latent.device):
        check(_lib.load().wg_simcalib_forward(n, bank.shape[0], d, ptr(latent), ptr(bank), ptr(inv_conf), float(tau),
                                              ptr(t), ptr(stats), stream_handle(latent.device)), "simcalib_forward")
    return t, stats


class _SimilarityTemperature(torch.autograd.Function):
    @staticmethod
    def forward(ctx, latent, bank, inv_conf, tau, t_min, t_max):
        t, stats = _forward(latent, bank, inv_conf, tau)
        ctx.save_for_backward(latent, bank, inv_conf, t, stats)
        ctx.tau, ctx.t_min, ctx.t_max = tau, t_min, t_max
        return t.clamp(min=t_min, max=t_max)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        latent, bank, inv_conf, t, stats = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        # torch's clamp passes the gradient where min <= t <= max (a NaN t gets none)
        g = (g.to(torch.float32) * ((t >= ctx.t_min) & (t <= ctx.t_max))).contiguous()
        gx = torch.empty_like(latent)
        n, d = latent.shape
        with torch.cuda.device(latent.device):
            check(_lib.load().wg_simcalib_backward(n, bank.shape[0], d, ptr(latent), ptr(bank), ptr(inv_conf),
                                                   float(ctx.tau), ptr(stats), ptr(g), ptr(gx),
                                                   stream_handle(latent.device)), "simcalib_backward")
        return gx, None, None, None, None, None


def _prepare(latent, bank, inv_conf, tau):
    if isinstance(bank, SimilarityBank):
        if inv_conf is not None:
            raise ValueError("pass either a SimilarityBank or (bank, inv_conf)")
        bank, inv_conf = bank.bank, bank.inv_conf
    device = require_gpu(bank.device if bank.is_cuda else None)
    if latent.dim() != 2 or bank.dim() != 2 or latent.shape[1] != bank.shape[1]:
        raise ValueError(f"expected (n, d) latent rows and an (m, d) bank, got {tuple(latent.shape)} and "
                         f"{tuple(bank.shape)}")
    if bank.shape[0] == 0:
        raise ValueError("similarity_temperature needs at least one bank row")
    if inv_conf is None or tuple(inv_conf.shape) != (bank.shape[0],):
        raise ValueError("inv_conf must have one entry per bank row")
    if not (float(tau) > 0.0):
        raise ValueError(f"tau must be positive, not {tau}")
    latent = latent.to(device=device, dtype=torch.float32).contiguous()
    bank = bank.detach().to(device=device, dtype=torch.float32).contiguous()
    inv_conf = inv_conf.detach().to(device=device, dtype=torch.float32).contiguous()
    return latent, bank, inv_conf


def similarity_temperature(latent: torch.Tensor, bank, inv_conf: torch.Tensor | None = None, tau: float = 0.1,
                           t_min: float = 0.1, t_max: float = 5.0) -> torch.Tensor:
    """``clamp(softmax(normalize(latent) @ bank.T / tau, dim=1) @ inv_conf, t_min, t_max)`` (SimCalib.py:49-58,
    :91-106) without the (n, m) matrices.  ``bank`` (m, d): L2-normalised rows (or a ``SimilarityBank``, then
    ``inv_conf`` stays None); ``latent`` (n, d) is normalised in the kernel.  Returns (n,) float32 temperatures,
    differentiable w.r.t. ``latent`` only; clamped rows get a zero gradient, as with ``torch.clamp``.  n == 0 gives
    an empty result; an empty bank raises ``ValueError``."""
    latent, bank, inv_conf = _prepare(latent, bank, inv_conf, tau)
    if latent.shape[0] == 0:
        return latent.new_zeros(0)
    return _SimilarityTemperature.apply(latent, bank, inv_conf, float(tau), float(t_min), float(t_max))


def raw_similarity_temperature(latent: torch.Tensor, bank, inv_conf: torch.Tensor | None = None,
                               tau: float = 0.1) -> torch.Tensor:
    """The unclamped temperatures (SimCalib.py:105), no gradient."""
    latent, bank, inv_conf = _prepare(latent.detach(), bank, inv_conf, tau)
    if latent.shape[0] == 0:
        return latent.new_zeros(0)
    return _forward(latent, bank, inv_conf, float(tau))[0]


class SimCalib(nn.Module):
    """SimCalib.py:18-120 with the reference's positional surface.  ``adj``: the dense (N, N) adjacency on any
    device, or a ``RowNormalizedAdjacency``."""

    def __init__(self, base_model, features, labels, adj, val_mask, k: int = 10, epsilon: float = 1e-8, *,
                 tau: float = 0.1):
        super().__init__()
        self.device = require_gpu()
        self.k, self.epsilon, self.tau = k, epsilon, float(tau)
        self.x = features.to(self.device)
        self.y = labels.to(self.device)
        self.adj = adj.to(self.device) if torch.is_tensor(adj) else adj
        self.val_mask = val_mask.to(self.device)
        self.base_model = base_model.to(self.device)
        self._initialize_calibration()

    @property
    def _sparse_base(self) -> bool:
        return isinstance(self.base_model, SparseCompatibleGCN)

    def _initialize_calibration(self):
        """SimCalib.py:38-47: the validation rows of the latent features and their confidences."""
        self.base_model.eval()
        with torch.no_grad():
            logits, latent = self._logits_and_latent(self.x, self.adj)
            self.features_val = latent[self.val_mask]
            self.val_confidence = F.softmax(logits[self.val_mask], dim=1).max(dim=1).values
        self.bank = SimilarityBank(self.features_val, self.val_confidence, self.epsilon, self.device)

    def compute_similarity_matrix(self, X1, X2):
        """SimCalib.py:49-58, dense: an (n1, n2) matrix, for small inputs only (``forward`` never builds it)."""
        return torch.mm(F.normalize(X1, p=2, dim=1), F.normalize(X2, p=2, dim=1).t())

    def _operator(self, adj) -> RowNormalizedAdjacency:
        if isinstance(adj, RowNormalizedAdjacency):
            return adj
        if self._sparse_base:
            return self.base_model.operator(adj)
        if adj.requires_grad:
            raise NotImplementedError("SimCalib has no gradient w.r.t. a dense adj leaf (N x N); use a "
                                      "SparseCompatibleGCN base model and probe=EdgeProbe(rows, cols)")
        return RowNormalizedAdjacency.from_dense(adj.to(self.device))

    def latent_feature_1(self, x, adj, probe: EdgeProbe | None = None):
        """SimCalib.py:60-76: ``relu(gc1(adj_norm @ x))``, the propagation on the HIP SpMM."""
        x = x.to(self.device)
        return F.relu(self.base_model.gc1(propagate(self._operator(adj), x, probe)))

    def _logits_and_latent(self, x, adj, **kwargs):
        x = x.to(self.device)
        if self._sparse_base:
            probe = kwargs.pop("probe", None)
            if kwargs:
                raise TypeError(f"unexpected arguments {sorted(kwargs)}")
            op = self._operator(adj)
            h = F.relu(self.base_model.gc1(propagate(op, x, probe)))      # model.py:47-48 = SimCalib.py:72-73
            return self.base_model.gc2(propagate(op, h, probe)), h        # model.py:51-52 (eval: no dropout)
        if not hasattr(self.base_model, "gc1"):
            raise ValueError("SimCalib needs a base model with a first layer gc1 (SimCalib.py:73)")
        if torch.is_tensor(adj):
            adj = adj.to(self.device)
        return self.base_model(x, adj, **kwargs), self.latent_feature_1(x, adj)   # SimCalib.py:85, :88

    def temperatures(self, latent):
        """SimCalib.py:91-106 for the given latent rows."""
        return similarity_temperature(latent, self.bank, None, self.tau, 0.1, 5.0)

    def forward(self, x, adj, **kwargs):
        self.base_model.eval()                                            # SimCalib.py:82
        logits, latent = self._logits_and_latent(x, adj, **kwargs)
        t = self.temperatures(latent)
        return F.log_softmax(logits / t.unsqueeze(1), dim=1)              # SimCalib.py:109-111

    def calib_train(self):
        """SimCalib.py:113-120: post-hoc, nothing to train."""
        return self

    fit = calib_train
