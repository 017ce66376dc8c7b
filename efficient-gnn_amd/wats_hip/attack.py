"""``Calib_FGA`` of the reference (``calib_attack/calib_fga.py``) on the sparse path (DESIGN.md 4.3 "Attack step").

Same class name, constructor, method names, positional order and keywords as the reference, so an attack script
switches over by changing the import.  One step is

* one forward of the surrogate with ``EdgeProbe.for_target(n, t)`` and ``torch.autograd.grad`` at ``probe.delta``
  for the loss and, where the reference reranks, for ``p_max`` and ``p_smax`` (``calib_fga.py:877-890``);
* :func:`flip_select` (``wg_flip_select``, ``csrc/attack.hip``): the scores of ``:880-897`` and their argmax in one
  pass, without a dense row of the adjacency;
* the flip as a ``with_flips`` view of the adjacency the attack started from;
* the candidate's logits: :func:`target_logits` (``wg_target_logits``: the 2-hop ball of ``t`` only) when the
  surrogate is a bare ``SparseCompatibleGCN`` or a ``WATS`` over one and the graph is unweighted, else one no-grad
  forward through the view.

The adjacency of a step is the start adjacency plus a *toggle set*: the partners ``j`` of ``t`` whose entries
``(t, j)`` / ``(j, t)`` have been flipped an odd number of times.  The reference's quirks are kept: the rerank reads
the row gradient only, compares with ``> 0`` and masks the self entry with ``-10``; the "beam" pops up to
``beam_width`` members that each yield one child, so it holds one; ``attack`` / ``rerank*`` stop at the first label
change, the beam method does not; the best-so-far rules use ``<=`` / ``>=`` / ``<`` as written per method;
``strategy='max'`` of ``attack`` calls ``kl_divergence_target`` with two arguments and raises ``TypeError``, as the
reference does.  Not kept: ``check_adj``'s dense ``(N, N)`` symmetry test.

Results: ``flips`` (the partners in the order flipped), ``best_flips`` (the toggle set that gave the best
confidence, ascending), ``modified_op`` (that adjacency as a view: ``.materialize()`` / ``.to_graph()``),
``modified_adj`` (a dense tensor when ``ori_adj`` was dense; otherwise ``AttributeError``), ``trace`` (one dict per
evaluated candidate: partner, logits row, label, confidence).

``Calib_FGA.attack_many`` runs one of the four methods for many targets of one graph in lock step (DESIGN.md 4.3
"Batched attack step"): the gradient's row and column in closed form by :func:`fga_scores` (``wg_fga_scores``,
``csrc/fga.hip``), the children by ``wg_trial_logits``, no whole-graph pass in the loop.

Further down: ``Calib_IGA`` (``calib_attack/calib_iga.py``) and the random baselines ``Calib_Random`` / ``Calib_RND``
(``calib_attack/calib_random.py``, ``calib_rnd.py``; DESIGN.md 4.3 "Random trials") with ``trial_logits``
(``wg_trial_logits``: all trials of a step in one launch).
"""
from __future__ import annotations

import ctypes
import heapq
import time

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, ptr
from .flips import FlippedAdjacency
from .gcn import EdgeProbe, RowNormalizedAdjacency, SparseCompatibleGCN
from .laplacian import require_gpu, stream_handle

try:  # optional: the reference's verbose tables
    from tabulate import tabulate as _tabulate
except ImportError:  # pragma: no cover
    _tabulate = None


# ------------------------------------------------------------------------------------------------ the loss functions
def _target_probs(logits, labels):
    probs = F.softmax(logits, dim=1)
    return probs, probs[torch.arange(len(labels)), labels]


def underconfidence_objective(logits, labels):
    """``-mean(p_label - max of the other classes' p)`` (``calib_attack_loss.py:158-178``)."""
    probs, own = _target_probs(logits, labels)
    keep = torch.ones_like(probs)
    keep[torch.arange(len(labels)), labels] = 0
    others, _ = torch.max(probs * keep, dim=1)
    return -torch.mean(own - others)


def overconfidence_objective(logits, labels):
    """``-mean(1 - p_label)`` (``calib_attack_loss.py:181-208``)."""
    _, own = _target_probs(logits, labels)
    return -torch.mean(1 - own)


def kl_divergence_with_uniform(logits, labels):
    """``-KL(uniform || softmax(logits))``, batch mean (``calib_attack_loss.py:68-79``); ``labels`` is unused."""
    probs = F.softmax(logits, dim=1)
    uniform = torch.full_like(probs, 1.0 / logits.shape[1])
    return -F.kl_div(probs.log(), uniform, reduction='batchmean')


def kl_divergence_target(logits, target_label, res_gt):
    """``-KL(target distribution || softmax(logits))`` with the reference's four-way target distribution
    (``calib_attack_loss.py:101-154``)."""
    probs = F.softmax(logits, dim=1)
    predicted = torch.argmax(probs, dim=1)
    n_classes = logits.shape[1]
    dist = torch.zeros_like(probs)
    for i in range(logits.shape[0]):
        if predicted[i] == target_label[i]:
            if res_gt[i] == target_label[i]:
                dist[i] = torch.full((n_classes,), 1.0 / n_classes, dtype=probs.dtype, device=probs.device)
            else:
                dist[i, target_label[i]] = 1.0
        elif res_gt[i] != target_label[i]:
            dist[i] = torch.full((n_classes,), 1.0 / (n_classes - 1), dtype=probs.dtype, device=probs.device)
            dist[i, target_label[i]] = 0.0
        else:
            dist[i, target_label[i]] = 0.5
            dist[i, predicted[i]] = 0.5
    return -F.kl_div(probs.log(), dist, reduction='batchmean')


def _restore_loss(output, label):
    return -F.nll_loss(output, label)


# ------------------------------------------------------------------------------------------------ the two kernels
def select_workspace(device) -> torch.Tensor:
    """The buffer ``wg_flip_select`` merges its workgroups' partial lists in (reusable across calls on a stream)."""
    nbytes = ctypes.c_int64(0)
    check(_lib.load().wg_flip_select_workspace(ctypes.byref(nbytes)), "flip_select_workspace")
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)


def flip_select(n: int, t: int, grad_loss: torch.Tensor, indptr: torch.Tensor, indices: torch.Tensor,
                values: torch.Tensor | None = None, toggled: torch.Tensor | None = None,
                grad_pmax: torch.Tensor | None = None, grad_psmax: torch.Tensor | None = None,
                p_top2: torch.Tensor | None = None, topk: int = 1, n_workgroups: int = 0, return_scores: bool = False,
                workspace: torch.Tensor | None = None):
    """``wg_flip_select``: ``(best_ids int32 [topk], best_scores float32 [topk])`` and, with ``return_scores``, the
    score vector ``[n]``.  Tensors are taken as they are (device float32 / int64 / int32, any 4-byte alignment)."""
    device = require_gpu(grad_loss.device if grad_loss.is_cuda else None)
    lib = _lib.load()
    best_ids = torch.empty(topk, dtype=torch.int32, device=device)
    best_scores = torch.empty(topk, dtype=torch.float32, device=device)
    scores = torch.empty(n, dtype=torch.float32, device=device) if return_scores else None
    if workspace is None:
        workspace = select_workspace(device)
    n_toggled = 0 if toggled is None else int(toggled.numel())
    with torch.cuda.device(device):
        check(lib.wg_flip_select(n, t, ptr(grad_loss), ptr(grad_pmax), ptr(grad_psmax), ptr(p_top2), ptr(indptr),
                                 ptr(indices) if indices is not None and indices.numel() else None, ptr(values),
                                 n_toggled, ptr(toggled) if n_toggled else None, topk, n_workgroups, ptr(workspace),
                                 ptr(scores), ptr(best_ids), ptr(best_scores), stream_handle(device)), "flip_select")
    return (best_ids, best_scores, scores) if return_scores else (best_ids, best_scores)


def target_logits(n: int, indptr: torch.Tensor, indices: torch.Tensor, z: torch.Tensor, b1: torch.Tensor,
                  W2: torch.Tensor, b2: torch.Tensor, t: int, candidates) -> torch.Tensor:
    """``wg_target_logits``: the ``(B, C)`` logits of node ``t`` of the two-layer base model under the candidate
    toggle sets ``candidates`` (a list of lists of partners, or ``(cand_ptr, cand_ids)`` int32 device tensors that
    were checked by the caller).  ``z = x @ W1.T``."""
    device = require_gpu(z.device if z.is_cuda else None)
    if isinstance(candidates, tuple):
        cand_ptr, cand_ids = candidates
    else:
        ptrs, ids = [0], []
        for S in candidates:
            S = [int(j) for j in S]
            if any(b <= a for a, b in zip(S, S[1:])) or any(j == int(t) or not 0 <= j < n for j in S):
                raise ValueError("a candidate's partners must be ascending, distinct, inside [0, n) and not the target")
            ids += S
            ptrs.append(len(ids))
        cand_ptr = torch.tensor(ptrs, dtype=torch.int32).to(device)
        cand_ids = torch.tensor(ids, dtype=torch.int32).to(device)
    B, C, Hd = int(cand_ptr.numel()) - 1, int(W2.shape[0]), int(z.shape[1])
    if z.shape[0] != n or W2.shape[1] != Hd or b1.numel() != Hd or b2.numel() != C:
        raise ValueError("target_logits: z (n, Hd), b1 [Hd], W2 (C, Hd), b2 [C] expected")
    out = torch.empty((B, C), dtype=torch.float32, device=device)
    nnz = int(indices.numel())
    with torch.cuda.device(device):
        check(_lib.load().wg_target_logits(n, nnz, ptr(indptr), ptr(indices) if nnz else None, Hd, ptr(z), ptr(b1),
                                           ptr(W2), ptr(b2), C, int(t), B, ptr(cand_ptr),
                                           ptr(cand_ids) if cand_ids.numel() else None, ptr(out),
                                           stream_handle(device)), "target_logits")
    return out


def fga_scores_workspace(n: int, Hd: int, B: int, G: int, local_cap: int, device) -> torch.Tensor:
    """The buffer of ``wg_fga_scores``: the coefficients, the local lists (``local_cap`` entries: at least the sum over
    the targets of ``|N(t)| + |S_b|``) and the partial top-k lists."""
    nbytes = ctypes.c_int64(0)
    check(_lib.load().wg_fga_scores_workspace(n, Hd, B, G, local_cap, ctypes.byref(nbytes)), "fga_scores_workspace")
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)


def _pack_toggles(n, targets, toggles, device):
    """(targets, tog_ptr, tog_ids) int32 on the device (one copy) from host lists, checked"""
    ptrs, ids = [0], []
    for t, S in zip(targets, toggles):
        S = [int(j) for j in S]
        if not 0 <= int(t) < n:
            raise ValueError(f"target {t} outside [0, {n})")
        if any(b <= a for a, b in zip(S, S[1:])) or any(j == int(t) or not 0 <= j < n for j in S):
            raise ValueError("a target's toggled partners must be ascending, distinct, inside [0, n) and not the target")
        ids += S
        ptrs.append(len(ids))
    from .flips import _upload
    d = _upload(device, dict(t=torch.tensor([int(t) for t in targets], dtype=torch.int32),
                             ptr=torch.tensor(ptrs, dtype=torch.int32), ids=torch.tensor(ids, dtype=torch.int32)))
    return d["t"], d["ptr"], d["ids"]


def fga_scores(n: int, indptr: torch.Tensor, indices: torch.Tensor, z: torch.Tensor, h: torch.Tensor, b1: torch.Tensor,
               W2: torch.Tensor, targets, toggles, g_logits: torch.Tensor, rerank: torch.Tensor | None = None,
               p_top2: torch.Tensor | None = None, topk: int = 1, n_workgroups: int = 0, return_grads: bool = False,
               return_scores: bool = False, workspace: torch.Tensor | None = None, local_cap: int | None = None):
    """``wg_fga_scores``: ``(best_ids int32 (B, topk), best_scores float32 (B, topk))`` and, on request, the gradients
    ``(B, G, 2 n)`` in the target probe's layout and the score matrix ``(B, n)`` (``calib_fga.py:864-898`` for every
    target in one pass over ``z`` and ``h``).  ``targets`` / ``toggles``: host lists (a target and its ascending
    toggled partners), or int32 device tensors ``targets`` and ``toggles = (tog_ptr, tog_ids)`` that the caller
    checked.  ``g_logits (B, G, C)``: d L / d out_t of the loss and, with ``G == 3``, of ``p_max`` and ``p_smax``;
    ``rerank`` int32 ``[B]`` and ``p_top2 (B, 2)`` go with ``G == 3``.  ``local_cap``: see ``fga_scores_workspace``
    (computed with one host read when not given)."""
    device = require_gpu(z.device if z.is_cuda else None)
    if isinstance(toggles, tuple):
        tog_ptr, tog_ids = toggles
    else:
        targets, tog_ptr, tog_ids = _pack_toggles(n, targets, toggles, device)
    B, Hd, C = int(targets.numel()), int(z.shape[1]), int(W2.shape[0])
    if g_logits.dim() != 3 or g_logits.shape[0] != B or g_logits.shape[2] != C or int(tog_ptr.numel()) != B + 1:
        raise ValueError("fga_scores: g_logits (B, G, C) and tog_ptr [B + 1] of the same targets expected")
    G = int(g_logits.shape[1])
    if z.shape[0] != n or h.shape != z.shape or W2.shape[1] != Hd or b1.numel() != Hd:
        raise ValueError("fga_scores: z, h (n, Hd), b1 [Hd], W2 (C, Hd) expected")
    if rerank is not None and (G != 3 or p_top2 is None or tuple(p_top2.shape) != (B, 2) or rerank.numel() != B):
        raise ValueError("fga_scores: rerank [B] needs G == 3 and p_top2 (B, 2)")
    if local_cap is None:
        tl = targets.long()
        local_cap = int((indptr[tl + 1] - indptr[tl]).sum()) + int(tog_ids.numel())
    best_ids = torch.empty((B, topk), dtype=torch.int32, device=device)
    best_scores = torch.empty((B, topk), dtype=torch.float32, device=device)
    grads = torch.empty((B, G, 2 * n), dtype=torch.float32, device=device) if return_grads else None
    scores = torch.empty((B, n), dtype=torch.float32, device=device) if return_scores else None
    if workspace is None:
        workspace = fga_scores_workspace(n, Hd, B, G, local_cap, device)
    nnz = int(indices.numel())
    with torch.cuda.device(device):
        check(_lib.load().wg_fga_scores(n, nnz, ptr(indptr), ptr(indices) if nnz else None, Hd, ptr(z), ptr(h), ptr(b1),
                                        ptr(W2), C, B, ptr(targets), ptr(tog_ptr),
                                        ptr(tog_ids) if tog_ids.numel() else None, G, ptr(g_logits), ptr(rerank),
                                        ptr(p_top2), topk, n_workgroups, local_cap, ptr(workspace), ptr(grads),
                                        ptr(scores), ptr(best_ids), ptr(best_scores), stream_handle(device)),
              "fga_scores")
    out = (best_ids, best_scores)
    if return_grads:
        out += (grads,)
    if return_scores:
        out += (scores,)
    return out


def _loss_rows(out, kinds, labels, res_gt=None):
    """The criteria of ``Calib_FGA`` applied to each row of ``out (B, C)`` on its own (a batch of one: the mean of one
    value), as a vector ``[B]``: ``kinds[b]`` is ``over`` / ``under`` (the two objectives), ``kl`` (``kl_divergence_
    with_uniform``), ``target`` (``kl_divergence_target`` with ``labels[b]`` as the target label and ``res_gt[b]``) or
    ``restore`` (``-nll_loss``).  A row's gradient does not depend on which rows share the call."""
    loss = out.new_zeros(out.shape[0])
    n_classes = out.shape[1]
    for kind in sorted(set(kinds)):
        # each criterion on its own rows only: a row never meets the log of another kind's underflowed probability
        where = [b for b, k in enumerate(kinds) if k == kind]
        idx = torch.tensor(where, device=out.device)
        o, lab = out[idx], labels[idx]
        rows = torch.arange(len(where), device=out.device)
        if kind == "restore":
            value = o[rows, lab]
        else:
            probs = F.softmax(o, dim=1)
            own = probs[rows, lab]
            if kind == "over":
                value = -(1 - own)
            elif kind == "under":
                keep = torch.ones_like(probs)
                keep[rows, lab] = 0
                others, _ = torch.max(probs * keep, dim=1)
                value = -(own - others)
            else:
                dist = torch.full_like(probs, 1.0 / n_classes)
                if kind == "target":
                    predicted = torch.argmax(probs, dim=1)
                    for i, b in enumerate(where):
                        tl, pred, gt = int(lab[i]), int(predicted[i]), int(res_gt[b])
                        dist[i] = 0.0
                        if pred == tl:
                            if gt == tl:
                                dist[i] = 1.0 / n_classes
                            else:
                                dist[i, tl] = 1.0
                        elif gt != tl:
                            dist[i] = 1.0 / (n_classes - 1)
                            dist[i, tl] = 0.0
                        else:
                            dist[i, tl] = 0.5
                            dist[i, pred] = 0.5
                value = -F.kl_div(probs.log(), dist, reduction='none').sum(dim=1)
        loss = loss.index_put((idx,), value)
    return loss


def _row_gradients(raw, head, kinds, labels, rerank, res_gt=None):
    """``g_logits (B, G, C)`` = d / d raw of each row's loss and, where any row reranks (``G == 3``), of its ``p_max``
    and ``p_smax`` (``calib_fga.py:877-890`` on the ``(B, C)`` block of base logits ``raw`` under the calibrator's
    row map ``head``), and ``p_top2 (B, 2)``."""
    leaf = raw.detach().clone().requires_grad_(True)
    out = head(leaf)
    loss = _loss_rows(out, kinds, labels, res_gt).sum()
    need = any(rerank)
    gs = [torch.autograd.grad(loss, leaf, retain_graph=need, allow_unused=True)[0]]
    top2 = None
    if need:
        top2 = torch.topk(F.softmax(out, dim=1), 2, dim=1)[0]
        gs.append(torch.autograd.grad(top2[:, 0].sum(), leaf, retain_graph=True)[0])
        gs.append(torch.autograd.grad(top2[:, 1].sum(), leaf)[0])
        top2 = top2.detach().contiguous()
    gs = [torch.zeros_like(leaf) if g is None else g for g in gs]
    return torch.stack(gs, dim=1).contiguous(), top2


class _ManyResult(dict):
    """One target's result of ``attack_many``; ``modified_op`` is made when it is first read with ``r["modified_op"]``
    or ``r.get("modified_op")`` (a ``with_flips`` view).  ``keys()``, ``items()`` and ``dict(r)`` hold it only after
    that first read."""

    def __init__(self, start, **fields):
        super().__init__(**fields)
        self._start = start

    def __missing__(self, key):
        if key != "modified_op":
            raise KeyError(key)
        best = self["best_flips"]
        self[key] = self._start.with_flips([self["target"]] * len(best), best)
        return self[key]

    def __contains__(self, key):
        return key == "modified_op" or super().__contains__(key)

    def get(self, key, default=None):
        return self[key] if key in self else default


METHODS = ("attack", "rerank_attack", "rerank_hybridloss_attack", "flip_beam_hybridloss_attack")


# ------------------------------------------------------------------------------------------------ the attack
class Calib_FGA(torch.nn.Module):
    """The reference's calibrated fast gradient attack on a sparse surrogate.  ``local_eval=False`` evaluates every
    candidate by a forward through the flipped view (always the case for surrogates other than
    ``SparseCompatibleGCN`` or ``WATS`` over it, and for valued graphs)."""

    def __init__(self, model, feature_shape=None, attack_features=False, device=None, logits=True, *,
                 local_eval: bool = True, record_scores: bool = False):
        super().__init__()
        assert not attack_features, "not support attacking features"
        self.surrogate = model
        self.attack_structure, self.attack_features = True, False
        self.device = require_gpu(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.local_eval, self.record_scores = bool(local_eval), bool(record_scores)
        self.modified_features = None
        self.modified_op = None
        self.flips, self.best_flips, self.trace = [], [], []
        self._z_key = self._z = None
        self._workspace = None

    def __getattr__(self, name):
        if name == "modified_adj":
            raise AttributeError("modified_adj is a dense (N, N) tensor and exists only when ori_adj was dense; "
                                 "read modified_op (.materialize() gives an operator, .to_graph() a CSR)")
        return super().__getattr__(name)

    # -------------------------------------------------------------------------------------------- logging
    @staticmethod
    def _log_attack_header(strategy, target_node, budget, original_label, original_confidence):
        print("\n" + "=" * 80)
        print(f"[{strategy.upper()}][Node {target_node}] Starting attack | budget={budget}")
        print(f"Baseline label={original_label} | confidence={original_confidence:.4f}")
        print("-" * 80)

    @staticmethod
    def _log_iteration(strategy, target_node, step, budget, action, edge_idx, prev_confidence, new_confidence,
                       baseline_confidence, predicted_label, loss=None, log_rows=None):
        step_delta, total_delta = new_confidence - prev_confidence, new_confidence - baseline_confidence
        message = (f"[{strategy.upper()}][Node {target_node}][Step {step}/{budget}] "
                   f"{action} edge ({target_node}, {edge_idx}) | pred {predicted_label} | "
                   f"conf {new_confidence:.4f} (Δ step {step_delta:+.4f}, Δ total {total_delta:+.4f})")
        if loss is not None:
            message += f" | loss {loss:.4f}"
        print(message)
        if log_rows is not None:
            log_rows.append([step, action, predicted_label, f"{new_confidence:.4f}", f"{step_delta:+.4f}",
                             f"{total_delta:+.4f}", f"{loss:.4f}" if loss is not None else "-"])

    @staticmethod
    def _log_attack_summary(strategy, target_node, used, budget, original_label, final_label, baseline_confidence,
                            final_confidence):
        status = "preserved" if final_label == original_label else "CHANGED"
        print(f"[{strategy.upper()}][Node {target_node}] Perturbations used: {used}/{budget}")
        print(f"Label: {original_label} -> {final_label} ({status})")
        print(f"Confidence: {baseline_confidence:.4f} -> {final_confidence:.4f} "
              f"(Δ {final_confidence - baseline_confidence:+.4f})")
        print("=" * 80 + "\n")

    @staticmethod
    def _print_table(rows, headers):
        if _tabulate is not None:
            print(_tabulate(rows, headers=headers, tablefmt="grid"))
        else:
            print(" | ".join(headers))
            for row in rows:
                print(" | ".join(str(v) for v in row))

    # -------------------------------------------------------------------------------------------- one attack's state
    def _begin(self, ori_features, ori_adj, target_node):
        """The start adjacency as an operator or view, its CSR, and what the fast evaluation needs."""
        self._dense = None
        self.__dict__.pop("modified_adj", None)
        if torch.is_tensor(ori_adj):
            self._dense = ori_adj.detach()
            start = RowNormalizedAdjacency.from_dense(self._dense.to(self.device))
        elif isinstance(ori_adj, RowNormalizedAdjacency):
            start = ori_adj
        else:
            raise TypeError("ori_adj must be a dense tensor, a RowNormalizedAdjacency or a FlippedAdjacency")
        self._start = start
        self._n, self._t = int(start.n), int(target_node)
        if not 0 <= self._t < self._n:
            raise ValueError(f"target {self._t} outside [0, {self._n})")
        self._x = ori_features.detach().to(start.device)
        self._csr = start.csr() if isinstance(start, FlippedAdjacency) else (start.indptr, start.indices, start.values)
        self._probe = EdgeProbe.for_target(self._n, self._t, device=start.device)
        self.flips, self.best_flips, self.trace = [], [], []
        self._last_scores = None
        self.surrogate.eval()
        if self._workspace is None:
            self._workspace = select_workspace(self.device)
        self._local = self._local_model()

    def _local_model(self):
        """(gcn, calibrator or None) when ``wg_target_logits`` applies, else None.  The calibrator is a WATS or one
        of the node-wise calibrators of ``scaling.py`` (TS, VS, MS, ETS), whose map is applied to the (B, C) block."""
        if not self.local_eval:
            return None
        model, wats = self.surrogate, None
        from .WATS import WATS
        from .scaling import _Scaling
        if isinstance(model, WATS) and not getattr(model, "fused_head", False):
            model, wats = model.base_model, model
        elif isinstance(model, _Scaling):
            model, wats = model._base, model
        if type(model) is not SparseCompatibleGCN:
            return None
        if model.gc1.out_features > 256 or model.gc2.out_features > 256:
            return None
        values = self._csr[2]
        if values is not None and not bool((values == 1).all()):
            return None     # a valued graph: the view path
        return model, wats

    def _view(self, toggles):
        toggles = sorted(toggles)
        return self._start.with_flips([self._t] * len(toggles), toggles)

    def _forward_probe(self, toggles):
        adj = self._view(toggles) if toggles else self._start
        return self.surrogate(self._x, adj, probe=self._probe)[[self._t]]

    def _grad(self, value, **kw):
        g = torch.autograd.grad(value, self._probe.delta, **kw)[0]
        return torch.zeros_like(self._probe.delta) if g is None else g.contiguous()

    def _select(self, toggles, grad_loss, rerank=None):
        """The partner to flip (``calib_fga.py:880-898``) from the probe's gradients."""
        indptr, indices, values = self._csr
        tog = torch.tensor(sorted(toggles), dtype=torch.int32).to(self.device) if toggles else None
        gp = gs = top2 = None
        if rerank is not None:
            top2, gp, gs = rerank
        res = flip_select(self._n, self._t, grad_loss, indptr, indices, values, tog, gp, gs, top2, topk=1,
                          return_scores=self.record_scores, workspace=self._workspace)
        self._last_scores = res[2].cpu() if self.record_scores else None
        return int(res[0][0])

    def _rerank_terms(self, output):
        """``p_max`` / ``p_smax`` and their gradients (``calib_fga.py:886-890``)."""
        probabilities = F.softmax(output, dim=1)
        top2 = torch.topk(probabilities, 2, dim=1)[0][0]
        g_pmax = self._grad(top2[0], retain_graph=True)
        g_psmax = self._grad(top2[1], retain_graph=True)
        return top2.detach().contiguous(), g_pmax, g_psmax

    def _evaluate(self, toggles):
        """The surrogate's output row ``[[t]]`` on the start adjacency with ``toggles`` flipped, without gradient."""
        with torch.no_grad():
            if self._local is None:
                return self.surrogate(self._x, self._view(toggles) if toggles else self._start)[[self._t]]
            model, wats = self._local
            w1 = model.gc1.weight
            key = (self._x.data_ptr(), self._x._version, tuple(self._x.shape), w1.data_ptr(), w1._version)
            if self._z_key != key:
                self._z, self._z_key = (self._x.to(torch.float32) @ w1.t()).contiguous(), key
            out = target_logits(self._n, self._csr[0], self._csr[1], self._z, model.gc1.bias.detach(),
                                model.gc2.weight.detach().contiguous(), model.gc2.bias.detach(), self._t,
                                [sorted(toggles)])
            if wats is not None and hasattr(wats, "row_map"):
                out = wats.row_map(out)
            elif wats is not None:
                out = F.log_softmax(out / wats.temperatures()[self._t], dim=1)
            return out

    @staticmethod
    def _toggle(toggles, j):
        """The toggle set after one more flip of partner ``j`` (a second flip of the same edge cancels the first)."""
        new = set(toggles)
        new.symmetric_difference_update({j})
        return new

    def _is_edge(self, toggles, j):
        """Whether (t, j) is an entry of the current adjacency (unit graphs: for the verbose "Added" / "Removed")."""
        indptr, indices, values = self._csr
        s, e = (int(v) for v in indptr[self._t:self._t + 2])
        present = bool((indices[s:e] == j).any())
        return present != (j in toggles)

    def _finish(self, best_toggles):
        self.best_flips = sorted(best_toggles)
        self.modified_op = self._view(self.best_flips)
        if self._dense is not None:
            adj = self._dense.clone()
            t = self._t
            for j in self.best_flips:                        # calib_fga.py:901-904
                v = -2 * adj[t][j] + 1
                adj[t][j] += v
                adj[j][t] += v
            self.__dict__["modified_adj"] = adj
        with torch.no_grad():
            final_output = self.surrogate(self._x, self.modified_op).detach()[[self._t]]
        final_label = int(final_output.argmax(dim=1).item())
        return final_label, float(F.softmax(final_output, dim=1)[0, final_label].item())

    def _record(self, j, new_output, label, confidence):
        self.flips.append(j)
        self.trace.append(dict(partner=j, logits=new_output.detach().cpu()[0], label=label, confidence=confidence,
                               scores=self._last_scores))

    # -------------------------------------------------------------------------------------------- the four methods
    def attack(self, ori_features, ori_adj, target_node, n_perturbations, strategy, *, target_label=0, res_gt=None,
               verbose=False, **kwargs):
        """``calib_fga.py:128-344``: flip the best-scoring edge while the label holds; strategies ``over``,
        ``under``, ``under_kl``, ``target``, ``max``."""
        display_strategy = strategy
        self._begin(ori_features, ori_adj, target_node)
        original_output = self._evaluate_start()
        if res_gt is None:
            raise ValueError("res_gt must be provided for Calib_FGA attacks")
        res_gt = res_gt[[target_node]].to(self.device)
        original_label = original_output.argmax(1)
        original_label_item = int(original_label.item())
        best_confidence = F.softmax(original_output, dim=1)[0, original_label_item].item()
        initial_confidence = best_confidence
        self._log_attack_header(display_strategy, target_node, n_perturbations, original_label_item, initial_confidence)
        if strategy == 'over':
            criterion = overconfidence_objective
        elif strategy == 'under':
            criterion = underconfidence_objective
        elif strategy == 'under_kl':
            strategy = "under"
            criterion = kl_divergence_with_uniform
        elif strategy == 'target':
            criterion = kl_divergence_target
        elif strategy == 'max':
            criterion = kl_divergence_target
            target_label = original_label
        else:
            raise ValueError(f"Unknown strategy: {strategy}")
        toggles, best = set(), set()
        attack_times = 0
        table_rows = [] if verbose else None
        for i in range(n_perturbations):
            output = self._forward_probe(toggles)
            current_label = output.argmax(dim=1)
            prev_confidence = F.softmax(output.detach(), dim=1)[0, current_label].item() if verbose else None
            if strategy != 'target':
                loss = criterion(output, current_label)     # 'max': TypeError, as in the reference
            else:
                loss = criterion(output, torch.tensor([target_label], device=output.device), res_gt)
            j = self._select(toggles, self._grad(loss, allow_unused=True))
            added = not self._is_edge(toggles, j) if verbose else None
            toggles = self._toggle(toggles, j)
            new_output = self._evaluate(toggles)
            new_label = new_output.argmax(dim=1)
            if new_label != original_label:
                self._record(j, new_output, int(new_label.item()), float("nan"))
                print(f"[{display_strategy.upper()}][Node {target_node}] "
                      f"Early stop at step {i + 1}: label flipped to {int(new_label.item())}")
                break
            attack_times += 1
            predicted_label = int(new_label.item())
            current_confidence = F.softmax(new_output, dim=1)[0, predicted_label].item()
            self._record(j, new_output, predicted_label, current_confidence)
            if strategy == 'over' and current_confidence >= best_confidence:
                best_confidence, best = current_confidence, set(toggles)
            elif strategy == 'under' and current_confidence <= best_confidence:
                best_confidence, best = current_confidence, set(toggles)
            elif strategy == 'target':
                if (target_label == original_label and target_label == res_gt.item()) or \
                   (target_label != original_label and target_label == res_gt.item()):
                    if current_confidence <= best_confidence:
                        best_confidence, best = current_confidence, set(toggles)
                elif current_confidence >= best_confidence:
                    best_confidence, best = current_confidence, set(toggles)
            if verbose:
                self._log_iteration(display_strategy, target_node, i + 1, n_perturbations,
                                    "Added" if added else "Removed", j, prev_confidence, current_confidence,
                                    initial_confidence, predicted_label, loss.item(), log_rows=table_rows)
        kwargs["n_perturb"].append(attack_times)
        kwargs["best_conf"].append(best_confidence)
        final_label, final_confidence = self._finish(best)
        if verbose and table_rows:
            self._print_table(table_rows, ["Step", "Action", "Pred", "Conf", "Δ step", "Δ total", "Loss"])
        self._log_attack_summary(display_strategy, target_node, attack_times, n_perturbations, original_label_item,
                                 final_label, initial_confidence, final_confidence)

    def _evaluate_start(self):
        with torch.no_grad():
            return self.surrogate(self._x, self._start).detach()[[self._t]]

    def rerank_attack(self, ori_features, ori_adj, target_node, n_perturbations, strategy, *, target_label=0,
                      res_gt=None, verbose=False, **kwargs):
        """``calib_fga.py:346-540``: ``attack`` with the label-flip rerank (``under`` only)."""
        if strategy != 'under':
            raise ValueError(f"rerank_attack only supports 'under' strategy, got '{strategy}'")
        self._greedy(ori_features, ori_adj, target_node, n_perturbations, strategy, res_gt, verbose, kwargs,
                     hybrid=False)

    def rerank_hybridloss_attack(self, ori_features, ori_adj, target_node, n_perturbations, strategy, *,
                                 target_label=0, res_gt=None, verbose=False, **kwargs):
        """``calib_fga.py:542-749``: the rerank with the hybrid loss (``under`` only)."""
        if strategy != 'under':
            raise ValueError(f"rerank_hybridloss_attack only supports 'under' strategy, got '{strategy}'")
        self._greedy(ori_features, ori_adj, target_node, n_perturbations, strategy, res_gt, verbose, kwargs,
                     hybrid=True)

    def _hybrid_step(self, toggles, original_label, hybrid):
        """One scored step of the rerank methods: (partner, loss, loss mode, output)."""
        output = self._forward_probe(toggles)
        current_label = output.argmax(dim=1)
        same = bool(current_label == original_label)
        if same or not hybrid:
            loss, mode = kl_divergence_with_uniform(output, current_label), "calib"
        else:
            loss, mode = _restore_loss(output, original_label), "restore"
        grad = self._grad(loss, retain_graph=True)
        rerank = self._rerank_terms(output) if (same or not hybrid) else None
        return self._select(toggles, grad, rerank), loss, mode, output

    def _greedy(self, ori_features, ori_adj, target_node, n_perturbations, strategy, res_gt, verbose, kwargs, hybrid):
        display_strategy = strategy
        self._begin(ori_features, ori_adj, target_node)
        original_output = self._evaluate_start()
        if res_gt is None:
            raise ValueError("res_gt must be provided for Calib_FGA attacks")
        original_label = original_output.argmax(1)
        original_label_item = int(original_label.item())
        best_confidence = F.softmax(original_output, dim=1)[0, original_label_item].item()
        initial_confidence = best_confidence
        self._log_attack_header(display_strategy, target_node, n_perturbations, original_label_item, initial_confidence)
        toggles, best = set(), set()
        attack_times = 0
        table_rows = [] if verbose else None
        for i in range(n_perturbations):
            j, loss, mode, output = self._hybrid_step(toggles, original_label, hybrid)
            prev_confidence = F.softmax(output.detach(), dim=1)[0].max().item() if verbose else None
            added = not self._is_edge(toggles, j) if verbose else None
            toggles = self._toggle(toggles, j)
            new_output = self._evaluate(toggles)
            new_label = new_output.argmax(dim=1)
            if new_label != original_label:
                self._record(j, new_output, int(new_label.item()), float("nan"))
                print(f"[{display_strategy.upper()}][Node {target_node}] "
                      f"Early stop at step {i + 1}: label flipped to {int(new_label.item())}")
                break
            predicted_label = int(new_label.item())
            current_confidence = F.softmax(new_output, dim=1)[0, predicted_label].item()
            self._record(j, new_output, predicted_label, current_confidence)
            attack_times += 1
            if current_confidence <= best_confidence:
                best_confidence, best = current_confidence, set(toggles)
            if verbose:
                action = "Added" if added else "Removed"
                if hybrid:
                    action = f"{action} [{mode}]"
                self._log_iteration(display_strategy, target_node, i + 1, n_perturbations, action, j, prev_confidence,
                                    current_confidence, initial_confidence, predicted_label, loss.item(),
                                    log_rows=table_rows)
        kwargs["n_perturb"].append(attack_times)
        kwargs["best_conf"].append(best_confidence)
        final_label, final_confidence = self._finish(best)
        if verbose and table_rows:
            self._print_table(table_rows, ["Step", "Action", "Pred", "Conf", "Δ step", "Δ total", "Loss"])
        self._log_attack_summary(display_strategy, target_node, attack_times, n_perturbations, original_label_item,
                                 final_label, initial_confidence, final_confidence)

    def flip_beam_hybridloss_attack(self, ori_features, ori_adj, target_node, n_perturbations, strategy, *,
                                    target_label=0, res_gt=None, verbose=False, **kwargs):
        """``calib_fga.py:751-969``: the beam search with the hybrid loss and the rerank (``under`` only).  Each
        iteration pops up to ``beam_width`` members and each yields one child, so the beam holds one member."""
        if strategy != 'under':
            raise ValueError(f"flip_beam_hybridloss_attack only supports 'under' strategy, got '{strategy}'")
        display_strategy = strategy
        self._begin(ori_features, ori_adj, target_node)
        original_output = self._evaluate_start()
        if res_gt is None:
            raise ValueError("res_gt must be provided for Calib_FGA attacks")
        original_label = original_output.argmax(1)
        original_label_item = int(original_label.item())
        beam_width = kwargs.get('beam_width', 3)
        initial_confidence = F.softmax(original_output, dim=1)[0, original_label_item].item()
        self._log_attack_header(display_strategy, target_node, n_perturbations, original_label_item, initial_confidence)
        seq = 0                                        # orders equal (confidence, count) pairs: the reference's queue
        beam = [(initial_confidence, 0, seq, frozenset())]          # would compare tensors there and raise
        best, best_confidence, attack_times = frozenset(), initial_confidence, 0
        table_data = []
        start_time = time.time()
        for iteration in range(n_perturbations):
            next_beam = []
            for _ in range(beam_width):
                if not beam:
                    break
                _, count, _, toggles = heapq.heappop(beam)
                if count >= n_perturbations:
                    continue
                j, _, _, _ = self._hybrid_step(set(toggles), original_label, hybrid=True)
                child = frozenset(self._toggle(toggles, j))
                new_output = self._evaluate(child)
                new_label = new_output.argmax(dim=1)
                new_confidence = F.softmax(new_output, dim=1)[0, new_label].item()
                self._record(j, new_output, int(new_label.item()), new_confidence)
                seq += 1
                heapq.heappush(next_beam, (new_confidence, count + 1, seq, child))
                if new_label == original_label and new_confidence < best_confidence:
                    best_confidence, best, attack_times = new_confidence, child, count + 1
            beam = next_beam
            table_data.append([iteration + 1, f"{initial_confidence:.4f}", f"{best_confidence:.4f}", attack_times])
        elapsed_time = time.time() - start_time
        if verbose:
            self._print_table(table_data, ["Iteration", "Initial Confidence", "Best Confidence", "Perturbations"])
            print(f"Attack completed in {elapsed_time:.4f} seconds")
        kwargs["n_perturb"].append(attack_times)
        kwargs["best_conf"].append(best_confidence)
        if "runtime" in kwargs:
            kwargs["runtime"].append(elapsed_time)
        final_label, final_confidence = self._finish(best)
        if final_label != original_label_item:
            raise ValueError("Final label does not match original label!")
        self._log_attack_summary(display_strategy, target_node, attack_times, n_perturbations, original_label_item,
                                 final_label, initial_confidence, final_confidence)

    # -------------------------------------------------------------------------------------------- many targets
    def attack_many(self, ori_features, ori_adj, targets, n_perturbations, strategy, *,
                    method="flip_beam_hybridloss_attack", res_gt=None, target_label=0, beam_width=3, verbose=False,
                    **kwargs):
        """One of the four methods for several targets of one graph, every target starting from ``ori_adj`` (the
        reference's per-node loop, ``exp/ablation/ugca_full_multi_dataset.py:372-411``).  The targets run in lock step,
        each its own copy of the single-target state machine; a step is one ``wg_trial_logits`` launch for the
        children, autograd on the ``(B, C)`` block of logits and one ``wg_fga_scores`` call: no whole-graph pass.
        Returns one dict per target, in target order: ``target``, ``flips``, ``best_flips``, ``n_perturb``,
        ``best_conf``, ``original_label``, ``final_label``, ``final_confidence``, ``trace`` and ``modified_op`` (made
        when first read by key or ``get``; iterating the dict shows it only after that).  Where ``wg_target_logits``
        does not apply (``_local_model``) the single-target method is called per target and the same dicts are
        returned."""
        if method not in METHODS:
            raise ValueError(f"Unknown method: {method}")
        if method != "attack" and strategy != 'under':
            raise ValueError(f"{method} only supports 'under' strategy, got '{strategy}'")
        if method == "attack" and strategy not in ('over', 'under', 'under_kl', 'target', 'max'):
            raise ValueError(f"Unknown strategy: {strategy}")
        if res_gt is None:
            raise ValueError("res_gt must be provided for Calib_FGA attacks")
        targets = [int(t) for t in targets]
        if not targets:
            return []
        start_time = time.time()
        self._begin(ori_features, ori_adj, targets[0])
        for t in targets:
            if not 0 <= t < self._n:
                raise ValueError(f"target {t} outside [0, {self._n})")
        if self._local is None or (method == "attack" and strategy == 'max'):
            results = self._many_by_loop(ori_features, ori_adj, targets, n_perturbations, strategy, method, res_gt,
                                         target_label, beam_width, verbose)
        else:
            results = self._many_local(targets, int(n_perturbations), strategy, method, res_gt, target_label,
                                       int(beam_width))
        elapsed = time.time() - start_time
        for r in results:
            kwargs.get("n_perturb", []).append(r["n_perturb"])
            kwargs.get("best_conf", []).append(r["best_conf"])
            if method == "flip_beam_hybridloss_attack":
                kwargs.get("runtime", []).append(elapsed / len(results))
            if verbose:
                self._log_attack_summary(strategy, r["target"], r["n_perturb"], n_perturbations, r["original_label"],
                                         r["final_label"], r["original_confidence"], r["final_confidence"])
        if method == "flip_beam_hybridloss_attack":
            for r in results:
                if r["final_label"] != r["original_label"]:
                    raise ValueError("Final label does not match original label!")
        return results

    def _many_by_loop(self, ori_features, ori_adj, targets, n_perturbations, strategy, method, res_gt, target_label,
                      beam_width, verbose):
        """The single-target method per target (any surrogate, valued graphs, ``local_eval=False``)."""
        import contextlib
        import io
        results = []
        for t in targets:
            kw = dict(n_perturb=[], best_conf=[])
            if method == "flip_beam_hybridloss_attack":
                kw["beam_width"] = beam_width
            with contextlib.nullcontext() if verbose else contextlib.redirect_stdout(io.StringIO()):
                try:
                    getattr(self, method)(ori_features, ori_adj, t, n_perturbations, strategy,
                                          target_label=target_label, res_gt=res_gt, verbose=verbose, **kw)
                except ValueError as e:                # raised by attack_many after every target has run
                    if "Final label" not in str(e):
                        raise
                with torch.no_grad():
                    first = self._evaluate_start()
                    last = self.surrogate(self._x, self._view(self.best_flips))[[t]]
            label0, label1 = int(first.argmax(dim=1)), int(last.argmax(dim=1))
            results.append(_ManyResult(
                self._start, target=t, flips=list(self.flips), best_flips=list(self.best_flips),
                n_perturb=kw["n_perturb"][0], best_conf=kw["best_conf"][0], original_label=label0,
                original_confidence=float(F.softmax(first, dim=1)[0, label0]), final_label=label1,
                final_confidence=float(F.softmax(last, dim=1)[0, label1]),
                trace=[{k: s[k] for k in ("partner", "logits", "label", "confidence")} for s in self.trace]))
        return results

    def _many_local(self, targets, budget, strategy, method, res_gt, target_label, beam_width):
        model, wats = self._local
        device, n = self.device, self._n
        indptr, indices, _ = self._csr
        w1 = model.gc1.weight
        key = (self._x.data_ptr(), self._x._version, tuple(self._x.shape), w1.data_ptr(), w1._version)
        with torch.no_grad():
            if self._z_key != key:
                self._z, self._z_key = (self._x.to(torch.float32) @ w1.t()).contiguous(), key
            z = self._z
            b1, W2, b2 = model.gc1.bias.detach(), model.gc2.weight.detach().contiguous(), model.gc2.bias.detach()
            h = F.relu(self._start @ z + b1).contiguous()           # the base graph's hidden rows, once per call
            node = torch.tensor(targets, dtype=torch.int64, device=device)
            temps = None
            if wats is not None and not hasattr(wats, "row_map"):
                temps = wats.temperatures()
            start_out = self.surrogate(self._x, self._start).detach()[node]
        row_len = (indptr[node + 1] - indptr[node]).cpu().tolist()
        gt = res_gt.to(device)[node]

        def head_of(rows):
            """the calibrator's row map of a (len(rows), C) block of base logits; rows: positions in `targets`"""
            if wats is None:
                return lambda raw: raw
            if temps is None:
                return wats.row_map
            tr = temps[node[rows]].unsqueeze(1)
            return lambda raw: F.log_softmax(raw / tr, dim=1)

        def evaluate(rows, sets):
            """one launch: (raw logits on the device, head outputs, labels and confidences on the host)"""
            with torch.no_grad():
                raw = trial_logits(n, indptr, indices, z, b1, W2, b2, [(targets[r], sorted(S), None)
                                                                      for r, S in zip(rows, sets)])
                out = head_of(rows)(raw)
                host, labels, confs = _RandomAttack._read(out)
            return raw, host, labels, confs

        def scored_step(rows, sets, raws, kinds, labels, rerank):
            """the partner every member flips next (one wg_fga_scores call)"""
            g, top2 = _row_gradients(raws, head_of(rows), kinds, labels, rerank,
                                     gt[rows] if "target" in kinds else None)
            tg, tog_ptr, tog_ids = _pack_toggles(n, [targets[r] for r in rows], [sorted(S) for S in sets], device)
            rr = torch.tensor([int(v) for v in rerank], dtype=torch.int32).to(device) if top2 is not None else None
            cap = sum(row_len[r] + len(S) for r, S in zip(rows, sets))
            best_ids, _ = fga_scores(n, indptr, indices, z, h, b1, W2, tg, (tog_ptr, tog_ids), g, rr, top2, topk=1,
                                     local_cap=cap)
            return best_ids[:, 0].cpu().tolist()

        B = len(targets)
        label0 = start_out.argmax(dim=1).cpu().tolist()
        conf0 = F.softmax(start_out, dim=1).gather(1, start_out.argmax(dim=1, keepdim=True))[:, 0].cpu().tolist()
        flips, trace = [[] for _ in targets], [[] for _ in targets]
        best, best_conf, used = [frozenset()] * B, list(conf0), [0] * B
        every = list(range(B))
        raw0 = evaluate(every, [()] * B)[0] if budget > 0 else None

        def record(r, j, host_row, label, conf):
            flips[r].append(j)
            trace[r].append(dict(partner=j, logits=host_row.clone(), label=label, confidence=conf))

        if method == "flip_beam_hybridloss_attack":
            seq = [0] * B
            beams = [[(conf0[r], 0, 0, frozenset(), raw0[r])] for r in every] if budget > 0 else [[] for _ in every]
            for _ in range(budget):
                nexts = [[] for _ in every]
                for _ in range(beam_width):
                    rows, members = [], []
                    for r in every:
                        if not beams[r]:
                            continue
                        m = heapq.heappop(beams[r])
                        if m[1] >= budget:
                            continue
                        rows.append(r)
                        members.append(m)
                    if not rows:
                        break
                    raws = torch.stack([m[4] for m in members])
                    cur = head_of(rows)(raws).argmax(dim=1)
                    same = (cur.cpu() == torch.tensor([label0[r] for r in rows])).tolist()
                    kinds = ["kl" if s else "restore" for s in same]
                    labels = torch.where(torch.tensor(same, device=device), cur,
                                         torch.tensor([label0[r] for r in rows], device=device))
                    js = scored_step(rows, [m[3] for m in members], raws, kinds, labels, same)
                    children = [frozenset(self._toggle(m[3], j)) for m, j in zip(members, js)]
                    raw, host, labs, confs = evaluate(rows, children)
                    for i, r in enumerate(rows):
                        record(r, js[i], host[i], labs[i], confs[i])
                        seq[r] += 1
                        count = members[i][1] + 1
                        heapq.heappush(nexts[r], (confs[i], count, seq[r], children[i], raw[i]))
                        if labs[i] == label0[r] and confs[i] < best_conf[r]:
                            best_conf[r], best[r], used[r] = confs[i], children[i], count
                beams = nexts
        else:
            active = list(every) if budget > 0 else []
            sets = {r: frozenset() for r in active}
            raws = {r: raw0[r] for r in active}
            hybrid = method == "rerank_hybridloss_attack"
            for _ in range(budget):
                if not active:
                    break
                rows = active
                block = torch.stack([raws[r] for r in rows])
                cur = head_of(rows)(block).argmax(dim=1)
                if method == "attack":
                    kind = {"over": "over", "under": "under", "under_kl": "kl", "target": "target"}[strategy]
                    kinds, rerank = [kind] * len(rows), [False] * len(rows)
                    labels = torch.full_like(cur, int(target_label)) if kind == "target" else cur
                else:
                    same = (cur.cpu() == torch.tensor([label0[r] for r in rows])).tolist()
                    calib = [s or not hybrid for s in same]
                    kinds, rerank = ["kl" if c else "restore" for c in calib], calib
                    labels = torch.where(torch.tensor(calib, device=device), cur,
                                         torch.tensor([label0[r] for r in rows], device=device))
                js = scored_step(rows, [sets[r] for r in rows], block, kinds, labels, rerank)
                children = [frozenset(self._toggle(sets[r], j)) for r, j in zip(rows, js)]
                raw, host, labs, confs = evaluate(rows, children)
                still = []
                for i, r in enumerate(rows):
                    if labs[i] != label0[r]:                     # the label moved: this target stops here
                        record(r, js[i], host[i], labs[i], float("nan"))
                        continue
                    record(r, js[i], host[i], labs[i], confs[i])
                    used[r] += 1
                    sets[r], raws[r] = children[i], raw[i]
                    still.append(r)
                    if method != "attack" or strategy in ('under', 'under_kl'):
                        better = confs[i] <= best_conf[r]
                    elif strategy == 'over':
                        better = confs[i] >= best_conf[r]
                    else:
                        tl, g_t = int(target_label), int(gt[r])
                        under = (tl == label0[r] and tl == g_t) or (tl != label0[r] and tl == g_t)
                        better = confs[i] <= best_conf[r] if under else confs[i] >= best_conf[r]
                    if better:
                        best_conf[r], best[r] = confs[i], children[i]
                active = still
        _, _, final_labels, final_confs = evaluate(every, best)
        return [_ManyResult(self._start, target=targets[r], flips=flips[r], best_flips=sorted(best[r]),
                            n_perturb=used[r], best_conf=best_conf[r], original_label=label0[r],
                            original_confidence=conf0[r], final_label=final_labels[r],
                            final_confidence=final_confs[r], trace=trace[r]) for r in every]


# ------------------------------------------------------------------------------------------------ integrated gradients
def iga_max_topk() -> int:
    return int(_lib.load().wg_iga_max_topk())


def iga_path_logits(n: int, indptr: torch.Tensor, indices: torch.Tensor, z: torch.Tensor, h: torch.Tensor,
                    zsum: torch.Tensor, hsum: torch.Tensor, b1: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor,
                    targets: torch.Tensor, steps: int):
    """``wg_iga_path_logits``: ``(logits (B, P, C) float32, state (B, P, 2 Hd + 2) float64)`` of the
    ``P = 2 (steps + 1)`` path points of each target's row (``calib_iga.py:185-211``).  ``targets``: int32 device."""
    device = require_gpu(z.device if z.is_cuda else None)
    B, Hd, C, P = int(targets.numel()), int(z.shape[1]), int(W2.shape[0]), 2 * (int(steps) + 1)
    if z.shape[0] != n or h.shape != z.shape or zsum.numel() != Hd or hsum.numel() != Hd or W2.shape[1] != Hd \
            or b1.numel() != Hd or b2.numel() != C:
        raise ValueError("iga_path_logits: z, h (n, Hd), zsum, hsum, b1 [Hd], W2 (C, Hd), b2 [C] expected")
    logits = torch.empty((B, P, C), dtype=torch.float32, device=device)
    state = torch.empty((B, P, 2 * Hd + 2), dtype=torch.float64, device=device)
    nnz = int(indices.numel())
    with torch.cuda.device(device):
        check(_lib.load().wg_iga_path_logits(n, nnz, ptr(indptr), ptr(indices) if nnz else None, Hd, ptr(z), ptr(h),
                                             ptr(zsum), ptr(hsum), ptr(b1), ptr(W2), ptr(b2), C, B, ptr(targets),
                                             int(steps), ptr(logits), ptr(state), stream_handle(device)),
              "iga_path_logits")
    return logits, state


def iga_scores_workspace(B: int, Hd: int, device) -> torch.Tensor:
    nbytes = ctypes.c_int64(0)
    check(_lib.load().wg_iga_scores_workspace(B, Hd, ctypes.byref(nbytes)), "iga_scores_workspace")
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)


def iga_scores(n: int, indptr: torch.Tensor, indices: torch.Tensor, z: torch.Tensor, h: torch.Tensor, b1: torch.Tensor,
               W2: torch.Tensor, targets: torch.Tensor, steps: int, g_logits: torch.Tensor, state: torch.Tensor,
               topk: int = 10, n_workgroups: int = 0, return_scores: bool = False, return_coeffs: bool = False,
               workspace: torch.Tensor | None = None):
    """``wg_iga_scores``: ``(best_ids int32 (B, topk), best_scores float32 (B, topk))`` and, on request, the score
    matrix ``(B, n)`` and the coefficients ``(B, 2, 2 Hd + 1)`` float64 (``calib_iga.py:217-233`` for every target in
    one pass over ``z`` and ``h``)."""
    device = require_gpu(z.device if z.is_cuda else None)
    B, Hd, C = int(targets.numel()), int(z.shape[1]), int(W2.shape[0])
    P = 2 * (int(steps) + 1)
    if tuple(g_logits.shape) != (B, P, C) or tuple(state.shape) != (B, P, 2 * Hd + 2) or h.shape != z.shape:
        raise ValueError("iga_scores: g_logits (B, P, C) and state (B, P, 2 Hd + 2) of the same targets expected")
    best_ids = torch.empty((B, topk), dtype=torch.int32, device=device)
    best_scores = torch.empty((B, topk), dtype=torch.float32, device=device)
    scores = torch.empty((B, n), dtype=torch.float32, device=device) if return_scores else None
    coeffs = torch.empty((B, 2, 2 * Hd + 1), dtype=torch.float64, device=device) if return_coeffs else None
    if workspace is None:
        workspace = iga_scores_workspace(B, Hd, device)
    nnz = int(indices.numel())
    with torch.cuda.device(device):
        check(_lib.load().wg_iga_scores(n, nnz, ptr(indptr), ptr(indices) if nnz else None, Hd, ptr(z), ptr(h), ptr(b1),
                                        ptr(W2), C, B, ptr(targets), int(steps), ptr(g_logits), ptr(state), topk,
                                        n_workgroups, ptr(workspace), ptr(coeffs), ptr(scores), ptr(best_ids),
                                        ptr(best_scores), stream_handle(device)), "iga_scores")
    out = (best_ids, best_scores)
    if return_scores:
        out += (scores,)
    if return_coeffs:
        out += (coeffs,)
    return out


def _criterion_rows(out, labels, strategy):
    """``overconfidence_objective`` / ``underconfidence_objective`` applied to each row on its own (a batch of one:
    the mean of one value, ``calib_iga.py:211-215``), summed over the rows.  Written as a sum so that a row's gradient
    does not depend on how many rows share the call."""
    probs, own = _target_probs(out, labels)
    if strategy == 'over':
        return -(1 - own).sum()
    keep = torch.ones_like(probs)
    keep[torch.arange(len(labels)), labels] = 0
    others, _ = torch.max(probs * keep, dim=1)
    return -(own - others).sum()


class Calib_IGA(torch.nn.Module):
    """``Calib_IGA`` of the reference (``calib_attack/calib_iga.py``) on the sparse path (DESIGN.md 4.3
    "Integrated-gradient scores"): the same constructor, ``attack`` and ``calc_calibration_importance_edge``.

    The reference's ``(N - 1) (steps + 1)`` dense forward / backward passes per target are, on the two-layer base
    model, a closed form: ``wg_iga_path_logits`` evaluates the path points of row ``t``, the head and the criterion
    run in torch autograd on those ``(P, C)`` logits, ``wg_iga_scores`` turns their gradient into the ``n`` scores and
    the best partners, and one ``wg_target_logits`` call evaluates the prefixes of that ranking.

    Surrogates: a bare ``SparseCompatibleGCN``, or a ``WATS`` over one without the fused head, on a unit graph.
    Kept from the reference: the scores are computed once; the flips are cumulative and symmetric; the loop stops at
    the first label change; ``>=`` for ``over`` and ``<=`` for ``under``.  Not kept: the stray ``print(i)``;
    ``check_adj``'s dense test; a ranking that reaches ``t`` itself (its ``-10``) ends the loop there instead of
    flipping the self entry.  Results as ``Calib_FGA`` names them: ``flips``, ``best_flips``, ``modified_op``,
    ``modified_adj`` (dense input only), ``trace``."""

    def __init__(self, model, nnodes=None, device=None):
        super().__init__()
        self.surrogate = model
        self.nnodes = nnodes
        self.attack_structure, self.attack_features = True, False
        self.device = require_gpu(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.modified_op = None
        self.target_node = None
        self.flips, self.best_flips, self.trace = [], [], []
        self._z_key = self._cache = None

    def __getattr__(self, name):
        if name == "modified_adj":
            raise AttributeError("modified_adj is a dense (N, N) tensor and exists only when ori_adj was dense; "
                                 "read modified_op (.materialize() gives an operator, .to_graph() a CSR)")
        return super().__getattr__(name)

    # -------------------------------------------------------------------------------------------- the graph's cache
    def _model(self, values):
        why = ("Calib_IGA on the sparse path needs {}: a path point has a dense row t, which no sparse operator holds, "
               "so the scores come from the closed form of the two-layer base model on a unit graph")
        model, wats = self.surrogate, None
        from .WATS import WATS
        if isinstance(model, WATS):
            if getattr(model, "fused_head", False):
                raise NotImplementedError(why.format("a WATS surrogate without the fused head"))
            model, wats = model.base_model, model
        if type(model) is not SparseCompatibleGCN:
            raise NotImplementedError(why.format("a SparseCompatibleGCN surrogate, bare or under WATS (a calibrator "
                                                 f"whose head reads neighbours, here {type(model).__name__}, is not "
                                                 "covered)"))
        if model.gc1.out_features > 256 or model.gc2.out_features > 256:
            raise NotImplementedError(why.format("Hd and C of at most 256"))
        if values is not None and not bool((values == 1).all()):
            raise NotImplementedError(why.format("an unweighted graph (this one has values other than 1)"))
        return model, wats

    def _begin(self, features, adj):
        self._dense = None
        if torch.is_tensor(adj):
            self._dense = adj.detach()
            start = self.surrogate_operator(self._dense)
        elif isinstance(adj, RowNormalizedAdjacency):
            start = adj
        else:
            raise TypeError("ori_adj must be a dense tensor, a RowNormalizedAdjacency or a FlippedAdjacency")
        self._start = start
        self._n = int(start.n)
        csr = start.csr() if isinstance(start, FlippedAdjacency) else (start.indptr, start.indices, start.values)
        model, wats = self._model(csr[2])
        self._csr = csr
        self.surrogate.eval()
        x = features.detach().to(start.device)
        w1 = model.gc1.weight
        key = (x.data_ptr(), x._version, tuple(x.shape), w1.data_ptr(), w1._version, model.gc1.bias._version,
               id(start) if self._dense is None else (self._dense.data_ptr(), self._dense._version))
        if self._z_key != key:
            with torch.no_grad():
                x32 = x.to(torch.float32)
                z = (x32 @ w1.t()).contiguous()
                h = F.relu(model.gc1(start @ x32)).contiguous()       # the surrogate's own first layer (model.py:47-48)
                self._cache = (z, h, z.double().sum(0), h.double().sum(0))
            self._z_key = key
        self._x = x
        return model, wats

    def surrogate_operator(self, dense):
        return RowNormalizedAdjacency.from_dense(dense.to(self.device))

    # -------------------------------------------------------------------------------------------- the scores
    def _score(self, model, wats, targets, strategy, steps, topk, return_scores=False):
        """(best_ids (B, topk), best_scores, scores or None) for the targets (a list of ints)"""
        if strategy not in ('over', 'under'):
            raise ValueError("strategy must be 'over' or 'under'")
        for t in targets:
            if not 0 <= int(t) < self._n:
                raise ValueError(f"target {t} outside [0, {self._n})")
        if not 1 <= topk <= iga_max_topk():
            raise ValueError(f"n_perturbations = {topk} outside [1, {iga_max_topk()}] (wg_iga_max_topk)")
        z, h, zsum, hsum = self._cache
        indptr, indices, _ = self._csr
        tg = torch.tensor([int(t) for t in targets], dtype=torch.int32).to(self.device)
        b1, W2, b2 = model.gc1.bias.detach(), model.gc2.weight.detach().contiguous(), model.gc2.bias.detach()
        logits, state = iga_path_logits(self._n, indptr, indices, z, h, zsum, hsum, b1, W2, b2, tg, steps)
        B, P, C = logits.shape
        leaf = logits.requires_grad_(True)
        out = leaf
        if wats is not None:
            with torch.no_grad():
                temps = wats.temperatures()[tg.long()]
            out = F.log_softmax(leaf / temps.view(B, 1, 1), dim=2)
        out = out.reshape(B * P, C)
        loss = _criterion_rows(out, out.argmax(dim=1), strategy)     # each path point's own label (calib_iga.py:212)
        g = torch.autograd.grad(loss, leaf)[0].contiguous()
        res = iga_scores(self._n, indptr, indices, z, h, b1, W2, tg, steps, g, state, topk=topk,
                         return_scores=return_scores)
        return res if return_scores else res + (None,)

    def calc_calibration_importance_edge(self, features, adj, target_node, strategy, steps=10, verbose=False):
        """``calib_iga.py:152-235``: the importance of every partner of ``target_node``, a numpy vector ``[n]``."""
        model, wats = self._begin(features, adj)
        _, _, scores = self._score(model, wats, [target_node], strategy, steps, 1, return_scores=True)
        return scores[0].cpu().numpy().astype("float64")

    # -------------------------------------------------------------------------------------------- the attack
    def attack(self, ori_features, ori_adj, target_node, n_perturbations, strategy, res_gt=None, steps=10,
               verbose=False, **kwargs):
        """``calib_iga.py:38-150``."""
        if res_gt is None:
            raise ValueError("res_gt must be provided for calibration attacks")
        if strategy not in ['over', 'under']:
            raise ValueError("strategy must be 'over' or 'under'")
        self.__dict__.pop("modified_adj", None)
        r = self.attack_many(ori_features, ori_adj, [target_node], n_perturbations, strategy, res_gt, steps=steps,
                             verbose=verbose)[0]
        self.target_node = target_node
        self.flips, self.best_flips, self.trace = r["flips"], r["best_flips"], r["trace"]
        self.modified_op = r["modified_op"]
        if "modified_adj" in r:
            self.__dict__["modified_adj"] = r["modified_adj"]
        kwargs.get("n_perturb", []).append(r["n_perturb"])
        kwargs.get("best_conf", []).append(r["best_conf"])

    def attack_many(self, features, adj, targets, n_perturbations, strategy, res_gt, steps=10, verbose=False):
        """``attack`` for several targets of one graph: all of them are scored by one ``wg_iga_scores`` launch.  Returns
        one dict per target: ``flips``, ``best_flips``, ``n_perturb``, ``best_conf``, ``trace``, ``modified_op``,
        ``original_label``, ``original_conf`` (and ``modified_adj`` for a dense ``adj``)."""
        if res_gt is None:
            raise ValueError("res_gt must be provided for calibration attacks")
        if strategy not in ['over', 'under']:
            raise ValueError("strategy must be 'over' or 'under'")
        targets = [int(t) for t in targets]
        model, wats = self._begin(features, adj)
        results = []
        if n_perturbations < 1:
            ids = [[] for _ in targets]
        else:
            ids = self._score(model, wats, targets, strategy, steps, int(n_perturbations))[0].cpu().tolist()
        z = self._cache[0]
        indptr, indices, _ = self._csr
        temps = None
        if wats is not None:
            with torch.no_grad():
                temps = wats.temperatures()
        for t, ranking in zip(targets, ids):
            order = []
            for j in ranking:                      # the ranking ends at a missing slot or at t itself (its -10)
                if j < 0 or j == t:
                    break
                order.append(int(j))
            with torch.no_grad():                  # one launch: the start graph, then every prefix of the ranking
                out = target_logits(self._n, indptr, indices, z, model.gc1.bias.detach(),
                                    model.gc2.weight.detach().contiguous(), model.gc2.bias.detach(), t,
                                    [sorted(order[:k]) for k in range(len(order) + 1)])
                if temps is not None:
                    out = F.log_softmax(out / temps[t], dim=1)
                labels = out.argmax(dim=1).cpu().tolist()
                probs = F.softmax(out, dim=1).cpu()
            original_label = labels[0]
            best_confidence = original_confidence = probs[0, original_label].item()
            if verbose:
                print(f"[{strategy.upper()}][Node {t}] Starting calibration attack")
                print(f"Original label: {original_label}, confidence: {original_confidence:.4f}")
            attack_times, best, flips, trace = 0, [], [], []
            for k, j in enumerate(order, start=1):
                new_label = labels[k]
                new_confidence = probs[k, new_label].item()
                flips.append(j)
                trace.append(dict(partner=j, logits=out[k].cpu(), label=new_label, confidence=new_confidence))
                if new_label != original_label:
                    if verbose:
                        print(f"[{strategy.upper()}][Node {t}] Early stop at step {k}: label flipped")
                    break
                attack_times += 1
                if strategy == 'over' and new_confidence >= best_confidence:
                    best_confidence, best = new_confidence, sorted(order[:k])
                elif strategy == 'under' and new_confidence <= best_confidence:
                    best_confidence, best = new_confidence, sorted(order[:k])
                if verbose:
                    print(f"[{strategy.upper()}][Node {t}][Step {k}] flipped edge to node {j}")
                    print(f"Confidence: {original_confidence:.4f} -> {new_confidence:.4f} "
                          f"(Δ {new_confidence - original_confidence:+.4f})")
            r = dict(target=t, flips=flips, best_flips=best, n_perturb=attack_times, best_conf=best_confidence,
                     trace=trace, modified_op=self._start.with_flips([t] * len(best), best),
                     original_label=original_label, original_conf=original_confidence)
            if self._dense is not None:
                dense = self._dense.clone()
                for j in best:                                       # calib_iga.py:103-109
                    v = 1 - dense[t, j]
                    dense[t, j] = v
                    dense[j, t] = v
                r["modified_adj"] = dense
            if verbose:
                print(f"[{strategy.upper()}][Node {t}] Attack completed")
                print(f"Perturbations used: {attack_times}/{n_perturbations}")
            results.append(r)
        return results


# ------------------------------------------------------------------------------------------------ the random attacks
def trial_logits(n: int, indptr: torch.Tensor, indices: torch.Tensor, z: torch.Tensor, b1: torch.Tensor,
                 W2: torch.Tensor, b2: torch.Tensor, trials, W1: torch.Tensor | None = None) -> torch.Tensor:
    """``wg_trial_logits``: the ``(B, C)`` logits of B trials of the random attacks in one launch.  ``trials`` is a
    list of ``(t, partners, {feature: delta})`` (partners ascending and distinct, ``t`` itself allowed: its self loop;
    the dict may be empty or None), or prebuilt int32 / float32 device arrays that the caller checked:
    ``(trial_t, cand_ptr, cand_ids)`` or ``(trial_t, cand_ptr, cand_ids, feat_ptr, feat_ids, feat_delta)``.
    ``z = x @ W1.T``; ``W1 (Hd, nfeat)`` is read only with feature deltas."""
    device = require_gpu(z.device if z.is_cuda else None)
    Hd, C = int(z.shape[1]), int(W2.shape[0])
    if z.shape[0] != n or W2.shape[1] != Hd or b1.numel() != Hd or b2.numel() != C:
        raise ValueError("trial_logits: z (n, Hd), b1 [Hd], W2 (C, Hd), b2 [C] expected")
    feat_ptr = feat_ids = feat_delta = None
    if isinstance(trials, tuple):
        trial_t, cand_ptr, cand_ids = trials[:3]
        if len(trials) == 6:
            feat_ptr, feat_ids, feat_delta = trials[3:]
    else:
        nfeat = None if W1 is None else int(W1.shape[1])
        ts, ptrs, ids, fptrs, fids, fdel = [], [0], [], [0], [], []
        for t, S, feats in trials:
            t, S = int(t), [int(j) for j in S]
            if not 0 <= t < n:
                raise ValueError(f"a trial's target {t} is outside [0, {n})")
            if any(b <= a for a, b in zip(S, S[1:])) or any(not 0 <= j < n for j in S):
                raise ValueError("a trial's partners must be ascending, distinct and inside [0, n)")
            ts.append(t)
            ids += S
            ptrs.append(len(ids))
            for f in sorted(feats or ()):
                if nfeat is None or not 0 <= int(f) < nfeat:
                    raise ValueError("a trial's features need W1 (Hd, nfeat) and ids inside [0, nfeat)")
                fids.append(int(f))
                fdel.append(float(feats[f]))
            fptrs.append(len(fids))
        packed = dict(t=torch.tensor(ts, dtype=torch.int32), ptr=torch.tensor(ptrs, dtype=torch.int32),
                      ids=torch.tensor(ids, dtype=torch.int32))
        if fids:
            packed.update(fptr=torch.tensor(fptrs, dtype=torch.int32), fids=torch.tensor(fids, dtype=torch.int32),
                          fdel=torch.tensor(fdel, dtype=torch.float32))
        from .flips import _upload
        d = _upload(device, packed)                              # one copy
        trial_t, cand_ptr, cand_ids = d["t"], d["ptr"], d["ids"]
        if fids:
            feat_ptr, feat_ids, feat_delta = d["fptr"], d["fids"], d["fdel"]
    B = int(trial_t.numel())
    if int(cand_ptr.numel()) != B + 1 or (feat_ptr is not None and int(feat_ptr.numel()) != B + 1):
        raise ValueError("trial_logits: cand_ptr / feat_ptr need B + 1 entries")
    nfeat = 0
    if feat_ptr is not None:
        if W1 is None or W1.dim() != 2 or W1.shape[0] != Hd:
            raise ValueError("trial_logits: feature deltas need W1 (Hd, nfeat)")
        W1 = W1.detach().to(device, torch.float32).contiguous()
        nfeat = int(W1.shape[1])
    out = torch.empty((B, C), dtype=torch.float32, device=device)
    nnz = int(indices.numel())
    opt = lambda v: ptr(v) if v is not None and v.numel() else None
    with torch.cuda.device(device):
        check(_lib.load().wg_trial_logits(n, nnz, ptr(indptr), opt(indices), Hd, ptr(z), ptr(b1), ptr(W2), ptr(b2), C,
                                          B, ptr(trial_t), ptr(cand_ptr), opt(cand_ids), nfeat,
                                          ptr(W1) if feat_ptr is not None else None,
                                          ptr(feat_ptr) if feat_ptr is not None else None, opt(feat_ids),
                                          opt(feat_delta), ptr(out), stream_handle(device)), "trial_logits")
    return out


def _nth_absent(occupied, idx):
    """The ``idx``-th id (from 0) that is not in the ascending list ``occupied``."""
    j = idx
    for e in occupied:
        if e <= j:
            j += 1
        else:
            break
    return j


class _Target:
    """One target's state: the accepted toggles and feature row, its random stream and what it has recorded."""

    def __init__(self, t, rng, base_row, x_row):
        self.t, self.rng = t, rng
        self.base_row = base_row                   # row t of the start CSR: ascending host ints
        self.toggles = set()                       # partners whose entry differs from the start adjacency
        self.x0 = x_row                            # host float32 copies of row t of the features
        self.x = x_row.copy()
        self.changed = {}                          # feature -> current - original, where it is not 0
        self.flips, self.feature_flips, self.trace = [], {}, []
        self.attack_times = 0
        self.label = self.best_conf = self.conf0 = None

    def present(self):
        return sorted(set(self.base_row).symmetric_difference(self.toggles))


class _RandomAttack(torch.nn.Module):
    """What ``Calib_Random`` and ``Calib_RND`` share (their loops are the same draws in the same order: ``randint(0,
    k - 1)`` and ``choice`` of a k-list both take one ``_randbelow(k)``)."""

    _default_strategy = "under"
    _name = "CALIB_RANDOM"

    def __init__(self, model, attack_structure=True, attack_features=False, device=None, *, local_eval: bool = True):
        super().__init__()
        assert attack_features or attack_structure, 'attack_features or attack_structure cannot be both False'
        self.surrogate = model
        self.attack_structure, self.attack_features = bool(attack_structure), bool(attack_features)
        self.device = require_gpu(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.local_eval = bool(local_eval)
        self.modified_features = None
        self.modified_op = None
        self.target_node = None
        self.flips, self.best_flips, self.feature_flips, self.trace = [], [], {}, []
        self._z_key = self._z = None

    def __getattr__(self, name):
        if name == "modified_adj":
            raise AttributeError("modified_adj exists only when ori_adj was dense (Calib_RND: or scipy); read "
                                 "modified_op (.materialize() gives an operator, .to_graph() a CSR)")
        return super().__getattr__(name)

    # -------------------------------------------------------------------------------------------- inputs
    def _operator(self, ori_adj):
        """(start operator, the dense tensor it came from or None)"""
        if torch.is_tensor(ori_adj):
            dense = ori_adj.detach()
            return RowNormalizedAdjacency.from_dense(dense.to(self.device).float()), dense
        if isinstance(ori_adj, RowNormalizedAdjacency):
            return ori_adj, None
        raise TypeError("ori_adj must be a dense tensor, a RowNormalizedAdjacency or a FlippedAdjacency")

    def _features(self, ori_features):
        return ori_features

    def _begin(self, ori_features, ori_adj):
        self.__dict__.pop("modified_adj", None)
        start, self._dense = self._operator(ori_adj)
        self._start, self._n = start, int(start.n)
        self._x_in = self._features(ori_features)
        self._x = self._x_in.detach().to(start.device)
        self._nfeat = int(self._x.shape[1])
        self._csr = start.csr() if isinstance(start, FlippedAdjacency) else (start.indptr, start.indices, start.values)
        self.surrogate.eval()
        self._local = self._local_model()
        self._x_trial = None                       # the view path's clone of x, made once per attack

    def _local_model(self):
        """(gcn, calibrator or None) when ``wg_trial_logits`` applies (as ``Calib_FGA._local_model``); feature trials
        only for the bare model and the node-wise calibrators of ``scaling.py``."""
        got = Calib_FGA._local_model(self)
        if got is not None and self.attack_features and got[1] is not None and not hasattr(got[1], "row_map"):
            return None
        return got

    def _new_target(self, t, rng):
        t = int(t)
        if not 0 <= t < self._n:
            raise ValueError(f"target {t} outside [0, {self._n})")
        indptr, indices, _ = self._csr
        s, e = (int(v) for v in indptr[t:t + 2].cpu())
        return _Target(t, rng, indices[s:e].cpu().tolist(), self._x[t].to(torch.float32).cpu().numpy().copy())

    # -------------------------------------------------------------------------------------------- one trial
    def _draw(self, T, present, occupied):
        """The draws of one trial (``calib_random.py:133-149``, ``:354-393``, ``:413-424``): ("edge", add, j),
        ("feature", add, f, new value) or None when nothing can be perturbed."""
        rng = T.rng
        if self.attack_structure and self.attack_features:
            structure = rng.choice([True, False])
        else:
            structure = self.attack_structure
        if structure:
            n_absent = self._n - len(occupied)
            if not (n_absent or present):
                return None
            if n_absent and present:
                add = rng.choice([True, False])
            else:
                add = bool(n_absent)
            if add:
                return "edge", True, _nth_absent(occupied, rng.randint(0, n_absent - 1))
            return "edge", False, present[rng.randint(0, len(present) - 1)]
        if self._nfeat == 0:
            return None
        f = rng.randint(0, self._nfeat - 1)
        cur = T.x[f]
        new = type(cur)(1 - cur)
        return "feature", bool(new > cur), f, new

    def _draw_step(self, T, max_trials):
        """The ``max_trials`` trials of one step drawn ahead, and what puts the stream back after trial k: the state
        before the step and the lists the draws were made over (``_rewind`` draws k + 1 trials again, which costs less
        than a ``getstate`` per trial)."""
        present = T.present()
        occupied = sorted(set(present) | {T.t})
        state = T.rng.getstate()
        return [self._draw(T, present, occupied) for _ in range(max_trials)], (state, present, occupied)

    def _rewind(self, T, rewind, k):
        """The random state after trial ``k`` of the step: where the reference stopped drawing."""
        state, present, occupied = rewind
        T.rng.setstate(state)
        for _ in range(k + 1):
            self._draw(T, present, occupied)

    def _trial_spec(self, T, d):
        """(partners, {feature: delta}) of the accepted state with the trial applied"""
        if d[0] == "edge":
            return sorted(T.toggles.symmetric_difference({d[2]})), T.changed
        feats = dict(T.changed)
        delta = float(d[3]) - float(T.x0[d[2]])
        if delta == 0.0:
            feats.pop(d[2], None)
        else:
            feats[d[2]] = delta
        return sorted(T.toggles), feats

    def _map(self, out, targets):
        """The calibrator's row map of a (B, C) block of base logits; ``targets``: each row's node."""
        wats = self._local[1]
        if wats is None:
            return out
        if hasattr(wats, "row_map"):
            return wats.row_map(out)
        temps = wats.temperatures()[torch.tensor(targets, dtype=torch.int64, device=out.device)]
        return F.log_softmax(out / temps.unsqueeze(1), dim=1)

    def _launch(self, specs):
        """One ``wg_trial_logits`` launch and one host read: (logits (B, C) on the host, labels, confidences)."""
        model = self._local[0]
        w1 = model.gc1.weight
        key = (self._x.data_ptr(), self._x._version, tuple(self._x.shape), w1.data_ptr(), w1._version)
        if self._z_key != key:
            self._z, self._z_key = (self._x.to(torch.float32) @ w1.t()).contiguous(), key
        with torch.no_grad():
            out = trial_logits(self._n, self._csr[0], self._csr[1], self._z, model.gc1.bias.detach(),
                               model.gc2.weight.detach().contiguous(), model.gc2.bias.detach(), specs,
                               W1=w1.detach() if any(s[2] for s in specs) else None)
            out = self._map(out, [s[0] for s in specs])
            return self._read(out)

    @staticmethod
    def _read(out):
        label = out.argmax(dim=1)
        conf = F.softmax(out, dim=1).gather(1, label.unsqueeze(1))
        host = torch.cat([out.float(), conf.float(), label.unsqueeze(1).float()], dim=1).cpu()
        C = out.shape[1]
        return host[:, :C], host[:, C + 1].long().tolist(), host[:, C].tolist()

    def _view(self, toggles):
        toggles = sorted(toggles)
        return self._start.with_flips([self._t_view] * len(toggles), toggles, self_loops=True) if toggles else self._start

    def _forward_view(self, T, partners, feats):
        """The surrogate's row t through a view of the start adjacency (any surrogate, valued graphs)."""
        self._t_view = T.t
        x = self._x
        if feats:
            if self._x_trial is None:
                self._x_trial = self._x.clone()
            x = self._x_trial
            row = T.x0.copy()
            for f, delta in feats.items():
                row[f] = T.x0[f] + delta
            x[T.t] = torch.from_numpy(row).to(x.dtype).to(x.device)
        with torch.no_grad():
            out = self.surrogate(x, self._view(partners))[[T.t]]
        if feats:
            x[T.t] = self._x[T.t]
        return self._read(out)

    # -------------------------------------------------------------------------------------------- the loop
    @staticmethod
    def _better(strategy):
        if strategy in ("under", "under_kl"):
            return lambda new, best: new < best
        if strategy == "over":
            return lambda new, best: new > best
        raise ValueError(f"Unknown strategy: {strategy}. Supported: 'under', 'over', 'under_kl'")

    def _accept(self, T, d, logits, label, conf, step, verbose):
        if d[0] == "edge":
            T.toggles.symmetric_difference_update({d[2]})
            T.flips.append(d[2])
        else:
            f, new = d[2], d[3]
            T.x[f] = new
            delta = float(new) - float(T.x0[f])
            if delta == 0.0:
                T.changed.pop(f, None)
                T.feature_flips.pop(f, None)
            else:
                T.changed[f] = delta
                T.feature_flips[f] = float(new)
        T.best_conf = conf
        T.attack_times += 1
        T.trace.append(dict(action=("Add" if d[1] else "Remove") + (" edge" if d[0] == "edge" else " feature"),
                            index=d[2], logits=logits.clone(), label=label, confidence=conf, step=step))
        if verbose:
            print(f"Step {step + 1}: {'Add' if d[1] else 'Remove'} {'edge' if d[0] == 'edge' else 'feature'} "
                  f"({T.t}, {d[2]})")
            print(f"New Confidence: {conf:.4f}")
            print(f"Best Confidence: {T.best_conf:.4f}")

    def _run(self, targets, n_perturbations, strategy, max_trials, verbose):
        """The targets in lock step.  Fast path: one launch and one host read per step for all of them."""
        better = self._better(strategy)
        if self._local is not None:
            _, labels, confs = self._launch([(T.t, [], None) for T in targets])
        else:
            labels, confs = [], []
            for T in targets:
                _, lab, cf = self._forward_view(T, [], None)
                labels.append(lab[0])
                confs.append(cf[0])
        for T, lab, cf in zip(targets, labels, confs):
            T.label, T.best_conf, T.conf0 = lab, cf, cf
            T.evaluated = []                       # every evaluated trial: (step, draw, logits, label, confidence)
            if verbose:
                print("-" * 25, f"  {self._name} ATTACK BEGINS  ", "-" * 25)
                print(f'Target Node: {T.t}')
                print(f'Number of perturbations: {n_perturbations}')
                print(f'Strategy: {strategy}')
                print(f'Max trials per perturbation: {max_trials}')
                print(f"Before Attack Label: {T.label}")
                print(f"Before Attack Confidence: {T.best_conf:.4f}")
                print("-" * 50)
        for step in range(n_perturbations):
            if self._local is not None:
                drawn = [self._draw_step(T, max_trials) for T in targets]
                specs, owner = [], []
                for i, T in enumerate(targets):
                    for k, d in enumerate(drawn[i][0]):
                        if d is not None:
                            specs.append((T.t,) + self._trial_spec(T, d))
                            owner.append((i, k))
                if specs:
                    logits, labels, confs = self._launch(specs)
                found = [False] * len(targets)
                for row, (i, k) in enumerate(owner):
                    if found[i]:
                        continue
                    T, d = targets[i], drawn[i][0][k]
                    T.evaluated.append((step, d, logits[row], labels[row], confs[row]))
                    if labels[row] == T.label and better(confs[row], T.best_conf):
                        found[i] = True
                        self._rewind(T, drawn[i][1], k)
                        self._accept(T, d, logits[row], labels[row], confs[row], step, verbose)
            else:
                found = []
                for T in targets:
                    present = T.present()
                    occupied = sorted(set(present) | {T.t})
                    ok = False
                    for _ in range(max_trials):
                        d = self._draw(T, present, occupied)
                        if d is None:
                            continue
                        logits, lab, cf = self._forward_view(T, *self._trial_spec(T, d))
                        T.evaluated.append((step, d, logits[0], lab[0], cf[0]))
                        if lab[0] == T.label and better(cf[0], T.best_conf):
                            ok = True
                            self._accept(T, d, logits[0], lab[0], cf[0], step, verbose)
                            break
                    found.append(ok)
            if verbose:
                for T, ok in zip(targets, found):
                    if not ok:
                        print(f"Step {step + 1}: No improvement found after {max_trials} trials")

    def _result(self, T):
        best = sorted(T.toggles)
        r = dict(target=T.t, flips=T.flips, best_flips=best, feature_flips=dict(T.feature_flips), trace=T.trace,
                 n_perturb=T.attack_times, best_conf=T.best_conf, original_label=T.label, original_conf=T.conf0,
                 evaluated=T.evaluated,
                 modified_op=self._start.with_flips([T.t] * len(best), best, self_loops=True))
        if T.changed:
            x = self._x_in.clone() if torch.is_tensor(self._x_in) else self._x.clone()
            x[T.t] = torch.from_numpy(T.x).to(x.dtype).to(x.device)
            r["modified_features"] = x
        else:
            r["modified_features"] = self._x_in
        if self._dense is not None:
            adj = self._dense.clone()
            present = set(T.base_row)
            for j in best:                          # calib_random.py:382-390: set to 1 or to 0, both entries
                adj[T.t, j] = adj[j, T.t] = 0 if j in present else 1
            r["modified_adj"] = adj
        return r

    def _publish(self, r, kwargs):
        self.target_node = r["target"]
        self.flips, self.best_flips, self.feature_flips = r["flips"], r["best_flips"], r["feature_flips"]
        self.trace, self.evaluated = r["trace"], r["evaluated"]
        self.modified_op, self.modified_features = r["modified_op"], r["modified_features"]
        if "modified_adj" in r:
            self.__dict__["modified_adj"] = r["modified_adj"]
        kwargs.setdefault("n_perturb", []).append(r["n_perturb"])
        kwargs.setdefault("best_conf", []).append(r["best_conf"])

    def attack(self, ori_features, ori_adj, target_node, n_perturbations, strategy=None, max_trials=100, verbose=False,
               **kwargs):
        """``calib_random.py:46-203`` / ``calib_rnd.py:78-254``, drawing from the global ``random`` stream.  The lists
        ``n_perturb`` / ``best_conf`` given as keywords are appended to."""
        import random
        strategy = self._default_strategy if strategy is None else strategy
        self._better(strategy)
        self._begin(ori_features, ori_adj)
        T = self._new_target(target_node, random)
        self._run([T], int(n_perturbations), strategy, int(max_trials), verbose)
        r = self._result(T)
        self._publish(r, kwargs)
        if verbose:
            print("-" * 50)
            print(f"Attack completed with {r['n_perturb']} perturbations")
            print(f"Final confidence: {r['best_conf']:.4f}")
            print("-" * 50)

    def attack_many(self, ori_features, ori_adj, targets, n_perturbations, strategy=None, max_trials=100, verbose=False,
                    seed=None):
        """``attack`` for several targets of one graph in lock step: one ``wg_trial_logits`` launch of
        ``len(targets) * max_trials`` trials and one host read per step.  Each target draws from its own
        ``random.Random``: ``seed`` is a list of one seed per target, an int that a ``random.Random`` turns into them,
        or None for one draw of the global stream per target.  Returns one dict per target (``seed`` among its keys);
        a target's result is that of ``attack`` alone after ``random.seed`` of its seed."""
        import random
        strategy = self._default_strategy if strategy is None else strategy
        self._better(strategy)
        targets = [int(t) for t in targets]
        if seed is None:
            seeds = [random.randrange(2 ** 63) for _ in targets]
        elif isinstance(seed, (list, tuple)):
            if len(seed) != len(targets):
                raise ValueError("attack_many: one seed per target expected")
            seeds = [int(s) for s in seed]
        else:
            src = random.Random(int(seed))
            seeds = [src.randrange(2 ** 63) for _ in targets]
        self._begin(ori_features, ori_adj)
        states = [self._new_target(t, random.Random(s)) for t, s in zip(targets, seeds)]
        if self._local is not None:
            self._run(states, int(n_perturbations), strategy, int(max_trials), verbose)
        else:
            for T in states:
                self._run([T], int(n_perturbations), strategy, int(max_trials), verbose)
        results = []
        for T, s in zip(states, seeds):
            r = self._result(T)
            r["seed"] = s
            results.append(r)
        return results


class Calib_Random(_RandomAttack):
    """``Calib_Random`` of the reference (``calib_attack/calib_random.py``) on the sparse path (DESIGN.md 4.3 "Random
    trials"): the same constructor and ``attack``.  A step's ``max_trials`` trials are drawn ahead with the reference's
    ``random`` calls in the reference's order, evaluated by one ``wg_trial_logits`` launch, the first accepted one is
    taken and the random state is put back to where the reference would have stopped drawing.  ``ori_adj``: a dense
    tensor, a ``RowNormalizedAdjacency`` or a ``FlippedAdjacency``.

    Fast path: a bare ``SparseCompatibleGCN``, an unfused ``WATS`` over one (structure trials only) or a calibrator of
    ``scaling.py``, on a unit graph with ``Hd, C <= 256``.  Everything else, and ``local_eval=False``, evaluates trial
    by trial through ``with_flips`` views; on a valued graph a removal there is the view's ``1 - 2 a`` toggle, which
    is the reference's "set to 0" only for entries equal to 1.  Results: ``flips`` / ``best_flips`` (partners, ``t``
    itself for its self loop), ``feature_flips`` (``{f: value}``), ``trace`` (per accepted step), ``evaluated`` (every
    evaluated trial), ``modified_op``, ``modified_features``, ``modified_adj`` (dense input only)."""

    _default_strategy = "under"
    _name = "CALIB_RANDOM"


class Calib_RND(_RandomAttack):
    """``Calib_RND`` of the reference (``calib_attack/calib_rnd.py``): the same trials as ``Calib_Random`` (its
    ``random.choice`` of an array takes the draw ``random.randint`` takes there), ``under_kl`` by default, scipy /
    numpy inputs accepted, ``modified_adj`` as a scipy CSR when the input was scipy, numpy or a dense tensor.
    Not kept: ``check_adj``'s dense test.  ``random_node_injection`` is not built: it changes ``n``."""

    _default_strategy = "under_kl"
    _name = "CALIB_RND"

    def _operator(self, ori_adj):
        import numpy as np
        import scipy.sparse as sp
        self._scipy_out = True
        if sp.issparse(ori_adj):
            M = sp.csr_matrix(ori_adj, dtype=np.float32)
            M.sum_duplicates()
            M.eliminate_zeros()
            M.sort_indices()
            unit = bool((M.data == 1).all())
            op = RowNormalizedAdjacency(M.shape[0], torch.from_numpy(M.indptr.astype(np.int64)).to(self.device),
                                        torch.from_numpy(M.indices.astype(np.int32)).to(self.device),
                                        None if unit else torch.from_numpy(M.data).to(self.device), device=self.device)
            return op, None
        if isinstance(ori_adj, np.ndarray):
            ori_adj = torch.from_numpy(np.asarray(ori_adj, np.float32))
        if isinstance(ori_adj, RowNormalizedAdjacency):
            self._scipy_out = False
        return super()._operator(ori_adj)

    def _features(self, ori_features):
        import numpy as np
        import scipy.sparse as sp
        if sp.issparse(ori_features):
            return torch.from_numpy(np.asarray(ori_features.todense(), np.float32))
        if isinstance(ori_features, np.ndarray):
            return torch.from_numpy(np.asarray(ori_features, np.float32))
        return ori_features

    def _result(self, T):
        import scipy.sparse as sp
        r = super()._result(T)
        if self._scipy_out:
            indptr, indices, values = r["modified_op"].csr()
            r["modified_adj"] = sp.csr_matrix((values.cpu().numpy(), indices.cpu().numpy(), indptr.cpu().numpy()),
                                              shape=(self._n, self._n))
        return r

    def random_node_injection(self, *args, **kwargs):
        raise NotImplementedError("Calib_RND.random_node_injection adds nodes: it changes n, which neither the "
                                  "with_flips views nor wg_trial_logits model (DESIGN.md 8, \"Not built\")")
