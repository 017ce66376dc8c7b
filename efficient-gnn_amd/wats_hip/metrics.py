"""Expected Calibration Error on the device.

Torch restatement of the reference's ``utils/ece.py:8-89`` (what the harness
scores every calibrator with, ``benchmark_calibration_methods.py:122``), so
the WATS evaluation needs no host copy.  Same binning quirks:

* ``np.digitize(p, linspace(0,1,n_bins+1), right=True) - 1`` (ece.py:40): bin i
  holds ``edges[i] < p <= edges[i+1]``; a probability of exactly 0 falls in no bin;
* bins with fewer than 4 samples are skipped (ece.py:49);
* ECE = sum |mean(p) - mean(label)| * bin_fraction (ece.py:60);
  ``calculate_average_ece`` = mean over classes (ece.py:64-89).

Inputs may be numpy arrays or torch tensors (any device); the result is a
Python float.  (This evaluation is plain torch: it is not on the wavelet hot
path.)

The evaluation step of the harness itself -- what it runs after every
calibrator (``benchmark_calibration_methods.py:87-158``) and before / after
every attack (``ugca_calib_attack.py:78-104``) -- is ``calibration_report``
and the drop-ins built on it, below: one fused HIP binning pass
(``csrc/calib.hip``, ``wg_calib_bins`` + ``wg_calib_ece``) and one host read.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check
from .laplacian import require_gpu, stream_handle


def _as_tensor(x, device=None):
    t = torch.as_tensor(x)
    return t.to(device) if device is not None else t


def calculate_ece(model_outputs, labels, pos_class: int, logits: bool = True, n_bins: int = 10) -> float:
    out = _as_tensor(model_outputs)
    lab = _as_tensor(labels, out.device)
    if out.shape[0] != lab.shape[0]:
        raise ValueError("Input arrays must have the same number of elements.")
    return float(_ece_all(out, lab, logits, n_bins, classes=[pos_class])[0])


def calculate_average_ece(model_outputs, labels, n_classes: int, logits: bool = True, n_bins: int = 10) -> float:
    out = _as_tensor(model_outputs)
    lab = _as_tensor(labels, out.device)
    if out.shape[0] != lab.shape[0]:
        raise ValueError("Input arrays must have the same number of elements.")
    return float(_ece_all(out, lab, logits, n_bins, classes=list(range(n_classes))).mean())


def _ece_all(out: torch.Tensor, lab: torch.Tensor, logits: bool, n_bins: int, classes) -> torch.Tensor:
    """Per-class ECE for the given classes, all classes in one pass (float64)."""
    probs = torch.softmax(out.double(), dim=1) if logits else out.double()
    p = probs[:, classes]                                        # (N, C)
    y = (lab.reshape(-1, 1) == torch.as_tensor(classes, device=lab.device).reshape(1, -1)).double()
    edges = torch.linspace(0, 1, n_bins + 1, dtype=torch.float64, device=p.device)
    b = torch.bucketize(p, edges, right=False) - 1               # == np.digitize(right=True) - 1
    n, C = p.shape
    valid = (b >= 0) & (b < n_bins)
    b = torch.where(valid, b, torch.zeros_like(b))
    idx = b + n_bins * torch.arange(C, device=p.device).reshape(1, -1)
    w = valid.double()
    cnt = torch.zeros(C * n_bins, dtype=torch.float64, device=p.device).index_add_(0, idx.flatten(), w.flatten())
    sp = torch.zeros_like(cnt).index_add_(0, idx.flatten(), (p * w).flatten())
    sy = torch.zeros_like(cnt).index_add_(0, idx.flatten(), (y * w).flatten())
    ok = cnt >= 4
    safe = torch.where(ok, cnt, torch.ones_like(cnt))
    term = torch.where(ok, (sp / safe - sy / safe).abs() * (cnt / n), torch.zeros_like(cnt))
    return term.reshape(C, n_bins).sum(dim=1)


# ----------------------------------------------------------------------------------------------------------------
# The harness's evaluation step on the device (csrc/calib.hip)
# ----------------------------------------------------------------------------------------------------------------
KINDS = {"probs": 0, "exp": 1, "logits": 2}
_QUANTUM = float(2 ** 40)
_edges_cache: dict = {}


@dataclass
class CalibrationReport:
    """What the harness prints and plots for one set of outputs over the listed rows.

    ``accuracy`` is the share of rows whose first maximal column is the label (``torch.argmax``), ``ece`` the class
    mean of ``utils/ece.py:64-89`` (over the first ``n_classes`` classes), ``ece_top_label`` the same sum on the
    row maxima.  ``avg_confidence`` and ``brier`` are means over the rows whose ``p`` are all finite
    (``nonfinite_rows`` counts the others), ``nll`` over the rows with a label in range and ``p_label > 0``.
    ``outside`` counts the class entries with ``p`` outside [0, 1] (``reliability_curves`` refuses those).
    ``table`` is the kernel's ``(C + 1, n_bins + 2, 3)`` uint64 table, ``counts`` / ``label_counts`` / ``sum_p`` its
    bins as ``(C + 1, n_bins)`` arrays (slice ``C``: the top label).
    """
    n: int
    accuracy: float
    avg_confidence: float
    ece: float
    ece_per_class: np.ndarray
    ece_top_label: float
    nll: float
    brier: float
    nonfinite_rows: int
    outside: int
    n_bins: int
    table: np.ndarray
    counts: np.ndarray
    label_counts: np.ndarray
    sum_p: np.ndarray


def _edges(n_bins: int, device) -> torch.Tensor:
    key = (n_bins, str(device))
    if key not in _edges_cache:   # numpy's own edges: edges[3] of 10 bins is 0.30000000000000004
        _edges_cache[key] = torch.from_numpy(np.linspace(0, 1, n_bins + 1)).to(device)
    return _edges_cache[key]


def _calib_rows(rows, n: int, device):
    """``rows`` (None, a boolean mask or an index tensor) as an int64 device list, or None.  Index values are
    checked by the kernel (it counts the ids it refuses), so an index tensor costs no host read here; a mask costs
    the read of its count."""
    if rows is None:
        return None
    rows = torch.as_tensor(rows).to(device)
    if rows.dtype == torch.bool:
        if rows.shape != (n,):
            raise ValueError(f"a boolean mask must have shape ({n},), not {tuple(rows.shape)}")
        return torch.nonzero(rows).flatten().contiguous()
    if rows.dim() != 1 or rows.is_floating_point() or rows.is_complex():
        raise ValueError("rows must be a boolean mask or a 1-D integer index tensor")
    return rows.to(torch.int64).contiguous()


def _calib_launch(out: torch.Tensor, labels: torch.Tensor, rows, kind: int, n_bins: int, min_count: int,
                  n_workgroups: int = 0):
    """Both launches on ``out`` (G, n, C); returns the device buffer ``[table | scalars | ece_class | ece_top]`` in
    8-byte slots and the slot offsets."""
    lib = _lib.load()
    G, n, C = out.shape
    n_rows = n if rows is None else rows.numel()
    device = out.device
    cells = (C + 1) * (n_bins + 2) * 3
    off = np.cumsum([0, G * cells, G * 8, G * C, G])
    buf = torch.empty(max(1, int(off[-1])), dtype=torch.int64, device=device)
    nbytes = ctypes.c_int64(0)
    check(lib.wg_calib_workspace(G, C, n_bins, n_rows, ctypes.byref(nbytes)), "calib_workspace")
    ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=device)
    base = buf.data_ptr()
    with torch.cuda.device(device):
        stream = stream_handle(device)
        check(lib.wg_calib_bins(G, n, C, kind, out.data_ptr(), labels.data_ptr(), n_rows,
                                None if rows is None else rows.data_ptr(), n_bins, _edges(n_bins, device).data_ptr(),
                                n_workgroups, ws.data_ptr(), base, base + 8 * int(off[1]), stream), "calib_bins")
        check(lib.wg_calib_ece(G, C, n_bins, n_rows, min_count, base, base + 8 * int(off[2]),
                               base + 8 * int(off[3]), stream), "calib_ece")
    return buf, off, n_rows


def _as_sets(outputs, device):
    """``outputs`` as a (G, n, C) float32 device tensor and whether a list of reports is wanted."""
    many = isinstance(outputs, (list, tuple))
    if many:
        outs = [torch.as_tensor(o).detach() for o in outputs]
        if not outs:
            raise ValueError("an empty list of outputs")
        if any(o.dim() != 2 or o.shape != outs[0].shape for o in outs):
            raise ValueError("every set of outputs must have the same (n, C) shape")
        out = torch.stack([o.to(device=device, dtype=torch.float32) for o in outs])
    else:
        out = torch.as_tensor(outputs).detach()
        if out.dim() == 3:
            many = True
        elif out.dim() == 2:
            out = out.unsqueeze(0)
        else:
            raise ValueError(f"outputs must be (n, C) or (G, n, C), not {tuple(out.shape)}")
        out = out.to(device=device, dtype=torch.float32)
    return out.contiguous(), many


def calibration_report(outputs, labels, rows=None, kind: str = "probs", n_bins: int = 10, min_count: int = 4,
                       n_classes: int | None = None):
    """The accuracy / confidence / ECE triple of the harness, the per-class and top-label ECE, NLL, Brier and the
    binned table, from one binning pass in HIP and one host read.

    ``outputs``: ``(n, C)`` gives a ``CalibrationReport``; ``(G, n, C)`` or a list of ``(n, C)`` gives a list of
    reports from the same launch (before / after an attack, several calibrators), sharing ``labels`` and ``rows``.
    ``kind``: ``"probs"``; ``"exp"`` (``p = exp(x)``, not normalised: what the harness does to whatever a model
    returns); ``"logits"`` (the float64 softmax rounded once).  ``rows``: None, a boolean mask or an index tensor
    (repeats count twice, as ``probs[idx]``); an index outside ``[0, n)`` raises ``IndexError``.  Inputs on the
    host are copied to the current GPU first; there is no CPU path.
    """
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, not {kind!r}")
    first = outputs[0] if isinstance(outputs, (list, tuple)) and len(outputs) else outputs
    device = require_gpu(first.device if isinstance(first, torch.Tensor) and first.is_cuda else None)
    out, many = _as_sets(outputs, device)
    G, n, C = out.shape
    lab = torch.as_tensor(labels).to(device)
    if lab.dim() != 1 or lab.shape[0] != n or lab.is_floating_point() or lab.dtype == torch.bool:
        raise ValueError(f"labels must be {n} integers, not {tuple(lab.shape)} {lab.dtype}")
    lab = lab.to(torch.int64).contiguous()
    n_bins, min_count = int(n_bins), int(min_count)
    if n_classes is None:
        n_classes = C
    if not 1 <= int(n_classes) <= C:
        raise ValueError(f"n_classes = {n_classes} outside [1, {C}]")
    idx = _calib_rows(rows, n, device)
    buf, off, n_rows = _calib_launch(out, lab, idx, KINDS[kind], n_bins, min_count)
    host = buf.cpu().numpy()                                    # the one host read
    table = host[off[0]:off[1]].view(np.uint64).reshape(G, C + 1, n_bins + 2, 3)
    scalars = host[off[1]:off[2]].view(np.float64).reshape(G, 8)
    ece_class = host[off[2]:off[3]].view(np.float64).reshape(G, C)
    ece_top = host[off[3]:off[4]].view(np.float64).reshape(G)
    if scalars[:, 7].any():
        raise IndexError(f"rows outside [0, {n}): {int(scalars[0, 7])} of {n_rows}")
    reports = []
    nan = float("nan")
    for g in range(G):
        t, s = table[g], scalars[g]
        taken, fin = int(s[0]), int(s[1])
        bins = t[:, :n_bins]
        low, high = t[:C, n_bins], t[:C, n_bins + 1]
        reports.append(CalibrationReport(
            n=taken,
            accuracy=float(t[C, :, 1].sum()) / taken if taken else nan,
            avg_confidence=s[3] / fin if fin else nan,
            ece=float(np.mean(ece_class[g, :int(n_classes)])),
            ece_per_class=ece_class[g].copy(),
            ece_top_label=float(ece_top[g]),
            nll=s[4] / s[5] if s[5] else nan,
            brier=s[6] / fin if fin else nan,
            nonfinite_rows=taken - fin,
            outside=int(high[:, 0].sum() + low[:, 0].sum() - low[:, 2].sum()),
            n_bins=n_bins,
            table=t.copy(),
            counts=bins[..., 0].astype(np.int64),
            label_counts=bins[..., 1].astype(np.int64),
            sum_p=bins[..., 2].astype(np.float64) / _QUANTUM,
        ))
    return reports if many else reports[0]


def _print_results(model_name: str, acc: float, conf: float, ece: float) -> None:
    print(f"{model_name} Results:")
    print(f"  Test Accuracy: {acc:.4f}")
    print(f"  Average Confidence: {conf:.4f}")
    print(f"  Expected Calibration Error (ECE): {ece:.4f}")


def evaluate_calibration(model, x, y, adj, test_mask, model_name="Model", *, kind: str = "exp", verbose: bool = True):
    """``benchmark_calibration_methods.py:87-127``: the model's eval-mode output over ``test_mask`` scored on the
    device; no ``(n, C)`` array leaves it.  Returns ``(acc, avg_confidence, ece)`` as Python floats and prints the
    reference's lines.  ``kind="exp"`` is what the reference does to WHATEVER the model returns (every tensor has
    ``.exp``, :102-103): pass ``kind="logits"`` to score a base model that returns raw logits properly."""
    if hasattr(model, "eval"):
        model.eval()          # and left in eval mode, as the reference leaves it (:98)
    with torch.no_grad():
        out = model(x, adj)
    r = calibration_report(out, y, rows=test_mask, kind=kind)
    if verbose:
        _print_results(model_name, r.accuracy, r.avg_confidence, r.ece)
    return r.accuracy, r.avg_confidence, r.ece


def evaluate_calibration_probs(probs, y, test_mask, model_name="Model", *, kind: str = "probs", verbose: bool = True):
    """``benchmark_calibration_methods.py:130-158`` on the device."""
    r = calibration_report(probs, y, rows=test_mask, kind=kind)
    if verbose:
        _print_results(model_name, r.accuracy, r.avg_confidence, r.ece)
    return r.accuracy, r.avg_confidence, r.ece


def reliability_curves(outputs, labels, n_classes: int, n_bins: int = 10, kind: str = "probs"):
    """Per class ``c < n_classes`` the ``(prob_true, prob_pred)`` of sklearn's ``calibration_curve((labels == c),
    probs[:, c], n_bins=n_bins)``: what ``ece_chart`` plots (``utils/ece.py:111-115``).  sklearn's rule differs from
    the ECE's only in putting ``p == 0`` into bin 0 (sum 0), so the same table serves; empty bins are dropped.
    Raises ``ValueError`` when any ``p`` lies outside [0, 1], as sklearn does."""
    r = calibration_report(outputs, labels, kind=kind, n_bins=n_bins, n_classes=n_classes)
    if isinstance(r, list):
        raise ValueError("reliability_curves takes one (n, C) set of outputs")
    if r.outside:
        raise ValueError("y_prob has values outside [0, 1].")
    curves = []
    for c in range(int(n_classes)):
        cnt = r.counts[c].astype(np.float64)
        true = r.label_counts[c].astype(np.float64)
        cnt[0] += float(r.table[c, n_bins, 0])       # the exact zeros
        true[0] += float(r.table[c, n_bins, 1])
        nz = cnt != 0
        curves.append((true[nz] / cnt[nz], r.sum_p[c][nz] / cnt[nz]))
    return curves


def average_ece_many(outputs_list, labels, n_classes: int, n_bins: int = 10, kind: str = "probs"):
    """The list ``draw_multiple_ece_charts`` returns (``utils/ece.py:249-251``): the average ECE of every set, one
    launch for all of them.  With two sets it is the before / after pair of ``exp/ablation/calculate_ece.py``."""
    reports = calibration_report(list(outputs_list), labels, kind=kind, n_bins=n_bins, n_classes=n_classes)
    return [r.ece for r in reports]
