"""The reference's four node-wise calibrators on the HIP path: ``TemperatureScaling`` (``TS``,
reference ``calibration/TS.py``), ``VectorScaling`` (``VS``, ``VS.py``), ``MatrixScaling`` (``MS``, ``MS.py``) and
``ETS`` (``ETS.py``).

All four are row-wise maps of the base model's logits ``z``:

* TS / VS: ``log_softmax(z * s)`` with ``s = log(exp(temperature) + 1.1)``, one ``s`` or one per class (it
  MULTIPLIES, TS.py:42-43);
* MS: ``z' = z - z[:, -1:]``, ``z' @ W + b`` returned RAW (MS.py:43-57), ``W = ones(C, C)`` and ``b = ones(C)`` at
  the start (MS.py:28-29); ``normalize=True`` gives ``log_softmax`` of it (Guo et al.'s matrix scaling);
* ETS: ``log(w1 softmax(z / temp) + w2 softmax(z) + w3 / C)``, ``temp = log(exp(tau) + 1.1)`` of its own ``TS``
  (it DIVIDES, ETS.py:24-25), while ``fit`` divides by the RAW ``tau`` (ETS.py:43, :57).  Both are kept as found.

Here:

* ``scaled_log_probs(logits, mode, *params, rows=None, normalize=False)``: the map as one fused pass per direction
  (``wg_scale_forward`` / ``wg_scale_backward``, ``csrc/scale.hip``), differentiable to first order w.r.t. the logits
  and every parameter; ``rows`` (an index tensor or a boolean mask) restricts it to some rows.
* ``train_scaling(mode, logits, y, rows, ...)``: ``calib_train`` (TS.py:45-83) with one ``wg_scale_epoch`` launch per
  epoch.  Forward, loss, gradients, accuracy, torch's Adam step (lr 0.01, L2 weight decay 5e-4) and the
  early-stopping state stay in one device block; ``logits`` is a tensor (all epochs are enqueued back to back, the
  state is read once) or a callable ``epoch -> logits`` (the host reads the stopped flag every ``sync_every``
  epochs).  The master parameters and Adam moments are float64; the module's parameters are their float32 rounding.
* the classes, with the reference's positional order ``(base_model, x, y, adj, val_idx)``, attribute and parameter
  names (``temperature``; ``W``, ``b``; ``w1``, ``w2``, ``w3``, ``temp_model.temperature``; ``base_model`` in TS and
  VS, ``model`` in MS and ETS), ``forward(x, adj, **kwargs)`` (keywords go to the base model: ``probe=``),
  ``calib_train(patience=10)`` (VS: also the unused ``alpha``), ``ETS.fit(masks)``, and the
  ``calibrate_with_*_scaling`` functions.  Keyword-only extras: ``verbose``, ``epochs=250``, ``frozen_logits``,
  ``normalize`` (MS).

``frozen_logits=False`` (the default) mirrors the reference: ``self.train()`` at the top of each epoch puts the base
model into train mode too, so its dropout is live during calibration training (TS.py:60, model.py:49) and the logits
are recomputed every epoch, dropout drawn from torch's generator.  ``frozen_logits=True`` takes the logits once
from an eval-mode forward.  With a base model without dropout both give the same bits.

``ETS.fit`` runs the reference's SLSQP (bounds, constraint, start, ``tol``, no ``jac``) on the two float64 vectors
``softmax(z / tau)[i, y_i]`` and ``softmax(z)[i, y_i]`` from ``wg_ets_label_probs``: with a one-hot label nothing else
enters the objective, and no ``(n_val, C)`` array leaves the device.  As in the reference ``fit`` leaves ``w1`` ..
``w3`` as 0-dim float64 tensors.

Not built: second-order gradients, more than ``max_classes(mode)`` classes (256; MS: 64), a CPU path, the plotting
helpers of TS.py.  ``verbose`` prints the reference's line per epoch after the run, not during it.
"""
from __future__ import annotations

import ctypes
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import check, ptr
from .gcn import SparseCompatibleGCN
from .laplacian import require_gpu, stream_handle

MODES = {"ts": 0, "vs": 1, "ms": 2, "ets": 3}
LR, WEIGHT_DECAY, MS_LAMBDA = 0.01, 5e-4, 1.0      # TS.py:58, MS.py:30


def _mode(mode) -> int:
    if isinstance(mode, str):
        if mode.lower() not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}, not {mode!r}")
        return MODES[mode.lower()]
    if int(mode) not in MODES.values():
        raise ValueError(f"mode must be 0 .. 3, not {mode}")
    return int(mode)


def max_classes(mode) -> int:
    """The widest row the kernels take (``wg_scale_max_c``): 256, for MS 64 (a lane keeps a column of dW in
    registers)."""
    return int(_lib.load().wg_scale_max_c(_mode(mode)))


def _row_list(rows, n: int, device):
    """``rows`` (None, a boolean mask or an index tensor) as a checked int32 device list, or None."""
    if rows is None:
        return None
    rows = torch.as_tensor(rows).to(device)
    if rows.dtype == torch.bool:
        if rows.shape != (n,):
            raise ValueError(f"a boolean mask must have shape ({n},), not {tuple(rows.shape)}")
        rows = torch.nonzero(rows).flatten()
    if rows.dim() != 1 or rows.is_floating_point():
        raise ValueError("rows must be a boolean mask or a 1-D integer index tensor")
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
        raise IndexError(f"rows outside [0, {n})")
    return rows.to(torch.int32).contiguous()


def _param_shapes(mode: int, C: int):
    return {0: [(1,)], 1: [(C,)], 2: [(C, C), (C,)], 3: [(1,), (1,), (1,), (1,)]}[mode]


def _check_params(mode: int, C: int, params, device):
    shapes = _param_shapes(mode, C)
    if len(params) != len(shapes):
        raise ValueError(f"mode {mode} takes {len(shapes)} parameters, got {len(params)}")
    out = []
    for p, shape in zip(params, shapes):
        if p.numel() != int(np.prod(shape)):
            raise ValueError(f"a parameter of mode {mode} with C = {C} has {int(np.prod(shape))} entries, got "
                             f"{tuple(p.shape)}")
        out.append(p.to(device=device, dtype=torch.float32).reshape(shape).contiguous())
    return out + [None] * (4 - len(out))


class _ScaledLogProbs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, rows, mode, flags, *params):
        n, C = logits.shape
        n_rows = n if rows is None else rows.numel()
        out = torch.empty((n_rows, C), dtype=torch.float32, device=logits.device)
        p = _check_params(mode, C, [q.detach() for q in params], logits.device)
        with torch.cuda.device(logits.device):
            check(_lib.load().wg_scale_forward(mode, flags, n, n_rows, C, ptr(logits), ptr(rows), *(ptr(q) for q in p),
                                               ptr(out), stream_handle(logits.device)), "scale_forward")
        ctx.save_for_backward(logits, *p[:len(params)])
        ctx.rows, ctx.mode, ctx.flags = rows, mode, flags
        ctx.shapes, ctx.dtypes = [q.shape for q in params], [q.dtype for q in params]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logits, *params = ctx.saved_tensors
        n, C = logits.shape
        rows, mode = ctx.rows, ctx.mode
        n_rows = n if rows is None else rows.numel()
        g = g.to(torch.float32).contiguous()
        p = params + [None] * (4 - len(params))
        want = [ctx.needs_input_grad[4 + k] for k in range(len(params))]
        gp = [torch.empty_like(q) if w else None for q, w in zip(params, want)] + [None] * (4 - len(params))
        g_logits = torch.empty((n_rows, C), dtype=torch.float32, device=logits.device) \
            if ctx.needs_input_grad[0] else None
        lib = _lib.load()
        ws = None
        if any(want):
            nbytes = ctypes.c_int64()
            check(lib.wg_scale_backward_workspace(mode, n_rows, C, ctypes.byref(nbytes)), "scale_backward_workspace")
            ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=logits.device)
        if g_logits is not None or any(want):
            with torch.cuda.device(logits.device):
                check(lib.wg_scale_backward(mode, ctx.flags, n, n_rows, C, ptr(logits), ptr(rows),
                                            *(ptr(q) for q in p), ptr(g), ptr(g_logits), *(ptr(q) for q in gp),
                                            ptr(ws), stream_handle(logits.device)), "scale_backward")
        if g_logits is not None and rows is not None:       # a repeated row collects every copy's gradient
            g_logits = torch.zeros_like(logits).index_add_(0, rows.long(), g_logits)
        return (g_logits, None, None, None) + tuple(None if q is None else q.reshape(s).to(d)
                                                    for q, s, d in zip(gp, ctx.shapes, ctx.dtypes))


def scaled_log_probs(logits: torch.Tensor, mode, *params: torch.Tensor, rows=None,
                     normalize: bool = False) -> torch.Tensor:
    """The calibrator's row map of ``logits`` (n, C): ``mode`` ``'ts'`` (temperature (1,)), ``'vs'`` (temperature
    (C,)), ``'ms'`` (W (C, C), b (C); raw unless ``normalize``) or ``'ets'`` (tau, w1, w2, w3).  ``rows`` selects rows
    (index tensor, repeats allowed, or boolean mask); the result is (len(rows), C) float32.  Differentiable w.r.t. the
    logits and the parameters.  The kernels use no float atomics and give the same bits for the same input; with
    ``rows`` the compact ``g_logits`` is scattered back by ``torch.index_add_`` (float32 atomics), so the gradient of
    a REPEATED row is the sum of its copies in an order that may change from run to run."""
    mode = _mode(mode)
    device = require_gpu(logits.device if logits.is_cuda else None)
    if logits.dim() != 2:
        raise ValueError(f"logits must be (n, C), not {tuple(logits.shape)}")
    if logits.shape[1] > max_classes(mode):
        raise NotImplementedError(f"C = {logits.shape[1]} is above {max_classes(mode)} classes for mode {mode}")
    logits = logits.to(device=device, dtype=torch.float32).contiguous()
    rows = _row_list(rows, logits.shape[0], device)
    if normalize and mode != MODES["ms"]:
        raise ValueError("normalize belongs to matrix scaling only")
    return _ScaledLogProbs.apply(logits, rows, mode, 1 if normalize else 0, *params)


class _TrainingState:
    """The device state block of ``wg_scale_epoch`` for one run."""

    def __init__(self, mode: int, C: int, epochs: int, max_rows: int, patience: int, normalize: bool, device,
                 init=None, lr=LR, weight_decay=WEIGHT_DECAY, Lambda=MS_LAMBDA):
        self.mode, self.C, self.epochs, self.flags, self.device = mode, C, int(epochs), 1 if normalize else 0, device
        self.max_rows = int(max_rows)
        lib = _lib.load()
        nbytes = ctypes.c_int64()
        check(lib.wg_scale_state_bytes(mode, C, self.epochs, max_rows, ctypes.byref(nbytes)), "scale_state_bytes")
        self.block = torch.empty(nbytes.value // 8, dtype=torch.float64, device=device)
        if init is not None:
            init = torch.cat([p.detach().to(device=device, dtype=torch.float32).flatten() for p in init]).contiguous()
        with torch.cuda.device(device):
            check(lib.wg_scale_state_init(ptr(self.block), mode, self.flags, C, self.epochs, max_rows, int(patience),
                                          float(lr), float(weight_decay), float(Lambda), ptr(init),
                                          stream_handle(device)), "scale_state_init")

    def epoch(self, logits, rows, y, n_workgroups: int = 0):
        n = logits.shape[0]
        n_rows = n if rows is None else rows.numel()
        with torch.cuda.device(self.device):
            check(_lib.load().wg_scale_epoch(ptr(self.block), self.mode, self.flags, self.C, self.epochs, self.max_rows, n,
                                             n_rows,
                                             ptr(logits), ptr(rows), ptr(y), int(n_workgroups),
                                             stream_handle(self.device)), "scale_epoch")

    def read(self):
        """(parameters as float32 device tensors, info as a float64 host array) -- one host sync."""
        n_par = sum(int(np.prod(s)) for s in _param_shapes(self.mode, self.C))
        flat = torch.empty(n_par, dtype=torch.float32, device=self.device)
        info = torch.empty(5 + 2 * self.epochs, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(_lib.load().wg_scale_state_read(ptr(self.block), self.mode, self.C, self.epochs, ptr(flat),
                                                  ptr(info), stream_handle(self.device)), "scale_state_read")
        params, at = [], 0
        for s in _param_shapes(self.mode, self.C):
            k = int(np.prod(s))
            params.append(flat[at:at + k].reshape(s).clone())
            at += k
        return params, info.cpu().numpy()

    def partials(self, n_rows: int) -> torch.Tensor:
        """The chunk partials of the last epoch that ran on ``n_rows`` rows, (chunks, 2 + parameters) float64: the
        chunk's sum of -out[r, y_r], its correct count, and its share of the nll SUM's parameter gradients."""
        n_par = sum(int(np.prod(s)) for s in _param_shapes(self.mode, self.C))
        chunks = -(-n_rows // int(_lib.load().wg_scale_chunk_rows()))
        at = 16 + 3 * n_par + 2 * self.epochs
        return self.block[at:at + chunks * (2 + n_par)].reshape(chunks, 2 + n_par)

    def stopped(self) -> bool:
        return bool(self.block[1].item() != 0)     # the stopped slot of the header


def train_scaling(mode, logits, y: torch.Tensor, rows=None, *, epochs: int = 250, patience: int = 10,
                  normalize: bool = False, init=None, n_workgroups: int = 0, sync_every: int = 10):
    """``calib_train`` (TS.py:45-83, VS.py:51-89, MS.py:59-89) on the device.  ``logits``: the (n, C) logits of every
    epoch, or a callable ``epoch -> (n, C) logits`` (then the host reads the stopped flag every ``sync_every`` epochs
    and stops calling).  ``y`` (n,) int64 labels, ``rows`` the calibration rows.  Returns a namespace: ``params``
    (float32 tensors: temperature, or W and b), ``loss`` / ``acc`` (per epoch run), ``epochs_run``, ``stop_epoch``
    (the epoch early stopping fired in, else None), ``best_loss``, ``state`` (the device block)."""
    mode = _mode(mode)
    if mode == MODES["ets"]:
        raise ValueError("ETS has no trained parameters of its own (its TS is trained; then ETS.fit)")
    first = logits(0) if callable(logits) else logits
    device = require_gpu(first.device if first.is_cuda else None)
    if first.dim() != 2:
        raise ValueError(f"logits must be (n, C), not {tuple(first.shape)}")
    n, C = first.shape
    if C > max_classes(mode):
        raise NotImplementedError(f"C = {C} is above {max_classes(mode)} classes for mode {mode}")
    y = y.to(device=device, dtype=torch.int64).contiguous()
    if y.shape != (n,):
        raise ValueError(f"y must have shape ({n},), not {tuple(y.shape)}")
    rows = _row_list(rows, n, device)
    n_rows = n if rows is None else rows.numel()
    if n_rows == 0:
        raise ValueError("no calibration rows")
    picked = y if rows is None else y[rows.long()]
    if int(picked.min()) < 0 or int(picked.max()) >= C:
        raise IndexError(f"a label outside [0, {C})")
    st = _TrainingState(mode, C, epochs, n_rows, patience, normalize, device, init)

    def prepared(z):
        if z.shape != (n, C):
            raise ValueError(f"the logits changed shape: {tuple(z.shape)} after {(n, C)}")
        return z.detach().to(device=device, dtype=torch.float32).contiguous()

    if callable(logits):
        z = prepared(first)
        for epoch in range(epochs):
            if epoch:
                z = prepared(logits(epoch))
            st.epoch(z, rows, y, n_workgroups)
            if sync_every and (epoch + 1) % sync_every == 0 and st.stopped():
                break
    else:
        z = prepared(first)
        for _ in range(epochs):         # a launch that finds the stopped flag set touches nothing
            st.epoch(z, rows, y, n_workgroups)
    params, info = st.read()
    run = int(info[1])
    return SimpleNamespace(params=params, loss=info[5:5 + run].copy(), acc=info[5 + epochs:5 + epochs + run].copy(),
                           epochs_run=run, stop_epoch=run - 1 if info[0] == 1 else None, best_loss=float(info[4]),
                           patience_left=int(info[3]), state=st.block)


def ets_label_probs(logits: torch.Tensor, y: torch.Tensor, temperature: torch.Tensor, rows=None):
    """``softmax(z / tau)[i, y_i]`` and ``softmax(z)[i, y_i]`` of the listed rows as two float64 device vectors
    (``wg_ets_label_probs``): all that ETS's objective reads (ETS.py:50-76)."""
    device = require_gpu(logits.device if logits.is_cuda else None)
    logits = logits.detach().to(device=device, dtype=torch.float32).contiguous()
    n, C = logits.shape
    if C > max_classes("ets"):
        raise NotImplementedError(f"C = {C} is above {max_classes('ets')} classes")
    y = y.to(device=device, dtype=torch.int64).contiguous()
    rows = _row_list(rows, n, device)
    n_rows = n if rows is None else rows.numel()
    tau = temperature.detach().to(device=device, dtype=torch.float32).reshape(1).contiguous()
    p0 = torch.empty(n_rows, dtype=torch.float64, device=device)
    p1 = torch.empty(n_rows, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        check(_lib.load().wg_ets_label_probs(n, n_rows, C, ptr(logits), ptr(rows), ptr(y), ptr(tau), ptr(p0), ptr(p1),
                                             stream_handle(device)), "ets_label_probs")
    return p0, p1


def ensemble_weights(p0y: np.ndarray, p1y: np.ndarray, num_classes: int) -> np.ndarray:
    """ETS.py:50-76 on the label columns: SLSQP from (1, 0, 0) over ``w`` in [0, 1]^3 with ``sum w = 1``,
    ``tol=1e-12``, no ``jac`` (scipy's finite differences, as the reference)."""
    import scipy.optimize
    p2 = 1.0 / num_classes

    def ll_w(w):
        return -np.sum(np.log(w[0] * p0y + w[1] * p1y + w[2] * p2)) / p0y.shape[0]

    res = scipy.optimize.minimize(ll_w, (1.0, 0.0, 0.0), method="SLSQP",
                                  constraints={"type": "eq", "fun": lambda x: np.sum(x) - 1},
                                  bounds=((0.0, 1.0),) * 3, tol=1e-12, options={"disp": False})
    return res.x


class _Scaling(nn.Module):
    """What the four classes share: where the base model lives, its logits, the training driver."""

    _mode_name = "ts"
    _base_attr = "base_model"

    def _setup(self, base_model, x, y, adj, val_idx, verbose, epochs, frozen_logits):
        self.device = require_gpu()
        setattr(self, self._base_attr, base_model.to(self.device))
        self.x = x.to(self.device)
        self.y = y.to(self.device)
        self.adj = adj.to(self.device) if torch.is_tensor(adj) else adj   # or a RowNormalizedAdjacency
        self.val_idx = val_idx.to(self.device)
        self.verbose, self.epochs, self.frozen_logits = bool(verbose), int(epochs), bool(frozen_logits)
        for para in base_model.parameters():
            para.requires_grad = False

    @property
    def _base(self):
        return getattr(self, self._base_attr)

    def _logits(self, x, adj, **kwargs):
        x = x.to(self.device)
        if torch.is_tensor(adj):
            adj = adj.to(self.device)
        return self._base(x, adj, **kwargs)

    def _params(self):
        raise NotImplementedError

    def _flags(self) -> bool:
        return False

    def row_map(self, logits: torch.Tensor, rows=None) -> torch.Tensor:
        """The calibrator's map of given logits (any block of rows, e.g. one candidate row of an attack)."""
        return scaled_log_probs(logits, self._mode_name, *self._params(), rows=rows, normalize=self._flags())

    def forward(self, x, adj, **kwargs):
        return self.row_map(self._logits(x, adj, **kwargs))

    def _train_adj(self):
        if isinstance(self._base, SparseCompatibleGCN) and torch.is_tensor(self.adj):
            return self._base.operator(self.adj)       # built once, not per epoch
        return self.adj

    def _run_training(self, patience: int, logits=None):
        adj = self._train_adj()
        if logits is None and self.frozen_logits:
            self.eval()
            with torch.no_grad():
                logits = self._logits(self.x, adj)
        elif logits is None:
            def logits(epoch):                          # TS.py:60-62: train mode reaches the base model's dropout
                self.train()
                with torch.no_grad():
                    return self._logits(self.x, adj)
        t = time.time()
        run = train_scaling(self._mode_name, logits, self.y, self.val_idx, epochs=self.epochs, patience=patience,
                            normalize=self._flags(), init=[p.detach() for p in self._params()])
        self.eval()
        with torch.no_grad():
            for p, v in zip(self._params(), run.params):
                p.copy_(v.reshape(p.shape))
        if self.verbose:
            for e in range(run.epochs_run):
                print(f"epoch: {e}", f"loss_calibration: {run.loss[e]:.4f}", f"acc_calibration: {run.acc[e]:.4f}",
                      f"time: {time.time() - t:.4f}s")
            if run.stop_epoch is not None:
                print(f"Early stopping at epoch {run.stop_epoch}, best loss: {run.best_loss:.4f}")
        self.training_run = run
        return self


class TemperatureScaling(_Scaling):
    """TS.py:23-83.  ``logits=``: a tensor or callable for ``train_scaling`` instead of the base model's logits."""

    def __init__(self, base_model, x, y, adj, val_idx, *, verbose: bool = True, epochs: int = 250,
                 frozen_logits: bool = False):
        super().__init__()
        self.temperature = nn.Parameter(torch.ones(1) * 1.0)             # TS.py:26
        self._setup(base_model, x, y, adj, val_idx, verbose, epochs, frozen_logits)
        self.to(self.device)
        self.calib_train()

    def _params(self):
        return [self.temperature]

    def calib_train(self, patience=10, *, logits=None):
        return self._run_training(patience, logits)


class VectorScaling(_Scaling):
    """VS.py:1-89."""

    _mode_name = "vs"

    def __init__(self, base_model, x, y, adj, val_idx, *, verbose: bool = True, epochs: int = 250,
                 frozen_logits: bool = False):
        super().__init__()
        n_classes = int(y.max().item()) + 1                              # VS.py:32
        self.temperature = nn.Parameter(torch.ones(n_classes) * 1.0)     # VS.py:33
        self._setup(base_model, x, y, adj, val_idx, verbose, epochs, frozen_logits)
        self.to(self.device)
        self.calib_train()

    def _params(self):
        return [self.temperature]

    def calib_train(self, patience=10, alpha=0.5, *, logits=None):       # alpha: unused, as VS.py:51
        return self._run_training(patience, logits)


class MatrixScaling(_Scaling):
    """MS.py:7-89.  The output is RAW (no log_softmax) unless ``normalize=True``."""

    _mode_name = "ms"
    _base_attr = "model"

    def __init__(self, base_model, x, y, adj, val_idx, *, verbose: bool = True, epochs: int = 250,
                 frozen_logits: bool = False, normalize: bool = False):
        super().__init__()
        self.n_classes = int(y.max().item()) + 1                         # MS.py:27
        self.W = nn.Parameter(torch.ones(self.n_classes, self.n_classes))   # MS.py:28: ones, not the identity
        self.b = nn.Parameter(torch.ones(self.n_classes))                # MS.py:29
        self.Lambda = 1
        self.normalize = bool(normalize)
        self._setup(base_model, x, y, adj, val_idx, verbose, epochs, frozen_logits)
        self.to(self.device)
        self.calib_train()

    def _params(self):
        return [self.W, self.b]

    def _flags(self):
        return self.normalize

    def matrix_scale(self, logits):
        """MS.py:49-57 on already shifted logits, in torch (``forward`` runs the fused map)."""
        return torch.matmul(logits.to(self.device), self.W) + self.b

    def calib_train(self, patience=10, *, logits=None):
        return self._run_training(patience, logits)


class ETS(_Scaling):
    """ETS.py:8-76: ``ETS(model, x, y, adj, val_idx).fit([train_mask, val_mask, test_mask])``."""

    _mode_name = "ets"
    _base_attr = "model"

    def __init__(self, model, x, y, adj, val_idx, *, verbose: bool = True, epochs: int = 250,
                 frozen_logits: bool = False):
        super().__init__()
        self.w1 = nn.Parameter(torch.ones(1))
        self.w2 = nn.Parameter(torch.zeros(1))
        self.w3 = nn.Parameter(torch.zeros(1))
        self.num_classes = int(y.max().item()) + 1                       # ETS.py:15
        self._setup(model, x, y, adj, val_idx, verbose, epochs, frozen_logits)
        self.temp_model = TemperatureScaling(model, x, y, adj, val_idx, verbose=verbose, epochs=epochs,
                                             frozen_logits=frozen_logits)   # ETS.py:17: trained here
        self.to(self.device)

    def _params(self):
        return [self.temp_model.temperature, self.w1, self.w2, self.w3]

    def calib_train(self, patience=10):
        raise NotImplementedError("ETS trains its TS in the constructor and its weights in fit(masks)")

    def fit(self, masks):
        self.to(self.device)
        self.eval()
        with torch.no_grad():
            logits = self._logits(self.x, self._train_adj())             # ETS.py:39
        p0y, p1y = ets_label_probs(logits, self.y, self.temp_model.temperature, rows=masks[1])
        if p0y.numel() == 0:
            raise ValueError("ETS.fit needs at least one validation node")
        w = ensemble_weights(p0y.cpu().numpy(), p1y.cpu().numpy(), self.num_classes)
        self.w1.data = torch.tensor(w[0], device=self.device)            # ETS.py:45-47: 0-dim float64, as there
        self.w2.data = torch.tensor(w[1], device=self.device)
        self.w3.data = torch.tensor(w[2], device=self.device)
        return self


TS, VS, MS = TemperatureScaling, VectorScaling, MatrixScaling


def calibrate_with_temperature_scaling(base_model, x, y, adj, val_idx, **kwargs):
    """TS.py:86-100."""
    return TemperatureScaling(base_model, x, y, adj, val_idx, **kwargs)


def calibrate_with_vector_scaling(base_model, x, y, adj, val_idx, **kwargs):
    """VS.py:92-106."""
    return VectorScaling(base_model, x, y, adj, val_idx, **kwargs)


def calibrate_with_matrix_scaling(base_model, x, y, adj, val_idx, **kwargs):
    """MS.py:92-106."""
    return MatrixScaling(base_model, x, y, adj, val_idx, **kwargs)
