"""Fused WATS temperature head.

Reference ``calibration/WATS.py``: ``net = Linear(F,16) - ReLU - Linear(16,1)``
(:101-105); ``forward`` computes ``T = log(exp(net(H)) + 1.1)`` and
``log_softmax(logits / T)`` (:124-130), and ``calib_train`` backpropagates the
NLL through it every epoch (:145-151).  :func:`wats_head` is that whole
expression as two HIP kernels (``csrc/head.hip``): forward, and a backward
giving the logits gradient and the four parameter gradients.  Float64 sums in a
fixed order make the backward deterministic.

:func:`train_wats_head` is ``calib_train`` (:132-170) with one
``wg_wats_train_epoch`` launch per epoch (``csrc/watstrain.hip``): the head's
forward on the calibration rows only, the NLL, accuracy, all four parameter
gradients, torch's Adam step with L2 weight decay and the early-stopping state
stay in one device block, as ``scaling.train_scaling`` does for TS / VS / MS.
The master parameters and Adam moments are float64; the returned parameters are
their float32 rounding.

Non-finite values (``tests/test_head_precision.py``).  A row is computed from
its own row of ``H`` and ``logits`` alone, so a NaN in one row leaves every
other row of the output and of the logits gradient bitwise as it is without it.
The row itself becomes NaN in both (the ReLU hands a NaN on, as torch's does),
and ``g_W2`` and ``g_b2`` become NaN.  Where ``net(H) > 88.8``, ``exp`` is inf
in float32 and so is ``T``: that row of the output is finite and constant,
``-log(C)``, and its row of the logits gradient is 0, but ``d T / d net`` is
``inf / inf``, so the parameter gradients are NaN in the places where torch's
float32 expression has them NaN (``g_b2``, all of ``g_W2``, and the ``g_b1`` /
``g_W1`` rows of the hidden units active on that row).
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import torch

from . import _lib
from ._lib import check, ptr
from .laplacian import require_gpu, stream_handle


def _c(t):
    return t.detach().to(torch.float32).contiguous()


class _WATSHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, logits, W1, b1, W2, b2):
        dev = logits.device
        H, lg, W1c, b1c, W2c, b2c = (_c(t) for t in (H, logits, W1, b1, W2, b2))
        n, C = lg.shape
        F, hid = H.shape[1], W1c.shape[0]
        out = torch.empty(n, C, dtype=torch.float32, device=dev)
        t_save = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(_lib.load().wg_wats_head_forward(n, F, C, hid, ptr(H), ptr(lg), ptr(W1c), ptr(b1c), ptr(W2c),
                                                   ptr(b2c), ptr(out), ptr(t_save), stream_handle(dev)),
                  "wats_head_forward")
        ctx.save_for_backward(H, lg, W1c, b1c, W2c, b2c, out, t_save)
        return out

    @staticmethod
    def backward(ctx, g):
        H, lg, W1, b1, W2, b2, out, t_save = ctx.saved_tensors
        dev = lg.device
        n, C = lg.shape
        F, hid = H.shape[1], W1.shape[0]
        g = g.to(torch.float32).contiguous()
        need_logits = ctx.needs_input_grad[1]
        glog = torch.empty_like(lg) if need_logits else None
        gW1, gb1 = torch.empty_like(W1), torch.empty_like(b1)
        gW2, gb2 = torch.empty_like(W2), torch.empty_like(b2)
        lib = _lib.load()
        nbytes = ctypes.c_int64(0)
        check(lib.wg_wats_head_workspace(n, F, hid, ctypes.byref(nbytes)), "wats_head_workspace")
        ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib.wg_wats_head_backward(n, F, C, hid, ptr(H), ptr(lg), ptr(W1), ptr(b1), ptr(W2), ptr(b2),
                                            ptr(out), ptr(t_save), ptr(g), ptr(glog), ptr(gW1), ptr(gb1), ptr(gW2),
                                            ptr(gb2), ptr(ws), stream_handle(dev)), "wats_head_backward")
        return None, glog, gW1, gb1, gW2, gb2


def wats_head(H: torch.Tensor, logits: torch.Tensor, net: torch.nn.Sequential) -> torch.Tensor:
    """``log_softmax(logits / log(exp(net(H)) + 1.1))`` (WATS.py:124-130) with
    ``net = Sequential(Linear(F, hid), ReLU(), Linear(hid, 1))``."""
    l1, l2 = net[0], net[2]
    if H.dim() == 1:
        H = H.reshape(-1, 1)
    return _WATSHead.apply(H, logits, l1.weight, l1.bias, l2.weight, l2.bias)


def max_train_params() -> int:
    """The most parameters ``hid * F + 2 hid + 1`` the training kernel takes (``wg_wats_train_max_params``)."""
    return int(_lib.load().wg_wats_train_max_params())


class _HeadTrainingState:
    """The device state block of ``wg_wats_train_epoch`` for one run."""

    def __init__(self, F: int, hid: int, C: int, epochs: int, max_rows: int, patience: int, device, init,
                 lr: float, weight_decay: float):
        self.F, self.hid, self.C, self.epochs, self.max_rows = int(F), int(hid), int(C), int(epochs), int(max_rows)
        self.device = device
        lib = _lib.load()
        nbytes = ctypes.c_int64()
        check(lib.wg_wats_train_state_bytes(self.F, self.hid, self.epochs, self.max_rows, ctypes.byref(nbytes)),
              "wats_train_state_bytes")
        self.block = torch.empty(nbytes.value // 8, dtype=torch.float64, device=device)
        W1, b1, W2, b2 = (p.detach().to(device=device, dtype=torch.float32).contiguous() for p in init)
        if W1.shape != (self.hid, self.F) or b1.numel() != self.hid or W2.numel() != self.hid or b2.numel() != 1:
            raise ValueError(f"the head's parameters do not have the shapes of Linear({self.F}, {self.hid}) - ReLU - "
                             f"Linear({self.hid}, 1)")
        self._init = (W1, b1, W2, b2, int(patience), float(lr), float(weight_decay))
        self.reset()

    def reset(self):
        """Fill the block afresh from the initial parameters (on the current stream)."""
        W1, b1, W2, b2, patience, lr, weight_decay = self._init
        with torch.cuda.device(self.device):
            check(_lib.load().wg_wats_train_state_init(ptr(self.block), self.F, self.hid, self.C, self.epochs,
                                                       self.max_rows, patience, lr, weight_decay, ptr(W1), ptr(b1),
                                                       ptr(W2), ptr(b2), stream_handle(self.device)),
                  "wats_train_state_init")

    @property
    def n_params(self) -> int:
        return self.hid * self.F + 2 * self.hid + 1

    def epoch(self, H, logits, rows, y, n_workgroups: int = 0):
        n = logits.shape[0]
        n_rows = n if rows is None else rows.numel()
        with torch.cuda.device(self.device):
            check(_lib.load().wg_wats_train_epoch(ptr(self.block), self.F, self.hid, self.C, self.epochs, self.max_rows,
                                                  n, n_rows, ptr(H), ptr(logits), ptr(rows), ptr(y), int(n_workgroups),
                                                  stream_handle(self.device)), "wats_train_epoch")

    def read(self):
        """(W1, b1, W2, b2 as float32 device tensors, info as a float64 host array) -- one host sync."""
        W1 = torch.empty((self.hid, self.F), dtype=torch.float32, device=self.device)
        b1 = torch.empty(self.hid, dtype=torch.float32, device=self.device)
        W2 = torch.empty((1, self.hid), dtype=torch.float32, device=self.device)
        b2 = torch.empty(1, dtype=torch.float32, device=self.device)
        info = torch.empty(5 + 2 * self.epochs, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(_lib.load().wg_wats_train_state_read(ptr(self.block), self.F, self.hid, self.epochs, ptr(W1), ptr(b1),
                                                       ptr(W2), ptr(b2), ptr(info), stream_handle(self.device)),
                  "wats_train_state_read")
        return [W1, b1, W2, b2], info.cpu().numpy()

    def partials(self, n_rows: int) -> torch.Tensor:
        """The chunk partials of the last epoch that ran on ``n_rows`` rows, (chunks, 2 + P) float64: the chunk's sum
        of -out[r, y_r], its correct count, and its share of the nll SUM's gradients (gW1, gb1, gW2, gb2)."""
        chunks = -(-n_rows // int(_lib.load().wg_wats_train_chunk_rows()))
        at = 16 + 3 * self.n_params + 2 * self.epochs
        return self.block[at:at + chunks * (2 + self.n_params)].reshape(chunks, 2 + self.n_params)

    def stopped(self) -> bool:
        return bool(self.block[1].item() != 0)     # the stopped slot of the header


def train_wats_head(H: torch.Tensor, logits, y: torch.Tensor, rows, net: torch.nn.Sequential, *, epochs: int = 250,
                    patience: int = 10, lr: float = 0.01, weight_decay: float = 5e-4, n_workgroups: int = 0,
                    sync_every: int = 10):
    """``calib_train`` (WATS.py:132-170) on the device.  ``H`` (n, F) wavelet features; ``logits``: the (n, C) logits
    of every epoch, or a callable ``epoch -> (n, C) logits`` (then the host reads the stopped flag every ``sync_every``
    epochs and stops calling); ``y`` (n,) int64 labels; ``rows`` the calibration rows (None, a boolean mask or an
    index tensor); ``net = Sequential(Linear(F, hid), ReLU(), Linear(hid, 1))`` gives the initial parameters and is
    not written.  Returns a namespace: ``params`` (float32 tensors shaped as ``net``'s: W1, b1, W2, b2), ``loss`` /
    ``acc`` (per epoch run), ``epochs_run``, ``stop_epoch`` (the epoch early stopping fired in, else None),
    ``best_loss``, ``patience_left``, ``state`` (the device block)."""
    from .scaling import _row_list, max_classes
    first = logits(0) if callable(logits) else logits
    device = require_gpu(first.device if first.is_cuda else None)
    if first.dim() != 2:
        raise ValueError(f"logits must be (n, C), not {tuple(first.shape)}")
    n, C = first.shape
    if C > max_classes("ts"):
        raise NotImplementedError(f"C = {C} is above {max_classes('ts')} classes")
    if H.dim() == 1:
        H = H.reshape(-1, 1)
    if H.dim() != 2 or H.shape[0] != n:
        raise ValueError(f"H must be ({n}, F), not {tuple(H.shape)}")
    H = H.detach().to(device=device, dtype=torch.float32).contiguous()
    l1, l2 = net[0], net[2]
    hid, F = l1.weight.shape
    if F != H.shape[1] or tuple(l2.weight.shape) != (1, hid):
        raise ValueError(f"net is Linear({F}, {hid}) - Linear{tuple(l2.weight.shape)}, H has {H.shape[1]} columns")
    if hid > 64:
        raise NotImplementedError(f"{hid} hidden units are above the 64 lanes of a wave")
    if hid * F + 2 * hid + 1 > max_train_params():
        raise NotImplementedError(f"{hid * F + 2 * hid + 1} parameters are above {max_train_params()}")
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
    st = _HeadTrainingState(F, hid, C, epochs, n_rows, patience, device, [l1.weight, l1.bias, l2.weight, l2.bias],
                            lr, weight_decay)

    def prepared(z):
        if z.shape != (n, C):
            raise ValueError(f"the logits changed shape: {tuple(z.shape)} after {(n, C)}")
        return z.detach().to(device=device, dtype=torch.float32).contiguous()

    z = prepared(first)
    if callable(logits):
        for epoch in range(epochs):
            if epoch:
                z = prepared(logits(epoch))
            st.epoch(H, z, rows, y, n_workgroups)
            if sync_every and (epoch + 1) % sync_every == 0 and st.stopped():
                break
    else:
        for _ in range(epochs):         # a launch that finds the stopped flag set touches nothing
            st.epoch(H, z, rows, y, n_workgroups)
    params, info = st.read()
    run = int(info[1])
    return SimpleNamespace(params=params, loss=info[5:5 + run].copy(), acc=info[5 + epochs:5 + epochs + run].copy(),
                           epochs_run=run, stop_epoch=run - 1 if info[0] == 1 else None, best_loss=float(info[4]),
                           patience_left=int(info[3]), state=st.block)
