"""Float64 restatement, in numpy, of the WATS calibrator's training (reference calibration/WATS.py:101-105 net,
:124-130 forward, :132-170 calib_train): the head on the calibration rows, the loss, the four parameter gradients, the
correct count, torch's Adam with L2 weight decay (scaling_ref.adam_step) and the loop with its early stopping.  Helper
of tests/test_wats_train_host.py, tests/test_wats_train.py and tools/gen_golden_wats_train.py; not a test.

Parameters are a list in the order of the kernel's state: [W1 (hid, F), b1 (hid,), W2 (hid,), b2 (1,)] (torch keeps W2
as (1, hid); it is flattened here).  With H (n, F), z (n, C), labels y of the LISTED rows:

    pre = b1 + H W1^T,  r = relu(pre) (active iff pre > 0; a NaN goes on),  t = b2 + r W2,
    T = log(exp(t) + c), c = (double)1.1f,  v = z / T,  out = v - max v - log sum exp(v - max v),
    loss = -mean out[i, y_i].

Absolute sums (``*_abs``), what a bound of 1e-12 (about 4500 x 2^-53) is a fraction of.  The float64 evaluation of t
errs by a few 2^-53 of t_abs = |b2| + sum_j |W2_j| pre_abs_j with pre_abs_j = |b1_j| + sum_f |W1_jf H_f| over the
active units; T inherits it (|dT / dt| <= 1), so v = z / T errs by |v| t_abs / T relative to 2^-53, and exp(v - m) by
that times |v - m| <= 2 max |v|.  Hence per row amp = (1 + 2 max_c |v_c|) (1 + t_abs / T), and

    loss_abs   = mean (|v_y| + |m| + |lse|) (1 + t_abs / T)
    dt_abs     = amp (sum_c (p_c + [c = y]) |z_c|) / T^2 * dT/dt          (the absolute terms of d loss_i / d t)
    gb2_abs    = mean dt_abs,  gW2_abs_j = mean dt_abs pre_abs_j [active],
    gb1_abs_j  = mean dt_abs |W2_j| [active],  gW1_abs_jf = mean dt_abs |W2_j| |H_f| [active].

MUTANTS are WRONG on purpose, one per way the arithmetic could be misread; the host test holds each of them outside
the bounds:
  decoupled_wd      AdamW's decoupled decay instead of torch Adam's L2 term
  no_bias_decay     the weight decay leaves b1 and b2 out (torch decays every tensor of the group)
  multiply_T        z * T instead of z / T (TS.py multiplies, WATS.py:129 divides)
  relu_grad_at_zero a gradient of 1 at pre == 0 (torch's threshold backward gives 0)
  best_le           loss <= best_loss resets the patience (WATS.py:162 is <)
  mean_n_total      the mean over all n rows instead of the listed ones
  shift_double      c = 1.1 as a double instead of the float32 tensor's value
"""
import json
import os

import numpy as np

import scaling_ref as SR

F64 = np.float64
EPS32 = SR.EPS32
SHIFT = float(np.float32(1.1))
LR, WD = SR.LR, SR.WD
MUTANTS = ("decoupled_wd", "no_bias_decay", "multiply_T", "relu_grad_at_zero", "best_le", "mean_n_total",
           "shift_double")
f64 = SR.f64


def as_params(params):
    """[W1 (hid, F), b1 (hid,), W2 (hid,), b2 (1,)] as float64 arrays"""
    W1, b1, W2, b2 = (f64(p) for p in params)
    hid = b1.size
    return [W1.reshape(hid, -1), b1.reshape(hid), W2.reshape(hid), b2.reshape(1)]


def head(H, params, mutant=None):
    """dict(pre, pre_abs, act, r, t, t_abs, T, dTdt) of every row of H"""
    W1, b1, W2, b2 = as_params(params)
    H = f64(H)
    c = 1.1 if mutant == "shift_double" else SHIFT
    with np.errstate(invalid="ignore", over="ignore"):
        pre = H @ W1.T + b1
        pre_abs = np.abs(H) @ np.abs(W1).T + np.abs(b1)
        act = pre > 0
        r = np.where(act, pre, np.where(np.isnan(pre), pre, 0.0))
        t = b2[0] + (r * W2).sum(axis=1)
        t_abs = np.abs(b2[0]) + (np.where(act, pre_abs, 0.0) * np.abs(W2)).sum(axis=1)
        e = np.exp(t)
        T = np.log(e + c)
        dTdt = e / (e + c)
    return dict(pre=pre, pre_abs=pre_abs, act=act, r=r, t=t, t_abs=t_abs, T=T, dTdt=dTdt)


def forward(H, z, params, mutant=None):
    """log_softmax(z / T) (n, C), float64"""
    h = head(H, params, mutant)
    z = f64(z)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        v = z * h["T"][:, None] if mutant == "multiply_T" else z / h["T"][:, None]
        m, e, S = SR._softmax_parts(v)
        return v - m - np.log(S)


def epoch(H, z, y, params, mutant=None, n_total=None):
    """One epoch's quantities on the LISTED rows (H, z, y already indexed): dict(loss, correct, grads [gW1, gb1, gW2,
    gb2] -- what the optimiser receives before the weight decay --, loss_abs, grads_abs, pre, pre_abs)."""
    H, z, y = f64(H), f64(z), np.asarray(y, dtype=np.int64)
    W1, b1, W2, b2 = as_params(params)
    n, C = z.shape
    den = float(n_total if mutant == "mean_n_total" else n)
    h = head(H, params, mutant)
    T, ar = h["T"][:, None], np.arange(n)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        v = z * T if mutant == "multiply_T" else z / T
        m, e, S = SR._softmax_parts(v)
        lse = np.log(S)
        out = v - m - lse
        cond = 1.0 + h["t_abs"] / h["T"]
        loss = -out[ar, y].sum() / den
        loss_abs = ((np.abs(v[ar, y]) + np.abs(m[:, 0]) + np.abs(lse[:, 0])) * cond).sum() / den
        p = e / S
        hot = np.zeros_like(z)
        hot[ar, y] = 1.0
        dts = ((p - hot) * z).sum(axis=1)                       # d (n loss_i) / d v . z
        dts_abs = ((p + hot) * np.abs(z)).sum(axis=1)
        amp = (1.0 + 2.0 * np.abs(v).max(axis=1)) * cond
        if mutant == "multiply_T":
            dt, dt_abs = dts * h["dTdt"], dts_abs * h["dTdt"] * amp
        else:
            dt, dt_abs = -dts / h["T"] ** 2 * h["dTdt"], dts_abs / h["T"] ** 2 * h["dTdt"] * amp
        act = h["pre"] >= 0 if mutant == "relu_grad_at_zero" else h["act"]
        dz = np.where(act, dt[:, None] * W2, 0.0)
        dz_abs = np.where(act, dt_abs[:, None] * np.abs(W2), 0.0)
        grads = [dz.T @ H / den, dz.sum(axis=0) / den, (dt[:, None] * h["r"]).sum(axis=0) / den,
                 np.array([dt.sum() / den])]
        grads_abs = [dz_abs.T @ np.abs(H) / den, dz_abs.sum(axis=0) / den,
                     (dt_abs[:, None] * np.where(h["act"] | np.isnan(h["pre"]), h["pre_abs"], 0.0)).sum(axis=0) / den,
                     np.array([dt_abs.sum() / den])]
    return dict(loss=loss, correct=int((SR.argmax_first(out) == y).sum()), grads=grads, loss_abs=loss_abs,
                grads_abs=grads_abs, pre=h["pre"], pre_abs=h["pre_abs"])


def kink_margin(q):
    """min |pre_j| / pre_abs_j over the listed rows and units: below 1e-9 a rounding could flip a ReLU"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmin(np.abs(q["pre"]) / q["pre_abs"]))


def step(params, grads, m, v, k, lr=LR, wd=WD, mutant=None):
    """torch's Adam step k (1-based) on the four tensors, in place on the lists"""
    for i in range(4):
        w = 0.0 if (mutant == "no_bias_decay" and i in (1, 3)) else wd
        params[i], m[i], v[i] = SR.adam_step(params[i], grads[i], m[i], v[i], k, lr=lr, wd=w, mutant=mutant)


def train(H, logits, y, rows, init, epochs=250, patience=10, lr=LR, wd=WD, mutant=None):
    """calib_train (WATS.py:132-170): logits is one (n, C) array or a callable epoch -> array; rows a boolean mask or
    an index array; init the head's parameters.  Returns dict(params, loss [epochs run], acc, epochs_run, stop_epoch
    (None: ran out of epochs), best_loss, patience_left) -- scaling_ref.train's."""
    y = np.asarray(y, dtype=np.int64)
    rows = np.asarray(rows)
    idx = np.nonzero(rows)[0] if rows.dtype == bool else rows.astype(np.int64)
    H = f64(H).reshape(len(y), -1)
    first = logits(0) if callable(logits) else logits
    params = [p.copy() for p in as_params(init)]
    m = [np.zeros_like(p) for p in params]
    v = [np.zeros_like(p) for p in params]
    best, left, losses, accs, stop = np.inf, patience, [], [], None
    for e in range(epochs):
        z = first if (e == 0 or not callable(logits)) else logits(e)
        q = epoch(H[idx], np.asarray(z)[idx], y[idx], params, mutant=mutant, n_total=len(y))
        step(params, q["grads"], m, v, e + 1, lr, wd, mutant)
        losses.append(q["loss"])
        accs.append(q["correct"] / len(idx))
        if (q["loss"] <= best) if mutant == "best_le" else (q["loss"] < best):
            best, left = q["loss"], patience
        else:
            left -= 1
        if left <= 0:
            stop = e
            break
    return dict(params=params, loss=np.array(losses), acc=np.array(accs), epochs_run=len(losses), stop_epoch=stop,
                best_loss=best, patience_left=left)


def stop_gaps(losses, patience=10):
    """min |loss_e - best_loss| over the comparisons WATS.py:162 makes (the first, against inf, left out), the stop"""
    best, left, gaps, stop = np.inf, patience, [], -1
    for e, v in enumerate(losses):
        if np.isfinite(best):
            gaps.append(abs(v - best))
        if v < best:
            best, left = v, patience
        else:
            left -= 1
        if left <= 0:
            stop = e
            break
    return (min(gaps) if gaps else np.inf), stop


def dist(a, b):
    return float(np.max(np.abs(np.asarray(a, F64) - np.asarray(b, F64))))


# ------------------------------------------------------------------------------------------------- the fixtures
CASES = ("stop120", "full96")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wats_train")
NET_KEYS = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias")


def load_manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def load_case(name):
    """(arrays, the case's manifest entry) of tests/golden/wats_train/<name>.npz"""
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as d:
        arrays = {k: d[k] for k in d.files}
    return arrays, load_manifest()["cases"][name]


def case_base(d):
    """the base model's arrays (gc1.weight, ...)"""
    return {k[len("base__"):]: v for k, v in d.items() if k.startswith("base__")}


def case_init(d):
    return as_params([d["init__" + k] for k in NET_KEYS])


def case_trained(d):
    return as_params([d["p__" + k] for k in NET_KEYS])


def case_rows(d):
    val = d["val"]
    return np.nonzero(val)[0] if val.dtype == bool else val.astype(np.int64)
