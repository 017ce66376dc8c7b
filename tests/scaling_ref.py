"""Float64 restatement, in numpy, of the reference's four node-wise calibrators (calibration/TS.py, VS.py, MS.py,
ETS.py): the forwards, their gradients, one training epoch, torch's Adam with L2 weight decay, the training loop with
its early stopping, and ETS's objective and fit.  Helpers of tests/test_scaling_host.py, tests/test_scaling.py and
tools/gen_golden_scaling.py; not a test.

Parameters are lists in the order of the kernels' state: TS [temperature (1,)], VS [temperature (C,)], MS [W (C, C),
b (C,)], ETS [tau (1,), w1, w2, w3].  Every function also returns, where a bound needs it, the same expression with
each added term replaced by its absolute value (``*_abs``): the float64 evaluation errs by a few 2^-53 of that sum,
which the tests allow as 1e-12 of it.

MUTANTS are WRONG on purpose, one per way the arithmetic could be misread; the host test holds each of them outside the
fixtures or the bounds:
  ts_divide            TS divides by s instead of multiplying (TS.py:43 multiplies)
  ets_fit_softplus     ETS.fit divides by log(exp(tau) + 1.1) instead of the raw tau (ETS.py:43, :57)
  ets_forward_multiply ETS.forward multiplies by temp instead of dividing (ETS.py:25)
  ms_identity_init     W starts as the identity (MS.py:28 says ones)
  ms_no_shift          z' = z (MS.py:45-46 subtracts the last column)
  decoupled_wd         AdamW's decoupled decay instead of torch Adam's L2 term
  sign0_is_1           sign(0) = 1 in the L1 term's gradient
  f32_loss             the loss summed in one sequential float32 accumulator
"""
import numpy as np

F64 = np.float64
EPS32 = 2.0 ** -24
LR, WD, BETA1, BETA2, ADAM_EPS, MS_LAMBDA = 0.01, 5e-4, 0.9, 0.999, 1e-8, 1.0
MUTANTS = ("ts_divide", "ets_fit_softplus", "ets_forward_multiply", "ms_identity_init", "ms_no_shift", "decoupled_wd",
           "sign0_is_1", "f32_loss")


def f64(a):
    return np.asarray(a, dtype=F64)


def softplus_scale(t):
    """s = log(exp(t) + 1.1) and ds / dt"""
    e = np.exp(f64(t))
    return np.log(e + 1.1), e / (e + 1.1)


def _softmax_parts(v):
    """m, e = exp(v - m), S as the kernels form them (a NaN stays in its row)"""
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.fmax.reduce(v, axis=1, keepdims=True)
        e = np.exp(v - m)
        return m, e, e.sum(axis=1, keepdims=True)


def initial_params(mode, C, mutant=None):
    if mode == "ts":
        return [np.ones(1)]
    if mode == "vs":
        return [np.ones(C)]
    if mode == "ms":
        return [np.eye(C) if mutant == "ms_identity_init" else np.ones((C, C)), np.ones(C)]
    raise ValueError(mode)


def forward(mode, z, params, normalize=False, mutant=None, with_abs=False):
    """out (n, C) float64; with_abs: also the per-element sum of the absolute terms that made it"""
    z = f64(z)
    p = [f64(q) for q in params]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mode in ("ts", "vs"):
            s, _ = softplus_scale(p[0])
            v = z / s if mutant == "ts_divide" else z * s
            m, e, S = _softmax_parts(v)
            out = v - m - np.log(S)
            ab = np.abs(v) + np.abs(m) + np.abs(np.log(S))
        elif mode == "ms":
            zp = z if mutant == "ms_no_shift" else z - z[:, -1:]
            o = zp @ p[0] + p[1]
            ab = np.abs(zp) @ np.abs(p[0]) + np.abs(p[1])
            if normalize:
                m, e, S = _softmax_parts(o)
                o = o - m - np.log(S)
                ab = ab + np.abs(m) + np.abs(np.log(S))
            out = o
        elif mode == "ets":
            temp, _ = softplus_scale(p[0])
            a = z * temp if mutant == "ets_forward_multiply" else z / temp
            _, e0, S0 = _softmax_parts(a)
            _, e1, S1 = _softmax_parts(z)
            w1, w2, w3 = (float(np.ravel(q)[0]) for q in p[1:])
            pr = w1 * (e0 / S0) + w2 * (e1 / S1) + w3 / z.shape[1]
            out = np.log(pr)
            # log p errs by the relative error of p, which exp(a - m) carries in units of |a - m|
            ab = 1.0 + np.abs(out) + np.abs(a).max(axis=1, keepdims=True) * 2 + np.abs(z).max(axis=1, keepdims=True) * 2
            ab = np.broadcast_to(ab, out.shape)
        else:
            raise ValueError(mode)
    return (out, ab) if with_abs else out


def backward(mode, z, params, g, normalize=False):
    """(g_logits, [parameter gradients], abs) from g = d loss / d out, all float64.  abs = (per-element absolute sum of
    g_logits' terms, [the same per parameter])."""
    z, g = f64(z), f64(g)
    p = [f64(q) for q in params]
    n, C = z.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mode in ("ts", "vs"):
            s, ds = softplus_scale(p[0])
            v = z * s
            _, e, S = _softmax_parts(v)
            sm = e / S
            gs = g.sum(axis=1, keepdims=True)
            gv = g - sm * gs
            gv_abs = np.abs(g) + sm * np.abs(g).sum(axis=1, keepdims=True)
            gz, gz_abs = gv * s, gv_abs * np.abs(s)
            gt, gt_abs = (gv * z * ds).sum(axis=0), (gv_abs * np.abs(z) * ds).sum(axis=0)
            if mode == "ts":
                gt, gt_abs = gt.sum(keepdims=True), gt_abs.sum(keepdims=True)
            return gz, [gt], (gz_abs, [gt_abs])
        if mode == "ms":
            W, b = p
            zp = z - z[:, -1:]
            go, go_abs = g, np.abs(g)
            if normalize:
                _, e, S = _softmax_parts(zp @ W + b)
                sm = e / S
                go = g - sm * g.sum(axis=1, keepdims=True)
                go_abs = np.abs(g) + sm * np.abs(g).sum(axis=1, keepdims=True)
            gzp, gzp_abs = go @ W.T, go_abs @ np.abs(W).T
            gz, gz_abs = gzp.copy(), gzp_abs.copy()
            gz[:, -1] -= gzp.sum(axis=1)
            gz_abs[:, -1] += gzp_abs.sum(axis=1)
            return gz, [zp.T @ go, go.sum(axis=0)], (gz_abs, [np.abs(zp).T @ go_abs, go_abs.sum(axis=0)])
        if mode == "ets":
            temp, dtemp = softplus_scale(p[0])
            temp, dtemp = float(temp[0]), float(dtemp[0])
            w1, w2, w3 = (float(np.ravel(q)[0]) for q in p[1:])
            a = z / temp
            _, e0, S0 = _softmax_parts(a)
            _, e1, S1 = _softmax_parts(z)
            p0, p1 = e0 / S0, e1 / S1
            pr = w1 * p0 + w2 * p1 + w3 / C
            gp = g / pr
            d0, d1 = (gp * p0).sum(axis=1, keepdims=True), (gp * p1).sum(axis=1, keepdims=True)
            ga = w1 * p0 * (gp - d0)
            gz = ga / temp + w2 * p1 * (gp - d1)
            agp = np.abs(gp)
            a0, a1 = (agp * p0).sum(axis=1, keepdims=True), (agp * p1).sum(axis=1, keepdims=True)
            ga_abs = abs(w1) * p0 * (agp + a0)
            gz_abs = (ga_abs / temp + abs(w2) * p1 * (agp + a1)) * (1.0 + np.abs(a).max(axis=1, keepdims=True)
                                                                    + np.abs(z).max(axis=1, keepdims=True))
            gtau = (-(ga * z).sum() / temp ** 2) * dtemp
            amp = 1.0 + np.abs(a).max() + np.abs(z).max()
            gtau_abs = ((ga_abs * np.abs(z)).sum() / temp ** 2) * dtemp * amp
            grads = [np.array([gtau]), np.array([d0.sum()]), np.array([d1.sum()]), np.array([gp.sum() / C])]
            gabs = [np.array([gtau_abs]), np.array([a0.sum() * amp]), np.array([a1.sum() * amp]),
                    np.array([agp.sum() / C * amp])]
            return gz, grads, (gz_abs, gabs)
    raise ValueError(mode)


def argmax_first(out):
    """the first index of each row's maximum, a NaN ranking above every number (np.argmax, torch.max)"""
    return np.argmax(out, axis=1)


def epoch(mode, z_val, y_val, params, normalize=False, Lambda=MS_LAMBDA, mutant=None):
    """One epoch's quantities on the validation rows: dict(loss, grads, correct, loss_abs, grads_abs) -- the loss and
    the gradients the optimiser receives, L1 term and 1 / n included, before the weight decay."""
    z_val, y_val = f64(z_val), np.asarray(y_val, dtype=np.int64)
    n, C = z_val.shape
    out = forward(mode, z_val, params, normalize, mutant=mutant)
    picked = out[np.arange(n), y_val]
    if mutant == "f32_loss":
        acc = np.float32(0.0)
        for v in picked.astype(np.float32):
            acc = np.float32(acc - v)
        loss = float(acc) / n
    else:
        loss = -picked.sum() / n
    loss_abs = np.abs(picked).sum() / n
    g = np.zeros_like(z_val)
    g[np.arange(n), y_val] = -1.0 / n
    if mutant in ("ts_divide", "ms_no_shift"):
        grads = _numeric_param_grads(mode, z_val, y_val, params, normalize, mutant)
        grads_abs = [np.abs(q) for q in grads]
    else:
        _, grads, (_, grads_abs) = backward(mode, z_val, params, g, normalize)
    grads = [q.reshape(np.shape(p)) for q, p in zip(grads, params)]
    grads_abs = [q.reshape(np.shape(p)) for q, p in zip(grads_abs, params)]
    if mode == "ms":
        W = f64(params[0])
        d = W - np.eye(C)
        loss = loss + Lambda * np.abs(d).sum()
        loss_abs = loss_abs + Lambda * np.abs(d).sum()
        sg = np.sign(d)
        if mutant == "sign0_is_1":
            sg = np.where(d == 0, 1.0, sg)
        grads[0] = grads[0] + Lambda * sg
        grads_abs[0] = grads_abs[0] + Lambda * np.abs(sg)
    return dict(loss=loss, grads=grads, correct=int((argmax_first(out) == y_val).sum()), loss_abs=loss_abs,
                grads_abs=grads_abs)


def _numeric_param_grads(mode, z, y, params, normalize, mutant, h=1e-6):
    """central differences of the mutant's nll (mutants only: their forwards have no analytic backward here)"""
    def nll(ps):
        out = forward(mode, z, ps, normalize, mutant=mutant)
        return -out[np.arange(z.shape[0]), y].sum() / z.shape[0]
    grads = []
    for k, p in enumerate(params):
        p = f64(p)
        g = np.zeros_like(p)
        for idx in np.ndindex(p.shape):
            hi, lo = [f64(q).copy() for q in params], [f64(q).copy() for q in params]
            hi[k][idx] += h
            lo[k][idx] -= h
            g[idx] = (nll(hi) - nll(lo)) / (2 * h)
        grads.append(g)
    return grads


def adam_step(theta, g, m, v, step, lr=LR, wd=WD, mutant=None):
    """torch.optim.Adam's single-tensor step (weight_decay as an L2 term in the gradient), in place on copies;
    step is the 1-based count of this update"""
    theta, g, m, v = f64(theta).copy(), f64(g), f64(m), f64(v)
    if mutant == "decoupled_wd":
        theta = theta * (1.0 - lr * wd)
    else:
        g = g + wd * theta
    m = BETA1 * m + (1.0 - BETA1) * g
    v = BETA2 * v + (1.0 - BETA2) * g * g
    bc1, bc2 = 1.0 - BETA1 ** step, 1.0 - BETA2 ** step
    theta = theta - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + ADAM_EPS))
    return theta, m, v


def train(mode, logits, y, rows, epochs=250, patience=10, normalize=False, init=None, mutant=None):
    """calib_train (TS.py:45-83): logits is one (n, C) array or a callable epoch -> array; rows a boolean mask or an
    index array.  Returns dict(params, loss [epochs run], acc, epochs_run, stop_epoch (None: ran out of epochs),
    best_loss, patience_left)."""
    y = np.asarray(y, dtype=np.int64)
    rows = np.asarray(rows)
    idx = np.nonzero(rows)[0] if rows.dtype == bool else rows.astype(np.int64)
    first = logits(0) if callable(logits) else logits
    C = first.shape[1]
    params = [f64(q).copy() for q in (init if init is not None else initial_params(mode, C, mutant))]
    m = [np.zeros_like(q) for q in params]
    v = [np.zeros_like(q) for q in params]
    best, left, losses, accs, stop = np.inf, patience, [], [], None
    for e in range(epochs):
        z = first if (e == 0 or not callable(logits)) else logits(e)
        q = epoch(mode, np.asarray(z)[idx], y[idx], params, normalize, mutant=mutant)
        for k in range(len(params)):
            params[k], m[k], v[k] = adam_step(params[k], q["grads"][k], m[k], v[k], e + 1, mutant=mutant)
        losses.append(q["loss"])
        accs.append(q["correct"] / len(idx))
        if q["loss"] < best:
            best, left = q["loss"], patience
        else:
            left -= 1
        if left <= 0:
            stop = e
            break
    return dict(params=params, loss=np.array(losses), acc=np.array(accs), epochs_run=len(losses), stop_epoch=stop,
                best_loss=best, patience_left=left)


def ets_label_probs(z_val, y_val, tau, mutant=None):
    """softmax(z / t)[i, y_i] and softmax(z)[i, y_i] with the RAW tau as the divisor (ETS.py:43, :57)"""
    z_val, y_val = f64(z_val), np.asarray(y_val, dtype=np.int64)
    t = float(np.ravel(f64(tau))[0])
    if mutant == "ets_fit_softplus":
        t = float(np.log(np.exp(t) + 1.1))
    _, e0, S0 = _softmax_parts(z_val / t)
    _, e1, S1 = _softmax_parts(z_val)
    r = np.arange(z_val.shape[0])
    return (e0 / S0)[r, y_val], (e1 / S1)[r, y_val]


def ets_objective(w, p0y, p1y, C):
    return -np.sum(np.log(w[0] * p0y + w[1] * p1y + w[2] / C)) / p0y.shape[0]


def ets_fit(p0y, p1y, C):
    """ETS.py:62-67: SLSQP from (1, 0, 0), bounds [0, 1]^3, sum w = 1, tol 1e-12, finite differences"""
    import scipy.optimize
    res = scipy.optimize.minimize(ets_objective, (1.0, 0.0, 0.0), args=(p0y, p1y, C), method="SLSQP",
                                  constraints={"type": "eq", "fun": lambda x: np.sum(x) - 1},
                                  bounds=((0.0, 1.0),) * 3, tol=1e-12, options={"disp": False})
    return res.x


def one_rounding_ok(got, truth, absum, what=""):
    """got (float32) is within one float32 rounding of truth: 0.5 ulp (2^-24 |truth|, or half the smallest
    subnormal) plus the float64 evaluation's 1e-12 of the absolute sum.  Non-finite entries must match in kind."""
    got, truth, absum = f64(got), f64(truth), f64(absum)
    assert got.shape == truth.shape, f"{what}: shape {got.shape} vs {truth.shape}"
    fin = np.isfinite(truth) & (np.abs(truth) < 3.4028234e38)
    assert np.array_equal(np.isnan(got), np.isnan(truth)), f"{what}: NaNs differ"
    inf = np.isinf(truth)
    assert np.array_equal(got[inf], truth[inf]), f"{what}: infinities differ"
    err = np.abs(got[fin] - truth[fin])
    bound = EPS32 * np.abs(truth[fin]) + 2.0 ** -150 + 1e-12 * np.where(np.isfinite(absum[fin]), absum[fin], 0.0)
    worst = float((err / bound).max()) if err.size else 0.0
    assert worst <= 1.0, f"{what}: {worst:.3f} of the one-rounding bound"
    return worst


# ------------------------------------------------------------------ the base model and torch float64 restatements
def base_logits(P, x, adj):
    """The two-layer base model (src/gnn/model.py:40-53) in eval mode, float64: P maps gc1.weight, gc1.bias,
    gc2.weight, gc2.bias to arrays."""
    x, adj = f64(x), f64(adj)
    deg = adj.sum(axis=1, keepdims=True)
    deg[deg == 0] = 1
    an = adj / deg
    h = np.maximum((an @ x) @ f64(P["gc1.weight"]).T + f64(P["gc1.bias"]), 0.0)
    return (an @ h) @ f64(P["gc2.weight"]).T + f64(P["gc2.bias"])


def torch_forward(mode, z, params, normalize=False):
    """The same forwards in torch ops (float64 tensors in, autograd through them): the dense-autograd yardstick of
    the analytic gradients above."""
    import torch
    if mode in ("ts", "vs"):
        return torch.log_softmax(z * torch.log(torch.exp(params[0]) + 1.1), dim=1)
    if mode == "ms":
        o = (z - z[:, -1:]) @ params[0] + params[1]
        return torch.log_softmax(o, dim=1) if normalize else o
    if mode == "ets":
        temp = torch.log(torch.exp(params[0]) + 1.1)
        p = params[1] * torch.softmax(z / temp, dim=1) + params[2] * torch.softmax(z, dim=1) \
            + params[3] / z.shape[1]
        return torch.log(p)
    raise ValueError(mode)


def torch_base_logits(P, x, adj):
    import torch
    deg = adj.sum(dim=1, keepdim=True)
    deg = torch.where(deg == 0, torch.ones_like(deg), deg)
    an = adj / deg
    h = torch.relu((an @ x) @ P["gc1.weight"].T + P["gc1.bias"])
    return (an @ h) @ P["gc2.weight"].T + P["gc2.bias"]


def adjacency_gradient(mode, P, params, x, adj, weight, rows, cols, normalize=False):
    """d sum(weight * out) / d adj at (rows, cols) through a dense float64 leaf"""
    import torch
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=F64))   # noqa: E731
    a = t(adj).requires_grad_(True)
    out = torch_forward(mode, torch_base_logits({k: t(v) for k, v in P.items()}, t(x), a), [t(q) for q in params],
                        normalize)
    (out * t(weight)).sum().backward()
    return a.grad[torch.as_tensor(np.asarray(rows, np.int64)), torch.as_tensor(np.asarray(cols, np.int64))].numpy()


# ------------------------------------------------------------------------------------------------- the fixtures
CASES = ("plain120", "wide96")
CALIBRATORS = ("ts", "vs", "ms", "ets")


def load_case(name):
    """(arrays, the case's manifest entry, the file's manifest entry) of tests/golden/scaling/<name>.npz"""
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scaling")
    with np.load(os.path.join(here, name + ".npz"), allow_pickle=False) as d:
        arrays = {k: d[k] for k in d.files}
    with open(os.path.join(here, "manifest.json")) as f:
        manifest = json.load(f)
    return arrays, manifest["cases"][name], manifest["files"][name + ".npz"]


def load_manifest():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scaling", "manifest.json")) as f:
        return json.load(f)


def case_base(d, c="ts"):
    """the base model's arrays (gc1.weight, ...) as stored with calibrator c"""
    pre = f"p__{c}__" + ("base_model." if c in ("ts", "vs") else "model.")
    return {k[len(pre):]: v for k, v in d.items() if k.startswith(pre)}


def case_params(d, c):
    """the reference's trained parameters of calibrator c in state order"""
    if c in ("ts", "vs"):
        return [d[f"p__{c}__temperature"]]
    if c == "ms":
        return [d["p__ms__W"], d["p__ms__b"]]
    return [d["p__ets__temp_model.temperature"], d["p__ets__w1"], d["p__ets__w2"], d["p__ets__w3"]]


def case_rows(d):
    val = d["val"]
    return np.nonzero(val)[0] if val.dtype == bool else val.astype(np.int64)
