"""The integrated-gradient scores of calib_attack/calib_iga.py in closed form (csrc/iga.hip, wats_hip/attack.py
Calib_IGA), numpy only but for the criterion's gradient.  Helpers of tests/test_iga_host.py, tests/test_iga.py and
tools/gen_golden_iga.py; not a test.

  path_points       wg_iga_path_logits: the 2 (steps + 1) path points of row t (remove path first, k ascending) from
                    the gathered neighbour sums and the column sums, in any float format; `absolute` gives the same
                    expression with every term's absolute value (the unit of the one-rounding bound)
  head_grad         d (sum of the rows' criteria) / d logits by torch autograd, each row with its own argmax
  coefficients      (U, V, c) per path from the state and g_logits
  scores            s_j = +-(U h_j + V z_j + c), s_t = -10
  importance        all of the above on a dense adjacency and a state dict: the closed form
  dense_importance  the reference's loop restated on a dense leaf with torch autograd: one backward per path point
                    (the reference repeats the same path for every j and reads one entry of the same gradient)
  attack_loop       calib_iga.py:89-137 on a given importance vector
  MUTANTS           WRONG on purpose: "orig_label" (the label of the original output at every path point),
                    "row_col" (the gradient's row plus its column), "no_V", "no_c", "deg0" (a row sum of 0 left at 0:
                    the division gives NaN, which the mutant reads as 0), "add_for_existing" (the add path's sums
                    for the existing entries)
"""
import numpy as np
import torch
import torch.nn.functional as F

import attack_ref as R

EPS = R.EPS
LD = np.longdouble
MUTANTS = ("orig_label", "row_col", "no_V", "no_c", "deg0", "add_for_existing")


def lambdas(steps):
    """(path, lambda) of the P path points: path 0 = remove, 1 = add"""
    return [(path, k / steps) for path in (0, 1) for k in range(steps + 1)]


def path_points(row_cols, n, t, steps, z, h, zsum, hsum, b1, W2, b2, dt=np.float64, absolute=False):
    """dict(logits (P, C), p (P, Hd), q (P, Hd), deg [P] (the row sum as summed: 0 for a zero row), w_t [P])"""
    ab = np.abs if absolute else (lambda v: v)
    cols = np.asarray(row_cols, np.int64)
    z, h = np.asarray(z, np.float32), np.asarray(h, np.float32)
    Hd = z.shape[1]
    sz, sh = np.zeros(Hd, dt), np.zeros(Hd, dt)
    for j in cols:                                           # ascending, sequential
        sz = sz + ab(z[j]).astype(dt)
        sh = sh + ab(h[j]).astype(dt)
    a_t = dt(1 if t in cols else 0)
    zs, hs = ab(np.asarray(zsum, np.float64)).astype(dt), ab(np.asarray(hsum, np.float64)).astype(dt)
    ht, b1d = ab(h[t]).astype(dt), ab(np.asarray(b1, np.float32)).astype(dt)
    W2d, b2d = ab(np.asarray(W2, np.float32)).astype(dt), ab(np.asarray(b2, np.float32)).astype(dt)
    out = dict(logits=[], p=[], q=[], deg=[], w_t=[])
    for path, lam in lambdas(steps):
        lam = dt(lam)
        if path == 0:
            deg, wt = lam * dt(len(cols)), lam * a_t
            pz, qh = lam * sz, lam * sh
        else:
            deg, wt = (dt(1) - lam) * dt(n) + lam * dt(len(cols)), dt(1) - lam * (dt(1) - a_t)
            pz, qh = (dt(1) - lam) * zs + lam * sz, (dt(1) - lam) * hs + lam * sh
        d = deg if deg != 0 else dt(1)
        p = pz / d
        hp = p + b1d
        if not absolute:
            hp = np.maximum(hp, dt(0))
            q = (qh - wt * ht + wt * hp) / d
        else:
            q = (qh + wt * ht + wt * hp) / d
        logit = np.zeros(W2d.shape[0], dt)
        for f in range(Hd):                                  # columns ascending
            logit = logit + W2d[:, f] * q[f]
        out["logits"].append(logit + b2d)
        out["p"].append(p), out["q"].append(q), out["deg"].append(deg), out["w_t"].append(wt)
    return {k: np.asarray(v, dt) for k, v in out.items()}


def path_logits_ref(row_cols, n, t, steps, z, h, zsum, hsum, b1, W2, b2):
    """(truth float64 (P, C) from np.longdouble, unit (P, C)): the unit is 2^-24 of the row's absolute sum plus the
    float64 chain's (2 Hd + 2) 2^-52 of it"""
    args = (row_cols, n, t, steps, z, h, zsum, hsum, b1, W2, b2)
    truth = path_points(*args, dt=LD)["logits"].astype(np.float64)
    absolute = path_points(*args, dt=LD, absolute=True)["logits"].astype(np.float64)
    Hd = np.asarray(z).shape[1]
    return truth, (EPS + (2 * Hd + 2) * 2.0 ** -52) * absolute


def rows_criterion(out, labels, strategy):
    """the sum over the rows of overconfidence_objective / underconfidence_objective (calib_attack_loss.py:158-208),
    each applied to one row (a mean of one value)"""
    probs = F.softmax(out, dim=1)
    own = probs[torch.arange(len(labels)), labels]
    if strategy == "over":
        return -(1 - own).sum()
    keep = torch.ones_like(probs)
    keep[torch.arange(len(labels)), labels] = 0
    others, _ = torch.max(probs * keep, dim=1)
    return -(own - others).sum()


def head_grad(logits, strategy, temp=None, labels=None, dtype=torch.float64):
    """g_logits (P, C): the gradient of the summed criterion at the path points' logits; temp: the WATS temperature of
    the target (out = log_softmax(logits / temp)); labels: given labels in place of each row's argmax (a mutant)"""
    x = torch.as_tensor(np.asarray(logits, np.float64)).to(dtype).requires_grad_(True)
    out = x if temp is None else F.log_softmax(x / float(temp), dim=1)
    lab = out.argmax(dim=1) if labels is None else torch.as_tensor(labels)
    g = torch.autograd.grad(rows_criterion(out, lab, strategy), x)[0]
    return g.numpy().astype(np.float64)


def coefficients(state, g_logits, b1, W2, steps, mutant=None, absolute=False):
    """(2, 2 Hd + 1) float64: U, V, c of the remove path and of the add path; `absolute`: the same sums of the terms'
    absolute values (the scale their float64 error is measured in)"""
    W2, b1 = np.asarray(W2, np.float64), np.asarray(b1, np.float64)
    if absolute:
        mask = [(np.asarray(state["p"][i], np.float64) + b1) > 0 for i in range(len(state["deg"]))]
        state = {k: np.abs(np.asarray(v, np.float64)) for k, v in state.items()}
        W2, g_logits = np.abs(W2), np.abs(np.asarray(g_logits, np.float64))
    Hd = W2.shape[1]
    co = np.zeros((2, 2 * Hd + 1))
    for i, (path, _) in enumerate(lambdas(steps)):
        deg, wt = float(state["deg"][i]), float(state["w_t"][i])
        p, q = np.asarray(state["p"][i], np.float64), np.asarray(state["q"][i], np.float64)
        gq = np.zeros(Hd)
        for c in range(W2.shape[0]):                         # classes ascending
            gq = gq + W2[c] * float(g_logits[i, c])
        zero = deg == 0
        if zero and mutant == "deg0":
            continue                                         # 0 / 0 everywhere: read as 0
        d = 1.0 if zero else deg
        u = gq / d
        v = (wt / (d * d)) * (gq * (mask[i] if absolute else (p + b1) > 0))
        c_k = 0.0 if zero else -(float(u @ q) + float(v @ p))
        c_k = abs(c_k) if absolute else c_k
        co[path, :Hd] += u
        if mutant != "no_V":
            co[path, Hd:2 * Hd] += v
        if mutant != "no_c":
            co[path, 2 * Hd] += c_k
    return co


def scores(co, z, h, row_cols, t, mutant=None):
    """float64 [n]"""
    z, h = np.asarray(z, np.float64), np.asarray(h, np.float64)
    Hd = z.shape[1]
    val = lambda c: h @ c[:Hd] + z @ c[Hd:2 * Hd] + c[2 * Hd]
    a = np.zeros(len(z), bool)
    a[np.asarray(row_cols, np.int64)] = True
    s = np.where(a, -val(co[1] if mutant == "add_for_existing" else co[0]), val(co[1]))
    s[t] = -10.0
    return s


def first_layer(P, x, adj):
    """(Z, H, row t's columns are read from adj by the caller): float64 Z = x W1^T and H = relu(A_hat Z + b1)"""
    x, adj = np.asarray(x, np.float64), np.asarray(adj, np.float64)
    deg = adj.sum(1, keepdims=True)
    deg[deg == 0] = 1
    Z = x @ np.asarray(P["gc1.weight"], np.float64).T
    H = np.maximum((adj / deg) @ Z + np.asarray(P["gc1.bias"], np.float64), 0)
    return Z, H


def importance(P, x, adj, t, strategy, steps, temp=None, mutant=None, dtype=np.float64):
    """the closed form on a dense adjacency: the importance vector [n] (float64) and the intermediate results.
    dtype: the format Z and H are rounded to before the sums (float32: what the kernels are given)"""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    Z, H = first_layer(P, x, adj)
    Z, H = Z.astype(dtype), H.astype(dtype)
    n = len(Z)
    cols = np.flatnonzero(np.asarray(adj)[t])
    Zf, Hf = Z.astype(np.float64), H.astype(np.float64)
    args = (cols, n, t, steps, Zf, Hf, Zf.sum(0), Hf.sum(0), P["gc1.bias"], P["gc2.weight"], P["gc2.bias"])
    st = _points64(*args)
    labels = None
    if mutant == "orig_label":
        labels = np.full(len(st["logits"]), int(np.argmax(st["logits"][steps])))     # lambda = 1 of the remove path
    g = head_grad(st["logits"], strategy, temp, labels)
    co = coefficients(st, g, P["gc1.bias"], P["gc2.weight"], steps, mutant)
    return scores(co, Zf, Hf, cols, t, mutant), dict(state=st, g_logits=g, coeffs=co, Z=Z, H=H)


def _points64(cols, n, t, steps, z, h, zsum, hsum, b1, W2, b2):
    """path_points on float64 z and h (path_points itself takes the kernel's float32 arrays)"""
    cols = np.asarray(cols, np.int64)
    sz, sh = z[cols].sum(0), h[cols].sum(0)
    a_t = 1.0 if t in cols else 0.0
    out = dict(logits=[], p=[], q=[], deg=[], w_t=[])
    for path, lam in lambdas(steps):
        if path == 0:
            deg, wt, pz, qh = lam * len(cols), lam * a_t, lam * sz, lam * sh
        else:
            deg, wt = (1 - lam) * n + lam * len(cols), 1 - lam * (1 - a_t)
            pz, qh = (1 - lam) * zsum + lam * sz, (1 - lam) * hsum + lam * sh
        d = deg if deg != 0 else 1.0
        p = pz / d
        q = (qh - wt * h[t] + wt * np.maximum(p + b1, 0)) / d
        out["logits"].append(W2 @ q + b2)
        out["p"].append(p), out["q"].append(q), out["deg"].append(deg), out["w_t"].append(wt)
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ the dense restatement
def dense_importance(P, x, adj, t, strategy, steps, temps=None, dtype=torch.float64, mutant=None):
    """calib_iga.py:152-235 on a dense leaf in `dtype`.  Every j with an entry shares one path and every j without one
    the other, and the reference reads entry [t][j] of the same gradient for each of them, so one backward per path
    point gives the whole row.  The leaf is the matrix at the path point itself: the reference's baselines are clones
    inside the graph, which makes d (path point) / d (adjacency) the identity (:185-188).  Returns (importance [n],
    the path points' logits (P, C))."""
    P = {k: torch.as_tensor(v).to(dtype) for k, v in P.items()}
    x, adj = torch.as_tensor(x).to(dtype), torch.as_tensor(adj).to(dtype)
    temps = None if temps is None else torch.as_tensor(temps).to(dtype)
    n = adj.shape[0]
    a = adj[t].clone()
    criterion = (lambda o, l: rows_criterion(o, l, "over")) if strategy == "over" else \
        (lambda o, l: rows_criterion(o, l, "under"))
    original_label = R.dense_forward(P, x, adj, temps)[[t]].argmax(dim=1)
    total = torch.zeros(2, n, dtype=dtype)
    logits = []
    for i, (path, lam) in enumerate(lambdas(steps)):
        point = adj.clone()
        point[t] = lam * a if path == 0 else 1 - lam * (1 - a)
        point.requires_grad_(True)
        out = R.dense_forward(P, x, point, temps)[[t]]
        label = original_label if mutant == "orig_label" else out.argmax(dim=1)
        g = torch.autograd.grad(criterion(out, label), point)[0]
        total[path] += g[t] + (g[:, t] if mutant == "row_col" else 0)
        logits.append(out.detach()[0])
    present = a != 0
    s = torch.where(present, -total[0], total[1])
    s[t] = -10
    return s.numpy().astype(np.float64), torch.stack(logits).numpy()


def attack_loop(P, x, adj, t, budget, strategy, scores_vec, temps=None, dtype=torch.float64):
    """calib_iga.py:75-141 from a given importance vector: dict(partners, labels, confs, n_perturb, best_conf,
    best_set, gaps (|new_confidence - best_confidence| of every comparison made))"""
    P = {k: torch.as_tensor(v).to(dtype) for k, v in P.items()}
    x, cur = torch.as_tensor(x).to(dtype), torch.as_tensor(adj).to(dtype).clone()
    temps = None if temps is None else torch.as_tensor(temps).to(dtype)
    fwd = lambda m: R.dense_forward(P, x, m, temps)[[t]]
    with torch.no_grad():
        o = fwd(cur)
    label0 = int(o.argmax(1))
    best_conf = F.softmax(o, dim=1)[0, label0].item()
    s = np.array(scores_vec, np.float64)
    res = dict(partners=[], labels=[], confs=[], logits=[], gaps=[], n_perturb=0, best_set=[], original_label=label0,
               original_conf=best_conf)
    flipped = []
    for _ in range(budget):
        j = int(np.argmax(s))
        cur[t, j] = cur[j, t] = 1 - cur[t, j]
        with torch.no_grad():
            o = fwd(cur)
        label = int(o.argmax(1))
        conf = F.softmax(o, dim=1)[0, label].item()
        flipped.append(j)
        res["partners"].append(j), res["labels"].append(label), res["confs"].append(conf)
        res["logits"].append(o[0].numpy())
        if label != label0:
            break
        res["n_perturb"] += 1
        res["gaps"].append(abs(conf - best_conf))
        if (strategy == "over" and conf >= best_conf) or (strategy == "under" and conf <= best_conf):
            best_conf, res["best_set"] = conf, sorted(flipped)
        s[j] = -np.inf
    res["best_conf"] = best_conf
    return res


def fixture_conditions(P, x, adj, t, strategy, steps, temps, ref_importance, budget):
    """the conditions a recorded run has to meet (tools/gen_golden_iga.py): (None, why) or (dict of the float64
    restatement's results, 'ok')"""
    n = adj.shape[0]
    temp = None if temps is None else float(temps[t])
    s64, aux = importance(P, x, adj, t, strategy, steps, temp=temp)
    others = np.arange(n) != t
    top = float(np.abs(s64[others]).max())
    order64 = np.argsort(-s64, kind="stable")[:budget + 1]
    order_ref = np.argsort(-ref_importance, kind="stable")[:budget + 1]
    if not np.array_equal(order64, order_ref):
        return None, "the float64 ranking differs"
    ranked = s64[np.argsort(-s64, kind="stable")[:budget + 2]]
    gap = float(np.min(-np.diff(ranked)))
    if not gap > 1e-4 * top:
        return None, f"score gap {gap:.3e} of {top:.3e}"
    lg = aux["state"]["logits"]
    srt = np.sort(lg, axis=1)
    lgap = float((srt[:, -1] - srt[:, -2]).min())
    if not lgap > 1e-4 * float(np.abs(lg).max()):
        return None, f"path-point logit gap {lgap:.3e}"
    pb = np.abs(aux["state"]["p"] + np.asarray(P["gc1.bias"], np.float64))
    if not float(pb.min()) > 1e-4 * float(pb.max()):
        return None, f"|p + b1| reaches {pb.min():.3e} of {pb.max():.3e}"
    loop = attack_loop(P, x, adj, t, budget, strategy, s64, temps=temps)
    if loop["gaps"] and not min(loop["gaps"]) > 1e-5:
        return None, f"confidence gap {min(loop['gaps']):.3e}"
    ev = np.sort(np.asarray(loop["logits"]), axis=1)
    egap = float((ev[:, -1] - ev[:, -2]).min())
    if not egap > 1e-4 * float(np.abs(ev).max()):
        return None, f"evaluated logit gap {egap:.3e}"
    return dict(s64=s64, loop=loop, top=top, min_score_gap=gap / top), "ok"
