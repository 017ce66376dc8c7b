"""Float64 truth, row-wise error units, models and mutants of the gated expert aggregation (csrc/gatedagg.hip), and a
plain-torch float64 restatement of the GETS calibrator (reference calibration/GETS.py), in the manner of agg_ref.py.
Helpers of tests/test_gets_host.py, tests/test_gets.py, tools/gen_golden_gets.py and tools/gets_probe.py; not a test.

Every kernel quantity is an agg_ref.Ref:
  truth    on exactly the float32 inputs the entry receives, summed sequentially in np.longdouble, stored as float64
  second   the same in float64 in another order (np.add.reduceat, reversed columns)
  unit     2^-24 times the same expression with every added term replaced by its absolute value
  model    the arithmetic the header documents: float64 throughout, each output rounded once
  mutant   WRONG on purpose, (a): the same with one float32 accumulator in entry order
  bound    BOUND_ONE for t_save, o_save, g_z, g_gate, g_t, g_logits: one rounding, counted from the header.
The Ref of t_save also carries mutant_b: each O_s rounded to float32, then the mixture in float32, which is what the
composition of sym_norm_aggregate calls and torch's elementwise passes does.

`out` is no sum, so its Ref holds the bound itself as `unit` (with bound 1): per element
    2^-24 |truth| + 2 max_c |logits_ic| SLACK max_c unit_T[i, c],
one rounding of the result plus the float64 slack of T (SLACK units of T at most, agg_ref's accounting) carried
through |d out_c / d T_c'|: out_c = v_c - lse(v) with v = logits * softplus(T), |d v / d T| <= |logits| and
sum_c' |d out_c / d v_c'| <= 2.  The truth of `out` comes from the longdouble T.
"""
import numpy as np
import torch
import torch.nn.functional as F

import agg_ref as A
import cagcn_ref as CG
import cheb_ref as C
import gats_ref as G

EPS, LD, SLACK = A.EPS, A.LD, A.SLACK
BOUND_ONE, TRUTH_AGREE = A.BOUND_ONE, A.TRUTH_AGREE
f32, f64 = C.f32, C.f64
LONG = 128          # wg_gated_symnorm_long_row(), asserted by the GPU tests
WIDTHS = (1, 3, 4, 5, 7, 40, 41, 64, 65, 256)
EXPERTS = ((1, 1), (2, 1), (3, 2), (3, 3), (4, 2), (4, 4))   # (E, k)
KINDS = A.KINDS
EXPERT_CONFIGS = (("logits", "features"), ("logits", "degrees"), ("features", "degrees"),
                  ("logits", "features", "degrees"))


def _softplus(T):
    with np.errstate(over="ignore"):
        return np.where(T > 20, T, np.log1p(np.exp(np.minimum(T, 20))))


def _sigmoid20(T):
    with np.errstate(over="ignore"):
        return np.where(T > 20, np.ones_like(T), 1 / (1 + np.exp(-T)))


def _head(T, logits, dt):
    v = logits.astype(dt) * _softplus(T.astype(dt))
    m = v.max(1, keepdims=True)
    return v - m - np.log(np.exp(v - m).sum(1, keepdims=True))


# --------------------------------------------------------------------------------------------------- forward
def forward(indptr, indices, dinv, z, sel, gate, bias, logits):
    """wg_gated_symnorm_forward: dict(o_save, t_save, out) of Refs"""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    n, E, Cw = z.shape
    k = sel.shape[1]
    sel = np.asarray(sel, np.int64)
    b = np.zeros((E, Cw), np.float32) if bias is None else np.asarray(bias, np.float32)
    rows = A.row_ids(indptr)
    keys = ("truth", "second", "abs", "model", "mutant")
    O = {key: [] for key in keys}
    for s in range(k):
        xg = z[indices, sel[rows, s], :]
        bs = b[sel[:, s]]

        def terms(dt):
            return dinv[indices].astype(dt)[:, None] * xg.astype(dt)

        def fin(acc, dt):
            return dinv.astype(dt)[:, None] * acc + bs.astype(dt)

        t64 = terms(np.float64)
        O["truth"].append(fin(A.seg_sum(indptr, terms(LD), LD), LD))
        O["second"].append(fin(A.seg_reduce(indptr, t64), np.float64))
        O["abs"].append(np.abs(f64(dinv))[:, None] * A.seg_reduce(indptr, np.abs(t64)) + np.abs(f64(bs)))
        O["model"].append(fin(A.seg_sum(indptr, t64, np.float64), np.float64))
        O["mutant"].append(fin(f64(A.seg_sum(indptr, t64, np.float32)), np.float64))

    def stack(key):
        return np.stack(O[key], axis=1)

    o_ref = A.Ref(f64(stack("truth")), stack("second"), EPS * stack("abs"), f32(stack("model")), f32(stack("mutant")),
                  BOUND_ONE)

    def mix(Os, dt):
        T = np.zeros((n, Cw), dt)
        for s in range(k):
            T = T + gate[:, s].astype(dt)[:, None] * Os[s]
        return T

    T_ld = mix(O["truth"], LD)
    unit_T = EPS * sum(np.abs(f64(gate[:, s]))[:, None] * O["abs"][s] for s in range(k))
    T_model, T_mut = mix(O["model"], np.float64), mix(O["mutant"], np.float64)
    t_ref = A.Ref(f64(T_ld), mix(O["second"], np.float64), unit_T, f32(T_model), f32(T_mut), BOUND_ONE)
    tb = np.zeros((n, Cw), np.float32)
    for s in range(k):    # (b): float32 products of the rounded O_s, a float32 sum
        tb = (tb + (gate[:, s][:, None] * f32(O["model"][s])).astype(np.float32)).astype(np.float32)
    t_ref.mutant_b = tb
    out_truth = f64(_head(T_ld, logits, LD))
    out_bound = EPS * np.abs(out_truth) + 2 * np.abs(f64(logits)).max(1, keepdims=True) * SLACK * \
        unit_T.max(1, keepdims=True)
    out_ref = A.Ref(out_truth, _head(t_ref.second, logits, np.float64), out_bound,
                    f32(_head(T_model, logits, np.float64)), f32(_head(T_mut, logits, np.float64)), 1.0)
    return dict(o_save=o_ref, t_save=t_ref, out=out_ref)


# --------------------------------------------------------------------------------------------------- backward
def head_backward(g_out, out, logits, t_save, o_save):
    """wg_gets_head_backward on its own float32 inputs: dict(g_logits, g_t, g_gate) of Refs"""
    def ev(dt, order=slice(None), acc=None):
        go, o = g_out.astype(dt), o_save.astype(dt)
        if acc is None:
            S = go[:, order].sum(1, keepdims=True)
        else:   # one sequential accumulator of `acc`
            S = np.zeros((go.shape[0], 1), acc)
            for c in range(go.shape[1]):
                S = (S + go[:, c:c + 1]).astype(acc)
            S = S.astype(dt)
        T = t_save.astype(dt)
        g_cal = go - np.exp(out.astype(dt)) * S
        gl = g_cal * _softplus(T)
        gt = g_cal * logits.astype(dt) * _sigmoid20(T)
        if acc is None:
            gg = (gt[:, None, order] * o[:, :, order]).sum(2)
        else:
            gg = np.zeros(o.shape[:2], acc)
            for c in range(go.shape[1]):
                gg = (gg + gt[:, None, c] * o[:, :, c]).astype(acc)
            gg = gg.astype(dt)
        return gl, gt, gg

    truth = ev(LD)
    second = ev(np.float64, slice(None, None, -1))
    model = ev(np.float64)
    mutant = ev(np.float64, acc=np.float32)
    T = f64(t_save)
    u_cal = np.abs(f64(g_out)) + np.exp(f64(out)) * np.abs(f64(g_out)).sum(1, keepdims=True)
    u_gt = u_cal * np.abs(f64(logits) * _sigmoid20(T))
    units = (u_cal * np.abs(_softplus(T)), u_gt, (u_gt[:, None, :] * np.abs(f64(o_save))).sum(2))
    return {name: A.Ref(f64(truth[q]), second[q], EPS * units[q], f32(model[q]), f32(mutant[q]), BOUND_ONE)
            for q, name in enumerate(("g_logits", "g_t", "g_gate"))}


def transposed(t_indptr, t_indices, dinv, sel, gate, g_t, E):
    """wg_gated_symnorm_transposed: the Ref of g_z (n, E, C); t_indices lists the rows that gather each node"""
    i = np.asarray(t_indices, np.int64)
    refs = []
    for e in range(E):
        w = (gate * (np.asarray(sel) == e)).sum(1).astype(np.float32)    # at most one slot of a row holds e
        refs.append(A.aggregate(t_indptr, lambda dt, w=w: dinv[i].astype(dt) * w[i].astype(dt), g_t[i],
                                row_scale=dinv))
    return A.Ref(*(np.stack([getattr(r, key) for r in refs], axis=1)
                   for key in ("truth", "second", "unit", "model", "mutant")), BOUND_ONE)


def _abs_transposed(t_indptr, t_indices, dinv, sel, gate, v, E):
    """dinv_j sum_i dinv_i |w_ie| v_i for a non-negative v (n, C), in float64: (n, E, C)"""
    i = np.asarray(t_indices, np.int64)
    out = []
    for e in range(E):
        w = np.abs(f64(gate) * (np.asarray(sel) == e)).sum(1)
        out.append(f64(dinv)[:, None] * A.seg_reduce(t_indptr, (f64(dinv)[i] * w[i])[:, None] * v[i]))
    return np.stack(out, axis=1)


def autograd_bounds(indptr, indices, dinv, I, g_out):
    """Bounds on |gradient of gated_sym_norm_head - the float64 gradient| per element, for g_logits, g_gate, g_z and
    g_bias, as the sum of the documented bounds.  The backward reads what the forward saved, so each saved quantity
    carries its own documented error into the gradient:
      dT, dO   BOUND_ONE units of t_save / o_save; dout: the bound of out (this module's docstring)
      exp(out) errs by exp(out) (e^dout - 1); g_cal = g_out - exp(out) S by that times |S|
      softplus has slope <= 1 and sigmoid slope <= 1 / 4 in T; a saved T on the other side of the threshold 20 moves
      either by 2.1e-9 (log1p(e^20) - 20, 1 - sigmoid(20)) on top
      every product rule below is first order plus its cross term; each kernel output then takes its own rounding
      (BOUND_ONE units, the unit evaluated at the perturbed magnitudes)
      g_gate uses the float64 g_t (no rounding of g_t in it), g_z and g_bias the rounded one
      g_bias is torch's float32 (E, n) x (n, C) product: gamma_n = (n + 1) 2^-24 of the sum of absolute terms."""
    fwd = forward(indptr, indices, dinv, **I)
    T, O, out = fwd["t_save"].truth, fwd["o_save"].truth, fwd["out"].truth
    dT, dO, dout = BOUND_ONE * fwd["t_save"].unit, BOUND_ONE * fwd["o_save"].unit, fwd["out"].unit
    go, lg = f64(g_out), np.abs(f64(I["logits"]))
    S, Sabs = np.abs(go.sum(1, keepdims=True)), np.abs(go).sum(1, keepdims=True)
    ex = np.exp(out)
    dex = ex * np.expm1(dout)
    g_cal, d_cal = np.abs(go - ex * go.sum(1, keepdims=True)), dex * S
    u_cal = np.abs(go) + (ex + dex) * Sabs
    sp, sig = np.abs(_softplus(T)), _sigmoid20(T)
    jump = 2.1e-9 * (np.abs(T - 20) <= dT)
    dsp, dsig = dT + jump, 0.25 * dT + jump
    one = BOUND_ONE * EPS
    d_gl = d_cal * sp + (g_cal + d_cal) * dsp + one * u_cal * (sp + dsp)
    gt = g_cal * lg * sig
    d_gt64 = d_cal * lg * (sig + dsig) + g_cal * lg * dsig
    u_gt = u_cal * lg * (sig + dsig)
    d_gt = d_gt64 + one * u_gt
    absO = np.abs(O) + dO
    d_gg = (d_gt64[:, None, :] * absO + gt[:, None, :] * dO).sum(2) + one * (u_gt[:, None, :] * absO).sum(2)
    t_indptr, order = A.transpose_order(indptr, indices)
    t_indices = A.row_ids(np.asarray(indptr, np.int64))[order]
    n, E = I["z"].shape[:2]
    d_gz = _abs_transposed(t_indptr, t_indices, dinv, I["sel"], I["gate"], d_gt, E) + \
        one * _abs_transposed(t_indptr, t_indices, dinv, I["sel"], I["gate"], gt + d_gt, E)
    dense = np.zeros((n, E))
    np.put_along_axis(dense, np.asarray(I["sel"], np.int64), np.abs(f64(I["gate"])), axis=1)
    d_gb = dense.T @ d_gt + (n + 1) * EPS * (dense.T @ (gt + d_gt))
    return dict(g_logits=d_gl, g_gate=d_gg, g_z=d_gz, g_bias=d_gb)


# --------------------------------------------------------------------------------------------------- graphs, inputs
def star_edges(hub_entries, extra=12):
    """(src, dst, n): node 0 has exactly `hub_entries` entries with its self loop, as a row and as a column; node 1
    onwards are its leaves, the last `extra` nodes form a ring of short rows"""
    leaves = np.arange(1, hub_entries)
    ring = np.arange(hub_entries, hub_entries + extra)
    src = np.concatenate([leaves, np.zeros(len(leaves), np.int64), ring, np.roll(ring, -1)])
    dst = np.concatenate([np.zeros(len(leaves), np.int64), leaves, np.roll(ring, -1), ring])
    return src, dst, hub_entries + extra


def graph_csr(name):
    """(indptr, indices, n) by destination.  "path", "star127" / "star128" / "star129", "random300" carry one self
    loop per node; "hole" is the path with all entries of row 2 removed (an empty range: no loop either)"""
    if name in ("path", "hole"):
        src, dst, n = G.path_graph(6)
    elif name.startswith("star"):
        src, dst, n = star_edges(int(name[4:]))
    else:
        assert name == "random300", name
        src, dst, n = G.random_graph(300, 8, True, 7, loops=3)
    indptr, indices = A.by_destination(src, dst, n, True)
    if name == "hole":
        keep = A.row_ids(indptr) != 2
        indices = indices[keep]
        indptr = np.concatenate([[0], np.cumsum(np.bincount(A.row_ids(indptr)[keep], minlength=n))]).astype(np.int64)
    return indptr, indices, n


def dinv_of(indptr):
    """in-degree^-1/2 in float32, as SymNormGraph; a row with an empty range gets 1"""
    deg = np.diff(indptr).astype(np.float32)
    return np.where(deg > 0, deg, 1).astype(np.float32) ** np.float32(-0.5)


def head_inputs(n, E, k, Cw, kind, seed):
    """dict(z, sel, gate, bias, logits): z of `kind` (agg_ref.signal), a random distinct selection per row, gates a
    softmax, bias and logits normal.  "spread" puts T on both sides of the softplus threshold 20."""
    rng = np.random.default_rng(seed)
    z = A.signal(n, E * Cw, kind, seed).reshape(n, E, Cw)
    sel = np.argsort(rng.random((n, E)), axis=1)[:, :k].astype(np.int32)
    g = np.exp(rng.standard_normal((n, k)))
    gate = (g / g.sum(1, keepdims=True)).astype(np.float32)
    return dict(z=z, sel=sel, gate=gate, bias=A.signal(E, Cw, "normal", seed + 1),
                logits=(2 * A.signal(n, Cw, "normal", seed + 2)).astype(np.float32))


# --------------------------------------------------------------------------------------------------- torch restatements
def head_torch(src, dst, dinv, z, sel, gate, bias, logits, dtype=torch.float64):
    """The reference's composition (GETS.py:402-417) from z: every expert aggregated, the dense gates, the mixture,
    softplus, log_softmax; differentiable.  dinv None: deg^-1/2 in `dtype`."""
    n, E, Cw = z.shape
    agg = CG.sym_norm_edges(src, dst, z.reshape(n, E * Cw), dinv, None, False, dtype).reshape(n, E, Cw)
    if bias is not None:
        agg = agg + bias.to(dtype)
    gates = torch.zeros(n, E, dtype=dtype).scatter(1, sel.long(), gate.to(dtype))
    T = (agg * gates.unsqueeze(-1)).sum(1)
    return torch.log_softmax(logits.to(dtype) * F.softplus(T), dim=1)


def degrees_of(adj):
    """GETS.py:77 on edge_index = nonzero(adj): out-degree + in-degree of the entries of adj itself"""
    present = torch.as_tensor(adj) != 0
    return (present.sum(1) + present.sum(0)).long()


def cv_squared(x):
    return x.var() / (x.mean() ** 2 + 1e-10)


def calibrator_forward(P, x, adj, fit_adj, num_experts=3, k=2, train=False, noise=None, loss_coef=1e-2,
                       dtype=torch.float64):
    """GETSCalibrator.forward (GETS.py:390-417) on CompatibleGCN (tests/models.py) in `dtype`, eval mode or train mode
    with the gate's noise given and no dropout.  P: the calibrator's state_dict names plus base_model.gc1.weight ... ;
    adj: what the base model sees (may require a gradient); fit_adj: the experts' graph, as seen by fit.  Returns
    dict(out, gates, sel, aux_loss, clean_logits)."""
    P = {key: torch.as_tensor(v).to(dtype) if torch.as_tensor(v).is_floating_point() else torch.as_tensor(v)
         for key, v in P.items()}
    x, adj = torch.as_tensor(x).to(dtype), torch.as_tensor(adj).to(dtype)
    deg = adj.sum(1, keepdim=True)
    deg = torch.where(deg == 0, torch.ones_like(deg), deg)
    adj_norm = adj / deg
    h = torch.relu((adj_norm @ x) @ P["base_model.gc1.weight"].t() + P["base_model.gc1.bias"])
    logits = (adj_norm @ h) @ P["base_model.gc2.weight"].t() + P["base_model.gc2.bias"]
    gi = torch.cat([x @ P["proj_feature.weight"].t() + P["proj_feature.bias"], logits], dim=1)
    clean = gi @ P["w_gate"]
    if train:
        std = F.softplus(gi @ P["w_noise"]) + 1e-2
        noisy = clean + torch.as_tensor(noise).to(dtype) * std
        gl = noisy
    else:
        gl = clean
    top, idx = gl.topk(min(k + 1, num_experts), dim=1)
    sel, top_gates = idx[:, :k], torch.softmax(top[:, :k], dim=1)
    gates = torch.zeros_like(gl).scatter(1, sel, top_gates)
    if train and k < num_experts:
        normal = torch.distributions.normal.Normal(torch.zeros(1, dtype=dtype), torch.ones(1, dtype=dtype))
        th_in, th_out = top[:, k:k + 1], top[:, k - 1:k]
        load = torch.where(noisy > th_in, normal.cdf((clean - th_in) / std), normal.cdf((clean - th_out) / std)).sum(0)
    else:
        load = (gates > 0).sum(0).to(dtype)
    fit_adj = torch.as_tensor(fit_adj)
    n = fit_adj.shape[0]
    r, c = torch.nonzero(fit_adj, as_tuple=True)
    src, dst = G.with_self_loops(r.numpy(), c.numpy(), n)
    degrees = degrees_of(fit_adj)
    zs, bs = [], []
    for e in range(num_experts):
        config, pre = EXPERT_CONFIGS[e], f"experts.{e}."
        parts = []
        if "logits" in config:
            parts.append(logits)
        if "features" in config:
            parts.append(x @ P[pre + "proj_feature.weight"].t() + P[pre + "proj_feature.bias"])
        if "degrees" in config:
            parts.append(P[pre + "degree_embedder.weight"][degrees])
        hcur = torch.cat(parts, dim=-1)
        n_convs = sum(1 for key in P if key.startswith(pre + "convs.") and key.endswith(".lin.weight"))
        for layer in range(n_convs - 1):
            hcur = CG.gcn_conv(P[f"{pre}convs.{layer}.lin.weight"], P[f"{pre}convs.{layer}.bias"], src, dst, hcur,
                               None, True, dtype)
        zs.append(hcur @ P[f"{pre}convs.{n_convs - 1}.lin.weight"].t())
        bs.append(P[f"{pre}convs.{n_convs - 1}.bias"])
    out = head_torch(src, dst, None, torch.stack(zs, dim=1), sel, top_gates, torch.stack(bs), logits, dtype)
    aux = (cv_squared(gates.sum(0)) + cv_squared(load)) * loss_coef
    return dict(out=out, gates=gates, sel=sel, aux_loss=aux, clean_logits=clean, logits=logits)


def adjacency_gradient(P, x, adj, loss_weight, rows, cols, **kw):
    """d sum(loss_weight * out) / d adj at (rows, cols) through a dense leaf; the experts' graph stays adj's"""
    a = torch.as_tensor(adj).to(kw.get("dtype", torch.float64)).clone().requires_grad_(True)
    out = calibrator_forward(P, x, a, adj, **kw)["out"]
    (out * torch.as_tensor(loss_weight).to(out.dtype)).sum().backward()
    return a.grad[torch.as_tensor(rows).long(), torch.as_tensor(cols).long()]


def load_case(path):
    """a fixture as a dict of torch tensors (arrays only: allow_pickle=False)"""
    with np.load(path, allow_pickle=False) as f:
        return {key: torch.from_numpy(np.asarray(f[key])) for key in f.files}


def case_params(c):
    """the calibrator's state_dict entries (P) and the base model's of a fixture"""
    return {key[3:]: v for key, v in c.items() if key.startswith("p__")}
