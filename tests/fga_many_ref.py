"""numpy restatement of wg_fga_scores (csrc/fga.hip, include/wats_hip.h), rounding points included.  Helper of
tests/test_fga_many_host.py and tests/test_fga_many.py; not a test.

  closed_form    the two gradient entries of every partner of one target in any float format: row half d / d A[t, j],
                 column half d / d A[i, t], and the expression with every term's absolute value (the unit)
  grads_ref      an agg_ref.Ref over the (G, 2 n) gradient block: truth (np.longdouble), second (float64), unit,
                 model (float64 rounded once)
  scores         the float32 scores of wg_flip_select (attack_ref.select_scores) on float32 gradient rows
  MUTANTS        WRONG on purpose: "no_column" (the column half dropped), "base_h_removed" (a removed partner keeps the
                 base graph's h_j), "stale_y2" (the -q . y2 term of the base row kept on a row the toggles emptied: deg
                 not treated as the constant 1 there), "relu_ge" (>= at the ReLU kink)
"""
import numpy as np

import agg_ref as A
import attack_ref as R

F32, LD = np.float32, np.longdouble
MUTANTS = ("no_column", "base_h_removed", "stale_y2", "relu_ge")


def base_hidden(indptr, indices, z, b1):
    """h = relu(A_hat z + b1) of the base graph, float64 sums rounded once to float32 (the kernel's argument)"""
    n = len(indptr) - 1
    h = np.zeros(z.shape, np.float64)
    for i in range(n):
        ks = indices[indptr[i]:indptr[i + 1]]
        if len(ks):
            h[i] = z[ks].astype(np.float64).sum(0) / len(ks)
    return np.maximum(h + b1.astype(np.float64), 0).astype(F32)


def local_rows(indptr, indices, t, S):
    """(items = N'(t) in attack_ref's order, {j: N'(j)} for every local j = N(t) + S, removed partners included)"""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    items, rows = R.flipped_rows(indptr, indices, t, S)
    base = indices[indptr[t]:indptr[t + 1]]
    for j in np.asarray(S, np.int64):
        if j in base:                                         # removed: its row lost t
            rows[int(j)] = np.setxor1d(indices[indptr[j]:indptr[j + 1]], [t])
    return items, rows


def closed_form(indptr, indices, z, h, b1, W2, t, S, g, dt=np.float64, mutant=None):
    """(grow (G, n), gcol (G, n), unit_row, unit_col) in the format dt.  g: (G, C) = d L / d out_t"""
    n, Hd = z.shape
    zd, hd, bd = z.astype(dt), h.astype(dt).copy(), b1.astype(dt)
    q = np.asarray(g).astype(dt) @ W2.astype(dt)             # (G, Hd)
    items, rows = local_rows(indptr, indices, t, S)
    on = (lambda v: v >= 0) if mutant == "relu_ge" else (lambda v: v > 0)
    y1 = {}
    base_row = np.asarray(indices[indptr[t]:indptr[t + 1]], np.int64)
    for j, ks in rows.items():
        y1[j] = zd[ks].sum(0) / dt(max(len(ks), 1)) if len(ks) else np.zeros(Hd, dt)
        removed = j not in items
        if not (mutant == "base_h_removed" and removed):
            hd[j] = np.maximum(y1[j] + bd, dt(0))
    live = sorted(int(j) for j in items)
    deg_t = dt(max(len(live), 1))
    y1_t = zd[live].sum(0) / deg_t if live else np.zeros(Hd, dt)
    y2 = hd[live].sum(0) / deg_t if live else np.zeros(Hd, dt)
    if mutant == "stale_y2" and not live and len(base_row):
        y2 = h.astype(dt)[base_row].sum(0) / dt(len(base_row))
    a_tt = t in live
    grow = (q @ hd.T - (q @ y2)[:, None]) / deg_t
    unit_row = (np.abs(q) @ np.abs(hd).T + (np.abs(q) @ np.abs(y2))[:, None]) / deg_t
    if a_tt:
        m_t = np.where(on(y1_t + bd), q, dt(0))
        grow = grow + (m_t @ zd.T - (m_t @ y1_t)[:, None]) / (deg_t * deg_t)
        unit_row = unit_row + (np.abs(m_t) @ np.abs(zd).T + (np.abs(m_t) @ np.abs(y1_t))[:, None]) / (deg_t * deg_t)
    gcol = np.zeros((q.shape[0], n), dt)
    unit_col = np.zeros((q.shape[0], n), dt)
    if mutant != "no_column":
        for i in live:
            m_i = np.where(on(y1[i] + bd), q, dt(0))
            w = dt(1) / (deg_t * dt(max(len(rows[i]), 1)))
            gcol[:, i] = w * (m_i @ (zd[t] - y1[i]))
            unit_col[:, i] = w * (np.abs(m_i) @ (np.abs(zd[t]) + np.abs(y1[i])))
    return grow, gcol, unit_row, unit_col


def grads_ref(indptr, indices, z, h, b1, W2, t, S, g):
    """the (G, 2 n) block wg_fga_scores writes for one target, as an agg_ref.Ref (the slots of (t, t) are not defined:
    compare with .rows / a mask that leaves columns t and n + t out)"""
    def block(dt):
        grow, gcol, ur, uc = closed_form(indptr, indices, z, h, b1, W2, t, S, g, dt)
        return np.concatenate([grow, gcol], axis=1), np.concatenate([ur, uc], axis=1)
    truth, unit = block(LD)
    second, _ = block(np.float64)
    return A.Ref(truth, second, A.EPS * A.f64(unit), A.f32(second), A.f32(second), A.BOUND_ONE)


def current_row(indptr, indices, t, S):
    """the ids j with an entry (t, j) in the flipped graph"""
    return np.sort(np.asarray(local_rows(indptr, indices, t, S)[0], np.int64))


def scores(n, t, grads, indptr, indices, S, rerank=False, p_top2=None, mutant=None):
    """wg_flip_select's float32 scores on the float32 rows `grads` (G, 2 n) of one target"""
    base = np.asarray(indices[indptr[t]:indptr[t + 1]], np.int64)
    kw = dict(grad_pmax=grads[1], grad_psmax=grads[2], p_top2=p_top2) if rerank else {}
    return R.select_scores(n, t, grads[0], base, None, np.asarray(S, np.int64), mutant=mutant, **kw)


# ------------------------------------------------------------------------------------------------ the synthetic graph
def synthetic(n=150, seed=11, hub=140):
    """A seeded symmetric unit graph with self loops for the class tests: a hub (node 0, `hub` neighbours: a row past
    wg_target_long_row()), a sparse random rest, node n - 1 isolated (no entry at all), node n - 2 with its self
    loop only, node n - 3 of degree one without a self loop.  Returns (indptr int64, indices int32, dense bool)."""
    rng = np.random.default_rng(seed)
    adj = np.zeros((n, n), bool)
    for _ in range(3 * n):
        i, j = rng.integers(1, n - 3, 2)
        adj[i, j] = adj[j, i] = True
    adj[0, 1:hub + 1] = adj[1:hub + 1, 0] = True
    np.fill_diagonal(adj, True)
    adj[n - 1, :] = adj[:, n - 1] = False
    adj[n - 2, :] = adj[:, n - 2] = False
    adj[n - 2, n - 2] = True
    adj[n - 3, :] = adj[:, n - 3] = False
    adj[n - 3, 5] = adj[5, n - 3] = True
    indptr = np.concatenate([[0], np.cumsum(adj.sum(1))]).astype(np.int64)
    return indptr, np.nonzero(adj)[1].astype(np.int32), adj


SYN_TARGETS = (0, 7, 33, 147, 148, 149)        # the hub, two ordinary nodes, degree one, self loop only, isolated

# ------------------------------------------------------------------- the class against the single-target methods
# What tests/test_fga_many.py compares flip for flip, and tests/test_fga_many_host.py asserts the conditions of: every
# (method, strategy) of CLASS_CASES on every target of the graph (SYN_TARGETS; on a fixture graph the targets of its
# recorded runs), for a bare GCN ("gcn") and for a TemperatureScaling surrogate at CLASS_TEMPERATURE ("ts").  At 1.7
# the self-loop-only target 148 of the synthetic graph has a rerank condition 75 x its score distance from its switch.
CLASS_CASES = (("attack", "under"), ("rerank_attack", "under"), ("rerank_hybridloss_attack", "under"),
               ("flip_beam_hybridloss_attack", "under"), ("attack", "over"), ("attack", "under_kl"),
               ("attack", "target"))
CLASS_BUDGET = 4
CLASS_TEMPERATURE = 2.0
# Left out of the exact comparison: on the bare GCN of the fixture graphs these targets' unnormalised outputs are
# saturated, and the top two scores of a step lie within 100 x the float32-against-float64 score distance (0 to 46 x),
# so float32 autograd and the float64 closed form may pick different partners there.  The host file asserts that each
# entry does miss the condition, so the list cannot outlive its reason.
CLASS_LEFT_OUT = {("iso120", "gcn", "attack", "over"): (41, 48, 90),
                  ("hub96", "gcn", "attack", "over"): (1, 6, 20),
                  ("hub96", "gcn", "attack", "under"): (1,)}


def class_targets(graph, surrogate, method, strategy, targets):
    out = CLASS_LEFT_OUT.get((graph, surrogate, method, strategy), ())
    return [t for t in targets if t not in out]


def synthetic_model(adj, nfeat=12, nhid=16, nclass=4, seed=3):
    """(x float32 (n, nfeat), parameters of the two-layer base model as float32 arrays, labels) for `synthetic`"""
    rng = np.random.default_rng(seed)
    n = adj.shape[0]
    x = rng.standard_normal((n, nfeat)).astype(F32)
    P = {"gc1.weight": (0.6 * rng.standard_normal((nhid, nfeat))).astype(F32),
         "gc1.bias": (0.1 * rng.standard_normal(nhid)).astype(F32),
         "gc2.weight": (0.8 * rng.standard_normal((nclass, nhid))).astype(F32),
         "gc2.bias": (0.1 * rng.standard_normal(nclass)).astype(F32)}
    return x, P, rng.integers(0, nclass, n).astype(np.int64)
