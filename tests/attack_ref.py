"""Models, float64 truth and mutants of the attack step (csrc/attack.hip, wats_hip/attack.py).  Helpers of
tests/test_attack_host.py, tests/test_attack.py and tools/gen_golden_fga.py; not a test.

  select_model     wg_flip_select in numpy float32, bit-exact by construction: every operation is one IEEE single
                   operation on float32 arrays (numpy fuses nothing), the ranking a lexicographic sort
  target_logits    wg_target_logits as an agg_ref.Ref: truth (np.longdouble, sequential), second (float64, numpy's
                   pairwise sums), unit (2^-24 times the expression with every term's absolute value), model (float64
                   sequential, rounded once), mutant (one float32 accumulator per sum) and .mutant_deg (deg' taken from
                   the base row)
  attack_loop      the four methods of calib_attack/calib_fga.py restated on a dense adjacency in any torch dtype
                   (float64: the truth the fixtures' partners are checked against)
  SELECT_MUTANTS   WRONG on purpose: "sym_rerank" (the rerank reads the symmetric sum of grad_pmax / grad_psmax),
                   "ge" (c >= 0 for c > 0), "last_tie" (equal scores by larger index), "self_unmasked" (no -10)
"""
import numpy as np
import torch
import torch.nn.functional as F

import agg_ref as A

EPS = A.EPS
LD = np.longdouble
SELECT_MUTANTS = ("sym_rerank", "ge", "last_tie", "self_unmasked")
F32 = np.float32


# ------------------------------------------------------------------------------------------------ wg_flip_select
def rank(scores, topk, last_tie=False):
    """(ids int32 [topk], scores float32 [topk]): descending, a NaN above every number, equal scores (-0 == +0) by
    smaller index; slots past n: id -1, score -inf"""
    s = np.asarray(scores, F32)
    n = len(s)
    nan = np.isnan(s)
    clean = np.where(nan, F32(0), s).astype(np.float64) + 0.0
    idx = np.arange(n)
    order = np.lexsort((-idx if last_tie else idx, -clean, ~nan))[:topk]
    ids = np.full(topk, -1, np.int32)
    best = np.full(topk, -np.inf, F32)
    ids[:len(order)] = order
    best[:len(order)] = s[order]
    return ids, best


def select_scores(n, t, grad_loss, row_cols, row_vals=None, toggled=(), grad_pmax=None, grad_psmax=None, p_top2=None,
                  mutant=None):
    """the score vector of wg_flip_select (include/wats_hip.h), float32 operation for operation"""
    g = np.asarray(grad_loss, F32)
    a = np.zeros(n, F32)
    a[np.asarray(row_cols, np.int64)] = F32(1) if row_vals is None else np.asarray(row_vals, F32)
    tog = np.asarray(toggled, np.int64)
    if tog.size:
        a[tog] = a[tog] + (F32(1) - F32(2) * a[tog])
    d = F32(1) - F32(2) * a
    s = (g[:n] + g[n:]) * d
    if grad_pmax is not None:
        gp, gs = np.asarray(grad_pmax, F32), np.asarray(grad_psmax, F32)
        if mutant == "sym_rerank":
            gp_row, gs_row = gp[:n] + gp[n:], gs[:n] + gs[n:]
        else:
            gp_row, gs_row = gp[:n], gs[:n]
        p = np.asarray(p_top2, F32)
        with np.errstate(invalid="ignore"):
            c = ((p[0] + gp_row * d) - p[1]) - gs_row * d
            flag = np.where((c >= 0) if mutant == "ge" else (c > 0), F32(1), F32(-1))
        s = s * flag
    if mutant != "self_unmasked":
        s[t] = F32(-10)
    return s.astype(F32)


def select_model(n, t, grad_loss, row_cols, row_vals=None, toggled=(), grad_pmax=None, grad_psmax=None, p_top2=None,
                 topk=1, mutant=None):
    """(scores, best_ids, best_scores)"""
    s = select_scores(n, t, grad_loss, row_cols, row_vals, toggled, grad_pmax, grad_psmax, p_top2, mutant)
    ids, best = rank(s, topk, last_tie=(mutant == "last_tie"))
    return s, ids, best


def torch_scores(n, t, grad_loss, adj_row, grad_pmax=None, grad_psmax=None, p_top2=None):
    """the reference's composition (calib_fga.py:880-897) on torch tensors of any device, from the gradient's row and
    column halves and row t of the current dense adjacency"""
    delta = -2 * adj_row + 1
    grad = (grad_loss[:n] + grad_loss[n:]) * delta
    if grad_pmax is not None:
        cond = p_top2[0] + grad_pmax[:n] * delta - p_top2[1] - grad_psmax[:n] * delta
        grad = grad * torch.where(cond > 0, torch.tensor(1), torch.tensor(-1)).to(grad.device)
    grad[t] = -10
    return grad


# ------------------------------------------------------------------------------------------------ wg_target_logits
def flipped_rows(indptr, indices, t, S):
    """{j: ascending array of N'(j)} for j in N'(t) and N'(t) itself, in the kernel's item order (the base row's
    surviving entries ascending, then the added partners)"""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    row = lambda j: indices[indptr[j]:indptr[j + 1]]
    S = np.asarray(S, np.int64)
    Nt = row(t)
    items = np.concatenate([Nt[~np.isin(Nt, S)], S[~np.isin(S, Nt)]])
    rows = {}
    for j in items:
        if j == t:
            rows[int(j)] = np.sort(items)
        elif j in S:
            rows[int(j)] = np.setxor1d(row(j), [t])
        else:
            rows[int(j)] = row(j)
    return items, rows


def target_logits(indptr, indices, z, b1, W2, b2, t, S):
    """wg_target_logits for one candidate toggle set S: an agg_ref.Ref over the C logits"""
    z, b1, W2, b2 = (np.asarray(v, F32) for v in (z, b1, W2, b2))
    indptr = np.asarray(indptr, np.int64)
    base_len = np.diff(indptr)
    items, rows = flipped_rows(indptr, indices, t, S)

    def run(dt, seq, deg_of=None, absolute=False):
        """dt: the accumulators' format; seq: sequential sums (else numpy's); absolute: the unit's expression"""
        ab = (lambda v: np.abs(v)) if absolute else (lambda v: v)

        def total(terms, width):
            if not len(terms):
                return np.zeros(width, dt)
            if not seq:
                return np.asarray(terms, dt).sum(axis=0)
            acc = np.zeros(width, dt)
            for v in terms:
                acc = (acc + np.asarray(v, dt)).astype(dt)
            return acc
        hs = []
        for j in items:
            ks = rows[int(j)]
            deg = dt(deg_of(int(j)) if deg_of else max(len(ks), 1))
            y1 = (dt(1) / deg) * total([ab(z[k]) for k in ks], z.shape[1])
            h = y1 + ab(b1).astype(dt)
            hs.append(h if absolute else np.maximum(h, dt(0)))
        deg_t = dt(deg_of(int(t)) if deg_of else max(len(items), 1))
        y2 = (dt(1) / deg_t) * total(hs, z.shape[1])
        out = np.zeros(W2.shape[0], dt)
        for c in range(W2.shape[0]):
            out[c] = total([[ab(W2[c, f]).astype(dt) * y2[f]] for f in range(z.shape[1])], 1)[0]
        return out + ab(b2).astype(dt)

    truth = run(LD, True)
    ref = A.Ref(truth, run(np.float64, False), EPS * A.f64(run(LD, True, absolute=True)), A.f32(run(np.float64, True)),
                A.f32(A.f64(run(np.float32, True))), A.BOUND_ONE)
    ref.mutant_deg = A.f32(run(np.float64, True, deg_of=lambda j: max(int(base_len[j]), 1)))
    return ref


# ------------------------------------------------------------------------------------------------ the attack loop
def dense_forward(P, x, adj, temps=None):
    """CompatibleGCN.forward (src/gnn/model.py:43-52) in eval mode in the dtype of x; with `temps` (one temperature per
    node, WATS.py:124-130) the calibrated log-probabilities"""
    deg = adj.sum(dim=1, keepdim=True)
    deg = torch.where(deg == 0, torch.ones_like(deg), deg)
    an = adj / deg
    h = F.relu(F.linear(an @ x, P["gc1.weight"], P["gc1.bias"]))
    out = F.linear(an @ h, P["gc2.weight"], P["gc2.bias"])
    if temps is not None:
        out = F.log_softmax(out / temps.unsqueeze(1), dim=1)
    return out


def attack_loop(method, P, x, adj, t, budget, strategy="under", res_gt=None, target_label=0, temps=None,
                dtype=torch.float64, beam_width=3, select=None):
    """One of calib_fga.py's four methods on a dense leaf, in `dtype`.  Returns the per-step records (scores, p_top2,
    partner, logits, label, confidence; grads: the row / column halves of every gradient taken) and the run's
    n_perturb, best_conf, best adjacency and final label.  `select(scores_inputs) -> partner` replaces the argmax of
    the restated scores (a mutant's choice)."""
    from wats_hip import attack as L
    P = {k: torch.as_tensor(v).to(dtype) for k, v in P.items()}
    x, adj0 = torch.as_tensor(x).to(dtype), torch.as_tensor(adj).to(dtype)
    temps = None if temps is None else torch.as_tensor(temps).to(dtype)
    n = adj0.shape[0]
    fwd = lambda a: dense_forward(P, x, a, temps)[[t]]
    original_output = fwd(adj0).detach()
    original_label = original_output.argmax(1)
    conf0 = F.softmax(original_output, dim=1)[0, int(original_label)].item()
    gt = None if res_gt is None else torch.as_tensor(res_gt)[[t]]
    steps = []

    def step(cur, hybrid, rerank, criterion):
        leaf = cur.clone().detach().requires_grad_(True)
        output = fwd(leaf)
        current_label = output.argmax(dim=1)
        same = bool(current_label == original_label)
        if criterion is not None:
            if strategy != "target":
                loss = criterion(output, current_label)
            else:
                loss = criterion(output, torch.tensor([target_label]), gt)
            use_rerank = False
        elif same or not hybrid:
            loss, use_rerank = L.kl_divergence_with_uniform(output, current_label), rerank
        else:
            loss, use_rerank = -F.nll_loss(output, original_label), False
        g = torch.autograd.grad(loss, leaf, retain_graph=True)[0]
        halves = lambda m: torch.cat([m[t], m[:, t]]).detach()
        rec = dict(grad_loss=halves(g), adj_row=leaf[t].detach().clone())
        gp = gs = top2 = None
        if use_rerank:
            top2 = torch.topk(F.softmax(output, dim=1), 2, dim=1)[0][0]
            gp = halves(torch.autograd.grad(top2[0], leaf, retain_graph=True)[0])
            gs = halves(torch.autograd.grad(top2[1], leaf, retain_graph=True)[0])
            rec.update(grad_pmax=gp, grad_psmax=gs, p_top2=top2.detach())
        scores = torch_scores(n, t, rec["grad_loss"], rec["adj_row"], gp, gs, None if top2 is None else top2.detach())
        j = int(torch.argmax(scores)) if select is None else int(select(rec))
        new = leaf.detach().clone()
        v = -2 * new[t][j] + 1
        new[t][j] += v
        new[j][t] += v
        with torch.no_grad():
            new_output = fwd(new)
        new_label = new_output.argmax(dim=1)
        conf = F.softmax(new_output, dim=1)[0, int(new_label)].item()
        rec.update(scores=scores, partner=j, logits=new_output[0], label=int(new_label), confidence=conf)
        steps.append(rec)
        return new, new_label, conf

    best_adj, best_conf, attack_times = adj0.clone(), conf0, 0
    if method == "flip_beam_hybridloss_attack":
        beam = [(conf0, 0, adj0.clone())]
        for _ in range(budget):
            nxt = []
            for _ in range(beam_width):
                if not beam:
                    break
                beam.sort(key=lambda m: (m[0], m[1]))
                _, count, cur = beam.pop(0)
                if count >= budget:
                    continue
                new, new_label, conf = step(cur, True, True, None)
                nxt.append((conf, count + 1, new))
                if new_label == original_label and conf < best_conf:
                    best_conf, best_adj, attack_times = conf, new.clone(), count + 1
            beam = nxt
    else:
        criterion = None
        if method == "attack":
            criterion = {"over": L.overconfidence_objective, "under": L.underconfidence_objective,
                         "under_kl": L.kl_divergence_with_uniform, "target": L.kl_divergence_target}[strategy]
            if strategy == "under_kl":
                strategy = "under"
        cur = adj0.clone()
        for _ in range(budget):
            cur, new_label, conf = step(cur, method == "rerank_hybridloss_attack", method != "attack", criterion)
            if new_label != original_label:
                break
            attack_times += 1
            if method != "attack" or strategy == "under":
                better = conf <= best_conf
            elif strategy == "over":
                better = conf >= best_conf
            else:
                tl = target_label
                under = (tl == int(original_label) and tl == int(gt)) or (tl != int(original_label) and tl == int(gt))
                better = conf <= best_conf if under else conf >= best_conf
            if better:
                best_conf, best_adj = conf, cur.clone()
    final = fwd(best_adj)
    return dict(steps=steps, n_perturb=attack_times, best_conf=best_conf, best_adj=best_adj,
                final_label=int(final.argmax(1)), original_label=int(original_label), initial_confidence=conf0)
