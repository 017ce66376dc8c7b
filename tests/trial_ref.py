"""Truth and restated loop of the random attacks (csrc/attack.hip wg_trial_logits, wats_hip/attack.py Calib_Random /
Calib_RND).  Helpers of tests/test_random_attack.py, tests/test_random_attack_host.py and tools/gen_golden_random.py;
not a test.

  trial_logits   wg_trial_logits for one trial as an agg_ref.Ref, in the row unit of attack_ref.target_logits: truth
                 (np.longdouble, sequential), second (float64, numpy's sums), unit (2^-24 times the expression with
                 every term's absolute value, the feature deltas' products included), model, mutant; bound
                 agg_ref.BOUND_ONE
  random_loop    calib_random.py:127-186 / calib_rnd.py:169-236 restated on a dense adjacency in any torch dtype,
                 drawing from a given random.Random (or the random module); every trial is recorded
  LOOP_MUTANTS   WRONG on purpose: "no_self" (t left out of the connected list), "le" (<= for <), "no_rewind" (all
                 max_trials trials are drawn ahead and the state is not put back after the accepted one),
                 "always_draw" (the add / remove draw taken even when only one is possible), "dz_all_rows" (the
                 feature deltas reach z of every row), "no_dz_self" (dz dropped where row t gathers itself)
"""
import numpy as np
import torch
import torch.nn.functional as F

import agg_ref as A
import attack_ref as R

EPS = A.EPS
LD = np.longdouble
F32 = np.float32
LOOP_MUTANTS = ("no_self", "le", "no_rewind", "always_draw", "dz_all_rows", "no_dz_self")


# ------------------------------------------------------------------------------------------------ wg_trial_logits
def trial_logits(indptr, indices, z, b1, W2, b2, t, S, W1=None, feats=()):
    """One trial: target t, partners S (ascending, t allowed), feats = ((f, delta), ...) ascending in f"""
    z, b1, W2, b2 = (np.asarray(v, F32) for v in (z, b1, W2, b2))
    indptr = np.asarray(indptr, np.int64)
    items, rows = R.flipped_rows(indptr, indices, t, S)
    feats = [(int(f), F32(d)) for f, d in feats]
    W1 = None if W1 is None else np.asarray(W1, F32)

    def run(dt, seq, absolute=False):
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
        Hd = z.shape[1]
        dz = total([ab(d).astype(dt) * ab(W1[:, f]).astype(dt) for f, d in feats], Hd)
        hs = []
        for j in items:
            ks = rows[int(j)]
            deg = dt(max(len(ks), 1))
            s = total([ab(z[k]) for k in ks], Hd)
            if feats and np.any(ks == t):
                s = s + dz
            h = (dt(1) / deg) * s + ab(b1).astype(dt)
            hs.append(h if absolute else np.maximum(h, dt(0)))
        y2 = (dt(1) / dt(max(len(items), 1))) * total(hs, Hd)
        out = np.zeros(W2.shape[0], dt)
        for c in range(W2.shape[0]):
            out[c] = total([[ab(W2[c, f]).astype(dt) * y2[f]] for f in range(Hd)], 1)[0]
        return out + ab(b2).astype(dt)

    return A.Ref(run(LD, True), run(np.float64, False), EPS * A.f64(run(LD, True, absolute=True)),
                 A.f32(run(np.float64, True)), A.f32(A.f64(run(np.float32, True))), A.BOUND_ONE)


# ------------------------------------------------------------------------------------------------ the loop
def random_loop(P, x, adj, t, budget, strategy, max_trials, rng, attack_structure=True, attack_features=False,
                scale=None, dtype=torch.float64, mutant=None):
    """The reference's loop.  `scale`: the temperature scaling's factor log(exp(T) + 1.1) (TS.py:42; None: the bare
    model).  Returns dict(trials=[dict(step, kind, add, index, logits, label, conf, accepted)], n_perturb, best_conf,
    toggles (ascending), features (row t at the end), original_label, original_conf)."""
    assert attack_structure or attack_features
    P = {k: torch.as_tensor(v).to(dtype) for k, v in P.items()}
    x0, adj0 = torch.as_tensor(x).to(dtype), torch.as_tensor(adj).to(dtype)
    n, nfeat = adj0.shape[0], x0.shape[1]
    z0 = x0 @ P["gc1.weight"].t()

    def forward(adj_cur, xrow):
        deg = adj_cur.sum(dim=1, keepdim=True)
        deg = torch.where(deg == 0, torch.ones_like(deg), deg)
        an = adj_cur / deg
        dz = (xrow - x0[t]) @ P["gc1.weight"].t()
        zc = z0.clone()
        if mutant == "dz_all_rows":
            zc = zc + dz
        else:
            zc[t] = zc[t] + dz
        y1 = an @ zc
        if mutant == "no_dz_self":
            y1[t] = y1[t] - an[t, t] * dz
        h = F.relu(y1 + P["gc1.bias"])
        out = F.linear(an @ h, P["gc2.weight"], P["gc2.bias"])[[t]]
        if scale is not None:
            out = F.log_softmax(out * scale, dim=1)
        return out

    if strategy in ("under", "under_kl"):
        better = (lambda a, b: a <= b) if mutant == "le" else (lambda a, b: a < b)
    elif strategy == "over":
        better = (lambda a, b: a >= b) if mutant == "le" else (lambda a, b: a > b)
    else:
        raise ValueError(f"Unknown strategy: {strategy}")
    cur_adj, cur_row = adj0.clone(), x0[t].clone()
    out0 = forward(cur_adj, cur_row)
    label0 = int(out0.argmax(1))
    best_conf = conf0 = F.softmax(out0, dim=1)[0, label0].item()
    trials, attack_times = [], 0

    def draw():
        """one trial's draws: (kind, add, index) or None when nothing can be perturbed"""
        if attack_structure and attack_features:
            structure = rng.choice([True, False])
        else:
            structure = attack_structure
        if structure:
            row = cur_adj[t]
            connected = [int(j) for j in torch.nonzero(row > 0).flatten()]
            if mutant == "no_self":
                connected = [j for j in connected if j != t]
            absent = [int(j) for j in torch.nonzero(row == 0).flatten() if int(j) != t]
            if not (connected or absent):
                return None
            if (connected and absent) or mutant == "always_draw":
                add = rng.choice([True, False])
                if add and not absent:
                    add = False
                elif not add and not connected:
                    add = True
            else:
                add = bool(absent)
            pool = absent if add else connected
            return 0, int(add), pool[rng.randint(0, len(pool) - 1)]
        if nfeat == 0:
            return None
        return 1, -1, rng.randint(0, nfeat - 1)

    for step in range(budget):
        ahead = None
        if mutant == "no_rewind":      # the batched form without the rewind: every trial of the step is drawn first
            ahead = [draw() for _ in range(max_trials)]
        for k in range(max_trials):
            d = ahead[k] if ahead is not None else draw()
            if d is None:
                continue
            kind, add, index = d
            trial_adj, trial_row = cur_adj, cur_row
            if kind == 0:
                trial_adj = cur_adj.clone()
                trial_adj[t, index] = trial_adj[index, t] = 1.0 if add else 0.0
            else:
                trial_row = cur_row.clone()
                new = 1 - trial_row[index]
                add = int(new > trial_row[index])
                trial_row[index] = new
            out = forward(trial_adj, trial_row)
            label = int(out.argmax(1))
            conf = F.softmax(out, dim=1)[0, label].item()
            ok = label == label0 and better(conf, best_conf)
            trials.append(dict(step=step, kind=kind, add=add, index=index, logits=out[0].clone(), label=label,
                               conf=conf, accepted=ok, best_before=best_conf))
            if ok:
                best_conf, cur_adj, cur_row = conf, trial_adj, trial_row
                attack_times += 1
                break
    toggles = sorted(int(j) for j in torch.nonzero(cur_adj[t] != adj0[t]).flatten())
    return dict(trials=trials, n_perturb=attack_times, best_conf=best_conf, toggles=toggles, features=cur_row,
                original_label=label0, original_conf=conf0)
