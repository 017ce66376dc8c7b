"""CPU tests of the batched attack step (csrc/fga.hip, Calib_FGA.attack_many): the closed form of the gradient's row and
column (tests/fga_many_ref.py) against the dense float64 autograd of tests/attack_ref.attack_loop on every step of
every recorded run, with the per-row criteria of wats_hip.attack (the code attack_many runs) giving d L / d out_t; the
restatement's float32 scores reproducing every recorded partner; the conditions under which the GPU tests compare
partners exactly, asserted on every fixture step and on every (graph, surrogate, method, strategy, target) that
tests/test_fga_many.py compares with the single-target methods (fga_many_ref.CLASS_CASES); every mutant shown to fall
outside; the ABI's argument checks; the no-GPU refusal."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attack_ref as R
import fga_many_ref as M
import test_attack_host as H
import wats_hip
from wats_hip import attack as L

BOUND = 1e-12
_steps = {}


def step_spec(method, strategy, current, original, target_label=0):
    """(kind, label, rerank) of one scored step: which criterion calib_fga.py applies, to which label"""
    if method == "attack":
        kind = {"over": "over", "under": "under", "under_kl": "kl", "target": "target"}[strategy]
        return kind, (target_label if kind == "target" else current), False
    calib = current == original or method == "rerank_attack"
    return ("kl", current, True) if calib else ("restore", original, False)


def csr_of(adj):
    import scipy.sparse as sp
    m = sp.csr_matrix(np.asarray(adj, np.float64))
    m.sort_indices()
    return m.indptr.astype(np.int64), m.indices.astype(np.int32)


def head_of(temp):
    return (lambda raw: raw) if temp is None else (lambda raw: F.log_softmax(raw / temp, dim=1))


def steps_of(tag, method, strategy, P, x, adj, t, budget, y, temps):
    """every scored step of one run: the dense float64 truth and the closed form's inputs in float64 and float32"""
    if tag in _steps:
        return _steps[tag]
    truth = R.attack_loop(method, P, x, adj, t, budget, strategy, res_gt=y, temps=temps, dtype=torch.float64)
    single = R.attack_loop(method, P, x, adj, t, budget, strategy, res_gt=y, temps=temps, dtype=torch.float32)
    indptr, indices = csr_of(adj)
    n = adj.shape[0]
    P64 = {k: torch.as_tensor(v).double() for k, v in P.items()}
    x64, adj64 = torch.as_tensor(x).double(), torch.as_tensor(adj).double()
    W1, b1, W2 = (np.asarray(P[k], np.float32) for k in ("gc1.weight", "gc1.bias", "gc2.weight"))
    z64 = np.asarray(x, np.float64) @ W1.astype(np.float64).T
    z32 = (np.asarray(x, np.float32) @ W1.T).astype(np.float32)
    h32 = M.base_hidden(indptr, indices, z32, b1)
    h64 = np.maximum(np.stack([z64[indices[indptr[i]:indptr[i + 1]]].mean(0) if indptr[i + 1] > indptr[i]
                               else np.zeros(z64.shape[1]) for i in range(n)]) + b1.astype(np.float64), 0)
    temp = None if temps is None else float(temps[t])
    out = []
    for s, rec in enumerate(truth["steps"]):
        row = rec["adj_row"].numpy()
        S = np.flatnonzero(row != np.asarray(adj, np.float64)[t])
        cur = adj64.clone()
        cur[t, S] = 1 - cur[t, S]
        cur[S, t] = cur[t, S]
        raw = R.dense_forward(P64, x64, cur)[[t]].detach()
        label = int(head_of(temp)(raw).argmax(1))
        kind, lab, rerank = step_spec(method, strategy, label, truth["original_label"])
        gt = torch.as_tensor(y)[[t]]
        g64, top2 = L._row_gradients(raw, head_of(temp), [kind], torch.tensor([lab]), [rerank], gt)
        g32, top2_32 = L._row_gradients(raw.float(), head_of(temp), [kind], torch.tensor([lab]), [rerank], gt)
        out.append(dict(S=S, rec=rec, rerank=rerank, g64=g64[0].numpy(), g32=g32[0].numpy(),
                        top2=None if top2 is None else top2[0].numpy(),
                        top2_32=None if top2_32 is None else top2_32[0].numpy(),
                        partner32=single["steps"][s]["partner"] if s < len(single["steps"]) else None,
                        scores32=single["steps"][s]["scores"].numpy() if s < len(single["steps"]) else None))
    _steps[tag] = dict(steps=out, indptr=indptr, indices=indices, z64=z64, z32=z32, h64=h64, h32=h32, b1=b1, W2=W2, n=n,
                       t=t)
    return _steps[tag]


def fixture_steps(name, i):
    c, meta, _ = H.run_of(name, i)
    temps = c["wats_temps"] if meta.get("surrogate") == "WATS" else None
    return steps_of((name, i), meta["method"], meta["strategy"], c["P"], c["x"], c["adj"], meta["target"],
                    c["meta"]["budget"], c["y"], temps)


def halves(v, n, t):
    """the row and column halves without the entry (t, t)"""
    keep = np.arange(n) != t
    return np.concatenate([np.asarray(v)[:n][keep], np.asarray(v)[n:][keep]])


def scores64(D, st):
    """the scores of calib_fga.py:880-897 in float64 from the closed form, and the rerank's condition c_j"""
    n, t = D["n"], D["t"]
    grow, gcol, _, _ = M.closed_form(D["indptr"], D["indices"], D["z64"], D["h64"], D["b1"], D["W2"], t, st["S"],
                                     st["g64"])
    a = np.zeros(n)
    a[M.current_row(D["indptr"], D["indices"], t, st["S"])] = 1
    d = 1 - 2 * a
    s = (grow[0] + gcol[0]) * d
    cond = None
    if st["rerank"]:
        cond = st["top2"][0] + grow[1] * d - st["top2"][1] - grow[2] * d
        s = s * np.where(cond > 0, 1.0, -1.0)
    s[t] = -10
    return s, cond, grow, gcol


def scores32(D, st, mutant=None, select_mutant=None):
    grow, gcol, _, _ = M.closed_form(D["indptr"], D["indices"], D["z32"], D["h32"], D["b1"], D["W2"], D["t"], st["S"],
                                     st["g32"], mutant=mutant)
    grads = np.concatenate([grow, gcol], axis=1).astype(np.float32)
    return M.scores(D["n"], D["t"], grads, D["indptr"], D["indices"], st["S"], st["rerank"], st["top2_32"],
                    mutant=select_mutant)


@pytest.mark.parametrize("name,i", H.runs())
def test_closed_form_is_the_dense_float64_gradient_on_every_recorded_step(name, i):
    D = fixture_steps(name, i)
    n, t = D["n"], D["t"]
    assert len(D["steps"]) >= 3
    worst = 0.0
    for st in D["steps"]:
        _, _, grow, gcol = scores64(D, st)
        rec = st["rec"]
        keys = ["grad_loss"] + (["grad_pmax", "grad_psmax"] if st["rerank"] else [])
        assert st["rerank"] == ("grad_pmax" in rec)
        for g, key in enumerate(keys):
            got = halves(np.concatenate([grow[g], gcol[g]]), n, t)
            worst = max(worst, float(np.abs(got - halves(rec[key].numpy(), n, t)).max()))
    print(f"{name} run {i}: closed form against dense float64 autograd {worst:.2e} (bound {BOUND:.0e})")
    assert worst <= BOUND


@pytest.mark.parametrize("name,i", H.runs())
def test_float32_scores_reproduce_the_recorded_partners_and_their_conditions_hold(name, i):
    c, meta, r = H.run_of(name, i)
    D = fixture_steps(name, i)
    recorded = c["meta"]["f32_vs_f64"]["scores"]
    assert len(D["steps"]) == len(r["partner"])
    for s, st in enumerate(D["steps"]):
        s32 = scores32(D, st)
        s64, cond, _, _ = scores64(D, st)
        assert int(np.argmax(s32)) == int(r["partner"][s]) == int(np.argmax(s64)), (name, i, s)
        if cond is not None:
            smallest = float(np.abs(np.delete(cond, D["t"])).min())
            assert smallest >= 100 * recorded, (name, i, s, smallest, recorded)
        top = np.sort(s64)[::-1]
        d = float(np.abs(s32.astype(np.float64) - s64).max())
        assert top[0] - top[1] >= 100 * d, (name, i, s, top[0] - top[1], d)


def synthetic_case():
    indptr, indices, adj = M.synthetic()
    x, P, y = M.synthetic_model(adj)
    return indptr, indices, adj.astype(np.float32), x, P, y


def class_graph(graph):
    """(adj, x, P, y, targets) of a graph tests/test_fga_many.py runs the class on"""
    if graph == "synthetic":
        _, _, adj, x, P, y = synthetic_case()
        return adj, x, P, y, list(M.SYN_TARGETS)
    c = H.case(graph)
    return c["adj"], c["x"], c["P"], c["y"], sorted({r["target"] for r in c["meta"]["runs"]})


def conditions_of(D, t):
    """the smallest ratio of each condition to its bound over the steps of one run (the conditions hold from 1 up),
    and whether the float32 loop, the float64 loop and the closed form in both formats pick the same partners"""
    same, gap, switch = True, np.inf, np.inf
    for st in D["steps"]:
        s64, cond, grow, gcol = scores64(D, st)
        rec = st["rec"]
        got = halves(np.concatenate([grow[0], gcol[0]]), D["n"], t)
        assert np.abs(got - halves(rec["grad_loss"].numpy(), D["n"], t)).max() <= BOUND
        s32 = scores32(D, st)
        same = same and st["partner32"] == rec["partner"] == int(np.argmax(s64)) == int(np.argmax(s32))
        if st["scores32"] is None:                           # the float32 loop stopped before this step
            same = False
            continue
        recorded = float(np.abs(st["scores32"].astype(np.float64) - rec["scores"].numpy()).max())
        d = max(recorded, float(np.abs(s32.astype(np.float64) - s64).max()))
        top = np.sort(s64)[::-1]
        gap = min(gap, (top[0] - top[1]) / (100 * d))
        if cond is not None:
            switch = min(switch, float(np.abs(np.delete(cond, t)).min()) / (100 * recorded))
    return same, gap, switch


@pytest.mark.parametrize("method,strategy", M.CLASS_CASES)
@pytest.mark.parametrize("surrogate", ["gcn", "ts"])
@pytest.mark.parametrize("graph", ["synthetic", "iso120", "hub96"])
def test_conditions_hold_on_every_case_the_gpu_tests_compare_exactly(graph, surrogate, method, strategy):
    """what tests/test_fga_many.py relies on when it compares attack_many with the single-target methods flip for
    flip: on every target, for both surrogates, the float32 and float64 loops pick the same partners, no rerank
    condition is within 100 x the step's score distance of its switch and no top score is that near the second.  A
    target in fga_many_ref.CLASS_LEFT_OUT must miss a condition: the GPU test leaves it out for that reason alone."""
    adj, x, P, y, targets = class_graph(graph)
    temps = None if surrogate == "gcn" else np.full(adj.shape[0], M.CLASS_TEMPERATURE, np.float32)
    kept = M.class_targets(graph, surrogate, method, strategy, targets)
    assert graph != "synthetic" or kept == targets           # nothing is left out on the synthetic graph
    for t in targets:
        D = steps_of(("class", graph, surrogate, method, strategy, t), method, strategy, P, x, adj, t, M.CLASS_BUDGET,
                     y, temps)
        assert D["steps"]
        same, gap, switch = conditions_of(D, t)
        print(f"{graph} {surrogate} {method} {strategy} target {t}: top-2 gap {gap:.3g} x its bound, rerank "
              f"condition {switch:.3g} x its bound, same partners {same}")
        if t in kept:
            assert same and gap >= 1 and switch >= 1, (t, same, gap, switch)
        else:
            assert not (same and gap >= 1 and switch >= 1), (t, "is left out but holds every condition")


# ------------------------------------------------------------------------------------------------ the mutants
def far(a, b, n, t):
    return float(np.abs(halves(a, n, t) - halves(b, n, t)).max())


def test_mutant_without_the_column_half_and_mutant_with_a_removed_partners_base_h():
    hits = {"no_column": 0, "base_h_removed": 0}
    for name, i in H.runs():
        D = fixture_steps(name, i)
        for st in D["steps"]:
            args = (D["indptr"], D["indices"], D["z64"], D["h64"], D["b1"], D["W2"], D["t"], st["S"], st["g64"])
            good = np.concatenate(M.closed_form(*args)[:2], axis=1)[0]
            want = st["rec"]["grad_loss"].numpy()
            bad = np.concatenate(M.closed_form(*args, mutant="no_column")[:2], axis=1)[0]
            if far(good, bad, D["n"], D["t"]) > 0:
                assert far(bad, want, D["n"], D["t"]) > 1e3 * BOUND
                hits["no_column"] += 1
            base = D["indices"][D["indptr"][D["t"]]:D["indptr"][D["t"] + 1]]
            if np.isin(st["S"], base).any():                 # a removed partner
                bad = np.concatenate(M.closed_form(*args, mutant="base_h_removed")[:2], axis=1)[0]
                assert far(bad, want, D["n"], D["t"]) > 1e3 * BOUND, (name, i)
                hits["base_h_removed"] += 1
    assert hits["no_column"] > 50 and hits["base_h_removed"] > 0, hits


def test_mutant_that_keeps_y2_on_a_row_the_toggles_emptied():
    """a target without a self loop whose only neighbour is removed: deg' = 0 is the constant 1 and y2 = 0"""
    indptr, indices, adj, x, P, _ = synthetic_case()
    t = 147
    S = np.array([5])
    W1, b1, W2 = P["gc1.weight"], P["gc1.bias"], P["gc2.weight"]
    z = x.astype(np.float64) @ W1.astype(np.float64).T
    h = np.maximum(np.stack([z[indices[indptr[i]:indptr[i + 1]]].mean(0) if indptr[i + 1] > indptr[i]
                             else np.zeros(z.shape[1]) for i in range(len(indptr) - 1)]) + b1.astype(np.float64), 0)
    g = np.array([[0.3, -0.2, 0.5, -0.6]])
    good = M.closed_form(indptr, indices, z, h, b1, W2, t, S, g)
    bad = M.closed_form(indptr, indices, z, h, b1, W2, t, S, g, mutant="stale_y2")
    # the dense truth
    Pt = {k: torch.from_numpy(v).double() for k, v in P.items()}
    a = torch.from_numpy(adj).double()
    a[t, 5] = a[5, t] = 0
    leaf = a.clone().requires_grad_(True)
    out = R.dense_forward(Pt, torch.from_numpy(x).double(), leaf)[t]
    want = torch.autograd.grad((out * torch.from_numpy(g[0])).sum(), leaf)[0]
    n = adj.shape[0]
    assert np.abs(np.delete(good[0][0], t) - np.delete(want[t].numpy(), t)).max() <= BOUND
    assert np.abs(np.delete(bad[0][0], t) - np.delete(want[t].numpy(), t)).max() > 1e-3
    assert not good[1].any() and n == 150


def test_mutant_ge_at_the_relu_kink():
    """0 -> 1 -> 2, no other entry: y1_1 = z_2, and b1 = -z_2 puts every unit of node 1 exactly on the kink, where
    torch's ReLU has gradient 0"""
    indptr, indices = np.array([0, 1, 2, 2], np.int64), np.array([1, 2], np.int32)
    rng = np.random.default_rng(0)
    z = rng.standard_normal((3, 5)).astype(np.float32)
    b1 = -z[2]
    W2 = rng.standard_normal((3, 5)).astype(np.float32)
    g = rng.standard_normal((1, 3)).astype(np.float32)
    h = M.base_hidden(indptr, indices, z, b1)
    good = M.closed_form(indptr, indices, z, h, b1, W2, 0, [], g)
    bad = M.closed_form(indptr, indices, z, h, b1, W2, 0, [], g, mutant="relu_ge")
    assert good[1][0, 1] == 0 and abs(bad[1][0, 1]) > 1e-3
    a = torch.zeros(3, 3, dtype=torch.float64)
    a[0, 1] = a[1, 2] = 1
    leaf = a.clone().requires_grad_(True)
    deg = leaf.sum(1, keepdim=True)
    an = leaf / torch.where(deg == 0, torch.ones_like(deg), deg)
    hh = torch.relu(an @ torch.from_numpy(z).double() + torch.from_numpy(b1).double())
    out = (an @ hh) @ torch.from_numpy(W2).double().t()
    want = torch.autograd.grad((out[0] * torch.from_numpy(g[0]).double()).sum(), leaf)[0]
    assert abs(float(want[1, 0]) - good[1][0, 1]) <= BOUND and abs(float(want[0, 2]) - good[0][0, 2]) <= BOUND


def test_mutants_of_the_select_on_the_closed_forms_gradients():
    """the symmetric rerank and the entry (t, t) counted from both halves, on the rows wg_fga_scores writes"""
    differs = unmasked = 0
    for name, i in H.runs():
        D = fixture_steps(name, i)
        for st in D["steps"]:
            good = scores32(D, st)
            both = scores32(D, st, select_mutant="self_unmasked")
            assert good[D["t"]] == np.float32(-10)
            unmasked += int(both[D["t"]] != np.float32(-10))
            if st["rerank"]:
                differs += int(not np.array_equal(good, scores32(D, st, select_mutant="sym_rerank")))
    assert unmasked > 50 and differs > 0                     # both mutants are visible on the closed form's own rows
    # the symmetric rerank reads the column half: a sign changes where that half outweighs the row half
    n, t = 6, 0
    grads = np.zeros((3, 2 * n), np.float32)
    grads[0, :n] = [0, 1, 2, 3, 4, 5]
    grads[1, n + 5] = -1
    p = np.array([0.6, 0.4], np.float32)
    indptr, indices = np.array([0, 1, 1, 1, 1, 1, 1], np.int64), np.array([0], np.int32)
    good = M.scores(n, t, grads, indptr, indices, [], True, p)
    bad = M.scores(n, t, grads, indptr, indices, [], True, p, mutant="sym_rerank")
    assert int(np.argmax(good)) == 5 and int(np.argmax(bad)) == 4
    print(f"fixture steps where the symmetric rerank changes a score: {differs}")


# ------------------------------------------------------------------------------------------------ the host side
def test_loss_rows_are_the_single_row_criteria():
    torch.manual_seed(1)
    out = torch.randn(5, 4, dtype=torch.float64)
    lab = out.argmax(1)
    gt = torch.tensor([0, 1, 2, 3, 0])
    tl = torch.zeros(5, dtype=torch.int64)
    kinds = ["over", "under", "kl", "target", "restore"]
    rows = L._loss_rows(out, kinds, torch.where(torch.tensor([k == "target" for k in kinds]), tl, lab), gt)
    one = lambda b: out[[b]]
    want = [L.overconfidence_objective(one(0), lab[[0]]), L.underconfidence_objective(one(1), lab[[1]]),
            L.kl_divergence_with_uniform(one(2), lab[[2]]), L.kl_divergence_target(one(3), tl[[3]], gt[[3]]),
            L._restore_loss(one(4), lab[[4]])]
    assert torch.allclose(rows, torch.stack(want), rtol=0, atol=1e-15)
    for b in range(5):                                       # every branch of the target distribution
        for tlab in range(4):
            got = L._loss_rows(out[[b]], ["target"], torch.tensor([tlab]), gt[[b]])
            assert torch.allclose(got[0], L.kl_divergence_target(out[[b]], torch.tensor([tlab]), gt[[b]]), atol=1e-15)


def test_a_rows_gradient_is_finite_beside_a_row_of_another_kind_and_the_same_as_alone():
    """a restore row whose softmax underflows to 0 shares the call with a kl row: each criterion is evaluated on its
    own rows, so the restore row's gradient is the one-hot it has alone, not 0 x inf from the kl branch's log"""
    raw = torch.tensor([[200.0, 0.0, -200.0, 0.0], [0.3, -0.2, 0.5, -0.6], [1.0, 2.0, -120.0, 0.5]])
    assert float(F.softmax(raw, dim=1)[0, 2]) == 0.0
    kinds, labels, rerank = ["restore", "kl", "over"], torch.tensor([1, 2, 1]), [False, True, False]
    g, top2 = L._row_gradients(raw, head_of(None), kinds, labels, rerank)
    assert bool(torch.isfinite(g).all()) and g.shape == (3, 3, 4)
    assert torch.equal(g[0, 0], torch.tensor([0.0, 1.0, 0.0, 0.0]))
    for b in range(3):
        alone, t2 = L._row_gradients(raw[[b]], head_of(None), [kinds[b]], labels[[b]], [True])
        assert torch.equal(alone[0], g[b]) and torch.equal(t2[0], top2[b]), b


def test_many_result_makes_the_view_on_first_read_by_key_get_or_in():
    class Start:
        made = 0

        def with_flips(self, rows, cols):
            Start.made += 1
            return ("view", tuple(rows), tuple(cols))

    r = L._ManyResult(Start(), target=4, best_flips=[2, 9], flips=[9, 2])
    assert "modified_op" in r and "nothing" not in r and r.get("nothing", 7) == 7 and Start.made == 0
    assert "modified_op" not in list(r)                      # iterating forces no view
    assert r.get("modified_op") == ("view", (4, 4), (2, 9)) and r["modified_op"] is r.get("modified_op")
    assert Start.made == 1 and "modified_op" in dict(r)
    with pytest.raises(KeyError):
        r["nothing"]


def test_abi_checks_arguments_before_any_device_work():
    lib = wats_hip._lib.load()
    nbytes = ctypes.c_int64(0)
    ws = lib.wg_fga_scores_workspace
    assert ws(100, 16, 4, 3, 50, None) == -1 and ws(0, 16, 4, 3, 50, nbytes) == -1
    assert ws(100, 16, 4, 2, 50, nbytes) == -1 and ws(100, 16, 4, 1, -1, nbytes) == -1
    assert ws(100, 257, 4, 1, 50, nbytes) == -4 and ws(2 ** 31, 16, 4, 1, 50, nbytes) == -4
    assert ws(100, 16, 4, 3, 50, nbytes) == 0 and nbytes.value > 0
    small = nbytes.value
    assert ws(100, 16, 4, 3, 500, nbytes) == 0 and nbytes.value > small
    p = [4096 + 256 * q for q in range(20)]
    sc = lib.wg_fga_scores
    #      0 n 1 nnz 2 indptr 3 indices 4 Hd 5 z 6 h 7 b1 8 W2 9 C 10 B 11 targets 12 tog_ptr 13 tog_ids 14 G
    ok = [5, 9, p[0], p[1], 4, p[2], p[3], p[4], p[5], 3, 2, p[6], p[7], p[8], 3,
          #  15 g_logits 16 rerank 17 p_top2 18 topk 19 nwg 20 cap 21 ws 22 grads 23 scores 24 ids 25 best 26 stream
          p[9], p[10], p[11], 1, 0, 20, p[12], None, None, p[13], p[14], None]

    def bad(code, word, **changes):
        args = list(ok)
        for k, v in changes.items():
            args[int(k[1:])] = v
        assert sc(*args) == code, changes
        assert word in lib.wg_last_error(), (changes, lib.wg_last_error())

    bad(-1, b"n=", a0=0)
    bad(-4, b"int32", a0=2 ** 31)
    bad(-1, b"nnz", a1=-1)
    bad(-4, b"int32", a1=2 ** 31)
    bad(-1, b">= 1", a4=0)
    bad(-4, b"256", a4=257)
    bad(-1, b">= 1", a9=0)
    bad(-4, b"256", a9=257)
    bad(-1, b">= 1", a10=0)
    bad(-1, b"G=", a14=2)
    bad(-1, b"G=", a14=0)
    bad(-1, b"topk", a18=0)
    bad(-1, b"topk", a18=9)
    bad(-1, b"n_workgroups", a19=513)
    bad(-1, b"n_workgroups", a19=-1)
    bad(-1, b"local_cap", a20=-1)
    for pos in (2, 5, 6, 7, 8, 11, 12, 15, 24, 25):
        bad(-1, b"NULL", **{f"a{pos}": None})
    bad(-1, b"indices", a3=None)
    bad(-1, b"p_top2", a17=None)
    bad(-1, b"workspace", a21=None)
    bad(-1, b"workspace", a21=p[12] + 8)


def test_argument_checks_of_the_python_wrappers():
    assert {"fga_scores", "fga_scores_workspace"} <= set(dir(wats_hip)) and hasattr(wats_hip.Calib_FGA, "attack_many")
    many = L.Calib_FGA.attack_many
    with pytest.raises(ValueError, match="Unknown method"):
        many(None, None, None, [1], 2, "under", method="sideways", res_gt=1)
    with pytest.raises(ValueError, match="only supports 'under'"):
        many(None, None, None, [1], 2, "over", res_gt=1)
    with pytest.raises(ValueError, match="Unknown strategy"):
        many(None, None, None, [1], 2, "sideways", method="attack", res_gt=1)
    with pytest.raises(ValueError, match="res_gt"):
        many(None, None, None, [1], 2, "under")
    with pytest.raises(ValueError, match="ascending"):
        L._pack_toggles(5, [1], [[3, 2]], "cpu")
    with pytest.raises(ValueError, match="ascending"):
        L._pack_toggles(5, [1], [[1]], "cpu")                 # the target itself


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU refusal")
def test_refuses_to_run_without_a_gpu():
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        L.fga_scores(4, torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), z, z, torch.zeros(3),
                     torch.zeros(2, 3), [1], [[]], torch.zeros(1, 1, 2))
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        L.Calib_FGA(torch.nn.Linear(3, 3)).attack_many(None, None, [1], 1, 'under', res_gt=1)
