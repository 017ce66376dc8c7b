"""GPU tests of the integrated-gradient scores (csrc/iga.hip, wats_hip/attack.py Calib_IGA).

wg_iga_path_logits is held to one rounding per row in the units of tests/agg_ref.py (2^-24 of the row's absolute sum
plus the float64 chain's (2 Hd + 2) 2^-52 of it, tests/iga_ref.path_logits_ref); the coefficients of wg_iga_scores to
1e-12 of their terms' absolute sum against the float64 restatement from the same g_logits and the kernel's own state;
the scores to |s - truth| <= 2^-24 |truth| + 2^-42 (|U| |h_j| + |V| |z_j| + |cbar|); the selection to a numpy sort of
the kernel's own scores, exactly.  Calib_IGA reproduces every run the reference recorded (tests/golden/iga): partners,
attack_times, the best set and the labels exactly, best_confidence and the importance vector within twice the measured
distance of the CPU model from the recorded float32 reference (manifest model_vs_reference)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

import agg_ref as A  # noqa: E402
import attack_ref as R  # noqa: E402
import cheb_ref as CH  # noqa: E402
import iga_ref as I  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip import Calib_IGA, RowNormalizedAdjacency, SparseCompatibleGCN, iga_path_logits, iga_scores  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iga")
DEV = "cuda"
LD = np.longdouble
_cases = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def _np(t):
    return t.detach().cpu().numpy()


def dev(a, offset=0):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if offset:                                            # a 4-byte-aligned view that is not 16-byte aligned
        buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
        buf[offset:] = t.reshape(-1).to(DEV)
        return buf[offset:].view(t.shape)
    return t.to(DEV)


# ------------------------------------------------------------------------------------------------ the kernels' inputs
KINDS = ("empty", "self", "full", "plain")


def row_of(kind, n, t, rng):
    """row t's ascending columns: no entry; some entries and the self entry; every entry; some entries without t"""
    others = np.array([j for j in range(n) if j != t], np.int64)
    some = np.sort(rng.choice(others, min(len(others), max(1, n // 4)), replace=False)) if len(others) else others
    if kind == "empty":
        return others[:0]
    if kind == "full":
        return np.arange(n, dtype=np.int64)
    if kind == "self":
        return np.sort(np.concatenate([some, [t]]))
    return some


def make_inputs(n, Hd, C, B, seed, kind="normal"):
    """targets (with a duplicate when B > 1) whose rows cycle through KINDS; the other rows are empty"""
    rng = np.random.default_rng(seed)
    distinct = rng.choice(n, min(n, max(1, B - 1)), replace=False) if B > 1 else rng.choice(n, 1)
    targets = np.array([distinct[i % len(distinct)] for i in range(B)], np.int32)
    if B > 1:
        targets[-1] = targets[0]                          # a duplicate
    rows = {}
    for i, t in enumerate(distinct):
        rows[int(t)] = row_of(KINDS[(i + seed) % 4], n, int(t), rng)
    indptr = np.zeros(n + 1, np.int64)
    for t, r in rows.items():
        indptr[t + 1] = len(r)
    indptr = np.cumsum(indptr)
    indices = np.concatenate([rows[t] for t in sorted(rows)]).astype(np.int32) if rows else np.zeros(0, np.int32)
    z, h = A.signal(n, Hd, kind, seed), np.maximum(A.signal(n, Hd, kind, seed + 1), 0).astype(np.float32)
    return dict(n=n, Hd=Hd, C=C, targets=targets, rows=rows, indptr=indptr, indices=indices, z=z, h=h,
                zsum=z.astype(np.float64).sum(0), hsum=h.astype(np.float64).sum(0),
                b1=rng.standard_normal(Hd).astype(np.float32), W2=A.signal(C, Hd, kind, seed + 2, spread=1.0),
                b2=rng.standard_normal(C).astype(np.float32))


def run_path(Q, steps, offset=0):
    out = iga_path_logits(Q["n"], dev(Q["indptr"]), dev(Q["indices"]), dev(Q["z"], offset), dev(Q["h"], offset),
                          dev(Q["zsum"]), dev(Q["hsum"]), dev(Q["b1"]), dev(Q["W2"]), dev(Q["b2"]), dev(Q["targets"]),
                          steps)
    torch.cuda.synchronize()
    return _np(out[0]), _np(out[1])


def check_path(Q, steps, offset=0):
    logits, state = run_path(Q, steps, offset)
    again = run_path(Q, steps, offset)[0]
    assert np.array_equal(logits.view(np.int32), again.view(np.int32)), "a repeat gives other bits"
    Hd, worst = Q["Hd"], 0.0
    done = {}
    for b, t in enumerate(Q["targets"]):
        t = int(t)
        if t in done:                                     # a duplicate target: the same bits
            assert np.array_equal(logits[b].view(np.int32), logits[done[t]].view(np.int32))
            assert np.array_equal(state[b], state[done[t]])
            continue
        done[t] = b
        args = (Q["rows"][t], Q["n"], t, steps, Q["z"], Q["h"], Q["zsum"], Q["hsum"], Q["b1"], Q["W2"], Q["b2"])
        truth, unit = I.path_logits_ref(*args)
        c = CH.c_of(logits[b], truth, unit, f"target {t}")
        worst = max(worst, c)
        assert c <= 1.0, (t, len(Q["rows"][t]), c)
        pts = I.path_points(*args, dt=LD)
        scale = lambda v: 1e-12 * max(1.0, float(np.abs(v).max()))
        ab = I.path_points(*args, dt=LD, absolute=True)
        assert np.abs(state[b][:, :Hd] - pts["p"].astype(np.float64)).max() <= scale(ab["p"])
        assert np.abs(state[b][:, Hd:2 * Hd] - pts["q"].astype(np.float64)).max() <= scale(ab["q"])
        assert np.abs(state[b][:, 2 * Hd] - pts["deg"].astype(np.float64)).max() <= 1e-12 * Q["n"]
        assert np.array_equal(state[b][:, 2 * Hd] == 0, pts["deg"] == 0)             # the zero rows, exactly
        assert np.abs(state[b][:, 2 * Hd + 1] - pts["w_t"].astype(np.float64)).max() <= 1e-15
    print(f"n={Q['n']} Hd={Hd} C={Q['C']} steps={steps} B={len(Q['targets'])}: c = {worst:.4f} (bound 1)")
    return logits, state


# n, Hd, C, steps, B: every size of the list appears, the widths around 64 and 256 with short and long rows
PATH_SHAPES = [(1, 1, 2, 1, 1), (2, 3, 7, 2, 2), (63, 4, 40, 10, 2), (64, 64, 7, 10, 33), (65, 65, 2, 2, 2),
               (257, 256, 256, 1, 2), (1000, 1, 7, 10, 33), (1000, 64, 40, 10, 2), (1000, 256, 40, 2, 1),
               (257, 3, 256, 2, 33), (65, 4, 2, 1, 1), (1000, 65, 7, 1, 2)]


@pytest.mark.parametrize("n,Hd,C,steps,B", PATH_SHAPES)
def test_path_logits_one_rounding(n, Hd, C, steps, B):
    check_path(make_inputs(n, Hd, C, B, seed=n + Hd), steps)


@pytest.mark.parametrize("kind", KINDS)
def test_path_logits_row_kinds_and_signals(kind):
    """each kind of row as the only target, on every signal; n = 1000 at Hd = 1: a full row is four passes of the 256
    sub-groups, at Hd = 256 a thousand passes of the one"""
    for sig in A.KINDS:
        for n, Hd in ((1000, 1), (300, 256), (70, 16)):
            Q = make_inputs(n, Hd, 5, 1, seed=KINDS.index(kind), kind=sig)       # seed: the first row's kind
            t = int(Q["targets"][0])
            assert {"empty": len(Q["rows"][t]) == 0, "full": len(Q["rows"][t]) == n, "self": t in Q["rows"][t],
                    "plain": t not in Q["rows"][t] and len(Q["rows"][t]) > 0}[kind]
            logits, state = check_path(Q, 3)
            if kind == "empty":                           # every remove point: the zero row, deg 0 -> 1, out = b2
                assert np.array_equal(logits[0, :4], np.tile(Q["b2"], (4, 1))) and not state[0, :4, 2 * Hd].any()
            if kind == "full":                            # the add path is all ones at every lambda
                assert np.abs(state[0, 4:, 2 * Hd] - n).max() <= 1e-12 * n and np.abs(state[0, 4:, 2 * Hd + 1] - 1).max() <= 1e-15


def test_path_logits_misaligned_z():
    Q = make_inputs(257, 64, 7, 2, seed=5)
    a = check_path(Q, 10)[0]
    b = check_path(Q, 10, offset=1)[0]
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------------ wg_iga_scores
def run_scores(Q, steps, g, state, topk=10, n_workgroups=0, offset=0, coeffs=True, scores=True):
    out = iga_scores(Q["n"], dev(Q["indptr"]), dev(Q["indices"]), dev(Q["z"], offset), dev(Q["h"], offset), dev(Q["b1"]),
                     dev(Q["W2"]), dev(Q["targets"]), steps, dev(g), dev(state), topk=topk, n_workgroups=n_workgroups,
                     return_scores=scores, return_coeffs=coeffs)
    torch.cuda.synchronize()
    return tuple(_np(v) for v in out)


def state_dict_of(state_b, Hd):
    return dict(p=state_b[:, :Hd], q=state_b[:, Hd:2 * Hd], deg=state_b[:, 2 * Hd], w_t=state_b[:, 2 * Hd + 1])


def check_scores(Q, steps, topk=10, seed=0, offset=0):
    """coefficients, scores and selection of one launch; returns (ids, best, scores)"""
    rng = np.random.default_rng(seed)
    n, Hd, B = Q["n"], Q["Hd"], len(Q["targets"])
    _, state = run_path(Q, steps)
    g = rng.standard_normal((B, 2 * (steps + 1), Q["C"])).astype(np.float32)
    ids, best, scores, co = run_scores(Q, steps, g, state, topk, offset=offset)
    zl, hl = Q["z"].astype(LD), Q["h"].astype(LD)
    for b, t in enumerate(Q["targets"]):
        t = int(t)
        st = state_dict_of(state[b], Hd)
        want = I.coefficients(st, g[b], Q["b1"], Q["W2"], steps)
        scale = I.coefficients(st, g[b], Q["b1"], Q["W2"], steps, absolute=True)
        err = np.abs(co[b] - want)
        assert (err <= 1e-12 * np.maximum(scale, 1e-300)).all(), (b, t, float((err / np.maximum(scale, 1e-300)).max()))
        # the scores from the kernel's own coefficients
        a = np.zeros(n, bool)
        a[Q["rows"][t]] = True
        U, V, cb = co[b][:, :Hd].astype(LD), co[b][:, Hd:2 * Hd].astype(LD), co[b][:, 2 * Hd].astype(LD)
        val = [hl @ U[p] + zl @ V[p] + cb[p] for p in (0, 1)]
        mag = [np.abs(hl) @ np.abs(U[p]) + np.abs(zl) @ np.abs(V[p]) + abs(cb[p]) for p in (0, 1)]
        truth = np.where(a, -val[0], val[1]).astype(np.float64)
        bound = 2.0 ** -24 * np.abs(truth) + 2.0 ** -42 * np.where(a, mag[0], mag[1]).astype(np.float64)
        truth[t], bound[t] = -10.0, 0.0
        d = np.abs(scores[b].astype(np.float64) - truth)
        assert (d <= bound).all(), (b, t, int(np.argmax(d - bound)), float(d.max()))
        check_selection(scores[b], ids[b], best[b], topk)
    return ids, best, scores


def check_selection(scores_b, ids_b, best_b, topk):
    want_ids, want_best = R.rank(scores_b, topk)
    assert np.array_equal(ids_b, want_ids), (ids_b, want_ids)
    nan = np.isnan(want_best)
    assert np.array_equal(np.isnan(best_b), nan)
    assert np.array_equal(best_b.view(np.int32)[~nan], want_best.view(np.int32)[~nan])


SCORE_SHAPES = [(1, 1, 2, 1, 1), (2, 3, 7, 2, 2), (63, 4, 40, 10, 2), (64, 64, 7, 10, 33), (65, 65, 2, 2, 2),
                (257, 256, 256, 1, 2), (1000, 1, 7, 10, 33), (1000, 64, 40, 10, 2), (1000, 256, 40, 2, 33)]


@pytest.mark.parametrize("n,Hd,C,steps,B", SCORE_SHAPES)
def test_scores_coefficients_and_selection(n, Hd, C, steps, B):
    check_scores(make_inputs(n, Hd, C, B, seed=n + Hd + 1), steps, topk=10)      # topk > n at n = 1, 2


@pytest.mark.parametrize("topk", [1, 8, 10, 32])
def test_selection_topk_and_grids(topk):
    for n, Hd, B in ((20, 3, 2), (1000, 16, 5)):              # topk = 32 > n = 20
        Q = make_inputs(n, Hd, 4, B, seed=topk)
        steps = 2
        _, state = run_path(Q, steps)
        g = np.random.default_rng(topk).standard_normal((B, 6, 4)).astype(np.float32)
        first = None
        for nwg in (0, 1, 2, 7, 256):
            ids, best, scores = run_scores(Q, steps, g, state, topk, n_workgroups=nwg, coeffs=False)
            for b in range(B):
                check_selection(scores[b], ids[b], best[b], topk)
            if first is None:
                first = (ids, best, scores)
            else:                                             # the same bits on every grid
                assert np.array_equal(ids, first[0])
                assert np.array_equal(best.view(np.int32), first[1].view(np.int32))
                assert np.array_equal(scores.view(np.int32), first[2].view(np.int32))
        ids2, best2 = run_scores(Q, steps, g, state, topk, scores=False, coeffs=False)      # scores NULL
        assert np.array_equal(ids2, first[0]) and np.array_equal(best2.view(np.int32), first[1].view(np.int32))
        if topk > n:
            assert (first[0][:, n:] == -1).all() and np.isneginf(first[1][:, n:]).all()
            assert (np.sort(first[0][:, :n], axis=1) == np.arange(n)).all()


def test_selection_ties_go_by_the_smaller_index_and_misaligned_z():
    Q = make_inputs(300, 16, 4, 2, seed=3)
    for k in ("z", "h"):                                      # every row a copy of row 0: two scores per target
        Q[k][:] = Q[k][0]
    Q["zsum"], Q["hsum"] = Q["z"].astype(np.float64).sum(0), Q["h"].astype(np.float64).sum(0)
    for offset in (0, 1):
        ids, best, scores = check_scores(Q, 2, topk=8, seed=1, offset=offset)
        for b, t in enumerate(Q["targets"]):
            groups = {}
            for j in range(300):
                if j != int(t):
                    groups.setdefault(scores[b, j].tobytes(), []).append(j)
            assert len(groups) <= 2                           # the entries of row t and the others
            top = max(groups.values(), key=lambda js: scores[b, js[0]])
            assert list(ids[b][:min(8, len(top))]) == top[:8]


def test_selection_a_nan_row_ranks_first_only_where_it_reaches():
    Q = make_inputs(1000, 16, 4, 3, seed=7)
    steps = 2
    _, state = run_path(Q, steps)                             # the sums and the path points stay finite
    free = [j for j in range(1000) if all(j != int(t) and j not in Q["rows"][int(t)] for t in Q["targets"])]
    bad = free[len(free) // 2]
    Q["z"][bad] = np.nan
    g = np.random.default_rng(0).standard_normal((3, 6, 4)).astype(np.float32)
    ids, best, scores, co = run_scores(Q, steps, g, state, 8)
    assert np.isfinite(co).all()
    for b in range(3):
        assert np.isnan(scores[b, bad]) and np.isnan(scores[b]).sum() == 1
        assert ids[b, 0] == bad and np.isnan(best[b, 0]) and not np.isnan(best[b, 1:]).any()
        check_selection(scores[b], ids[b], best[b], 8)


# ------------------------------------------------------------------------------------------------ Calib_IGA
def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def case(name):
    if name not in _cases:
        with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as d:
            c = {k: d[k] for k in d.files}
        c["meta"] = manifest()["cases"][name]
        _cases[name] = c
    return _cases[name]


def gcn_of(c):
    if "gcn" not in c:
        P = {k[3:]: torch.from_numpy(v) for k, v in c.items() if k.startswith("p__")}
        m = SparseCompatibleGCN(c["x"].shape[1], nclass=P["gc2.weight"].shape[0], nhid=P["gc1.weight"].shape[0])
        m.load_state_dict(P)
        c["gcn"] = m.to(DEV).eval()
    return c["gcn"]


def wats_of(c):
    if "wats" not in c:
        with contextlib.redirect_stdout(io.StringIO()):
            w = wats_hip.WATS(gcn_of(c), torch.from_numpy(c["x"]), torch.from_numpy(c["y"]), torch.from_numpy(c["adj"]),
                              torch.from_numpy(c["val_mask"]), wavelet_feats=c["wats_feats"], verbose=False)
        w.net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in c.items() if k.startswith("w__")})
        c["wats"] = w.eval()
    return c["wats"]


def all_runs():
    return [(name, r["run"]) for name in sorted(manifest()["cases"]) for r in manifest()["cases"][name]["runs"]]


@pytest.mark.parametrize("name,i", all_runs())
def test_calib_iga_reproduces_the_recorded_run(name, i):
    c = case(name)
    meta = c["meta"]["runs"][i]
    r = {k.split("__", 1)[1]: v for k, v in c.items() if k.startswith(f"r{i}__")}
    surrogate = wats_of(c) if meta["surrogate"] == "WATS" else gcn_of(c)
    x, y = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["y"]).to(DEV)
    adj = torch.from_numpy(c["adj"]).to(DEV)
    as_operator = i % 2 == 1
    atk = Calib_IGA(surrogate, device=DEV)
    kw = dict(n_perturb=[], best_conf=[])
    t = meta["target"]
    with contextlib.redirect_stdout(io.StringIO()) as log:
        atk.attack(x, RowNormalizedAdjacency.from_dense(adj) if as_operator else adj, t, c["meta"]["budget"],
                   meta["strategy"], res_gt=y, steps=meta["steps"], **kw)
    assert log.getvalue() == ""                               # no stray print
    rec = c["meta"]["model_vs_reference"]
    assert atk.flips == [int(j) for j in r["partner"]], (atk.flips, r["partner"])
    assert [s["label"] for s in atk.trace] == [int(v) for v in r["label"]]
    assert kw["n_perturb"] == [int(r["n_perturb"])]
    assert atk.best_flips == [int(j) for j in r["best_set"]]
    d = abs(kw["best_conf"][0] - float(r["best_conf"]))
    print(f"best_conf distance {d:.3e} (tolerance {2 * rec['best_conf']:.3e})")
    assert d <= 2 * rec["best_conf"]
    imp = atk.calc_calibration_importance_edge(x, adj, t, meta["strategy"], steps=meta["steps"])
    assert isinstance(imp, np.ndarray) and imp.shape == (len(adj),) and imp[t] == -10
    others = np.arange(len(adj)) != t
    top = float(np.abs(r["importance"][others]).max())
    ds = float(np.abs(imp - r["importance"])[others].max() / top)
    print(f"{meta['surrogate']} {meta['strategy']} steps {meta['steps']} target {t}: importance distance {ds:.3e} of "
          f"the largest score (tolerance {2 * rec['scores']:.3e})")
    assert ds <= 2 * rec["scores"]
    want = c["adj"].copy()
    for j in r["best_set"]:
        want[t, j] = want[j, t] = 1 - want[t, j]
    if as_operator:                                           # an operator went in: modified_op, no dense matrix
        indptr, indices, values = atk.modified_op.csr()
        M = sp.csr_matrix(want)
        M.sort_indices()
        assert np.array_equal(_np(indptr), M.indptr) and np.array_equal(_np(indices), M.indices)
        with pytest.raises(AttributeError, match="modified_op"):
            atk.modified_adj
    else:
        assert torch.equal(atk.modified_adj.cpu(), torch.from_numpy(want))


def test_attack_many_equals_attack_bit_for_bit():
    for name in sorted(manifest()["cases"]):
        c = case(name)
        x, y = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["y"]).to(DEV)
        op = RowNormalizedAdjacency.from_dense(torch.from_numpy(c["adj"]).to(DEV))
        targets = sorted({r["target"] for r in c["meta"]["runs"]}) + [c["meta"]["runs"][0]["target"]]     # a duplicate
        for surrogate in (gcn_of(c), wats_of(c)):
            for strategy in ("over", "under"):
                atk = Calib_IGA(surrogate, device=DEV)
                many = atk.attack_many(x, op, targets, 10, strategy, y, steps=10)
                assert [m["target"] for m in many] == targets
                model, wats = atk._begin(x, op)
                all_scores = _np(atk._score(model, wats, targets, strategy, 10, 10, return_scores=True)[2])
                for b, (t, m) in enumerate(zip(targets, many)):
                    one = Calib_IGA(surrogate, device=DEV)
                    kw = dict(n_perturb=[], best_conf=[])
                    one.attack(x, op, t, 10, strategy, res_gt=y, **kw)
                    assert one.flips == m["flips"] and one.best_flips == m["best_flips"]
                    assert kw["n_perturb"] == [m["n_perturb"]] and kw["best_conf"] == [m["best_conf"]]
                    assert all(torch.equal(a["logits"], b_["logits"]) for a, b_ in zip(one.trace, m["trace"]))
                    imp = one.calc_calibration_importance_edge(x, op, t, strategy)
                    assert np.array_equal(imp.astype(np.float32).view(np.int32), all_scores[b].view(np.int32))


def test_calib_iga_refuses_what_the_closed_form_does_not_cover():
    c = case("loops120")
    x, y = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["y"]).to(DEV)
    adj = torch.from_numpy(c["adj"]).to(DEV)
    kw = dict(n_perturb=[], best_conf=[])
    atk = Calib_IGA(gcn_of(c), nnodes=len(adj), device=DEV)
    with pytest.raises(ValueError, match="res_gt"):
        atk.attack(x, adj, 3, 2, "under", **kw)
    with pytest.raises(ValueError, match="strategy"):
        atk.attack(x, adj, 3, 2, "sideways", res_gt=y, **kw)
    valued = c["adj"].copy()
    valued[valued > 0] = 0.5
    with pytest.raises(NotImplementedError, match="dense row t"):
        atk.attack(x, torch.from_numpy(valued).to(DEV), 3, 2, "under", res_gt=y, **kw)
    val_mask = torch.from_numpy(c["val_mask"]).to(DEV)
    with contextlib.redirect_stdout(io.StringIO()):
        gats = wats_hip.GATS(gcn_of(c), x, y, adj, val_mask, epochs=1, verbose=False).eval()
    with pytest.raises(NotImplementedError, match="dense row t"):
        Calib_IGA(gats, device=DEV).attack(x, adj, 3, 2, "under", res_gt=y, **kw)
    assert kw == dict(n_perturb=[], best_conf=[])
