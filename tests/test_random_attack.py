"""GPU tests of the random attacks (csrc/attack.hip wg_trial_logits, wats_hip/attack.py Calib_Random / Calib_RND).

wg_trial_logits is held to agg_ref.BOUND_ONE in the row unit of tests/trial_ref.trial_logits (one rounding) and to a
repeat's bits, and to wg_target_logits' bits on everything that entry accepts.  The classes reproduce every run the
reference recorded (tests/golden/random): the accepted trials, n_perturb, the final toggle set, the final feature row
and the position of the random stream exactly, best_conf and every trial's output row within 4 x the manifest's
float32-vs-float64 distance (the rule of tests/test_attack.py), with the batched launch and through the views."""
import contextlib
import io
import json
import os
import random

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

import agg_ref as A  # noqa: E402
import trial_ref as T  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip import (Calib_Random, Calib_RND, RowNormalizedAdjacency, SparseCompatibleGCN, target_logits,  # noqa: E402
                      trial_logits)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "random")
FGA = os.path.join(HERE, "golden", "fga")
DEV = "cuda"
_cases = {}
_worst = {"c": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()
    yield
    print(f"wg_trial_logits: worst c over this module = {_worst['c']:.4f} (bound {A.BOUND_ONE})")


def _np(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


# ------------------------------------------------------------------------------------------------ graphs
def csr_of(rows):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.array([c for r in rows for c in r], np.int32), len(rows)


def star(leaves):
    """node 0 joined to `leaves` leaves, every node with its self loop"""
    n = leaves + 1
    return csr_of([[0] + list(range(1, n))] + [[0, j] for j in range(1, n)])


def path_without_loops():
    """0 - 1 - 2 - 3 - 4 and a node 5 with no entry, no self loops"""
    return csr_of([[1], [0, 2], [1, 3], [2, 4], [3], []])


def lone_loops():
    """node 0 with its self loop alone, 1 - 2 with self loops, node 3 without any entry"""
    return csr_of([[0], [1, 2], [1, 2], []])


def two_nodes():
    return csr_of([[0, 1], [0, 1]])


def directed():
    """row 0 holds 1, 2 and its loop; row 1 holds 0; row 2 does not hold 0 (t = 0 is not in N(2)); row 3 holds 0"""
    return csr_of([[0, 1, 2], [0, 1], [2, 3], [0, 3]])


def fga_csr(name):
    with np.load(os.path.join(FGA, name + ".npz"), allow_pickle=False) as d:
        M = sp.csr_matrix(d["adj"])
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int32), M.shape[0]


def inputs(n, Hd, C, kind, seed, nfeat=24):
    rng = np.random.default_rng(seed)
    return dict(z=A.signal(n, Hd, kind, seed), b1=rng.standard_normal(Hd).astype(np.float32),
                W2=A.signal(C, Hd, kind, seed + 1, spread=1.0), b2=rng.standard_normal(C).astype(np.float32),
                W1=A.signal(Hd, nfeat, kind, seed + 2, spread=1.0))


def run_trials(graph, I, trials, offset=0, with_w1=True):
    indptr, indices, n = graph
    z = dev(I["z"])
    if offset:
        buf = torch.empty(z.numel() + offset, device=DEV)
        buf[offset:] = z.reshape(-1)
        z = buf[offset:].view_as(z)
    out = trial_logits(n, dev(indptr), dev(indices), z, dev(I["b1"]), dev(I["W2"]), dev(I["b2"]), trials,
                       W1=dev(I["W1"]) if with_w1 else None)
    torch.cuda.synchronize()
    return _np(out)


def check_trials(graph, trials, Hd, C, kind, what, nfeat=24, offset=0, seed=3):
    indptr, indices, n = graph
    I = inputs(n, Hd, C, kind, seed, nfeat)
    got = run_trials(graph, I, trials, offset)
    again = run_trials(graph, I, trials, offset)
    assert same_bits(got, again), f"{what}: a repeat gives other bits"
    worst = 0.0
    for b, (t, S, feats) in enumerate(trials):
        ref = T.trial_logits(indptr, indices, I["z"], I["b1"], I["W2"], I["b2"], t, S, I["W1"],
                             sorted((feats or {}).items()))
        c = ref.c(got[b], f"{what} trial {b}")
        worst = max(worst, c)
        assert c <= A.BOUND_ONE, (what, b, t, S, feats, c)
    _worst["c"] = max(_worst["c"], worst)
    print(f"{what} Hd={Hd} C={C} {kind}: c = {worst:.4f} (bound {A.BOUND_ONE})")
    return got, I


FEATS = {3: 1.0, 7: -1.0, 23: 0.5}
GRAPH_CASES = {
    # name: (graph, trials (t, S, feats))
    "star_hub": (lambda: star(300), [(0, [], None), (0, [5], FEATS), (0, [0, 5, 17, 299], None), (0, [0], FEATS)]),
    "star_leaf": (lambda: star(300), [(7, [], FEATS), (7, [3], None), (7, [0], FEATS), (7, [0, 3, 7, 9], FEATS)]),
    "iso_isolated": (lambda: fga_csr("iso120"), [(17, [], FEATS), (17, [3], FEATS), (17, [3, 16, 17], None)]),
    "iso_hub_neighbour": (lambda: fga_csr("iso120"), [(48, [], None), (48, [48, 84, 94], FEATS), (48, [16], FEATS)]),
    "hub96_degree_one": (lambda: fga_csr("hub96"), [(6, [], FEATS), (6, [0, 6, 65], None), (6, [6], FEATS)]),
    "hub96_hub": (lambda: fga_csr("hub96"), [(0, [0], FEATS), (0, [50], None), (0, [1, 2, 3, 4, 5], FEATS)]),
    "path_last_neighbour": (lambda: path_without_loops(), [(0, [1], FEATS), (0, [1, 2], None), (0, [0], FEATS),
                                                            (4, [5], None)]),     # a partner j = n - 1
    "lone_loops": (lambda: lone_loops(), [(0, [0], FEATS), (0, [], FEATS), (3, [], FEATS), (3, [3], FEATS),
                                          (1, [1, 3], None)]),
    "two_nodes": (lambda: two_nodes(), [(0, [], FEATS), (1, [0], FEATS), (1, [0, 1], FEATS), (0, [0], None)]),
    "directed": (lambda: directed(), [(0, [], FEATS), (0, [2], FEATS), (0, [3], FEATS), (0, [0, 1], FEATS)]),
}


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("name", sorted(GRAPH_CASES))
def test_trial_logits_one_rounding_on_every_graph(name, kind):
    make, trials = GRAPH_CASES[name]
    graph = make()
    for Hd, C in ((64, 40), (7, 3)):
        got, I = check_trials(graph, trials, Hd, C, kind, name)
    if name == "path_last_neighbour":      # no neighbour left: deg' 0 -> 1, y2 = 0, out = b2, and dz reaches nothing
        assert np.array_equal(got[0], I["b2"])
    if name == "lone_loops":
        assert np.array_equal(got[0], I["b2"])                   # the only entry, the self loop, removed
        assert np.array_equal(got[2], I["b2"])                   # no self loop and no neighbour: dz must not reach out
        assert not np.array_equal(got[3], I["b2"])               # the self loop added: z_t + dz is gathered
        no_dz = run_trials(graph, I, [(0, [], None), (3, [3], None)])
        assert not same_bits(got[1], no_dz[0]) and not same_bits(got[3], no_dz[1])
    if name == "directed":                  # t = 0 is not in N(2): row 2 carries no dz; flipping (0, 2) puts it there
        indptr, indices, n = graph
        ref = T.trial_logits(indptr, indices, I["z"], I["b1"], I["W2"], I["b2"], 0, [], I["W1"], sorted(FEATS.items()))
        assert ref.c(got[0]) <= A.BOUND_ONE


@pytest.mark.parametrize("Hd", [1, 3, 4, 64, 65, 256])
def test_trial_logits_hidden_widths(Hd):
    check_trials(star(300), [(7, [0, 3, 7], FEATS), (0, [], FEATS), (0, [0, 9], None)], Hd, 3, "positive", "star")
    check_trials(fga_csr("hub96"), [(1, [1, 50, 77], FEATS), (6, [], None)], Hd, 3, "normal", "hub96")


@pytest.mark.parametrize("C", [1, 3, 40, 41, 256])
def test_trial_logits_class_counts(C):
    check_trials(fga_csr("hub96"), [(1, [50, 77], FEATS), (1, [1, 11], None), (0, [0], FEATS)], 16, C, "spread", "hub96")


def random_trials(n, B, seed, nfeat=24, targets=None):
    rng = np.random.default_rng(seed)
    trials = []
    for _ in range(B):
        t = int(rng.integers(0, n)) if targets is None else int(rng.choice(targets))
        S = sorted(int(j) for j in rng.choice(n, rng.integers(0, 6), replace=False))
        feats = {int(f): float(rng.choice([-1.0, 1.0, 0.5])) for f in rng.choice(nfeat, rng.integers(0, 4), replace=False)}
        trials.append((t, S, feats or None))
    return trials


@pytest.mark.parametrize("B", [1, 3, 64, 257])
def test_trial_logits_batches(B):
    graph = fga_csr("iso120")
    trials = random_trials(graph[2], B, B)
    trials[0] = (trials[0][0], [], None)
    ref_every = 1 if B <= 64 else 8               # the float128 truth of every 8th trial of the largest batch
    indptr, indices, n = graph
    I = inputs(n, 16, 5, "normal", 3)
    got = run_trials(graph, I, trials)
    assert same_bits(got, run_trials(graph, I, trials))
    worst = 0.0
    for b in range(0, B, ref_every):
        t, S, feats = trials[b]
        ref = T.trial_logits(indptr, indices, I["z"], I["b1"], I["W2"], I["b2"], t, S, I["W1"],
                             sorted((feats or {}).items()))
        worst = max(worst, ref.c(got[b], f"B={B} trial {b}"))
    _worst["c"] = max(_worst["c"], worst)
    print(f"B={B}: c = {worst:.4f}")
    assert worst <= A.BOUND_ONE
    if B > 64:                                     # every trial alone: the same bits as in the batch
        for b in range(B):
            if b % ref_every:
                assert same_bits(run_trials(graph, I, [trials[b]])[0], got[b]), b


def test_trial_logits_interleaved_targets_duplicates_and_t_in_the_set():
    graph = fga_csr("hub96")
    n = graph[2]
    I = inputs(n, 64, 40, "normal", 5)
    per_target = {t: random_trials(n, 7, 10 + t, targets=[t]) for t in (0, 6, 50)}
    for t, tr in per_target.items():               # t first / in the middle / alone in S_b
        tr[0] = (t, sorted({t, 60, 70}), FEATS)
        tr[1] = (t, sorted({1, t, 95}), None)
        tr[2] = (t, [t], FEATS)
        tr[3] = tr[0]                              # a duplicated trial
    single = {t: run_trials(graph, I, tr) for t, tr in per_target.items()}
    mixed = [per_target[t][k] for k in range(7) for t in (0, 6, 50)]
    got = run_trials(graph, I, mixed)
    for k in range(7):
        for i, t in enumerate((0, 6, 50)):
            assert same_bits(got[3 * k + i], single[t][k]), (t, k)
    for t in (0, 6, 50):
        assert same_bits(single[t][0], single[t][3])
    check_trials(graph, mixed, 64, 40, "normal", "interleaved", seed=5)


@pytest.mark.parametrize("nfeat", [1, 24])
def test_trial_logits_features(nfeat):
    graph = fga_csr("iso120")
    last = nfeat - 1
    trials = [(48, [], {0: 1.0}), (48, [], None), (48, [16], {last: -1.0}), (48, [], {0: 0.0}),     # empty, delta 0
              (3, [3], {0: 1.0}), (17, [17], {last: 1.0}), (17, [], {0: 1.0})]
    got, I = check_trials(graph, trials, 64, 5, "normal", f"nfeat={nfeat}", nfeat=nfeat)
    assert same_bits(got[3], got[1])               # a delta of 0 (a feature flipped and flipped back) is no delta
    assert not same_bits(got[0], got[1])
    assert np.array_equal(got[6], I["b2"])         # node 17 has no entry at all: dz reaches nothing
    if nfeat > 1:                                  # deltas that cancel in the sum: +1 and -1 on one column of W1
        I["W1"][:, 1] = I["W1"][:, 0]
        a = run_trials(graph, I, [(48, [], {0: 1.0, 1: -1.0}), (48, [], None)])
        assert same_bits(a[0], a[1])


def test_trial_logits_misaligned_z_and_null_features():
    graph = fga_csr("hub96")
    trials = [(1, [1, 50], FEATS), (6, [], None), (0, [0, 3], FEATS)]
    check_trials(graph, trials, 64, 5, "normal", "z off by one float", offset=1)
    plain = [(t, S, None) for t, S, _ in trials]
    I = inputs(graph[2], 64, 5, "normal", 3)
    a = run_trials(graph, I, plain, with_w1=False)             # feat_ptr and W1 NULL
    b = run_trials(graph, I, plain, offset=1, with_w1=False)
    for k, (t, S, _) in enumerate(plain):
        ref = T.trial_logits(graph[0], graph[1], I["z"], I["b1"], I["W2"], I["b2"], t, S)
        assert ref.c(a[k]) <= A.BOUND_ONE and ref.c(b[k]) <= A.BOUND_ONE


def test_trial_logits_nan_outside_the_ball_stays_outside():
    indptr, indices, n = graph = path_without_loops()
    I = inputs(n, 8, 3, "normal", 3)
    I["z"][4] = np.nan                              # three hops from node 0, and node 5 has no entry
    I["z"][5] = np.nan
    got = run_trials(graph, I, [(0, [], FEATS), (0, [2], FEATS), (1, [1], None)])
    assert np.isfinite(got).all()
    I["z"][4] = np.inf                              # the kernel's max(., 0) drops a NaN; an infinity shows a gather
    assert np.isfinite(run_trials(graph, I, [(0, [], FEATS), (0, [2], FEATS), (1, [1], None)])).all()
    assert not np.isfinite(run_trials(graph, I, [(2, [], None)])).any()     # row 3 of this ball gathers z_4


def test_trial_logits_equals_target_logits_bit_for_bit():
    for name, (make, trials) in sorted(GRAPH_CASES.items()):
        graph = make()
        indptr, indices, n = graph
        for Hd, C in ((64, 40), (7, 3)):
            I = inputs(n, Hd, C, "normal", 3)
            for t in sorted({tr[0] for tr in trials}):
                cands = [[j for j in S if j != t] for tt, S, _ in trials if tt == t] + [[]]
                want = _np(target_logits(n, dev(indptr), dev(indices), dev(I["z"]), dev(I["b1"]), dev(I["W2"]),
                                         dev(I["b2"]), t, cands))
                got = run_trials(graph, I, [(t, S, None) for S in cands], with_w1=False)
                assert same_bits(got, want), (name, t, Hd)


def test_trial_logits_refuses_bad_arguments():
    lib = wats_hip._lib.load()
    indptr, indices, n = fga_csr("hub96")
    I = inputs(n, 16, 5, "normal", 3)
    d = {k: dev(v) for k, v in I.items()}
    ip, ix = dev(indptr), dev(indices)
    tt = dev(np.array([1, 6], np.int32))
    cp, ci = dev(np.array([0, 1, 1], np.int32)), dev(np.array([50], np.int32))
    fp, fi, fd = dev(np.array([0, 1, 1], np.int32)), dev(np.array([3], np.int32)), dev(np.array([1.0], np.float32))
    out = torch.empty((2, 5), device=DEV)
    p = wats_hip._lib.ptr
    ok = [n, len(indices), p(ip), p(ix), 16, p(d["z"]), p(d["b1"]), p(d["W2"]), p(d["b2"]), 5, 2, p(tt), p(cp), p(ci), 24,
          p(d["W1"]), p(fp), p(fi), p(fd), p(out), None]
    assert lib.wg_trial_logits(*ok) == 0
    invalid = [(0, 0), (1, -1), (2, None), (3, None), (4, 0), (5, None), (6, None), (7, None), (8, None), (9, 0), (10, 0),
               (11, None), (12, None), (14, 0), (15, None), (17, None), (18, None), (19, None)]
    for pos, v in invalid:
        args = list(ok)
        args[pos] = v
        assert lib.wg_trial_logits(*args) == -1, (pos, v)       # WG_ERR_INVALID
    for pos, v in ((4, 257), (9, 257), (0, 2 ** 31), (1, 2 ** 31), (10, 2 ** 31), (14, 2 ** 31)):
        args = list(ok)
        args[pos] = v
        assert lib.wg_trial_logits(*args) not in (0, -1), (pos, v)   # WG_ERR_UNSUPPORTED
    args = list(ok)                                              # no feature trial: W1, ids, deltas and nfeat unread
    args[14:19] = [0, None, None, None, None]
    assert lib.wg_trial_logits(*args) == 0
    torch.cuda.synchronize()
    z = d["z"]
    for bad in ([(n, [], None)], [(0, [3, 3], None)], [(0, [5, 4], None)], [(0, [n], None)], [(0, [], {24: 1.0})]):
        with pytest.raises(ValueError):
            trial_logits(n, ip, ix, z, d["b1"], d["W2"], d["b2"], bad, W1=d["W1"])
    with pytest.raises(ValueError):
        trial_logits(n, ip, ix, z, d["b1"], d["W2"], d["b2"], [(0, [], {1: 1.0})])     # features without W1


# ------------------------------------------------------------------------------------------------ the classes
def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def case(name):
    if name not in _cases:
        with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as d:
            c = {k: d[k] for k in d.files}
        with np.load(os.path.join(FGA, name + ".npz"), allow_pickle=False) as d:
            c["adj"] = d["adj"].astype(np.float32)
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


def ts_of(c):
    if "ts" not in c:
        x, y, adj = (torch.from_numpy(c[k]).to(DEV) for k in ("x", "y", "adj"))
        cal = wats_hip.TemperatureScaling(gcn_of(c), x, y, adj, torch.from_numpy(c["val_idx"]).to(DEV), verbose=False,
                                          epochs=1, frozen_logits=True)
        with torch.no_grad():
            cal.temperature.copy_(torch.from_numpy(c["ts__temperature"]).to(DEV))
        c["ts"] = cal.eval()
    return c["ts"]


def all_runs():
    return [(name, r["run"]) for name in ("iso120", "hub96") for r in manifest()["cases"][name]["runs"]]


def run_of(c, i):
    return {k.split("__", 1)[1]: v for k, v in c.items() if k.startswith(f"r{i}__")}


def attack_fixture(name, i, local_eval, cls=None, adj_kind="dense"):
    c = case(name)
    meta, r = c["meta"]["runs"][i], run_of(c, i)
    cls = cls or {"Calib_Random": Calib_Random, "Calib_RND": Calib_RND}[meta["cls"]]
    structure, features = {"structure": (True, False), "features": (False, True), "both": (True, True)}[meta["mode"]]
    x, adj = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["adj"]).to(DEV)
    if adj_kind == "operator":
        adj = RowNormalizedAdjacency.from_dense(adj)
    atk = cls(ts_of(c), attack_structure=structure, attack_features=features, device=DEV, local_eval=local_eval)
    kw = dict(n_perturb=[], best_conf=[])
    random.seed(meta["seed"])
    atk.attack(x, adj, meta["target"], c["meta"]["budget"], strategy=meta["strategy"],
               max_trials=c["meta"]["max_trials"], **kw)
    return c, meta, r, atk, kw, random.random()


def trials_of(atk):
    kinds = {"edge": 0, "feature": 1}
    return [(s, kinds[d[0]], int(d[1]), int(d[2])) for s, d, _, _, _ in atk.evaluated]


@pytest.mark.parametrize("local_eval", [True, False])
@pytest.mark.parametrize("name,i", all_runs())
def test_random_attacks_reproduce_the_recorded_run(name, i, local_eval):
    c, meta, r, atk, kw, next_random = attack_fixture(name, i, local_eval, adj_kind="operator" if i % 2 else "dense")
    rec = c["meta"]["f32_vs_f64"]
    assert (atk._local is not None) == local_eval
    want = list(zip(r["step"].tolist(), r["kind"].tolist(), r["add"].tolist(), r["index"].tolist()))
    assert trials_of(atk) == want
    accepted = [k for k, ok in enumerate(r["accepted"]) if ok]
    assert [(s["step"], s["index"]) for s in atk.trace] == [(int(r["step"][k]), int(r["index"][k])) for k in accepted]
    assert kw["n_perturb"] == [int(r["n_perturb"])]
    assert atk.best_flips == [int(j) for j in r["toggles"]]
    t = meta["target"]
    assert np.array_equal(_np(atk.modified_features[t]), r["features"])
    assert next_random == float(r["next_random"]), "the random stream is not where the reference left it"
    d = abs(kw["best_conf"][0] - float(r["best_conf"]))
    worst = max([float(np.abs(_np(e[2]).astype(np.float64) - r["logits"][k]).max())
                 for k, e in enumerate(atk.evaluated)] + [0.0])
    print(f"{meta['cls']} {meta['strategy']} {meta['mode']} target {t} local_eval={local_eval}: best_conf distance "
          f"{d:.3e} (tolerance {4 * rec['conf']:.3e}), logits distance {worst:.3e} (tolerance {4 * rec['logits']:.3e})")
    assert d <= 4 * rec["conf"]
    assert worst <= 4 * rec["logits"]
    want_adj = c["adj"].copy()
    for j in r["toggles"]:
        want_adj[t, j] = want_adj[j, t] = 1 - want_adj[t, j]
    M = sp.csr_matrix(want_adj)
    M.sort_indices()
    indptr, indices, _ = atk.modified_op.csr()
    assert np.array_equal(_np(indptr), M.indptr) and np.array_equal(_np(indices), M.indices)
    if i % 2:
        with pytest.raises(AttributeError, match="modified_op"):
            atk.modified_adj
    elif meta["cls"] == "Calib_RND":
        assert sp.issparse(atk.modified_adj) and (atk.modified_adj != M).nnz == 0
    else:
        assert torch.equal(atk.modified_adj.cpu(), torch.from_numpy(want_adj))
    if not len(r["toggles"]) and np.array_equal(r["features"], c["x"][t]):
        assert atk.modified_features.data_ptr() == atk._x_in.data_ptr()      # nothing changed: the input tensor


def test_both_classes_give_the_same_run_from_the_same_seed():
    for name, i in (("iso120", 2), ("hub96", 2)):
        a = attack_fixture(name, i, True, cls=Calib_Random)
        b = attack_fixture(name, i, True, cls=Calib_RND)
        assert trials_of(a[3]) == trials_of(b[3]) and a[4] == b[4] and a[5] == b[5]
        assert a[3].best_flips == b[3].best_flips and a[3].feature_flips == b[3].feature_flips


def test_attack_many_equals_the_single_attacks():
    c = case("hub96")
    x, adj = torch.from_numpy(c["x"]).to(DEV), RowNormalizedAdjacency.from_dense(torch.from_numpy(c["adj"]).to(DEV))
    targets, seeds = [1, 6, 50, 0], [11, 12, 13, 14]
    for cls, mode in ((Calib_Random, (True, True)), (Calib_RND, (True, False))):
        atk = cls(ts_of(c), attack_structure=mode[0], attack_features=mode[1], device=DEV)
        many = atk.attack_many(x, adj, targets, 5, strategy="under", max_trials=50, seed=seeds)
        for t, s, r in zip(targets, seeds, many):
            random.seed(s)
            kw = dict(n_perturb=[], best_conf=[])
            atk.attack(x, adj, t, 5, strategy="under", max_trials=50, **kw)
            assert r["seed"] == s and r["flips"] == atk.flips and r["best_flips"] == atk.best_flips
            assert r["feature_flips"] == atk.feature_flips and [r["n_perturb"]] == kw["n_perturb"]
            assert [r["best_conf"]] == kw["best_conf"]
            assert [(e[0], e[1]) for e in r["evaluated"]] == [(e[0], e[1]) for e in atk.evaluated]
            assert all(torch.equal(a[2], b[2]) for a, b in zip(r["evaluated"], atk.evaluated))
    random.seed(3)                                   # seed=None: one draw of the global stream per target
    first = atk.attack_many(x, adj, targets[:2], 2, max_trials=10)
    random.seed(3)
    assert [random.randrange(2 ** 63) for _ in range(2)] == [r["seed"] for r in first]


def test_a_cagcn_surrogate_takes_the_view_path():
    c = case("iso120")
    x, y, adj = (torch.from_numpy(c[k]).to(DEV) for k in ("x", "y", "adj"))
    cal = wats_hip.CaGCN(gcn_of(c), x, y, adj, torch.arange(0, 120, 3, device=DEV), graph=adj, epochs=2,
                         verbose=False).eval()
    atk = Calib_Random(cal, attack_structure=True, attack_features=True)
    kw = dict(n_perturb=[], best_conf=[])
    random.seed(1)
    atk.attack(x, RowNormalizedAdjacency.from_dense(adj), 48, 3, max_trials=8, **kw)
    assert atk._local is None and len(kw["n_perturb"]) == 1 and 0 <= kw["n_perturb"][0] <= 3
    assert 0.0 < kw["best_conf"][0] <= 1.0 and 1 <= len(atk.evaluated) <= 24


def test_a_flipped_adjacency_as_the_start():
    c, meta, r, atk, kw, _ = attack_fixture("hub96", 0, True)
    t = meta["target"]
    x = torch.from_numpy(c["x"]).to(DEV)
    op = RowNormalizedAdjacency.from_dense(torch.from_numpy(c["adj"]).to(DEV))
    j = next(k for k in range(c["adj"].shape[0]) if k != t and c["adj"][t, k] == 0)
    results = []
    for start in (op.with_flips([t], [j]), op.flipped([t], [j])):     # a view and the operator it stands for
        a = Calib_Random(ts_of(c), device=DEV)
        random.seed(5)
        a.attack(x, start, t, 3, max_trials=20)
        results.append((a.flips, trials_of(a), a.best_flips))
        assert isinstance(a.modified_op, wats_hip.FlippedAdjacency)
    assert results[0] == results[1]


def test_strategy_flags_and_node_injection():
    c = case("hub96")
    x, adj = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["adj"]).to(DEV)
    with pytest.raises(AssertionError, match="cannot be both False"):
        Calib_RND(ts_of(c), attack_structure=False, attack_features=False)
    with pytest.raises(ValueError, match="Unknown strategy"):
        Calib_Random(ts_of(c)).attack(x, adj, 1, 2, strategy="sideways")
    with pytest.raises(NotImplementedError, match="changes n"):
        Calib_RND(ts_of(c)).random_node_injection(x, adj, 1)
    atk = Calib_RND(ts_of(c))
    random.seed(2)
    with contextlib.redirect_stdout(io.StringIO()) as log:
        atk.attack(sp.csr_matrix(c["x"]), sp.csr_matrix(c["adj"]), 1, 2, max_trials=10, verbose=True)   # scipy inputs
    assert "CALIB_RND ATTACK BEGINS" in log.getvalue() and "Strategy: under_kl" in log.getvalue()
    assert sp.issparse(atk.modified_adj)
