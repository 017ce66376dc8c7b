"""CPU tests of the random attacks' fixtures (tests/golden/random, tools/gen_golden_random.py) and of the restated
loop (tests/trial_ref.py): the conditions the generator keeps, the loop against every recorded trial, and the
mutants of trial_ref.LOOP_MUTANTS, each rejected by the fixtures and shown on an input outside them."""
import hashlib
import json
import os
import random

import numpy as np
import pytest
import torch

import agg_ref as A
import trial_ref as T

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "random")
FGA = os.path.join(HERE, "golden", "fga")
CASES = ("iso120", "hub96")
MODES = {"structure": (True, False), "features": (False, True), "both": (True, True)}
EVENTS = ("self_loop_removal", "label_reject", "all_fail_step", "feature_accept", "feature_back")
_cache = {}


def manifest():
    if "manifest" not in _cache:
        with open(os.path.join(GOLDEN, "manifest.json")) as f:
            _cache["manifest"] = json.load(f)
    return _cache["manifest"]


def case(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as d:
            c = {k: d[k] for k in d.files}
        with np.load(os.path.join(FGA, name + ".npz"), allow_pickle=False) as d:
            c["adj"] = d["adj"].astype(np.float32)
        c["meta"] = manifest()["cases"][name]
        c["P"] = {k[3:]: v for k, v in c.items() if k.startswith("p__")}
        _cache[name] = c
    return _cache[name]


def run_of(c, i):
    return {k.split("__", 1)[1]: v for k, v in c.items() if k.startswith(f"r{i}__")}


def loop(c, meta, mutant=None):
    """the float64 loop on a recorded run's inputs, cached per (case, run, mutant)"""
    key = (c["meta"]["adjacency"], meta["run"], mutant)
    if key not in _cache:
        structure, features = MODES[meta["mode"]]
        rng = random.Random(meta["seed"])
        res = T.random_loop(c["P"], c["x"], c["adj"], meta["target"], c["meta"]["budget"], meta["strategy"],
                            c["meta"]["max_trials"], rng, structure, features, scale=c["meta"]["scale"], mutant=mutant)
        res["next_random"] = rng.random()
        _cache[key] = res
    return _cache[key]


def signature(res):
    return [(tr["step"], tr["kind"], int(tr["add"]), tr["index"], bool(tr["accepted"])) for tr in res["trials"]]


def recorded(r):
    return list(zip(r["step"].tolist(), r["kind"].tolist(), r["add"].tolist(), r["index"].tolist(),
                    r["accepted"].tolist()))


# ------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("name", CASES)
def test_fixture_files_are_data_and_match_the_manifest(name):
    m = manifest()
    path = os.path.join(GOLDEN, name + ".npz")
    with open(path, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == m["files"][name + ".npz"]["sha256"]
    assert os.path.getsize(path) < max(os.path.getsize(os.path.join(FGA, f)) for f in os.listdir(FGA))
    c = case(name)
    assert sorted(k for k in c if k not in ("adj", "meta", "P")) == m["files"][name + ".npz"]["keys"]
    n = c["adj"].shape[0]
    assert n <= 120 and c["x"].shape == (n, 24) and set(np.unique(c["x"])) <= {0.0, 1.0}
    assert np.array_equal(c["adj"], c["adj"].T) and c["meta"]["budget"] == 5 and c["meta"]["max_trials"] == 50
    assert np.isclose(c["meta"]["scale"], np.log(np.exp(np.float64(c["ts__temperature"][0])) + np.float64(np.float32(1.1))))


@pytest.mark.parametrize("name", CASES)
def test_fixture_conditions(name):
    c = case(name)
    runs = c["meta"]["runs"]
    assert len(runs) >= 12
    assert {r["cls"] for r in runs} == {"Calib_Random", "Calib_RND"}
    assert {r["strategy"] for r in runs} == {"under", "over", "under_kl"} and {r["mode"] for r in runs} == set(MODES)
    worst = c["meta"]["f32_vs_f64"]
    assert worst == {k: max(r["f32_vs_f64"][k] for r in runs) for k in ("logits", "conf")}
    seen = set()
    for meta in runs:
        r, t = run_of(c, meta["run"]), meta["target"]
        better = (lambda a, b: a > b) if meta["strategy"] == "over" else (lambda a, b: a < b)
        label0 = int(r["orig_logits"].argmax())
        best = float(torch.softmax(torch.from_numpy(r["orig_logits"])[None], dim=1)[0, label0])
        row, xrow = c["adj"][t].copy(), c["x"][t].copy()
        last = r["orig_logits"]
        per_step = {}
        for k in range(len(r["kind"])):
            step, kind, add, index = int(r["step"][k]), int(r["kind"][k]), int(r["add"][k]), int(r["index"][k])
            per_step[step] = per_step.get(step, 0) + 1
            conf, label, logits = float(r["conf"][k]), int(r["label"][k]), r["logits"][k]
            assert label == int(logits.argmax())
            tie = np.array_equal(logits, last)
            assert tie == bool(r["tie"][k])
            top2 = np.sort(logits)[-2:]
            assert top2[1] - top2[0] > 100 * worst["logits"], (meta["run"], k)
            if tie:                     # the same numbers summed: the strict comparison rejects it in any precision
                assert conf == best and not r["accepted"][k]
            else:
                assert abs(conf - best) > 100 * worst["conf"], (meta["run"], k, conf, best)
            assert bool(r["accepted"][k]) == (label == label0 and better(conf, best))
            if kind == 0:
                assert add == int(row[index] == 0) and (add == 0 or index != t)
                if not add and index == t:
                    seen.add("self_loop_removal")
            else:
                assert add == int(xrow[index] == 0)
                if xrow[index] != c["x"][t, index]:
                    seen.add("feature_back")
            if label != label0:
                seen.add("label_reject")
            if r["accepted"][k]:
                best, last = conf, logits
                if kind == 0:
                    row[index] = 1 - row[index]
                else:
                    xrow[index] = 1 - xrow[index]
                    seen.add("feature_accept")
            elif per_step[step] == 50:
                seen.add("all_fail_step")
        assert best == float(r["best_conf"]) and int(r["accepted"].sum()) == int(r["n_perturb"])
        assert np.array_equal(xrow, r["features"])
        assert sorted(np.nonzero(row != c["adj"][t])[0].tolist()) == r["toggles"].tolist()
        if not c["adj"][t].any():
            seen.add("isolated_target")
    assert set(EVENTS) <= seen, sorted(set(EVENTS) - seen)
    if name == "iso120":
        assert "isolated_target" in seen


@pytest.mark.parametrize("name", CASES)
def test_the_restated_loop_draws_and_accepts_the_recorded_trials(name):
    c = case(name)
    worst = c["meta"]["f32_vs_f64"]
    for meta in c["meta"]["runs"]:
        r, res = run_of(c, meta["run"]), loop(c, meta)
        assert signature(res) == recorded(r), meta["run"]
        assert res["n_perturb"] == int(r["n_perturb"]) and res["toggles"] == r["toggles"].tolist()
        assert np.array_equal(res["features"].numpy(), r["features"].astype(np.float64))
        assert res["next_random"] == float(r["next_random"])
        d_logits = max(float(np.abs(tr["logits"].numpy() - r["logits"][k]).max()) for k, tr in enumerate(res["trials"]))
        d_conf = max([abs(tr["conf"] - float(r["conf"][k])) for k, tr in enumerate(res["trials"])] +
                     [abs(res["best_conf"] - float(r["best_conf"]))])
        # the float64 loop itself moves in its last bits with the BLAS code path: 1e-6 of the distance, relatively
        assert d_logits <= worst["logits"] * (1 + 1e-6) and d_conf <= worst["conf"] * (1 + 1e-6)
        assert np.isclose(d_logits, meta["f32_vs_f64"]["logits"], rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------ the mutants
def small_input(seed=0):
    """outside the fixtures: 12 nodes, node 0 without any entry, node 1 with its self loop alone, a ring on the rest"""
    rng = np.random.default_rng(seed)
    n = 12
    adj = np.zeros((n, n), np.float32)
    for i in range(2, n):
        adj[i, i] = 1
        j = 2 + (i - 1) % (n - 2)
        adj[i, j] = adj[j, i] = 1
    adj[1, 1] = 1
    x = (rng.random((n, 6)) < 0.4).astype(np.float32)
    P = {"gc1.weight": rng.standard_normal((8, 6)), "gc1.bias": rng.standard_normal(8) * 0.1,
         "gc2.weight": rng.standard_normal((3, 8)), "gc2.bias": rng.standard_normal(3) * 0.1}
    return P, x, adj


def outside(mutant):
    """(right, wrong): the loop and its mutant on an input chosen for the mutant, outside the fixtures"""
    P, x, adj = small_input()
    t, strategy, mode = {"no_self": (5, "under", "structure"), "le": (0, "under", "features"),
                         "no_rewind": (5, "under", "structure"), "always_draw": (0, "under", "structure"),
                         "dz_all_rows": (5, "under", "features"), "no_dz_self": (1, "under", "features")}[mutant]
    out = []
    for mu in (None, mutant):
        rng = random.Random(4)
        res = T.random_loop(P, x, adj, t, 3, strategy, 20, rng, *MODES[mode], scale=1.3, mutant=mu)
        res["next_random"] = rng.random()
        out.append(res)
    return out


def differs(a, b):
    return (signature(a) != signature(b) or a["next_random"] != b["next_random"] or a["best_conf"] != b["best_conf"] or
            a["toggles"] != b["toggles"] or not torch.equal(a["features"], b["features"]))


@pytest.mark.parametrize("mutant", T.LOOP_MUTANTS)
def test_mutants_are_rejected_by_the_fixtures_and_outside_them(mutant):
    rejected = []
    for name in CASES:
        c = case(name)
        for meta in c["meta"]["runs"]:
            r, res = run_of(c, meta["run"]), loop(c, meta, mutant)
            worst = c["meta"]["f32_vs_f64"]
            off = (signature(res) != recorded(r) or res["next_random"] != float(r["next_random"]) or
                   abs(res["best_conf"] - float(r["best_conf"])) > 4 * worst["conf"] or
                   any(np.abs(tr["logits"].numpy() - r["logits"][k]).max() > 4 * worst["logits"]
                       for k, tr in enumerate(res["trials"])))
            if off:
                rejected.append((name, meta["run"]))
    print(f"{mutant}: rejected by {len(rejected)} recorded runs")
    assert rejected, f"no recorded run rejects the mutant {mutant}"
    right, wrong = outside(mutant)
    assert differs(right, wrong), f"{mutant} shows no difference on the small input"


def test_trial_truth_agrees_with_its_second_evaluation_and_the_target_truth():
    import attack_ref as R
    rng = np.random.default_rng(1)
    c = case("hub96")
    import scipy.sparse as sp
    M = sp.csr_matrix(c["adj"])
    M.sort_indices()
    n = M.shape[0]
    z, W1 = A.signal(n, 7, "normal", 1), A.signal(7, 24, "normal", 2, spread=1.0)
    b1, W2, b2 = rng.standard_normal(7).astype(np.float32), A.signal(3, 7, "normal", 3, spread=1.0), \
        rng.standard_normal(3).astype(np.float32)
    ref = T.trial_logits(M.indptr, M.indices, z, b1, W2, b2, 6, [0, 6, 65], W1, [(3, 1.0), (9, -1.0)])
    assert ref.agreement() <= A.TRUTH_AGREE
    plain = T.trial_logits(M.indptr, M.indices, z, b1, W2, b2, 6, [0, 65])
    want = R.target_logits(M.indptr, M.indices, z, b1, W2, b2, 6, [0, 65])
    assert np.array_equal(plain.truth, want.truth) and np.array_equal(plain.unit, want.unit)
    # the feature deltas as a change of z_t: the same truth from the plain expression on the changed z
    z2 = z.astype(np.float64).copy()
    z2[6] += 1.0 * W1[:, 3].astype(np.float64) - 1.0 * W1[:, 9].astype(np.float64)
    dense = c["adj"].astype(np.float64).copy()
    for j in (0, 65):
        dense[6, j] = dense[j, 6] = 1 - dense[6, j]
    dense[6, 6] = 1 - dense[6, 6]
    deg = dense.sum(1, keepdims=True)
    an = dense / np.where(deg == 0, 1, deg)
    h = np.maximum(an @ z2 + b1, 0)
    out = (an @ h)[6] @ W2.astype(np.float64).T + b2
    assert np.abs(out - ref.truth).max() <= 1e-12 * np.abs(out).max()
