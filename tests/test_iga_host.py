"""CPU tests of the integrated-gradient scores (tests/iga_ref.py, tests/golden/iga, the argument checks of
csrc/iga.hip): the closed form against the reference's loop restated with dense autograd, the fixtures' conditions,
and mutants of the closed form that the fixtures tell apart."""
import json
import os

import numpy as np
import pytest
import torch

import iga_ref as I
import wats_hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iga")
_cases = {}


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def case(name):
    if name not in _cases:
        with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as d:
            c = {k: d[k] for k in d.files}
        c["meta"] = manifest()["cases"][name]
        c["P"] = {k[3:]: v for k, v in c.items() if k.startswith("p__")}
        _cases[name] = c
    return _cases[name]


def all_runs():
    return [(name, r["run"]) for name in sorted(manifest()["cases"]) for r in manifest()["cases"][name]["runs"]]


def run_of(name, i):
    c = case(name)
    meta = c["meta"]["runs"][i]
    r = {k.split("__", 1)[1]: v for k, v in c.items() if k.startswith(f"r{i}__")}
    temps = c["wats_temps"] if meta["surrogate"] == "WATS" else None
    return c, meta, r, temps


def small_graph(seed):
    rng = np.random.default_rng(seed)
    n, nf, Hd, C = int(rng.integers(6, 30)), 5, int(rng.integers(1, 8)), int(rng.integers(2, 6))
    adj = (rng.random((n, n)) < 0.25).astype(np.float64)
    adj = np.maximum(adj, adj.T)
    np.fill_diagonal(adj, seed % 2)                           # both conventions
    adj[:, 2] = 1
    adj[2, :] = 1                                             # row 2: every entry, the self entry included
    adj[1, :] = 0                                             # row 1: no entry (the model reads rows: column 1 stays)
    adj[3, 3] = 1                                             # node 3: a self entry in either convention
    P = {"gc1.weight": rng.standard_normal((Hd, nf)), "gc1.bias": rng.standard_normal(Hd),
         "gc2.weight": rng.standard_normal((C, Hd)), "gc2.bias": rng.standard_normal(C)}
    temps = rng.uniform(0.5, 2.0, n) if seed % 3 == 0 else None
    return P, rng.standard_normal((n, nf)), adj, temps


@pytest.mark.parametrize("seed", range(24))
def test_closed_form_equals_the_dense_autograd_restatement(seed):
    P, x, adj, temps = small_graph(seed)
    n = len(adj)
    for t in (0, 1, 2, 3, n - 1):                             # 1 isolated, 2 a complete row, 3 a self entry
        for strategy, steps in (("over", 10), ("under", 3), ("under", 1)):
            s, aux = I.importance(P, x, adj, t, strategy, steps, temp=None if temps is None else temps[t])
            d, logits = I.dense_importance(P, x, adj, t, strategy, steps, temps=temps)
            scale = max(float(np.abs(d[np.arange(n) != t]).max()), 1e-300)
            assert np.abs(s - d).max() <= 1e-12 * scale, (seed, t, strategy, steps, np.abs(s - d).max() / scale)
            assert s[t] == -10.0 and d[t] == -10.0
            if temps is None:
                assert np.abs(logits - aux["state"]["logits"]).max() <= 1e-12 * max(1.0, np.abs(logits).max())
    # the kernel's model (float32 z and h, np.longdouble sums) is the same expression
    Z, H = I.first_layer(P, x, adj)
    Z32, H32 = Z.astype(np.float32), H.astype(np.float32)
    cols = np.flatnonzero(adj[2])
    pts = I.path_points(cols, n, 2, 3, Z32, H32, Z32.astype(np.float64).sum(0), H32.astype(np.float64).sum(0),
                        P["gc1.bias"].astype(np.float32), P["gc2.weight"].astype(np.float32),
                        P["gc2.bias"].astype(np.float32))
    assert np.allclose(pts["deg"][4:], n) and np.allclose(pts["w_t"][4:], 1.0)     # a full row: all ones at every lambda
    cols = np.flatnonzero(adj[1])
    pts = I.path_points(cols, n, 1, 3, Z32, H32, Z32.astype(np.float64).sum(0), H32.astype(np.float64).sum(0),
                        P["gc1.bias"].astype(np.float32), P["gc2.weight"].astype(np.float32),
                        P["gc2.bias"].astype(np.float32))
    assert not pts["deg"][:4].any() and not pts["p"][:4].any() and pts["deg"][7] == 0     # the zero row


def test_fixture_files_are_the_recorded_ones():
    import hashlib
    m = manifest()
    assert sum(len(c["runs"]) for c in m["cases"].values()) >= 24
    for name, info in m["files"].items():
        with open(os.path.join(GOLDEN, name), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == info["sha256"], name
    seen = {(c["loops"], r["steps"], r["strategy"], r["surrogate"]) for c in m["cases"].values() for r in c["runs"]}
    assert {k[0] for k in seen} == {True, False} and {k[1] for k in seen} == {3, 10}
    assert {k[2] for k in seen} == {"over", "under"} and {k[3] for k in seen} == {"GCN", "WATS"}


@pytest.mark.parametrize("name,i", all_runs())
def test_every_fixture_meets_its_conditions(name, i):
    c, meta, r, temps = run_of(name, i)
    budget = c["meta"]["budget"]
    ok, why = I.fixture_conditions(c["P"], c["x"], c["adj"], meta["target"], meta["strategy"], meta["steps"], temps,
                                   r["importance"], budget)
    assert ok is not None, why
    loop = ok["loop"]
    assert loop["partners"] == [int(j) for j in r["partner"]] and loop["labels"] == [int(v) for v in r["label"]]
    assert loop["n_perturb"] == int(r["n_perturb"]) and loop["best_set"] == [int(j) for j in r["best_set"]]
    assert loop["original_label"] == int(r["original_label"])
    # the measured distance of the closed form on float32 Z / H from the recorded reference
    s32, _ = I.importance(c["P"], c["x"], c["adj"], meta["target"], meta["strategy"], meta["steps"],
                          temp=None if temps is None else float(temps[meta["target"]]), dtype=np.float32)
    others = np.arange(len(s32)) != meta["target"]
    d = float(np.abs(s32 - r["importance"])[others].max() / ok["top"])
    print(f"{name} run {i}: closed form against the recorded float32 reference {d:.3e} of the largest score; "
          f"best_conf {abs(loop['best_conf'] - float(r['best_conf'])):.3e}")
    assert d <= c["meta"]["model_vs_reference"]["scores"] * (1 + 1e-6) + 1e-12
    assert abs(loop["best_conf"] - float(r["best_conf"])) <= c["meta"]["model_vs_reference"]["best_conf"] * (1 + 1e-6) + 1e-12


@pytest.mark.parametrize("mutant", I.MUTANTS)
def test_mutants_land_outside_a_fixture(mutant):
    """outside: further from the recorded importance than the GPU tests allow (twice the measured distance)"""
    caught = []
    for name, i in all_runs():
        c, meta, r, temps = run_of(name, i)
        t = meta["target"]
        if mutant == "row_col":
            s, _ = I.dense_importance(c["P"], c["x"], c["adj"], t, meta["strategy"], meta["steps"], temps=temps,
                                      mutant=mutant)
        else:
            s, _ = I.importance(c["P"], c["x"], c["adj"], t, meta["strategy"], meta["steps"],
                                temp=None if temps is None else float(temps[t]), mutant=mutant)
        others = np.arange(len(s)) != t
        top = float(np.abs(r["importance"][others]).max())
        d = float(np.abs(s - r["importance"])[others].max() / top)
        if d > 2 * c["meta"]["model_vs_reference"]["scores"]:
            caught.append((name, i, d))
    print(f"{mutant}: outside {len(caught)} of {len(all_runs())} fixtures")
    assert caught


def test_abi_checks_arguments_before_any_device_work():
    lib = wats_hip._lib.load()
    assert lib.wg_iga_max_topk() >= 32
    nbytes = wats_hip._lib.c_i64(0)
    assert lib.wg_iga_scores_workspace(4, 16, None) == -1 and lib.wg_iga_scores_workspace(0, 16, nbytes) == -1
    assert lib.wg_iga_scores_workspace(4, 16, nbytes) == 0 and nbytes.value > 0
    p = [4096 + 256 * q for q in range(20)]
    path = lib.wg_iga_path_logits
    #    n   nnz indptr indices Hd z     h     zsum  hsum  b1    W2    b2    C  B  targets steps logits state stream
    ok = [9, 20, p[0], p[1], 16, p[2], p[3], p[4], p[5], p[6], p[7], p[8], 5, 2, p[9], 10, p[10], p[11], None]
    for pos, v, code in ((0, 0, -1), (0, 2 ** 31, -4), (1, 2 ** 31, -4), (4, 0, -1), (4, 257, -4), (12, 257, -4), (13, 0, -1),
                         (15, 0, -1), (15, 5000, -4), (2, None, -1), (3, None, -1), (5, None, -1), (6, None, -1),
                         (7, None, -1), (8, None, -1), (14, None, -1), (16, None, -1), (17, None, -1), (17, p[11] + 4, -1)):
        args = list(ok)
        args[pos] = v
        assert path(*args) == code, (pos, v, lib.wg_last_error())
    sc = lib.wg_iga_scores
    #    n   nnz indptr indices Hd z     h     b1    W2    C  B  targets steps g     state topk nwg ws    coeffs scores ids   best  stream
    ok = [9, 20, p[0], p[1], 16, p[2], p[3], p[6], p[7], 5, 2, p[9], 10, p[12], p[11], 10, 0, p[13], None, None, p[14], p[15], None]
    for pos, v, code in ((0, 0, -1), (0, 2 ** 31, -4), (4, 257, -4), (9, 0, -1), (10, 0, -1), (12, 0, -1), (15, 0, -1), (15, 33, -1),
                         (16, -1, -1), (16, 513, -1), (17, None, -1), (17, p[13] + 4, -1), (13, None, -1), (14, None, -1),
                         (18, p[16] + 4, -1), (20, None, -1), (21, None, -1), (11, None, -1)):
        args = list(ok)
        args[pos] = v
        assert sc(*args) == code, (pos, v, lib.wg_last_error())
