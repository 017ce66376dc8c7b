"""CPU tests of the attack step's yardsticks (tests/attack_ref.py), of the fixtures the reference recorded
(tests/golden/fga, tools/gen_golden_fga.py) and of the host side of wats_hip.attack: the manifest's hashes, the
generator's conditions re-checked from the stored arrays, the numpy model of wg_flip_select equal bit for bit to what
the reference's torch composition recorded at every step, the documented model of wg_target_logits inside its bound,
every mutant shown to fail on a fixture or on a bound, and the ABI's argument checks."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import agg_ref as A
import attack_ref as R
import wats_hip
from wats_hip import attack as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fga")
CASES = ("iso120", "hub96")
_cases, _truth = {}, {}


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def case(name):
    if name not in _cases:
        with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as d:
            c = {k: d[k] for k in d.files}
        c["meta"] = manifest()["cases"][name]
        c["P"] = {k[3:]: torch.from_numpy(v) for k, v in c.items() if k.startswith("p__")}
        _cases[name] = c
    return _cases[name]


def runs():
    return [(name, r["run"]) for name in CASES for r in manifest()["cases"][name]["runs"]]


def run_of(name, i):
    c = case(name)
    meta = c["meta"]["runs"][i]
    assert meta["run"] == i
    return c, meta, {k.split("__", 1)[1]: v for k, v in c.items() if k.startswith(f"r{i}__")}


def truth_of(name, i, dtype=torch.float64, select=None):
    key = (name, i, dtype, select)
    if key not in _truth:
        c, meta, _ = run_of(name, i)
        temps = c["wats_temps"] if meta.get("surrogate") == "WATS" else None
        _truth[key] = R.attack_loop(meta["method"], c["P"], c["x"], c["adj"], meta["target"], c["meta"]["budget"],
                                    meta["strategy"], res_gt=c["y"], temps=temps, dtype=dtype, select=select)
    return _truth[key]


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def test_manifest_hashes():
    m = manifest()
    assert sorted(m["files"]) == sorted(c + ".npz" for c in CASES)
    for name, rec in m["files"].items():
        with open(os.path.join(GOLDEN, name), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == rec["sha256"], name
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 200 * 1024
    for name in CASES:
        metas = m["cases"][name]["runs"]
        for role in ("hub_neighbour", "low_degree", "degree_one"):
            got = sorted(r["method"] for r in metas if r["role"] == role)
            assert got == sorted(["attack", "rerank_attack", "rerank_hybridloss_attack", "flip_beam_hybridloss_attack"])
    assert any(r.get("surrogate") == "WATS" for r in m["cases"]["iso120"]["runs"])


def test_fixture_graphs_are_what_the_issue_asks():
    iso, hub = case("iso120"), case("hub96")
    for c in (iso, hub):
        assert np.array_equal(c["adj"], c["adj"].T) and set(np.unique(c["adj"])) == {0.0, 1.0}
    assert iso["adj"].shape == (120, 120) and hub["adj"].shape == (96, 96)
    assert len(iso["isolated"]) and not iso["adj"][iso["isolated"]].any()
    assert hub["adj"].sum(1).max() > 96 // 2                          # the hub: more than half the nodes
    for c in (iso, hub):
        deg = c["adj"].sum(1)
        by_role = {r["role"]: r["target"] for r in c["meta"]["runs"]}
        assert deg[by_role["degree_one"]] - 1 == 1                      # one neighbour and the self loop
        assert 3 <= deg[by_role["low_degree"]] <= 4
        assert c["adj"][int(deg.argmax()), by_role["hub_neighbour"]] == 1


@pytest.mark.parametrize("name,i", runs())
def test_generator_conditions_hold_on_the_stored_arrays(name, i):
    """no case and no step is left out: every step of every run"""
    c, meta, r = run_of(name, i)
    S = len(r["partner"])
    assert S >= 3 and S == meta["steps"]
    truth = truth_of(name, i)
    assert len(truth["steps"]) == S and truth["n_perturb"] == int(r["n_perturb"])
    d_logits = max(dist(r["logits"][s], truth["steps"][s]["logits"]) for s in range(S))
    for s in range(S):
        tr = truth["steps"][s]
        assert tr["partner"] == int(r["partner"][s]), (s, tr["partner"], int(r["partner"][s]))
        ds = dist(r["scores"][s], tr["scores"])
        top = np.sort(r["scores"][s])[::-1]
        assert top[0] - top[1] > 100 * ds, (s, top[0] - top[1], ds)
        lt = np.sort(r["logits"][s])[::-1]
        assert lt[0] - lt[1] > 100 * d_logits, (s, lt[0] - lt[1], d_logits)
        assert ds <= meta["f32_vs_f64"]["scores"] * (1 + 1e-6) and ds <= c["meta"]["f32_vs_f64"]["scores"]
        assert int(r["label"][s]) == tr["label"]
    assert d_logits <= meta["f32_vs_f64"]["logits"] * (1 + 1e-6)
    assert abs(float(r["best_conf"]) - truth["best_conf"]) <= meta["f32_vs_f64"]["best_conf"] * (1 + 1e-6) + 1e-12
    best = np.flatnonzero(truth["best_adj"][meta["target"]].numpy() != c["adj"][meta["target"]])
    assert np.array_equal(best, r["best_set"])


@pytest.mark.parametrize("name,i", runs())
def test_select_model_is_the_recorded_torch_composition_bit_for_bit(name, i):
    c, meta, r = run_of(name, i)
    n, t = c["adj"].shape[0], meta["target"]
    row_cols = np.flatnonzero(c["adj"][t])
    for s in range(len(r["partner"])):
        tog = r["toggled"][s][r["toggled"][s] >= 0]
        rerank = not np.isnan(r["p_top2"][s]).any()
        kw = dict(grad_pmax=r["grad_pmax"][s], grad_psmax=r["grad_psmax"][s], p_top2=r["p_top2"][s]) if rerank else {}
        scores, ids, best = R.select_model(n, t, r["grad_loss"][s], row_cols, None, tog, topk=3, **kw)
        assert np.array_equal(scores.view(np.int32), r["scores"][s].view(np.int32)), (name, i, s)
        assert ids[0] == r["partner"][s] and best[0].view(np.int32) == r["scores"][s][ids[0]].view(np.int32)
        assert np.array_equal(ids, np.argsort(-r["scores"][s].astype(np.float64), kind="stable")[:3])
        # the same from torch on the CPU, as calib_fga.py composes it
        row = torch.from_numpy(c["adj"][t].copy())
        row[torch.from_numpy(tog)] = 1 - row[torch.from_numpy(tog)]
        tk = {k: torch.from_numpy(np.concatenate([v, np.zeros(n, np.float32)]) if v.shape[0] == n else v)
              for k, v in kw.items()}
        ts = R.torch_scores(n, t, torch.from_numpy(r["grad_loss"][s]), row, **tk).numpy()
        assert np.array_equal(ts.view(np.int32), scores.view(np.int32))


def test_float32_restatement_reproduces_the_recorded_runs():
    """wats_hip.attack's loss functions and the loop of tests/attack_ref.py in float32 against what the reference
    recorded: the same partners, n_perturb and best set, scores and logits within 4 x the case's
    float32-vs-float64 distance (the rule the GPU tests use: both are float32 evaluations of the same expression)"""
    for name, i in runs():
        c, meta, r = run_of(name, i)
        got = truth_of(name, i, dtype=torch.float32)
        assert [s["partner"] for s in got["steps"]] == [int(j) for j in r["partner"]], (name, i)
        assert got["n_perturb"] == int(r["n_perturb"])
        for s, st in enumerate(got["steps"]):
            assert dist(st["scores"], r["scores"][s]) <= 4 * c["meta"]["f32_vs_f64"]["scores"]
            assert dist(st["logits"], r["logits"][s]) <= 4 * c["meta"]["f32_vs_f64"]["logits"]


# ------------------------------------------------------------------------------------------------ mutants of the select
def test_mutant_symmetric_rerank_is_a_different_attack():
    """The rerank on grad_pmax[t] + grad_pmax[:, t]: where the column half outweighs the row half the flag changes
    sign and another partner wins.  (On the recorded runs the two halves agree in sign at every partner, so the
    mutant is shown on inputs built for it; the fixtures' rerank does change signs: see negative_flags below.)"""
    n, t = 6, 0
    g = np.zeros(2 * n, np.float32)
    g[:n] = [0, 1, 2, 3, 4, 5]
    gp, gs = np.zeros(2 * n, np.float32), np.zeros(2 * n, np.float32)
    gp[n + 5] = -1                                       # column half only: d p_max / d a[5, t]
    p = np.array([0.6, 0.4], np.float32)
    good = R.select_model(n, t, g, [t], None, (), gp, gs, p)
    bad = R.select_model(n, t, g, [t], None, (), gp, gs, p, mutant="sym_rerank")
    assert good[1][0] == 5 and good[0][5] == 5
    assert bad[1][0] == 4 and bad[0][5] == -5
    # the fixtures exercise the rerank's -1 branch
    assert any(r["negative_flags"] > 0 for r in manifest()["cases"]["iso120"]["runs"])
    for name, i in runs():
        c, meta, r = run_of(name, i)
        n, t = c["adj"].shape[0], meta["target"]
        count = 0
        for s in range(len(r["partner"])):
            if np.isnan(r["p_top2"][s]).any():
                continue
            row = c["adj"][t].copy()
            tog = r["toggled"][s][r["toggled"][s] >= 0]
            row[tog] = 1 - row[tog]
            d = np.float32(1) - np.float32(2) * row
            cond = ((r["p_top2"][s][0] + r["grad_pmax"][s] * d) - r["p_top2"][s][1]) - r["grad_psmax"][s] * d
            cond[t] = 1
            count += int((~(cond > 0)).sum())
        assert count == meta["negative_flags"], (name, i)


def _synthetic(n=9, t=4):
    g = np.zeros(2 * n, np.float32)
    g[:n] = np.linspace(-1, 1, n)
    return n, t, g


def test_mutant_ge_differs_where_the_condition_is_exactly_zero():
    n, t, g = _synthetic()
    z = np.zeros(2 * n, np.float32)
    p = np.array([0.5, 0.5], np.float32)                  # c == 0 everywhere: the reference's `> 0` gives -1
    good = R.select_model(n, t, g, [t], None, (), z, z, p)
    bad = R.select_model(n, t, g, [t], None, (), z, z, p, mutant="ge")
    assert good[1][0] == 0 and bad[1][0] == n - 1
    assert not np.array_equal(good[0], bad[0])


def test_mutant_last_tie_differs_on_equal_scores():
    n, t = 7, 3
    g = np.ones(2 * n, np.float32)
    good = R.select_model(n, t, g, [], None, (), topk=3)
    bad = R.select_model(n, t, g, [], None, (), topk=3, mutant="last_tie")
    assert list(good[1]) == [0, 1, 2] and list(bad[1]) == [6, 5, 4]


def test_mutant_self_unmasked_differs_on_every_fixture_step():
    for name, i in runs():
        c, meta, r = run_of(name, i)
        n, t = c["adj"].shape[0], meta["target"]
        for s in range(len(r["partner"])):
            assert r["scores"][s][t] == np.float32(-10)
            tog = r["toggled"][s][r["toggled"][s] >= 0]
            bad = R.select_scores(n, t, r["grad_loss"][s], np.flatnonzero(c["adj"][t]), None, tog,
                                  mutant="self_unmasked")
            assert bad[t] != np.float32(-10)
    n, t, g = _synthetic()
    g[t] = 5                                             # the self entry would win
    assert R.select_model(n, t, g, [], None, ())[1][0] == n - 1
    assert R.select_model(n, t, g, [], None, (), mutant="self_unmasked")[1][0] == t


def test_rank_orders_nan_first_then_scores_then_index():
    s = np.array([1, np.nan, 3, 3, -0.0, 0.0, np.nan, -np.inf], np.float32)
    ids, best = R.rank(s, 8)
    assert list(ids) == [1, 6, 2, 3, 0, 4, 5, 7]
    ids, best = R.rank(s[:2], 4)
    assert list(ids) == [1, 0, -1, -1] and best[2] == -np.inf and np.isnan(best[0])


# ------------------------------------------------------------------------------------------------ wg_target_logits
def star(leaves):
    """node 0 joined to `leaves` leaves, every node with its self loop: canonical CSR"""
    n = leaves + 1
    rows = [[0] + list(range(1, n))] + [[0, j] for j in range(1, n)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32), n


def logits_inputs(n, Hd, C, kind, seed):
    rng = np.random.default_rng(seed)
    z = A.signal(n, Hd, kind, seed)
    W2 = A.signal(C, Hd, kind, seed + 1, spread=1.0)
    return z, rng.standard_normal(Hd).astype(np.float32), W2, rng.standard_normal(C).astype(np.float32)


def fixture_csr(name):
    import scipy.sparse as sp
    M = sp.csr_matrix(case(name)["adj"])
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int32), M.shape[0]


LOGIT_CASES = [("iso120", 16, [84, 94]), ("iso120", 17, [3]), ("iso120", 41, [45, 75]), ("hub96", 1, [50, 77]),
               ("hub96", 6, [0, 65]), ("star", 0, [5]), ("star", 7, [3, 9]), ("star", 7, [0])]


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("graph,t,S", LOGIT_CASES)
def test_target_logits_model_is_inside_one_rounding(graph, t, S, kind):
    indptr, indices, n = star(300) if graph == "star" else fixture_csr(graph)
    for Hd, C in ((16, 5), (65, 3)):
        ref = R.target_logits(indptr, indices, *logits_inputs(n, Hd, C, kind, 3), t, S)
        agree, c = ref.agreement(), ref.c(ref.model, "model")
        print(f"{graph} t={t} S={S} {kind} Hd={Hd}: truth vs second {agree:.2e}, model c = {c:.4f}")
        assert agree <= A.TRUTH_AGREE and c <= ref.bound


def test_target_logits_mutants_are_outside_the_bound():
    indptr, indices, n = star(300)
    z, b1, W2, b2 = logits_inputs(n, 16, 5, "positive", 3)
    # one float32 accumulator over the hub's 301 rows of one sign: many roundings
    ref = R.target_logits(indptr, indices, z, np.abs(b1), np.abs(W2), np.abs(b2), 7, [3])
    c = ref.c(ref.mutant, "float32 accumulator")
    print(f"float32 accumulator, star, t = leaf: c = {c:.2f}")
    assert c > ref.bound and ref.c(ref.model) <= ref.bound
    # deg' taken from the base row: wrong by a whole term wherever the candidate changes a degree
    c = ref.c(ref.mutant_deg, "deg' from the base row")
    print(f"deg' from the base row: c = {c:.3e}")
    assert c > 1e3
    ip, ix, n2 = fixture_csr("hub96")
    ref2 = R.target_logits(ip, ix, *logits_inputs(n2, 16, 5, "normal", 3), 6, [0, 65])
    assert ref2.c(ref2.mutant_deg) > 1e3 and ref2.c(ref2.model) <= ref2.bound
    # an empty candidate changes no degree: the mutant is then the model
    ref3 = R.target_logits(ip, ix, *logits_inputs(n2, 16, 5, "normal", 3), 6, [])
    assert np.array_equal(ref3.mutant_deg, ref3.model)


def test_target_logits_truth_is_the_dense_model_on_the_flipped_graph():
    """the semantics: (adj_norm' relu(adj_norm' (x W1^T) + b1)) W2^T + b2 at row t of the flipped dense matrix"""
    c = case("hub96")
    P = {k: v.double() for k, v in c["P"].items()}
    x, adj = torch.from_numpy(c["x"]).double(), torch.from_numpy(c["adj"]).double()
    indptr, indices, n = fixture_csr("hub96")
    z = (x.float() @ c["P"]["gc1.weight"].t()).numpy()
    for t, S in ((6, [0, 65]), (1, [50, 51, 77]), (20, [])):
        a = adj.clone()
        for j in S:
            a[t, j] = a[j, t] = 1 - a[t, j]
        deg = a.sum(1, keepdim=True)
        deg[deg == 0] = 1
        an = a / deg
        h = torch.relu(an @ torch.from_numpy(z).double() + P["gc1.bias"])
        want = ((an @ h) @ P["gc2.weight"].t() + P["gc2.bias"])[t].numpy()
        ref = R.target_logits(indptr, indices, z, c["P"]["gc1.bias"].numpy(), c["P"]["gc2.weight"].numpy(),
                              c["P"]["gc2.bias"].numpy(), t, S)
        assert np.abs(ref.truth - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


# ------------------------------------------------------------------------------------------------ the host side
def test_abi_checks_arguments_before_any_device_work():
    lib = wats_hip._lib.load()
    assert lib.wg_target_long_row() == 128 and lib.wg_flip_select_workspace(None) == -1
    p = [4096 + 256 * q for q in range(12)]
    sel = lib.wg_flip_select
    #       n  t  gl    gp    gs    top2  indptr indices values ntog tog  topk nwg ws    scores ids   best  stream
    ok = [5, 2, p[0], p[1], p[2], p[3], p[4], p[5], None, 0, None, 1, 1, p[6], None, p[7], p[8], None]

    def bad(f, base, code, word, **changes):
        args = list(base)
        for k, v in changes.items():
            args[int(k[1:])] = v
        assert f(*args) == code, (f.__name__, changes)
        assert word in lib.wg_last_error(), (f.__name__, changes, lib.wg_last_error())

    assert sel(*([0, 0] + [None] * 7 + [0, None, 1, 0] + [None] * 5)) == 0          # n == 0: WG_OK, no launch
    bad(sel, ok, -1, b"negative", a0=-1)
    bad(sel, ok, -1, b"target", a1=5)
    bad(sel, ok, -1, b"target", a1=-1)
    bad(sel, ok, -1, b"both", a3=None)                                     # only one rerank pointer
    bad(sel, ok, -1, b"both", a4=None)
    bad(sel, ok, -1, b"p_top2", a5=None)
    bad(sel, ok, -1, b"NULL", a2=None)
    bad(sel, ok, -1, b"NULL", a6=None)
    bad(sel, ok, -1, b"toggled", a9=2)
    bad(sel, ok, -1, b"negative", a9=-1)
    bad(sel, ok, -1, b"topk", a11=0)
    bad(sel, ok, -1, b"topk", a11=9)
    bad(sel, ok, -1, b"n_workgroups", a12=257)
    bad(sel, ok, -1, b"workspace", a12=2, a13=None)
    bad(sel, ok, -1, b"workspace", a12=2, a13=p[6] + 4)
    bad(sel, ok, -1, b"NULL", a15=None)
    bad(sel, ok, -1, b"NULL", a16=None)
    bad(sel, ok, -4, b"int32", a0=2 ** 31)
    tl = lib.wg_target_logits
    #        n  nnz indptr indices Hd z     b1    W2    b2    C  t  B  cptr  cids  out   stream
    ok = [5, 9, p[0], p[1], 4, p[2], p[3], p[4], p[5], 3, 2, 1, p[6], p[7], p[8], None]
    bad(tl, ok, -1, b"n=", a0=0)
    bad(tl, ok, -1, b"nnz", a1=-1)
    bad(tl, ok, -4, b"int32", a0=2 ** 31)
    bad(tl, ok, -4, b"int32", a1=2 ** 31)
    bad(tl, ok, -1, b">= 1", a4=0)
    bad(tl, ok, -1, b">= 1", a9=0)
    bad(tl, ok, -1, b">= 1", a11=0)
    bad(tl, ok, -4, b"256", a4=257)
    bad(tl, ok, -4, b"256", a9=257)
    bad(tl, ok, -1, b"target", a10=5)
    for pos in (2, 5, 6, 7, 8, 12, 14):
        bad(tl, ok, -1, b"NULL", **{f"a{pos}": None})
    bad(tl, ok, -1, b"indices", a3=None)


def test_loss_functions_against_their_formulas():
    torch.manual_seed(0)
    logits = torch.randn(1, 5, dtype=torch.float64)
    p = torch.softmax(logits, 1)[0]
    lab = torch.tensor([int(p.argmax())])
    others = torch.cat([p[:lab[0]], p[lab[0] + 1:]])
    assert torch.isclose(L.underconfidence_objective(logits, lab), -(p[lab[0]] - others.max()))
    assert torch.isclose(L.overconfidence_objective(logits, lab), -(1 - p[lab[0]]))
    u = torch.full((5,), 0.2, dtype=torch.float64)
    assert torch.isclose(L.kl_divergence_with_uniform(logits, lab), -(u * (u.log() - p.log())).sum())
    # the four branches of the target distribution
    other = torch.tensor([(int(lab[0]) + 1) % 5])
    kl = lambda d: -(d[d > 0] * (d[d > 0].log() - p.log()[d > 0])).sum()
    onehot = torch.zeros(5, dtype=torch.float64)
    onehot[lab[0]] = 1
    rest = torch.full((5,), 0.25, dtype=torch.float64)
    rest[other[0]] = 0
    half = torch.zeros(5, dtype=torch.float64)
    half[other[0]] = half[lab[0]] = 0.5
    assert torch.isclose(L.kl_divergence_target(logits, lab, lab), kl(u))
    assert torch.isclose(L.kl_divergence_target(logits, lab, other), kl(onehot))
    assert torch.isclose(L.kl_divergence_target(logits, other, lab), kl(rest))
    assert torch.isclose(L.kl_divergence_target(logits, other, other), kl(half))


def test_argument_checks_of_the_python_wrappers():
    with pytest.raises(ValueError, match="only supports 'under'"):
        L.Calib_FGA.rerank_attack(None, None, None, 0, 1, "over")
    with pytest.raises(ValueError, match="only supports 'under'"):
        L.Calib_FGA.flip_beam_hybridloss_attack(None, None, None, 0, 1, "over")
    assert {"Calib_FGA", "flip_select", "target_logits"} <= set(dir(wats_hip))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU refusal")
def test_refuses_to_run_without_a_gpu():
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        L.Calib_FGA(torch.nn.Linear(3, 3))
