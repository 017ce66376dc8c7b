"""GPU tests of the batched attack step (csrc/fga.hip wg_fga_scores, Calib_FGA.attack_many).

(a) wg_fga_scores against tests/fga_many_ref.py: the gradient rows inside one rounding of the float64 truth
(agg_ref.BOUND_ONE in the unit of the expression with every term's absolute value, the entry (t, t) left out); scores,
best ids and best scores bit for bit what wg_flip_select gives on the kernel's own gradient rows; the same bits on every
grid.  (b) attack_many reproduces every run the reference recorded, all runs of one method, strategy and surrogate as
one batch.  (c) attack_many against the single-target methods on the fixture graphs and on the synthetic graph of
fga_many_ref, on every case whose conditions tests/test_fga_many_host.py asserts (fga_many_ref.CLASS_CASES).  (d) a
target that stops early leaves the others as they are alone.  (e) the fallback route returns the same dicts."""
import contextlib
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import agg_ref as A  # noqa: E402
import cheb_ref as C  # noqa: E402
import fga_many_ref as M  # noqa: E402
import test_attack as T  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip import Calib_FGA, RowNormalizedAdjacency, SparseCompatibleGCN, fga_scores, flip_select  # noqa: E402
from wats_hip.attack import METHODS  # noqa: E402

DEV = "cuda"
_zoo = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def _np(t):
    return t.detach().cpu().numpy()


def dev(a, offset=0):
    a = np.ascontiguousarray(a)
    return T.on_device(a.reshape(-1), offset).view(a.shape) if offset else T.on_device(a)


# ------------------------------------------------------------------------------------------------ (a) the kernel
def zoo(n):
    """the graph of the kernel tests: fga_many_ref.synthetic (a hub whose row is past wg_target_long_row() at n = 257,
    an isolated node, a node with its self loop only, a node of degree one without a self loop)"""
    if n not in _zoo:
        if n == 1:
            _zoo[n] = (np.array([0, 1], np.int64), np.array([0], np.int32))
        elif n == 2:
            _zoo[n] = (np.array([0, 2, 4], np.int64), np.array([0, 1, 0, 1], np.int32))
        else:
            _zoo[n] = M.synthetic(n, seed=n, hub=min(200, n - 10))[:2]
    return _zoo[n]


def zoo_targets(n, B, seed):
    """B (target, toggle set) pairs: the special nodes first (hub, isolated, self loop only, degree one with its only
    neighbour removed, a hub neighbour), duplicates with different sets, sets that are empty, add only, remove only
    and mixed"""
    indptr, indices = zoo(n)
    rng = np.random.default_rng(seed)
    if n == 1:
        return [(0, [])] * B
    if n == 2:
        return [(b % 2, [] if b % 3 == 0 else [1 - b % 2]) for b in range(B)]
    special = [(0, []), (n - 1, []), (n - 2, [3]), (n - 3, [5]), (7, [0]), (0, [1, 2, n - 1]), (n - 3, []),
               (n - 1, [4, 9]), (7, [])]
    out = list(special[:B])
    while len(out) < B:
        t = int(rng.integers(0, n))
        row = indices[indptr[t]:indptr[t + 1]]
        present = [int(j) for j in row if j != t]
        absent = [int(j) for j in np.setdiff1d(np.arange(n), row) if j != t]
        kind = len(out) % 4
        add = list(rng.choice(absent, min(2, len(absent)), replace=False)) if kind in (1, 3) and absent else []
        rem = list(rng.choice(present, min(2, len(present)), replace=False)) if kind in (2, 3) and present else []
        out.append((t, sorted(int(j) for j in add + rem)))
    return out


def kernel_inputs(n, Hd, Cn, B, G, seed, kind="normal"):
    indptr, indices = zoo(n)
    rng = np.random.default_rng(seed)
    z = A.signal(n, Hd, kind, seed)
    b1 = (0.3 * rng.standard_normal(Hd)).astype(np.float32)
    W2 = A.signal(Cn, Hd, kind, seed + 1, spread=1.0)
    pairs = zoo_targets(n, B, seed)
    g = rng.standard_normal((B, G, Cn)).astype(np.float32)
    rerank = (np.arange(B) % 3 != 1).astype(np.int32) if G == 3 else None      # mixed flags
    p = np.sort(rng.uniform(0.05, 0.9, (B, 2)).astype(np.float32), axis=1)[:, ::-1].copy() if G == 3 else None
    return dict(n=n, indptr=indptr, indices=indices, z=z, h=M.base_hidden(indptr, indices, z, b1), b1=b1, W2=W2,
                pairs=pairs, g=g, rerank=rerank, p=p, G=G)


def run_kernel(I, topk=1, n_workgroups=0, z_offset=0):
    out = fga_scores(I["n"], dev(I["indptr"]), dev(I["indices"]), dev(I["z"], z_offset), dev(I["h"]), dev(I["b1"]),
                     dev(I["W2"]), [t for t, _ in I["pairs"]], [S for _, S in I["pairs"]], dev(I["g"]),
                     None if I["rerank"] is None else dev(I["rerank"]), None if I["p"] is None else dev(I["p"]),
                     topk=topk, n_workgroups=n_workgroups, return_grads=True, return_scores=True)
    torch.cuda.synchronize()
    return out


def check_kernel(I, topk=3, groups=(0, 1, 2, 7), what="", **kw):
    n = I["n"]
    first = None
    for nwg in groups:
        ids, best, grads, scores = run_kernel(I, topk, nwg, **kw)
        got = tuple(_np(v) for v in (ids, best, grads, scores))
        if first is not None:                                # another grid: the same bits
            assert np.array_equal(got[0], first[0]), (what, nwg)
            for a, b in zip(got[1:], first[1:]):
                T.bits_equal(a, b, f"{what}: {nwg} workgroups")
            continue
        first = got
        worst = 0.0
        for b, (t, S) in enumerate(I["pairs"]):
            ref = M.grads_ref(I["indptr"], I["indices"], I["z"], I["h"], I["b1"], I["W2"], t, S, I["g"][b])
            keep = np.ones(2 * n, bool)
            keep[[t, n + t]] = False                         # the entry (t, t) is not defined
            c = C.c_of(got[2][b][:, keep], ref.truth[:, keep], ref.unit[:, keep], f"{what} target {b}")
            assert C.c_of(ref.second[:, keep], ref.truth[:, keep], ref.unit[:, keep]) <= A.TRUTH_AGREE
            worst = max(worst, c)
            assert c <= A.BOUND_ONE, (what, b, t, S, c)
            # wg_flip_select on the kernel's own rows
            rr = I["G"] == 3 and bool(I["rerank"][b])
            tog = torch.tensor(S, dtype=torch.int32, device=DEV) if S else None
            want = flip_select(n, t, grads[b, 0], dev(I["indptr"]), dev(I["indices"]), None, tog,
                               grads[b, 1] if rr else None, grads[b, 2] if rr else None, dev(I["p"][b]) if rr else None,
                               topk=topk, return_scores=True)
            assert np.array_equal(got[0][b], _np(want[0])), (what, b, got[0][b], _np(want[0]))
            T.bits_equal(got[1][b], _np(want[1]), f"{what} target {b}: best scores")
            T.bits_equal(got[3][b], _np(want[2]), f"{what} target {b}: scores")
        print(f"{what}: c = {worst:.4f} (bound {A.BOUND_ONE})")
    return first


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_fga_scores_sizes_special_targets_and_topk(n):
    for G in (1, 3):
        for topk in (1, 3, 8):                               # topk > n at n = 1, 2
            check_kernel(kernel_inputs(n, 16, 5, min(9, 4 * n), G, seed=n + G), topk,
                         groups=(0, 1, 2, 7) if topk == 3 else (0,), what=f"n={n} G={G} topk={topk}")


@pytest.mark.parametrize("Hd,Cn", [(1, 2), (3, 40), (4, 256), (64, 40), (65, 2), (256, 40)])
def test_fga_scores_widths_and_class_counts(Hd, Cn):
    for kind in ("normal", "positive"):
        check_kernel(kernel_inputs(65, Hd, Cn, 5, 3, seed=Hd, kind=kind), what=f"Hd={Hd} C={Cn} {kind}")


@pytest.mark.parametrize("B", [1, 2, 32, 33])
def test_fga_scores_batches_with_duplicate_targets(B):
    I = kernel_inputs(257, 16, 5, B, 3, seed=B)
    assert B < 9 or len({t for t, _ in I["pairs"]}) < B      # duplicates, with different toggle sets
    check_kernel(I, what=f"B={B}")


def test_fga_scores_misaligned_z_and_repeat():
    I = kernel_inputs(257, 64, 40, 9, 3, seed=4)
    a = check_kernel(I, groups=(0,), what="aligned")
    b = check_kernel(I, groups=(0,), what="misaligned z", z_offset=1)
    for u, v in zip(a[1:], b[1:]):
        T.bits_equal(u, v, "aligned against misaligned z")
    assert np.array_equal(a[0], b[0])


def test_fga_scores_nan_containment():
    I = kernel_inputs(257, 16, 5, 6, 3, seed=6)
    n, indptr, indices = I["n"], I["indptr"], I["indices"]
    I["pairs"] = [(n - 1, []), (n - 2, [3]), (n - 3, [5]), (230, []), (240, [250]), (230, [231, 232])]   # no hub
    clean = tuple(_np(v) for v in run_kernel(I, 3))
    # a NaN row of z: node k outside every target's two-hop ball reaches the scores of k and of its neighbours (their
    # h_j) and nothing else
    near = set()
    for t, S in I["pairs"]:
        one = set(indices[indptr[t]:indptr[t + 1]]) | set(S) | {t}
        near |= one
        for j in one:
            near |= set(indices[indptr[j]:indptr[j + 1]])
    k = next(j for j in range(n - 4, 0, -1) if j not in near and indptr[j + 1] - indptr[j] > 2)
    J = dict(I)
    J["z"] = I["z"].copy()
    J["z"][k] = np.nan
    J["h"] = M.base_hidden(indptr, indices, J["z"], I["b1"])
    got = tuple(_np(v) for v in run_kernel(J, 3))
    allowed = np.zeros(n, bool)
    allowed[indices[indptr[k]:indptr[k + 1]]] = True
    allowed[k] = True
    for b in range(len(I["pairs"])):
        nan = np.isnan(got[3][b])
        assert not nan[~allowed].any() and nan[allowed].any(), b
        T.bits_equal(got[3][b][~allowed], clean[3][b][~allowed], f"target {b}: scores the NaN row does not enter")
    # a NaN g_logits row of one target: the other targets' bits are unchanged
    J = dict(I)
    J["g"] = I["g"].copy()
    J["g"][4] = np.nan
    got = tuple(_np(v) for v in run_kernel(J, 3))
    others = np.arange(len(I["pairs"])) != 4
    assert np.array_equal(got[0][others], clean[0][others])
    for u, v in zip(got[1:], clean[1:]):
        T.bits_equal(u[others], v[others], "the targets beside the NaN one")
    assert np.isnan(got[3][4]).any()


# ------------------------------------------------------------------------------------------------ the class
def quiet(f, *a, **kw):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        r = f(*a, **kw)
    return r, out.getvalue()


def fixture_groups():
    groups = {}
    for name in ("iso120", "hub96"):
        for r in T.manifest()["cases"][name]["runs"]:
            groups.setdefault((name, r["method"], r["strategy"], r.get("surrogate", "GCN")), []).append(r["run"])
    return sorted(groups.items())


@pytest.mark.parametrize("key,runs", fixture_groups(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else "")
def test_attack_many_reproduces_the_recorded_runs(key, runs):
    name, method, strategy, surrogate = key
    c = T.case(name)
    rec = c["meta"]["f32_vs_f64"]
    model = T.wats_of(c) if surrogate == "WATS" else T.gcn_of(c)
    x, y = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["y"]).to(DEV)
    op = RowNormalizedAdjacency.from_dense(torch.from_numpy(c["adj"]).to(DEV))
    metas = [c["meta"]["runs"][i] for i in runs]
    atk = Calib_FGA(model, device=DEV)
    recs = [{k.split("__", 1)[1]: v for k, v in c.items() if k.startswith(f"r{i}__")} for i in runs]
    kw = dict(n_perturb=[], best_conf=[], runtime=[])
    call = lambda ms, **lists: quiet(atk.attack_many, x, op, [m["target"] for m in ms], c["meta"]["budget"], strategy,
                                     method=method, res_gt=y, **lists)
    if any(bool(r["raised"]) for r in recs):                 # the reference's ValueError, after every target has run
        with pytest.raises(ValueError, match="Final label"):
            call(metas, n_perturb=[], best_conf=[])
        keep = [k for k, r in enumerate(recs) if not bool(r["raised"])]
        metas, recs, runs = [metas[k] for k in keep], [recs[k] for k in keep], [runs[k] for k in keep]
        if not runs:
            return
    results, log = call(metas, **kw)
    assert log == ""                                         # nothing is printed unless verbose
    assert atk._local is not None and len(results) == len(runs)
    assert kw["n_perturb"] == [int(r["n_perturb"]) for r in recs]
    for res, m, r in zip(results, metas, recs):
        assert res["target"] == m["target"]
        assert res["flips"] == [int(j) for j in r["partner"]], (m, res["flips"], r["partner"])
        assert [s["label"] for s in res["trace"]] == [int(v) for v in r["label"]]
        assert res["n_perturb"] == int(r["n_perturb"]) and res["best_flips"] == [int(j) for j in r["best_set"]]
        assert abs(res["best_conf"] - float(r["best_conf"])) <= 4 * rec["best_conf"]
        worst = max(float(np.abs(_np(s["logits"]).astype(np.float64) - r["logits"][k]).max())
                    for k, s in enumerate(res["trace"]))
        print(f"{method} target {m['target']}: logits distance {worst:.3e} (tolerance {4 * rec['logits']:.3e})")
        assert worst <= 4 * rec["logits"]
        assert res["final_label"] == res["original_label"] or method != "flip_beam_hybridloss_attack"
        indices = res["modified_op"].csr()[1]
        want = c["adj"].copy()
        for j in r["best_set"]:
            want[m["target"], j] = want[j, m["target"]] = 1 - want[m["target"], j]
        assert np.array_equal(_np(indices), np.nonzero(want)[1])


def single(atk, method, x, op, t, budget, strategy, y, **extra):
    """the single-target method as a dict of attack_many's fields (None when the beam method raised)"""
    kw = dict(n_perturb=[], best_conf=[])
    try:
        quiet(getattr(atk, method), x, op, t, budget, strategy, res_gt=y, **kw, **extra)
    except ValueError as e:
        assert "Final label" in str(e)
        return None
    return dict(flips=list(atk.flips), best_flips=list(atk.best_flips), n_perturb=kw["n_perturb"][0],
                best_conf=kw["best_conf"][0], confidences=[s["confidence"] for s in atk.trace],
                labels=[s["label"] for s in atk.trace])


def same_as_single(res, want, what):
    assert res["flips"] == want["flips"], (what, res["flips"], want["flips"])
    assert res["best_flips"] == want["best_flips"] and res["n_perturb"] == want["n_perturb"], what
    assert [s["label"] for s in res["trace"]] == want["labels"], what
    assert abs(res["best_conf"] - want["best_conf"]) <= 1e-6, what
    for s, cf in zip(res["trace"], want["confidences"]):
        assert (np.isnan(cf) and np.isnan(s["confidence"])) or abs(s["confidence"] - cf) <= 1e-6, what


def ts_of(base, x, y, adj, val_idx):
    cal = wats_hip.TemperatureScaling(base, x, y, adj, val_idx, verbose=False, epochs=1, frozen_logits=True)
    with torch.no_grad():
        cal.temperature.fill_(M.CLASS_TEMPERATURE)
    return cal.eval()


def synthetic_setup():
    indptr, indices, adj = M.synthetic()
    xs, P, ys = M.synthetic_model(adj)
    base = SparseCompatibleGCN(xs.shape[1], nclass=4, nhid=16)
    base.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    x, y = torch.from_numpy(xs).to(DEV), torch.from_numpy(ys).to(DEV)
    dense = torch.from_numpy(adj.astype(np.float32)).to(DEV)
    return base.to(DEV).eval(), x, y, dense, list(M.SYN_TARGETS), torch.arange(0, 150, 3, device=DEV)


def fixture_setup(name):
    c = T.case(name)
    x, y = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["y"]).to(DEV)
    dense = torch.from_numpy(c["adj"]).to(DEV)
    targets = sorted({r["target"] for r in c["meta"]["runs"]})
    return T.gcn_of(c), x, y, dense, targets, torch.arange(0, dense.shape[0], 3, device=DEV)


SETUPS = {"synthetic": synthetic_setup, "iso120": lambda: fixture_setup("iso120"),
          "hub96": lambda: fixture_setup("hub96")}


@pytest.mark.parametrize("surrogate", ["gcn", "ts"])
@pytest.mark.parametrize("graph", sorted(SETUPS))
def test_attack_many_is_the_single_target_methods(graph, surrogate):
    base, x, y, dense, targets, val_idx = SETUPS[graph]()
    model = base if surrogate == "gcn" else ts_of(base, x, y, dense, val_idx)
    op = RowNormalizedAdjacency.from_dense(dense)
    atk = Calib_FGA(model, device=DEV)
    budget = M.CLASS_BUDGET
    assert {m for m, _ in M.CLASS_CASES} == set(METHODS)
    for method, strategy in M.CLASS_CASES:
        # every target whose conditions tests/test_fga_many_host.py asserts (fga_many_ref.CLASS_LEFT_OUT has the rest)
        compared = M.class_targets(graph, surrogate, method, strategy, targets)
        wants = [single(atk, method, x, op, t, budget, strategy, y) for t in compared]
        keep = [t for t, w in zip(compared, wants) if w is not None]
        if not keep:
            continue
        results, _ = quiet(atk.attack_many, x, op, keep, budget, strategy, method=method, res_gt=y)
        assert atk._local is not None
        for res, want in zip(results, [w for w in wants if w is not None]):
            same_as_single(res, want, (graph, surrogate, method, strategy, res["target"]))
    with pytest.raises(TypeError):
        quiet(atk.attack_many, x, op, targets[:2], budget, "max", method="attack", res_gt=y)


def test_attack_many_a_target_that_stops_early_leaves_the_rest_alone():
    base, x, y, dense, targets, _ = synthetic_setup()
    op = RowNormalizedAdjacency.from_dense(dense)
    atk = Calib_FGA(base, device=DEV)
    every = list(range(0, 150, 5))
    budget = 6
    kw = dict(n_perturb=[], best_conf=[])
    results, _ = quiet(atk.attack_many, x, op, every, budget, "under", method="rerank_attack", res_gt=y, **kw)
    stopped = [r for r in results if len(r["flips"]) < budget or np.isnan(r["trace"][-1]["confidence"])]
    full = [r for r in results if r not in stopped]
    assert stopped and full, (len(stopped), len(full))       # both kinds are in the batch
    assert kw["n_perturb"] == [r["n_perturb"] for r in results]
    for r in full[:3] + stopped[:3]:
        alone, _ = quiet(atk.attack_many, x, op, [r["target"]], budget, "under", method="rerank_attack", res_gt=y)
        assert alone[0]["flips"] == r["flips"] and alone[0]["best_flips"] == r["best_flips"]
        assert alone[0]["best_conf"] == r["best_conf"] and alone[0]["final_label"] == r["final_label"]
        for s, w in zip(alone[0]["trace"], r["trace"]):
            assert torch.equal(s["logits"], w["logits"])      # the same bits alone and in the batch


def test_attack_many_fallback_route_returns_the_same_dicts():
    base, x, y, dense, targets, _ = synthetic_setup()
    op = RowNormalizedAdjacency.from_dense(dense)
    fast, slow = Calib_FGA(base, device=DEV), Calib_FGA(base, device=DEV, local_eval=False)
    for method in ("flip_beam_hybridloss_attack", "attack"):
        kf, ks = dict(n_perturb=[], best_conf=[]), dict(n_perturb=[], best_conf=[])
        a, _ = quiet(fast.attack_many, x, op, targets, 3, "under", method=method, res_gt=y, **kf)
        b, log = quiet(slow.attack_many, x, op, targets, 3, "under", method=method, res_gt=y, **ks)
        assert fast._local is not None and slow._local is None and log == ""
        assert kf["n_perturb"] == ks["n_perturb"]
        for ra, rb in zip(a, b):
            assert set(ra) == set(rb)
            for k in ("target", "flips", "best_flips", "n_perturb", "original_label", "final_label"):
                assert ra[k] == rb[k], (method, k, ra[k], rb[k])
            for k in ("best_conf", "original_confidence", "final_confidence"):
                assert abs(ra[k] - rb[k]) <= 1e-6, (method, k)
            assert [s["partner"] for s in ra["trace"]] == [s["partner"] for s in rb["trace"]]
            assert torch.equal(ra["modified_op"].csr()[1], rb["modified_op"].csr()[1])
