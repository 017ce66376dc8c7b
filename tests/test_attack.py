"""GPU tests of the attack step (csrc/attack.hip, wats_hip/attack.py).

wg_flip_select is compared bit for bit with the reference's torch composition on the device (calib_fga.py:880-897,
tests/attack_ref.torch_scores) and with the numpy model (attack_ref.select_model); a NaN score is compared as a NaN
(IEEE leaves a NaN's sign and payload to the implementation).  wg_target_logits is held to agg_ref.BOUND_ONE in its
own unit (one rounding, counted from the header); its distance to SparseCompatibleGCN on the flipped operator is
measured and printed, not bounded.  Calib_FGA reproduces every run the reference recorded (tests/golden/fga): the
partners, n_perturb, the best set and the labels exactly, best_conf and the per-step logits within 4 x the manifest's
float32-vs-float64 distance (the rule of tests/test_gets.py), once with the local evaluation and once through the
view."""
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
import wats_hip  # noqa: E402
from wats_hip import Calib_FGA, RowNormalizedAdjacency, SparseCompatibleGCN, flip_select, target_logits  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fga")
DEV = "cuda"
_cases = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def _np(t):
    return t.detach().cpu().numpy()


def bits_equal(got, want, what):
    """bit for bit, a NaN against a NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]), what


# ------------------------------------------------------------------------------------------------ wg_flip_select
def select_inputs(n, t, seed, valued=False, toggle="both", rerank=True):
    """(host arrays) one row of a CSR with n rows (the others empty), the gradients, the toggled partners"""
    rng = np.random.default_rng(seed)
    others = np.array([j for j in range(n) if j != t], np.int64)
    k = min(len(others), max(1, n // 5))
    row = np.sort(np.concatenate([rng.choice(others, k, replace=False) if k and len(others) else others[:0], [t]]))
    vals = (rng.uniform(0.25, 2.0, len(row)).astype(np.float32) if valued else None)
    present, absent = row[row != t], np.setdiff1d(others, row)
    pick = lambda a, m: rng.choice(a, min(m, len(a)), replace=False) if len(a) else a
    tog = {"none": others[:0], "remove": pick(present, 3), "add": pick(absent, 3),
           "both": np.concatenate([pick(present, 2), pick(absent, 2)])}[toggle]
    tog = np.sort(tog).astype(np.int32)
    g = rng.standard_normal(2 * n).astype(np.float32)
    gp = gs = p = None
    if rerank:
        gp, gs = (0.3 * rng.standard_normal(2 * n)).astype(np.float32), (0.3 * rng.standard_normal(2 * n)).astype(np.float32)
        p = np.array([0.55, 0.4], np.float32)
    indptr = np.zeros(n + 1, np.int64)
    indptr[t + 1:] = len(row)
    return dict(n=n, t=t, indptr=indptr, row=row.astype(np.int32), vals=vals, tog=tog, g=g, gp=gp, gs=gs, p=p)


def on_device(a, offset=0):
    """the array on the device; offset: that many float32 / int32 before it in its buffer (a 4-byte-aligned view)"""
    if a is None:
        return None
    t = torch.from_numpy(np.asarray(a))
    if offset:
        buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
        buf[offset:] = t.to(DEV)
        return buf[offset:]
    return t.to(DEV)


def run_select(I, topk=1, n_workgroups=0, offset=0, scores=True):
    d = {k: on_device(I[k], offset) for k in ("g", "gp", "gs", "p", "tog", "vals", "row")}
    indptr = on_device(I["indptr"])
    res = flip_select(I["n"], I["t"], d["g"], indptr, d["row"], d["vals"], d["tog"] if len(I["tog"]) else None,
                      d["gp"], d["gs"], d["p"], topk=topk, n_workgroups=n_workgroups, return_scores=scores)
    torch.cuda.synchronize()
    return tuple(None if r is None else _np(r) for r in res)


def torch_on_device(I):
    """calib_fga.py:880-897 on device tensors, the dense row built by the reference's update (:901-903)"""
    n, t = I["n"], I["t"]
    row = torch.zeros(n, device=DEV)
    row[torch.from_numpy(I["row"]).long().to(DEV)] = 1.0 if I["vals"] is None else torch.from_numpy(I["vals"]).to(DEV)
    for j in I["tog"]:
        value = -2 * row[int(j)] + 1
        row[int(j)] += value
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    return _np(R.torch_scores(n, t, dev(I["g"]), row, dev(I["gp"]), dev(I["gs"]), dev(I["p"])))


def check_select(I, topk, groups=(1, 0, 7, 256), **kw):
    model = R.select_model(I["n"], I["t"], I["g"], I["row"], I["vals"], I["tog"], I["gp"], I["gs"], I["p"], topk=topk)
    want_torch = torch_on_device(I)
    first = None
    for nwg in groups:
        ids, best, scores = run_select(I, topk, nwg, **kw)
        bits_equal(scores, model[0], "scores against the numpy model")
        bits_equal(scores, want_torch, "scores against torch on the device")
        assert np.array_equal(ids, model[1]), (nwg, ids, model[1])
        bits_equal(best, model[2], "best scores")
        if first is None:
            first = (ids, best, scores)
        else:                                            # one workgroup against many: the same bits
            assert np.array_equal(ids, first[0])
            bits_equal(best, first[1], "best scores across grids")
            bits_equal(scores, first[2], "scores across grids")


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 4097])
def test_flip_select_sizes_targets_and_topk(n):
    for t in sorted({0, n // 2, n - 1}):
        for topk in (1, 3, 8):                           # topk > n at n = 1, 2
            check_select(select_inputs(n, t, seed=n + t), topk)


@pytest.mark.parametrize("toggle", ["none", "remove", "add", "both"])
@pytest.mark.parametrize("valued", [False, True])
def test_flip_select_toggles_and_values(toggle, valued):
    for n, t in ((65, 7), (4097, 4000)):
        for rerank in (True, False):                     # no rerank pointers
            check_select(select_inputs(n, t, 5, valued=valued, toggle=toggle, rerank=rerank), 3)


def test_flip_select_equal_scores_go_by_index():
    for n, t in ((65, 64), (4097, 0)):
        I = select_inputs(n, t, 1, rerank=False, toggle="none")
        I["g"][:] = 0.5
        I["row"], I["indptr"] = I["row"][:0], np.zeros(n + 1, np.int64)     # an empty row: d = 1 everywhere
        check_select(I, 8)
        ids = run_select(I, 8, 256)[0]
        assert list(ids[:min(8, n - 1)]) == [j for j in range(n) if j != t][:8]
        I["g"][:] = 0.0                                   # +0 and -0 are one score
        I["g"][3] = I["g"][n + 3] = -0.0
        check_select(I, 8)


def test_flip_select_nan_ranks_first():
    for n, t in ((65, 3), (4097, 2048)):
        for where in ([n // 3], [n - 1, 5]):             # a NaN and two NaNs
            I = select_inputs(n, t, 2)
            I["g"][where] = np.nan
            check_select(I, 3)
            ids, best, _ = run_select(I, 3)
            assert list(ids[:len(where)]) == sorted(where) and np.isnan(best[:len(where)]).all()
            assert not np.isnan(best[len(where):]).any()
        I = select_inputs(n, t, 3)                        # a NaN in the rerank's condition: the flag is -1
        I["gp"][7] = np.nan
        check_select(I, 3)


def test_flip_select_misaligned_and_null_buffers():
    I = select_inputs(4097, 11, 9)
    check_select(I, 3, offset=1)                          # every float / int buffer 4 bytes off a 16-byte boundary
    ids, best = run_select(I, 3, 64, scores=False)[:2]    # scores NULL
    want = R.select_model(I["n"], I["t"], I["g"], I["row"], I["vals"], I["tog"], I["gp"], I["gs"], I["p"], topk=3)
    assert np.array_equal(ids, want[1])
    bits_equal(best, want[2], "best scores without the score vector")
    # workspace NULL with one workgroup
    lib = wats_hip._lib.load()
    d = {k: on_device(I[k]) for k in ("g", "gp", "gs", "p", "tog", "row", "indptr")}
    out_ids = torch.empty(3, dtype=torch.int32, device=DEV)
    out_best = torch.empty(3, device=DEV)
    p = wats_hip._lib.ptr
    args = [I["n"], I["t"], p(d["g"]), p(d["gp"]), p(d["gs"]), p(d["p"]), p(d["indptr"]), p(d["row"]), None,
            len(I["tog"]), p(d["tog"]), 3, 1, None, None, p(out_ids), p(out_best), None]
    assert lib.wg_flip_select(*args) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_np(out_ids), want[1])


def test_flip_select_refuses_bad_arguments():
    lib = wats_hip._lib.load()
    I = select_inputs(65, 3, 1)
    d = {k: on_device(I[k]) for k in ("g", "gp", "gs", "p", "tog", "row", "indptr")}
    ws = wats_hip.attack.select_workspace(DEV)
    out_ids, out_best = torch.empty(8, dtype=torch.int32, device=DEV), torch.empty(8, device=DEV)
    p = wats_hip._lib.ptr
    ok = [65, 3, p(d["g"]), p(d["gp"]), p(d["gs"]), p(d["p"]), p(d["indptr"]), p(d["row"]), None, len(I["tog"]),
          p(d["tog"]), 3, 0, p(ws), None, p(out_ids), p(out_best), None]
    assert lib.wg_flip_select(*ok) == 0
    for pos, v in ((0, -1), (1, 65), (3, None), (4, None), (5, None), (2, None), (6, None), (10, None), (11, 0), (11, 9),
                   (12, 257), (15, None), (16, None)):
        args = list(ok)
        args[pos] = v
        assert lib.wg_flip_select(*args) == -1, (pos, v)     # WG_ERR_INVALID
    args = list(ok)
    args[12], args[13] = 4, None
    assert lib.wg_flip_select(*args) == -1
    assert lib.wg_flip_select(*([0, 0] + [None] * 7 + [0, None, 1, 0] + [None] * 5)) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ wg_target_logits
def star(leaves):
    n = leaves + 1
    rows = [[0] + list(range(1, n))] + [[0, j] for j in range(1, n)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32), n


def path_without_loops():
    """0 - 1 - 2 - 3 - 4 and a node 5 with no entry, no self loops: node 0 has one entry"""
    rows = [[1], [0, 2], [1, 3], [2, 4], [3], []]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.array([c for r in rows for c in r], np.int32), len(rows)


def fixture_csr(name):
    c = case(name)
    M = sp.csr_matrix(c["adj"])
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int32), M.shape[0]


def logits_inputs(n, Hd, C, kind, seed):
    rng = np.random.default_rng(seed)
    return (A.signal(n, Hd, kind, seed), rng.standard_normal(Hd).astype(np.float32),
            A.signal(C, Hd, kind, seed + 1, spread=1.0), rng.standard_normal(C).astype(np.float32))


def run_logits(indptr, indices, n, z, b1, W2, b2, t, cands):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    out = target_logits(n, dev(indptr), dev(indices), dev(z), dev(b1), dev(W2), dev(b2), t, cands)
    torch.cuda.synchronize()
    return _np(out)


def check_logits(graph, t, cands, Hd, C, kind, what):
    indptr, indices, n = graph
    z, b1, W2, b2 = logits_inputs(n, Hd, C, kind, 3)
    got = run_logits(indptr, indices, n, z, b1, W2, b2, t, cands)
    again = run_logits(indptr, indices, n, z, b1, W2, b2, t, cands)
    assert np.array_equal(got.view(np.int32), again.view(np.int32)), f"{what}: a repeat gives other bits"
    worst = 0.0
    for b, S in enumerate(cands):
        ref = R.target_logits(indptr, indices, z, b1, W2, b2, t, S)
        c = ref.c(got[b], f"{what} candidate {b}")
        worst = max(worst, c)
        assert c <= A.BOUND_ONE, (what, b, S, c)
    print(f"{what} Hd={Hd} C={C} {kind}: c = {worst:.4f} (bound {A.BOUND_ONE})")
    return got


GRAPH_CASES = {
    # name: (graph, t, candidates)
    "star_hub": (lambda: star(300), 0, [[], [5], [5, 17, 299]]),
    "star_leaf": (lambda: star(300), 7, [[], [3], [0], [0, 3, 9]]),          # the hub's long row in the second hop
    "iso_isolated": (lambda: fixture_csr("iso120"), 17, [[], [3], [3, 16]]),      # an isolated t: no entry at all
    "iso_hub_neighbour": (lambda: fixture_csr("iso120"), 48, [[], [84, 94], [16]]),
    "hub96_degree_one": (lambda: fixture_csr("hub96"), 6, [[], [0, 65], [65]]),
    "hub96_hub": (lambda: fixture_csr("hub96"), 0, [[], [50], [1, 2, 3, 4, 5]]),
    "path_last_neighbour": (lambda: path_without_loops(), 0, [[1], [1, 2], []]),   # removes t's last neighbour; re-adds one
}


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("name", sorted(GRAPH_CASES))
def test_target_logits_one_rounding_on_every_graph(name, kind):
    make, t, cands = GRAPH_CASES[name]
    graph = make()
    for Hd, C in ((64, 40), (7, 3)):
        got = check_logits(graph, t, cands, Hd, C, kind, name)
    if name == "path_last_neighbour":
        b2 = logits_inputs(graph[2], 7, 3, kind, 3)[3]
        assert np.array_equal(got[0], b2)                  # no neighbour left: deg' 0 -> 1, y2 = 0, out = b2


@pytest.mark.parametrize("Hd", [1, 3, 4, 16, 64, 65, 256])
def test_target_logits_hidden_widths(Hd):
    check_logits(star(300), 7, [[0, 3], []], Hd, 3, "positive", "star_leaf")
    check_logits(fixture_csr("hub96"), 1, [[50, 77]], Hd, 3, "normal", "hub96")


@pytest.mark.parametrize("C", [1, 3, 40, 41])
def test_target_logits_class_counts(C):
    check_logits(fixture_csr("hub96"), 1, [[50, 77], [11]], 16, C, "spread", "hub96")


@pytest.mark.parametrize("B", [1, 3, 64])
def test_target_logits_batches(B):
    indptr, indices, n = fixture_csr("iso120")
    rng = np.random.default_rng(B)
    t = 3
    cands = [sorted(int(j) for j in rng.choice([j for j in range(n) if j != t], rng.integers(0, 6), replace=False))
             for _ in range(B)]
    cands[0] = []
    check_logits((indptr, indices, n), t, cands, 16, 5, "normal", f"B={B}")


def test_target_logits_misaligned_z_and_empty_candidate_is_the_base_row():
    c = case("hub96")
    indptr, indices, n = fixture_csr("hub96")
    model = gcn_of(c)
    x = torch.from_numpy(c["x"]).to(DEV)
    op = RowNormalizedAdjacency.from_dense(torch.from_numpy(c["adj"]).to(DEV))
    z = (x @ model.gc1.weight.t()).detach()
    buf = torch.empty(z.numel() + 1, device=DEV)
    buf[1:] = z.reshape(-1)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    args = (model.gc1.bias.detach(), model.gc2.weight.detach(), model.gc2.bias.detach())
    for t in (1, 6, 20):
        a = target_logits(n, dev(indptr), dev(indices), z, *args, t, [[]])
        b = target_logits(n, dev(indptr), dev(indices), buf[1:].view_as(z), *args, t, [[]])      # dword loads
        with torch.no_grad():
            want = model(x, op)[t]
        d = float((a[0] - want).abs().max())
        print(f"t={t}: empty candidate against the model's row: {d:.3e}; aligned against misaligned "
              f"{float((a - b).abs().max()):.3e}")
        assert d <= 1e-5 * float(want.abs().max())
        ref = R.target_logits(indptr, indices, _np(z), *(_np(v) for v in args), t, [])
        assert ref.c(_np(a[0])) <= A.BOUND_ONE and ref.c(_np(b[0])) <= A.BOUND_ONE


def test_target_logits_distance_to_the_model_on_the_flipped_operator_is_measured():
    """A (X W1^T) here, (A X) W1^T in the model: measured and printed, not bounded in advance"""
    worst = 0.0
    for name in ("iso120", "hub96"):
        c = case(name)
        indptr, indices, n = fixture_csr(name)
        model = gcn_of(c)
        x = torch.from_numpy(c["x"]).to(DEV)
        op = RowNormalizedAdjacency.from_dense(torch.from_numpy(c["adj"]).to(DEV))
        z = (x @ model.gc1.weight.t()).detach()
        dev = lambda a: torch.from_numpy(a).to(DEV)
        for r in c["meta"]["runs"][:12:4]:
            t, S = r["target"], sorted(set(r["partners"][:3]))
            got = target_logits(n, dev(indptr), dev(indices), z, model.gc1.bias.detach(), model.gc2.weight.detach(),
                                model.gc2.bias.detach(), t, [S])[0]
            with torch.no_grad():
                want = model(x, op.flipped([t] * len(S), S))[t]
            d = float((got - want).abs().max())
            worst = max(worst, d / float(want.abs().max()))
            print(f"{name} t={t} S={S}: |local - model on the flipped operator| = {d:.3e} "
                  f"(max |logit| {float(want.abs().max()):.3f})")
    print(f"largest relative distance: {worst:.3e}")
    assert np.isfinite(worst)


# ------------------------------------------------------------------------------------------------ Calib_FGA
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
    return [(name, r["run"]) for name in ("iso120", "hub96") for r in manifest()["cases"][name]["runs"]]


def run_fixture(name, i, local_eval, as_operator):
    c = case(name)
    meta = c["meta"]["runs"][i]
    r = {k.split("__", 1)[1]: v for k, v in c.items() if k.startswith(f"r{i}__")}
    surrogate = wats_of(c) if meta.get("surrogate") == "WATS" else gcn_of(c)
    x, y = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["y"]).to(DEV)
    adj = torch.from_numpy(c["adj"]).to(DEV)
    atk = Calib_FGA(surrogate, device=DEV, local_eval=local_eval)
    kw = dict(n_perturb=[], best_conf=[], runtime=[])
    raised = False
    with contextlib.redirect_stdout(io.StringIO()):
        try:
            getattr(atk, meta["method"])(x, RowNormalizedAdjacency.from_dense(adj) if as_operator else adj,
                                         meta["target"], c["meta"]["budget"], meta["strategy"], res_gt=y, **kw)
        except ValueError as e:
            assert "Final label" in str(e)
            raised = True
    return c, meta, r, atk, kw, raised


@pytest.mark.parametrize("local_eval", [True, False])
@pytest.mark.parametrize("name,i", all_runs())
def test_calib_fga_reproduces_the_recorded_run(name, i, local_eval):
    c, meta, r, atk, kw, raised = run_fixture(name, i, local_eval, as_operator=(i % 2 == 1))
    rec = c["meta"]["f32_vs_f64"]
    assert (atk._local is not None) == local_eval
    assert atk.flips == [int(j) for j in r["partner"]], (atk.flips, r["partner"])
    assert [s["label"] for s in atk.trace] == [int(v) for v in r["label"]]
    assert raised == bool(r["raised"])
    if not raised:
        assert kw["n_perturb"] == [int(r["n_perturb"])]
        assert atk.best_flips == [int(j) for j in r["best_set"]]
        d = abs(kw["best_conf"][0] - float(r["best_conf"]))
        print(f"best_conf distance {d:.3e} (tolerance {4 * rec['best_conf']:.3e})")
        assert d <= 4 * rec["best_conf"]
    worst = max(float(np.abs(_np(s["logits"]).astype(np.float64) - r["logits"][k]).max())
                for k, s in enumerate(atk.trace))
    print(f"{meta['method']} target {meta['target']} local_eval={local_eval}: logits distance {worst:.3e} "
          f"(tolerance {4 * rec['logits']:.3e})")
    assert worst <= 4 * rec["logits"]
    if meta["method"] == "flip_beam_hybridloss_attack":
        assert len(kw["runtime"]) == 1
    if not raised:
        want = c["adj"].copy()
        t = meta["target"]
        for j in r["best_set"]:
            want[t, j] = want[j, t] = 1 - want[t, j]
        if i % 2 == 1:                                    # an operator went in: modified_op, no dense matrix
            indptr, indices, values = atk.modified_op.csr()
            M = sp.csr_matrix(want)
            M.sort_indices()
            assert np.array_equal(_np(indptr), M.indptr) and np.array_equal(_np(indices), M.indices)
            assert np.array_equal(_np(values), M.data)
            with pytest.raises(AttributeError, match="modified_op"):
                atk.modified_adj
        else:
            assert torch.equal(atk.modified_adj.cpu(), torch.from_numpy(want))
            assert np.array_equal(_np(atk.modified_op.materialize().indices), sp.csr_matrix(want).indices)


def test_calib_fga_on_a_view_and_strategy_checks():
    c = case("hub96")
    meta = c["meta"]["runs"][3]
    x, y = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["y"]).to(DEV)
    op = RowNormalizedAdjacency.from_dense(torch.from_numpy(c["adj"]).to(DEV))
    t = meta["target"]
    first = meta["partners"][0]
    atk = Calib_FGA(gcn_of(c))
    kw = dict(n_perturb=[], best_conf=[])
    with contextlib.redirect_stdout(io.StringIO()) as log:
        atk.flip_beam_hybridloss_attack(x, op.with_flips([t], [first]), t, 2, "under", res_gt=y, verbose=True, **kw)
    assert atk.flips[0] == meta["partners"][1]            # the recorded run's second step, from a view of its first
    assert "Attack completed" in log.getvalue() and "Perturbations used" in log.getvalue()
    assert isinstance(atk.modified_op, wats_hip.FlippedAdjacency) and atk.modified_op.base is op
    with pytest.raises(ValueError, match="only supports 'under'"):
        atk.rerank_hybridloss_attack(x, op, t, 2, "over", res_gt=y, **kw)
    with pytest.raises(ValueError, match="Unknown strategy"):
        atk.attack(x, op, t, 2, "sideways", res_gt=y, **kw)
    with pytest.raises(ValueError, match="res_gt"):
        atk.attack(x, op, t, 2, "under", **kw)
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(TypeError):
        atk.attack(x, op, t, 2, "max", res_gt=y, **kw)    # the reference's own TypeError


def test_calib_fga_with_a_cagcn_surrogate_takes_the_view_path():
    """a smoke check of the general path: a calibrator whose head reads neighbours"""
    c = case("iso120")
    x, y = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["y"]).to(DEV)
    adj = torch.from_numpy(c["adj"]).to(DEV)
    cal = wats_hip.CaGCN(gcn_of(c), x, y, adj, torch.arange(0, 120, 3, device=DEV), graph=adj, epochs=2,
                         verbose=False).eval()
    atk = Calib_FGA(cal)
    kw = dict(n_perturb=[], best_conf=[])
    with contextlib.redirect_stdout(io.StringIO()):
        atk.rerank_hybridloss_attack(x, RowNormalizedAdjacency.from_dense(adj), 48, 3, "under", res_gt=y, **kw)
    assert atk._local is None and 1 <= len(atk.flips) <= 3 and len(kw["n_perturb"]) == 1
    assert 0.0 < kw["best_conf"][0] <= 1.0
