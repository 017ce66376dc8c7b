"""GPU tests that hold the two matrix-core kernel files (csrc/edgemlp.hip, csrc/simcalib.hip) to the bit-level models,
long-double truths and per-element units of tests/mfma_ref.py.  tests/test_mfma_precision_host.py derives the bounds on
the CPU and shows which wrong kernels they reject; none of them comes from a kernel run.

Edge MLP.  Forward: w must EQUAL model_edge_mlp_forward bit for bit at C = 1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48
(both edges of each of the six (NB0, NB1) instantiations), with and without dropout, on normal, positive and spread
embeddings.  Backward: the six parameter gradients and g_emb in units against the truth that takes its ReLU pattern
from the forward model, NO entry zeroed; a gradient through float32 chains is held to CHAIN_FACTOR times the documented
model's c on the same inputs (floor: the count of roundings), g_b2 and g_b3 to their counts of roundings.  Every C
runs on every graph: the star, nnz1023 / 1024 / 1025 / 2049, rmat300 and the hub of 2 * 1024 + 100 leaves.
Kink sides: an upstream gradient on entries whose forward weight is exactly 0 gives gradients that are exactly 0, and
one on the entries with w > 0 gives g_b3 = fl32(float64 sum of g_w): the recomputing backward takes the forward's side.

SimCalib.  stats[:, 0] (the running maximum) must EQUAL max_j of model_sim_scores bit for bit: that holds the MFMA
operand layout, the -inf masks of the rows past m and the maximum with no tolerance.  t == fl32(stats[:, 2]) bitwise,
1 <= stats[:, 1] <= m up to the exp allowance, and t under truth (A) and (B) and gx inside CHAIN_FACTOR times the
model's c plus the allowance for the device's expf (mfma_ref.expf_allowance).  Every test prints c, the bound and the
model's c.
"""
import itertools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cheb_ref as C  # noqa: E402
import mfma_ref as M  # noqa: E402
import test_dcgc as TD  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip import simcalib  # noqa: E402

DEV = "cuda"
BIG = 1e30
KINDS = ("normal", "positive", "spread")
PS = (0.0, 0.5)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()
    assert wats_hip.dcgc.edge_mlp_tile() == M.TILE


_graphs = {}


def device_graph(name):
    """test_dcgc.py's graphs, and `hub`: node 0 with 2 * 1024 + 100 leaves"""
    if name != "hub":
        return TD.device_graph(name)
    if name not in _graphs:
        import types
        n, rows, cols = M.hub_graph(2 * M.TILE + 100)
        indptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
        g = wats_hip.EdgeWeightGraph(types.SimpleNamespace(n=n, indptr=indptr, indices=cols.astype(np.int32)),
                                     device=DEV)
        _graphs[name] = (g, torch.from_numpy(rows), torch.from_numpy(cols))
    return _graphs[name]


def seed_of(gname, Cw, p):
    """test_dcgc.py's seeds (with its RESEED steps where the case is one of its own)"""
    names = TD.GRAPHS + ["hub"]
    return 1000 + 7 * Cw + int(10 * p) + 100 * names.index(gname) + 10000 * TD.RESEED.get((gname, Cw, p), 0)


def run_kernel(graph, emb, params, p, seed, g_w, want_emb=True):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    w, gp, ge = TD.run_kernel(graph, t(emb), [t(a) for a in params], p, seed, t(g_w), want_emb)
    return w.cpu().numpy(), [g.cpu().numpy() for g in gp], None if ge is None else ge.cpu().numpy()


# ---------------------------------------------------------------------------------------------- edge MLP, forward
FWD_GRAPHS = ["path", "directed", "star", f"nnz{M.TILE + 1}"]
FWD_CASES = [(g, Cw, PS[(gi + ci) % 2], KINDS[(gi + ci) % 3])
             for gi, g in enumerate(FWD_GRAPHS) for ci, Cw in enumerate(M.MLP_CS)]


def test_forward_cases_cover_every_pair():
    for i, j in itertools.combinations(range(4), 2):
        have = {(c[i], c[j]) for c in FWD_CASES}
        want = set(itertools.product(*[(FWD_GRAPHS, M.MLP_CS, PS, KINDS)[k] for k in (i, j)]))
        assert have == want, (i, j, want - have)
    assert {M.mlp_shape(Cw) for Cw in M.MLP_CS} == {(1, 1), (1, 2), (2, 3), (2, 4), (3, 5), (3, 6)}


@pytest.mark.parametrize("gname,Cw,p,kind", FWD_CASES)
def test_edge_mlp_forward_is_the_model_bit_for_bit(gname, Cw, p, kind):
    graph, rows, cols = device_graph(gname)
    rows, cols = rows.numpy(), cols.numpy()
    seed = seed_of(gname, Cw, p)
    emb, params, g_w = M.mlp_inputs(graph.n, rows, cols, Cw, p, seed, kind)
    fwd = M.model_edge_mlp_forward(emb, params, rows, cols, p, seed)
    val, unit = M.edge_mlp_truth(graph.n, emb, params, rows, cols, fwd, None)
    w = run_kernel(graph, emb, params, p, seed, g_w, want_emb=False)[0]
    share = float((fwd["w"] > 0).mean())
    diff = int(np.count_nonzero(w.view(np.int32) != fwd["w"].view(np.int32)))
    print(f"{gname} C={Cw} p={p} {kind}: {share:.0%} positive, c={C.c_of(w, val['w'], unit['w']):.3f} "
          f"model c={C.c_of(fwd['w'], val['w'], unit['w']):.3f} bound: equal bits ({diff} of {w.size} differ)")
    if len(rows) >= 16:
        assert 0.1 <= share <= 0.9, share        # both sides of the last ReLU are exercised
    assert torch.equal(torch.from_numpy(w), torch.from_numpy(fwd["w"]))


# ---------------------------------------------------------------------------------------------- edge MLP, backward
# every width on every graph
BWD_GRAPHS = ["star", f"nnz{M.TILE - 1}", f"nnz{M.TILE}", f"nnz{M.TILE + 1}", f"nnz{2 * M.TILE + 1}", "rmat300", "hub"]
BWD_CASES = [(g, Cw, PS[(gi + ci) % 2], KINDS[(gi + ci) % 3])
             for gi, g in enumerate(BWD_GRAPHS) for ci, Cw in enumerate(M.MLP_CS)]
# floors: the float32 roundings on one term's way (mfma_ref's docstring); b2 and b3 pass through no chain
COUNTED = {"b3": 1.0 + M.SLACK,     # d3 = g or 0 exactly, a float64 sum, one rounding
           "b2": 3.0 + M.SLACK}     # fl(fl(d3 w3) scale), a float64 sum, one rounding
FLOOR = 4.0 + M.SLACK               # d2's two roundings, one of d1 / h1 / h2 / the per-entry g_emb value, the result


def test_backward_cases_cover_every_width_on_every_graph():
    assert {(c[0], c[1]) for c in BWD_CASES} == set(itertools.product(BWD_GRAPHS, M.MLP_CS))
    assert {(c[0], c[2]) for c in BWD_CASES} == set(itertools.product(BWD_GRAPHS, PS))
    assert {(c[0], c[3]) for c in BWD_CASES} == set(itertools.product(BWD_GRAPHS, KINDS))


@pytest.mark.parametrize("gname,Cw,p,kind", BWD_CASES)
def test_edge_mlp_backward_in_units(gname, Cw, p, kind):
    graph, rows, cols = device_graph(gname)
    rows, cols = rows.numpy(), cols.numpy()
    n, seed = graph.n, seed_of(gname, Cw, p)
    emb, params, g_w = M.mlp_inputs(n, rows, cols, Cw, p, seed, kind)
    fwd = M.model_edge_mlp_forward(emb, params, rows, cols, p, seed)
    val, unit = M.edge_mlp_truth(n, emb, params, rows, cols, fwd, g_w)
    model = M.model_edge_mlp_backward(n, emb, params, rows, cols, p, fwd, g_w)
    w, gp, ge = run_kernel(graph, emb, params, p, seed, g_w)
    assert np.array_equal(w.view(np.int32), fwd["w"].view(np.int32))     # the pattern of the truth is the kernel's
    what = f"{gname} C={Cw} p={p} {kind}"
    got = dict(zip(M.NAMES, gp), g_emb=ge)
    failures = []
    for name in M.NAMES + ("g_emb",):
        parts = [("", slice(None))]
        if name == "g_emb" and gname in ("star", "hub"):
            parts += [(" hub", slice(0, 1)), (" leaves", slice(1, None))]
        for tag, sel in parts:
            c = C.c_of(got[name].reshape(val[name].shape)[sel], val[name][sel], unit[name][sel], f"{what} g_{name}")
            cm = C.c_of(model[name].reshape(val[name].shape)[sel], val[name][sel], unit[name][sel])
            bound = COUNTED.get(name) or max(M.CHAIN_FACTOR * cm, FLOOR)
            print(f"{what} g_{name}{tag}: c={c:.3f} bound={bound:.3f} model c={cm:.3f}")
            if c > bound:
                failures.append(f"g_{name}{tag}: c {c:.3f} > {bound:.3f}")
    assert not failures, f"{what}: " + "; ".join(failures)
    # without g_emb: the same parameter gradients, bit for bit
    _, gp2, none = run_kernel(graph, emb, params, p, seed, g_w, want_emb=False)
    assert none is None
    for a, b in zip(gp, gp2):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("Cw", M.MLP_CS)
@pytest.mark.parametrize("gname", ["star", f"nnz{2 * M.TILE + 1}"])
def test_backward_takes_the_forwards_side_of_the_last_kink(gname, Cw):
    graph, rows, cols = device_graph(gname)
    rows, cols = rows.numpy(), cols.numpy()
    p = PS[Cw % 2]
    seed = seed_of(gname, Cw, p)
    emb, params, g_w = M.mlp_inputs(graph.n, rows, cols, Cw, p, seed, "normal")
    w = run_kernel(graph, emb, params, p, seed, g_w, want_emb=False)[0]
    dead = w == 0
    assert 0.1 <= float(dead.mean()) <= 0.9
    _, gp, ge = run_kernel(graph, emb, params, p, seed, np.where(dead, g_w, np.float32(0)))
    for name, g in zip(M.NAMES + ("g_emb",), gp + [ge]):
        assert not np.any(g), f"{gname} C={Cw}: g_{name} is not zero with g_w on entries of weight 0 only"
    live = np.where(dead, np.float32(0), g_w)
    _, gp, _ = run_kernel(graph, emb, params, p, seed, live, want_emb=False)
    want = np.float32(math.fsum(float(v) for v in live))
    print(f"{gname} C={Cw} p={p}: g_b3={float(gp[5][0])!r} fl32(sum g_w over w > 0)={float(want)!r}")
    assert gp[5][0] == want


# -------------------------------------------------------------------------------------------------------- SimCalib
NS, MS, DS, TAUS = [1, 33, 129], [1, 4, 5, 32, 33, 257], [1, 32, 33, 64, 128, 129, 256], [0.01, 0.1, 1.0]
T_FLOOR = 2.0 + M.SLACK      # the rounding of x - max (in the unit), the result's
GX_FLOOR = 8.0 + M.SLACK     # v - thi, the two products of p, coef, a, a * fd, the difference, the quotient


def sim_shapes():
    seen, out = set(), []
    for n, m, d in [(129, 257, 256)] + list(itertools.product(NS, MS, DS)):
        pairs = {("nm", n, m), ("nd", n, d), ("md", m, d)}
        if not pairs <= seen:
            seen |= pairs
            out.append((n, m, d, TAUS[len(out) % 3]))
    return out


SIM_SHAPES = sim_shapes()


def test_simcalib_shapes_cover_every_pair():
    for a, b, key in ((NS, MS, lambda s: (s[0], s[1])), (NS, DS, lambda s: (s[0], s[2])),
                      (MS, DS, lambda s: (s[1], s[2]))):
        assert {key(s) for s in SIM_SHAPES} == set(itertools.product(a, b))
    assert {s[3] for s in SIM_SHAPES} == set(TAUS)


def sim_kernel(x, bank, v, gt, tau, bank_dev=None):
    """(t, stats, gx) of the HIP path; bank_dev: a device tensor to use as the bank as it stands"""
    xd = torch.from_numpy(x).to(DEV)
    bd = torch.from_numpy(bank).to(DEV) if bank_dev is None else bank_dev
    vd = torch.from_numpy(v).to(DEV)
    t, stats = simcalib._forward(xd, bd, vd, tau)
    xg = xd.clone().requires_grad_(True)
    t2 = wats_hip.similarity_temperature(xg, bd, vd, tau, -BIG, BIG)
    (t2 * torch.from_numpy(gt).to(DEV)).sum().backward()
    assert torch.equal(t, t2.detach())
    return t.cpu().numpy(), stats.cpu().numpy(), xg.grad.cpu().numpy()


def sim_check(x, bank, v, gt, tau, what, bank_dev=None):
    """every SimCalib assertion of the module docstring for one case; returns (gx c, the model's gx c)"""
    m = bank.shape[0]
    sc = M.model_sim_scores(x, bank, tau)
    tr = M.sim_truth(x, bank, v, gt, tau, sc)
    tm, sm, exps = M.model_sim_forward(sc["xs"], v)
    gm = M.model_sim_backward(x, bank, v, gt, sc, sm)
    t, stats, gx = sim_kernel(x, bank, v, gt, tau, bank_dev)
    same = np.array_equal(stats[:, 0].view(np.int64), sc["xs"].max(1).astype(np.float64).view(np.int64))
    print(f"{what}: row maxima {'equal' if same else 'DIFFER from'} the model's bits")
    assert same
    assert np.array_equal(t.view(np.int32), stats[:, 2].astype(np.float32).view(np.int32))
    tol = 2.0 * float(exps.max()) * M.EXPF_ULP * 2.0 ** -24 + 2.0 ** -40
    assert np.all(stats[:, 1] >= 1 - tol) and np.all(stats[:, 1] <= m * (1 + tol)), (stats[:, 1].min(), stats[:, 1].max())
    failures = []
    allow_t = M.expf_allowance(exps, tr["tA_exp"][1])
    for key in ("tA", "tB"):
        c = M.c_after(t, *tr[key], allow_t, f"{what} {key}")
        cm = C.c_of(tm, *tr[key])
        bound = max(M.CHAIN_FACTOR * cm, T_FLOOR)
        print(f"{what} t against truth ({key[1]}): c={c:.3f} bound={bound:.3f} model c={cm:.3f} "
              f"(raw c={C.c_of(t, *tr[key]):.3f}, up to {int(exps.max())} exps per term)")
        if c > bound:
            failures.append(f"{key}: c {c:.3f} > {bound:.3f}")
    # the backward's own exp, and the forward's den and t that it reads (their exps)
    c = M.c_after(gx, *tr["gx"], M.gx_allowance(exps, tr), f"{what} gx")
    cm = C.c_of(gm, *tr["gx"])
    bound = max(M.CHAIN_FACTOR * cm, GX_FLOOR)
    print(f"{what} gx: c={c:.3f} bound={bound:.3f} model c={cm:.3f} (raw c={C.c_of(gx, *tr['gx']):.3f})")
    if c > bound:
        failures.append(f"gx: c {c:.3f} > {bound:.3f}")
    assert not failures, f"{what}: " + "; ".join(failures)
    return C.c_of(gx, *tr["gx"]), cm


@pytest.mark.parametrize("n,m,d,tau", SIM_SHAPES)
def test_simcalib_shapes(n, m, d, tau):
    sim_check(*M.sim_inputs(n, m, d, 1000 * n + 10 * m + d), tau, f"n={n} m={m} d={d} tau={tau}")


@pytest.mark.parametrize("kind,n,m,d,tau", [("spread", 129, 33, 64, 0.1), ("spread", 33, 257, 129, 0.01),
                                            ("dominant", 129, 33, 128, 0.1), ("dominant", 33, 257, 32, 0.01),
                                            ("flat", 129, 257, 33, 0.1), ("flat", 33, 33, 64, 1.0)])
def test_simcalib_hard_inputs(kind, n, m, d, tau):
    """rows whose gx differ by 10^6 (spread), a weight near 1 (dominant), sum_j w_ij (v_j - t_i) with v nearly
    constant (flat: what the float32 pair for t_i is for)"""
    sim_check(*M.sim_inputs(n, m, d, 7 + n + m + d, kind), tau, f"{kind} n={n} m={m} d={d} tau={tau}")


@pytest.mark.parametrize("n,m,d", [(33, 33, 32), (129, 5, 64), (33, 257, 128)])
def test_simcalib_scalar_staging_of_a_misaligned_bank(n, m, d):
    """d % 4 == 0 and a bank base that is 4-byte but not 16-byte aligned: stage_tile's scalar path, never taken by the
    other tests; the same bits as the vector path"""
    x, bank, v, gt = M.sim_inputs(n, m, d, 31 + d)
    store = torch.zeros(m * d + 1, device=DEV)
    view = store[1:].view(m, d)
    view.copy_(torch.from_numpy(bank))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    sim_check(x, bank, v, gt, 0.1, f"misaligned bank n={n} m={m} d={d}", bank_dev=view)
    a, b = sim_kernel(x, bank, v, gt, 0.1), sim_kernel(x, bank, v, gt, 0.1, view)
    for u, w in zip(a, b):
        assert np.array_equal(u, w)


def test_simcalib_long_bank():
    """ga += P . B_tile is ONE float32 chain over the whole bank: its c at m = 4097 beside m = 257, the kernel's and
    the model's, both held to CHAIN_FACTOR times the model's (the workload's bank is 7 times longer)"""
    out = {}
    for m in (257, 4097):
        out[m] = sim_check(*M.sim_inputs(33, m, 32, 4097), 0.1, f"long bank m={m}")
    (c0, m0), (c1, m1) = out[257], out[4097]
    print(f"gx chain growth from m=257 to m=4097: kernel {c0:.3f} -> {c1:.3f} (x{c1 / c0:.2f}), "
          f"model {m0:.3f} -> {m1:.3f} (x{m1 / m0:.2f})")
