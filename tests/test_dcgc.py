"""GPU tests of the DCGC calibrator's kernels (csrc/edgemlp.hip, csrc/edgeagg.hip, wats_hip/dcgc.py) against the dense
restatement of tests/dcgc_ref.py.

The bound on every value is the project's rule (gats_ref.assert_close): err = max|kernel - ref64| must not exceed
max(2 * max|ref32 - ref64|, 4 * 2^-24 * max|ref64|), ref32 / ref64 the restatement on the CPU in float32 / float64
from the same float32 inputs and the same hashed dropout masks.  Gradient tests zero the upstream gradient of every
entry that has a pre-activation within 64 * 2^-24 * max|z| of a ReLU kink (a float32 run may take the other side
there); at most 2 % of the entries may be zeroed, which is asserted.  30-70 % of the weights must be positive.  For the
calibrator the fixture that the reference recorded is the float32 side, and the float64 side is the restatement from
the fixture's inputs.

Where the inputs differ from the issue's recipe, and why:
  * b3 is not -median(z3) but minus a point between two adjacent values of z3 near the median (median_split):
    -median(z3) itself puts the median entry's z3 at exactly zero, a kink in every case, and with dropout at C = 1 a
    large share of the entries ties at one value, which the median then sits on.
  * Four cases take a later seed (RESEED): at their first seed the inputs themselves miss the kink or positive-share
    condition.  The seeds were searched on the CPU from the float64 restatement alone, before any kernel run.
  * The positive-share assertion needs a share to speak of: it runs from 16 entries up, so not on the `loop` graph (one
    entry) nor on `path` and `directed` (ten entries each).  The kink condition is asserted on every graph.
"""
import ctypes
import itertools
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import dcgc_ref as R  # noqa: E402
import gats_ref  # noqa: E402
import wats_hip  # noqa: E402
from models import CompatibleGCN  # noqa: E402
from wats_hip import dcgc  # noqa: E402
from wats_hip.graphgen import rmat_graph  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dcgc")
TILE = 1024      # wg_edge_mlp_tile(), asserted below


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()
    assert dcgc.edge_mlp_tile() == TILE


# ---------------------------------------------------------------------------------------------------------
# graphs: (n, rows, cols) in row-major order, no duplicates
# ---------------------------------------------------------------------------------------------------------
def canonical(n, rows, cols):
    key = np.unique(np.asarray(rows, np.int64) * n + np.asarray(cols, np.int64))
    return n, key // n, key % n


def random_pattern(n, nnz, seed):
    key = np.sort(np.random.default_rng(seed).choice(n * n, nnz, replace=False))
    return n, key // n, key % n


def make_graph(name):
    if name == "empty":
        return 5, np.zeros(0, np.int64), np.zeros(0, np.int64)
    if name == "loop":
        return canonical(3, [1], [1])
    if name == "path":
        s = np.arange(5)
        return canonical(6, np.r_[s, s + 1], np.r_[s + 1, s])
    if name == "directed":     # row 3 and column 5 are empty
        return canonical(7, [0, 0, 1, 2, 2, 4, 5, 5, 6, 6], [1, 2, 2, 0, 3, 4, 0, 6, 1, 3])
    if name == "star":         # node 0: 300 entries as a row and as a column
        leaves = np.arange(1, 301)
        ids = np.arange(301)
        return canonical(301, np.r_[np.zeros(300, np.int64), leaves, ids], np.r_[leaves, np.zeros(300, np.int64), ids])
    if name == "rmat300":
        a = rmat_graph(300, 2400, seed=5).to_scipy().tocoo()
        ids = np.arange(300)
        return canonical(300, np.r_[a.row, a.col, ids], np.r_[a.col, a.row, ids])
    if name.startswith("nnz"):
        return random_pattern(200, int(name[3:]), 11)
    raise KeyError(name)


GRAPHS = ["empty", "loop", "path", "directed", "star", "rmat300", f"nnz{TILE - 1}", f"nnz{TILE}", f"nnz{TILE + 1}",
          f"nnz{2 * TILE + 1}"]
CS, PS = [1, 3, 7, 40, 41], [0.0, 0.5]
LARGEST = (f"nnz{2 * TILE + 1}", 41, 0.5)


def pairwise_cover():
    seen, out = set(), []
    for g, C, p in [LARGEST] + list(itertools.product(GRAPHS, CS, PS)):
        pairs = {("gc", g, C), ("gp", g, p), ("cp", C, p)}
        if not pairs <= seen:
            seen |= pairs
            out.append((g, C, p))
    return out


CASES = pairwise_cover()
_graphs = {}


def device_graph(name):
    if name not in _graphs:
        n, rows, cols = make_graph(name)
        indptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
        g = wats_hip.EdgeWeightGraph(types.SimpleNamespace(n=n, indptr=indptr, indices=cols.astype(np.int32)),
                                     device=DEV)
        _graphs[name] = (g, torch.from_numpy(rows), torch.from_numpy(cols))
    return _graphs[name]


def make_mlp(n, rows, cols, C, p, seed):
    """emb N(0, 1), default nn.Linear initialisation, b3 = -median(z3) with the masks of (p, seed)."""
    torch.manual_seed(seed)
    lin = [nn.Linear(2 * C, 4 * C), nn.Linear(4 * C, 2 * C), nn.Linear(2 * C, 1)]
    params = [t.detach().clone() for l in lin for t in (l.weight, l.bias)]
    emb = torch.randn(n, C)
    masks = R.dropout_masks(rows.numel(), C, p, seed, torch.float64) if p else None
    if rows.numel():
        z3 = R.edge_mlp(emb, params, rows, cols, masks, torch.float64)[3] - params[5].double()
        params[5] = (-median_split(z3)).float().reshape(1)
    g_w = torch.randn(rows.numel())
    return emb, params, masks, g_w


def median_split(z3):
    """The median of z3 as a point BETWEEN two of its values: -median(z3) itself makes the median entry's z3 exactly
    zero (a kink in every case), and with dropout a large share of the entries ties at one value (h2 == 0).  Of the
    midpoints of adjacent distinct values that leave 35-65 % of the entries above, the one in the widest gap; if
    there is none, the one closest to an even split; a single value: one below it."""
    v, counts = torch.unique(z3, return_counts=True)
    if v.numel() < 2:
        return v[0] - 1.0
    mids, gaps = (v[:-1] + v[1:]) / 2, v[1:] - v[:-1]
    above = 1.0 - counts.cumsum(0)[:-1].double() / z3.numel()     # the share of z3 above each midpoint
    ok = (above >= 0.35) & (above <= 0.65)
    if bool(ok.any()):
        return mids[torch.where(ok, gaps, torch.zeros_like(gaps)).argmax()]
    return mids[(above - 0.5).abs().argmin()]


# Cases whose first seed misses the conditions on the inputs (asserted in test_edge_mlp): on a graph of ten entries
# one entry on a kink is 10 %, and with C = 1 and dropout the two units of the second layer are dead or dropped
# together on most entries for some initialisations, so no offset leaves 30-70 % of the weights positive.  The value
# is the number of 10000-steps added to the seed until the inputs meet them (searched on the CPU, no kernel run).
RESEED = {("star", 1, 0.5): 1, (f"nnz{TILE - 1}", 1, 0.0): 1, (f"nnz{TILE}", 1, 0.5): 2, (f"nnz{2 * TILE + 1}", 1, 0.0): 2}


def case_seed(gname, C, p):
    return 1000 + 7 * C + int(10 * p) + 100 * GRAPHS.index(gname) + 10000 * RESEED.get((gname, C, p), 0)


def run_kernel(graph, emb, params, p, seed, g_w, want_emb=True):
    e = emb.to(DEV).requires_grad_(want_emb)
    leaves = [t.to(DEV).requires_grad_(True) for t in params]
    w = wats_hip.edge_mlp_weights(graph, e, leaves, p, seed)
    (w * g_w.to(DEV)).sum().backward()
    return w.detach(), [t.grad for t in leaves], e.grad


NAMES = ["W1", "b1", "W2", "b2", "w3", "b3"]


@pytest.mark.parametrize("gname,C,p", CASES)
def test_edge_mlp(gname, C, p):
    graph, rows, cols = device_graph(gname)
    seed = case_seed(gname, C, p)
    emb, params, masks, g_w = make_mlp(graph.n, rows, cols, C, p, seed)
    nnz = rows.numel()
    if nnz:
        kink = R.kink_entries(emb, params, rows, cols, masks)
        share = float(kink.float().mean())
        print(f"{gname} C={C} p={p}: {share:.2%} of the entries sit on a kink")
        assert share <= 0.02
        g_w[kink] = 0.0
    w32, gp32, ge32 = R.edge_mlp_and_grads(emb, params, rows, cols, g_w, masks, torch.float32)
    w64, gp64, ge64 = R.edge_mlp_and_grads(emb, params, rows, cols, g_w, masks, torch.float64)
    if nnz >= 16:
        positive = float((w64 > 0).double().mean())
        assert 0.3 <= positive <= 0.7, positive
    w, gp, ge = run_kernel(graph, emb, params, p, seed, g_w)
    what = f"{gname} C={C} p={p}"
    assert w.shape == (nnz,)
    gats_ref.assert_close(w, w32, w64, what + " w")
    for name, a, b, c in zip(NAMES, gp, gp32, gp64):
        gats_ref.assert_close(a, b, c, f"{what} g_{name}")
    gats_ref.assert_close(ge, ge32, ge64, what + " g_emb")
    # without g_emb: the same parameter gradients, bit for bit
    _, gp2, none = run_kernel(graph, emb, params, p, seed, g_w, want_emb=False)
    assert none is None
    for a, b in zip(gp, gp2):
        assert torch.equal(a, b)


def test_more_tiles_than_workgroups():
    """257 tiles and one entry: a backward workgroup walks more than one tile (its float64 partial and the node walk
    carry over), and every row of about 440 entries runs through a tile boundary's carry slot or ends beside one."""
    n, C, p, seed = 600, 3, 0.5, 77
    nnz = 257 * TILE + 1
    _, r, c = random_pattern(n, nnz, 3)
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=indptr[1:])
    graph = wats_hip.EdgeWeightGraph(types.SimpleNamespace(n=n, indptr=indptr, indices=c.astype(np.int32)), device=DEV)
    rows, cols = torch.from_numpy(r), torch.from_numpy(c)
    emb, params, masks, g_w = make_mlp(n, rows, cols, C, p, seed)
    kink = R.kink_entries(emb, params, rows, cols, masks)
    assert float(kink.float().mean()) <= 0.02
    g_w[kink] = 0.0
    w32, gp32, ge32 = R.edge_mlp_and_grads(emb, params, rows, cols, g_w, masks, torch.float32)
    w64, gp64, ge64 = R.edge_mlp_and_grads(emb, params, rows, cols, g_w, masks, torch.float64)
    w, gp, ge = run_kernel(graph, emb, params, p, seed, g_w)
    gats_ref.assert_close(w, w32, w64, "257 tiles w")
    for name, a, b, c64 in zip(NAMES, gp, gp32, gp64):
        gats_ref.assert_close(a, b, c64, f"257 tiles g_{name}")
    gats_ref.assert_close(ge, ge32, ge64, "257 tiles g_emb")


def hub_graph(leaves):
    """Node 0 with `leaves` entries as a row and as a column, and the self loops."""
    l, ids = np.arange(1, leaves + 1), np.arange(leaves + 1)
    z = np.zeros(leaves, np.int64)
    return canonical(leaves + 1, np.r_[z, l, ids], np.r_[l, z, ids])


def test_hub_longer_than_two_tiles():
    """A node whose entries fill whole tiles, as a row (CSR order) and as a column (transposed order): its sum is the
    first tile's own part plus a chain of carries, one of them from a tile that holds nothing else."""
    C, p, seed = 3, 0.5, 91
    n, r, c = hub_graph(2 * TILE + 100)
    assert int((r == 0).sum()) > 2 * TILE and int((c == 0).sum()) > 2 * TILE
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=indptr[1:])
    graph = wats_hip.EdgeWeightGraph(types.SimpleNamespace(n=n, indptr=indptr, indices=c.astype(np.int32)), device=DEV)
    rows, cols = torch.from_numpy(r), torch.from_numpy(c)
    emb, params, masks, g_w = make_mlp(n, rows, cols, C, p, seed)
    kink = R.kink_entries(emb, params, rows, cols, masks)
    assert float(kink.float().mean()) <= 0.02
    g_w[kink] = 0.0
    w32, gp32, ge32 = R.edge_mlp_and_grads(emb, params, rows, cols, g_w, masks, torch.float32)
    w64, gp64, ge64 = R.edge_mlp_and_grads(emb, params, rows, cols, g_w, masks, torch.float64)
    positive = float((w64 > 0).double().mean())
    assert 0.3 <= positive <= 0.7, positive
    w, gp, ge = run_kernel(graph, emb, params, p, seed, g_w)
    gats_ref.assert_close(w, w32, w64, "long hub w")
    for name, a, b, c64 in zip(NAMES, gp, gp32, gp64):
        gats_ref.assert_close(a, b, c64, f"long hub g_{name}")
    gats_ref.assert_close(ge, ge32, ge64, "long hub g_emb")
    gats_ref.assert_close(ge[:1], ge32[:1], ge64[:1], "long hub g_emb of the hub")


def test_every_value_and_pair_is_covered():
    for a, b, key in ((GRAPHS, CS, lambda s: (s[0], s[1])), (GRAPHS, PS, lambda s: (s[0], s[2])),
                      (CS, PS, lambda s: (s[1], s[2]))):
        assert {key(s) for s in CASES} == set(itertools.product(a, b))


def test_dropout_seeds_and_kept_share():
    graph, rows, cols = device_graph("rmat300")
    emb, params, _, g_w = make_mlp(graph.n, rows, cols, 7, 0.0, 3)
    a = run_kernel(graph, emb, params, 0.5, 1, g_w)[0]
    b = run_kernel(graph, emb, params, 0.5, 2, g_w)[0]
    c = run_kernel(graph, emb, params, 0.0, 1, g_w)[0]
    assert not torch.equal(a, b) and not torch.equal(a, c)
    for layer in (1, 2):
        keep = R.keep_mask(12345, layer, 4000, 28, 0.5)
        assert keep.size >= 10 ** 5 and abs(float(keep.mean()) - 0.5) <= 0.02
    # the kernel's masks ARE the hashed ones: with them the restatement reproduces a p = 0.5 run
    masks = R.dropout_masks(rows.numel(), 7, 0.5, 1, torch.float64)
    w32 = R.edge_mlp(emb, params, rows, cols, masks, torch.float32)[0]
    w64 = R.edge_mlp(emb, params, rows, cols, masks, torch.float64)[0]
    gats_ref.assert_close(a, w32, w64, "p=0.5 against the hashed masks")
    other = R.edge_mlp(emb, params, rows, cols, R.dropout_masks(rows.numel(), 7, 0.5, 2, torch.float64),
                       torch.float64)[0]
    assert float((a.double().cpu() - other).abs().max()) > 100 * gats_ref.error_bound(w32, w64)[0]


def test_two_calls_are_bit_identical():
    graph, rows, cols = device_graph(LARGEST[0])
    emb, params, _, g_w = make_mlp(graph.n, rows, cols, 41, 0.5, 4)
    a, b = run_kernel(graph, emb, params, 0.5, 9, g_w), run_kernel(graph, emb, params, 0.5, 9, g_w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    x = torch.randn(graph.n, 40)
    wts = torch.rand(graph.nnz)
    outs = []
    for _ in range(2):
        wd, xd = wts.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
        y = wats_hip.weighted_propagate(graph, wd, xd)
        y.square().sum().backward()
        outs.append((y.detach(), wd.grad, xd.grad))
    for u, v in zip(*outs):
        assert torch.equal(u, v)


def test_nan_row_reaches_only_its_incident_entries():
    graph, rows, cols = device_graph("rmat300")
    emb, params, _, g_w = make_mlp(graph.n, rows, cols, 7, 0.0, 5)
    clean = run_kernel(graph, emb, params, 0.0, 0, g_w)[0].cpu()
    emb[40, 2] = float("nan")
    w = run_kernel(graph, emb, params, 0.0, 0, g_w)[0].cpu()
    incident = (rows == 40) | (cols == 40)
    assert int(incident.sum()) > 1
    assert bool(torch.isnan(w[incident]).all())
    assert torch.equal(w[~incident], clean[~incident])


# ---------------------------------------------------------------------------------------------------------
# the value-carrying aggregation
# ---------------------------------------------------------------------------------------------------------
def dense_of(n, rows, cols, w, dtype):
    return torch.zeros(n, n, dtype=dtype).index_put((rows, cols), w.to(dtype))


@pytest.mark.parametrize("C", [1, 3, 4, 40, 41])
@pytest.mark.parametrize("gname", ["directed", "star", "rmat300"])
def test_aggregate_forms(gname, C):
    """Forward, transposed with the map, both scales on and off, an aligned and a misaligned x."""
    graph, rows, cols = device_graph(gname)
    n = graph.n
    g = torch.Generator().manual_seed(C)
    w = torch.rand(graph.nnz, generator=g) + 0.1
    x = torch.randn(n, C, generator=g)
    s = torch.rand(n, generator=g) + 0.5
    wd, sd = w.to(DEV), s.to(DEV)
    flat = torch.zeros(n * C + 1, device=DEV)
    flat[1:] = x.to(DEV).flatten()
    misaligned = flat[1:].view(n, C)
    assert misaligned.data_ptr() % 16 != 0 and misaligned.is_contiguous()
    for xd in (x.to(DEV), misaligned):
        for transposed in (False, True):
            for use_r, use_c in itertools.product((False, True), repeat=2):
                got = graph._aggregate(transposed, wd, sd if use_r else None, sd if use_c else None, xd)
                refs = []
                for dt in (torch.float32, torch.float64):
                    a = dense_of(n, rows, cols, w, dt)
                    a = a.t() if transposed else a
                    y = x.to(dt) * s.to(dt).unsqueeze(1) if use_c else x.to(dt)
                    y = a @ y
                    refs.append(y * s.to(dt).unsqueeze(1) if use_r else y)
                gats_ref.assert_close(got, refs[0], refs[1], f"{gname} C={C} T={transposed} r={use_r} c={use_c}")


@pytest.mark.parametrize("C", [3, 40])
@pytest.mark.parametrize("gname", ["directed", "star", "rmat300"])
def test_weighted_propagate_and_its_gradients(gname, C):
    """y, the gradient w.r.t. x and the value gradient (g . x_c - g . y_r) / deg_r in float64; one row's weights are
    all zero (deg -> 1, y = 0)."""
    graph, rows, cols = device_graph(gname)
    n = graph.n
    g = torch.Generator().manual_seed(10 + C)
    w = torch.rand(graph.nnz, generator=g) + 0.1
    zero_row = int(rows[len(rows) // 2])
    w[rows == zero_row] = 0.0
    x = torch.randn(n, C, generator=g)
    gy = torch.randn(n, C, generator=g)
    wd, xd = w.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    y = wats_hip.weighted_propagate(graph, wd, xd)
    (y * gy.to(DEV)).sum().backward()
    assert float(y.detach()[zero_row].abs().max()) == 0.0
    refs = []
    for dt in (torch.float32, torch.float64):
        wl, xl = w.detach().clone().to(dt).requires_grad_(True), x.detach().clone().to(dt).requires_grad_(True)
        yr = R.propagate(rows, cols, n, wl, xl, dt)
        (yr * gy.to(dt)).sum().backward()
        refs.append((yr.detach(), wl.grad, xl.grad))
    what = f"{gname} C={C}"
    gats_ref.assert_close(y, refs[0][0], refs[1][0], what + " y")
    gats_ref.assert_close(xd.grad, refs[0][2], refs[1][2], what + " gx")
    gats_ref.assert_close(wd.grad, refs[0][1], refs[1][1], what + " gw")
    # the documented formula in float64
    w64, x64, g64 = w.double(), x.double(), gy.double()
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, rows, w64)
    deg[deg == 0] = 1
    y64 = refs[1][0]
    formula = ((g64[rows] * x64[cols]).sum(1) - (g64[rows] * y64[rows]).sum(1)) / deg[rows]
    assert float((formula - refs[1][1]).abs().max()) <= 1e-12 * float(formula.abs().max())


def test_pair_inv_distance():
    graph, rows, cols = device_graph("rmat300")
    n, C, alpha = graph.n, 7, 0.5
    q = torch.softmax(torch.randn(n, C, generator=torch.Generator().manual_seed(1)), dim=1)
    q[11] = q[10]                                        # identical rows
    q[21] = q[20]
    q[21, 3] = torch.nextafter(q[20, 3], torch.tensor(2.0))     # rows that differ in the last bit
    got = dcgc.pair_inv_distance(graph, q.to(DEV), alpha).cpu()
    exact = np.float32(1.0 / alpha)
    loops = rows == cols
    assert int(loops.sum()) == n and bool((got[loops] == exact).all())
    same = ((rows == 10) & (cols == 11)) | ((rows == 11) & (cols == 10))
    pair = wats_hip.EdgeWeightGraph(torch.tensor([[10, 11, 20, 21], [11, 10, 21, 20]]), n, DEV)
    gp = dcgc.pair_inv_distance(pair, q.to(DEV), alpha).cpu()
    assert bool((got[same] == exact).all()) and float(gp[0]) == exact and float(gp[1]) == exact
    d = abs(float(q[21, 3].double() - q[20, 3].double()))
    assert d > 0 and float(gp[2]) == float(gp[3]) == float(np.float32(1.0 / (d + alpha)))
    ref = 1.0 / ((q.double()[rows] - q.double()[cols]).norm(dim=1) + alpha)
    assert float((got.double() - ref).abs().max()) <= 2.0 ** -24 * float(ref.max())
    hw = wats_hip.homophily_weights(graph, torch.randn(n, C).to(DEV), alpha, 10).cpu()
    assert bool((hw[loops] == exact).all())


def test_argument_errors_and_limits():
    lib = wats_hip._lib.load()
    cmax = dcgc.max_classes()
    assert cmax >= 41
    graph, rows, cols = device_graph("path")
    with pytest.raises(wats_hip.WaveletError, match="status -4"):
        wats_hip.edge_mlp_weights(graph, torch.zeros(graph.n, cmax + 1, device=DEV),
                                  [torch.zeros(s, device=DEV) for s in
                                   ((4 * (cmax + 1), 2 * (cmax + 1)), (4 * (cmax + 1),), (2 * (cmax + 1), 4 * (cmax + 1)),
                                    (2 * (cmax + 1),), (1, 2 * (cmax + 1)), (1,))])
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        wats_hip.edge_mlp_weights(graph, torch.zeros(graph.n, 2), [torch.zeros(s) for s in
                                                                   ((8, 4), (8,), (4, 8), (4,), (1, 4), (1,))], p=1.0)
    b = ctypes.c_int64()
    assert lib.wg_edge_mlp_workspace(-1, 0, 4, b) == -1
    assert lib.wg_edge_mlp_workspace(10, 10, cmax + 1, b) == -4
    p = 4096
    f = lambda **kw: lib.wg_edge_mlp_forward(*[kw.get(k, v) for k, v in dict(
        n=4, nnz=6, indptr=p, indices=p, C=3, emb=p, W1=p, b1=p, W2=p, b2=p, w3=p, b3=p, p=0.0, seed=0, ws=p, w=p,
        stream=None).items()])
    assert f(n=-1) == -1 and f(p=1.0) == -1 and f(p=-0.1) == -1 and f(emb=None) == -1 and f(C=0) == -1
    assert f(C=cmax + 1) == -4
    assert f(nnz=0, indptr=None, indices=None, emb=None, ws=None, w=None) == 0
    for n, nnz, C in ((50, 1, 1), (50, 3, 5), (200, 33, 41), (200, 513, 40), (1000, 5000, 41), (7, 100000, 48)):
        assert dcgc.edge_mlp_workspace(n, 2 * nnz, C) - dcgc.edge_mlp_workspace(n, nnz, C) <= 16 * nnz


def test_empty_graph_gives_empty_weights_and_zero_gradients():
    graph, rows, cols = device_graph("empty")
    emb, params, _, g_w = make_mlp(graph.n, rows, cols, 3, 0.0, 1)
    w, gp, ge = run_kernel(graph, emb, params, 0.0, 0, g_w)
    assert w.shape == (0,) and float(ge.abs().max()) == 0.0
    assert all(float(t.abs().max()) == 0.0 for t in gp)
    y = wats_hip.weighted_propagate(graph, w, torch.ones(graph.n, 3, device=DEV))
    assert float(y.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------
# the calibrator on the fixtures the reference recorded
# ---------------------------------------------------------------------------------------------------------
_cases = {}


def case(name):
    if name not in _cases:
        c = R.load_case(os.path.join(GOLDEN, name + ".npz"))
        base, ext = R.case_parts(c)
        alpha, beta = float(c["alpha"]), float(c["beta"])
        w, homo, out = R.forward(c["adj"], c["x"], base, ext, alpha, beta, torch.float64)
        grad = R.adjacency_gradient(c["adj"], c["x"], base, ext, c["loss_weight"], c["grad_rows"], c["grad_cols"],
                                    alpha, beta, torch.float64)
        c["ref64"] = dict(weights=w, homo=homo, out=out, grad=grad)
        c["mask"] = c["val_mask"].bool()
        _cases[name] = c
    return _cases[name]


def base_model(c, cls):
    nhid, nfeat = c["gc1_weight"].shape
    model = cls(nfeat=nfeat, nclass=c["gc2_weight"].shape[0], nhid=nhid)
    model.load_state_dict({"gc1.weight": c["gc1_weight"], "gc1.bias": c["gc1_bias"], "gc2.weight": c["gc2_weight"],
                           "gc2.bias": c["gc2_bias"]})
    return model.to(DEV)


def calibrator(c, adj, cls=None, **kw):
    cal = wats_hip.DCGC(base_model(c, cls or wats_hip.SparseCompatibleGCN), c["x"], c["y"], adj, c["mask"],
                        alpha=float(c["alpha"]), beta=float(c["beta"]), epochs=0, **kw)
    cal.model.extractor.load_state_dict({"0.weight": c["ext_w1"], "0.bias": c["ext_b1"], "3.weight": c["ext_w2"],
                                         "3.bias": c["ext_b2"], "6.weight": c["ext_w3"], "6.bias": c["ext_b3"]})
    return cal


@pytest.mark.parametrize("adj_kind", ["dense", "operator"])
@pytest.mark.parametrize("name", ["iso120", "wide96"])
def test_calibrator_matches_the_reference(name, adj_kind):
    c = case(name)
    ref = c["ref64"]
    adj = c["adj"].to(DEV)
    if adj_kind == "operator":
        adj = wats_hip.RowNormalizedAdjacency.from_dense(adj)
    cal = calibrator(c, adj)
    what = f"{name} {adj_kind}"
    with torch.no_grad():
        w = cal.model.get_weight(c["x"], adj)
        homo = cal.get_homo_weight(c["x"], adj, cal.alpha, cal.beta)
    assert w.shape == c["weights"].shape
    gats_ref.assert_close(w, c["weights"], ref["weights"], what + " weights")
    gats_ref.assert_close(homo, c["homo"], ref["homo"], what + " homophily weights")
    probe = wats_hip.EdgeProbe(c["grad_rows"], c["grad_cols"])
    out = cal(c["x"], adj, probe=probe)
    gats_ref.assert_close(out, c["out"], ref["out"], what + " logits")
    (out * c["loss_weight"].to(DEV)).sum().backward()
    gats_ref.assert_close(probe.grad, c["grad"], ref["grad"], what + " adjacency gradient")


@pytest.mark.parametrize("name", ["iso120", "wide96"])
def test_calibrator_on_a_dense_base_model(name):
    c = case(name)
    cal = calibrator(c, c["adj"], CompatibleGCN, graph=c["adj"])
    with torch.no_grad():
        out = cal(c["x"], c["adj"])
    gats_ref.assert_close(out, c["out"], c["ref64"]["out"], name + " dense base logits")


def test_flip_views_in_turn_each_get_their_own_pattern():
    """The attack's loop: one `with_flips` view per candidate, each dropped before the next is made (so that an
    object's address may be reused), every view with as many entries as the others.  Each call must sit on its own
    view's pattern: weights, logits and the probe's gradient are held to the restatement on that candidate's dense
    adjacency.  Extra keywords are ignored, as the reference ignores them."""
    c = case("iso120")
    base, ext = R.case_parts(c)
    alpha, beta = float(c["alpha"]), float(c["beta"])
    adj0 = c["adj"]
    op = wats_hip.RowNormalizedAdjacency.from_dense(adj0.to(DEV))
    cal = calibrator(c, op)
    absent = torch.nonzero((adj0 == 0) & (torch.arange(adj0.shape[0]).unsqueeze(1) < torch.arange(adj0.shape[0])))
    iso = int(c["isolated"][0])
    absent = absent[(absent != iso).all(1)][[3, 400, 2500, 4000]]       # four insertions: the same nnz every time
    seen = []
    for r, cc in absent.tolist():
        dense = adj0.clone()
        dense[r, cc] = dense[cc, r] = 1.0
        view = op.with_flips([r], [cc])
        graph = cal.model.graph_for(view)
        pr, pc = R.pattern(dense)
        assert graph.nnz == pr.numel() == int(adj0.count_nonzero()) + 2
        assert torch.equal(graph.rows.cpu().long(), pr) and torch.equal(graph.cols.cpu().long(), pc)
        assert cal.model.graph_for(view) is graph and all(graph is not g for g in seen)
        probe = wats_hip.EdgeProbe(c["grad_rows"], c["grad_cols"])
        out = cal(c["x"], view, probe=probe, epoch=3, verbose=False)
        (out * c["loss_weight"].to(DEV)).sum().backward()
        refs = []
        for dt in (torch.float32, torch.float64):
            w, _, o = R.forward(dense, c["x"], base, ext, alpha, beta, dt)
            g = R.adjacency_gradient(dense, c["x"], base, ext, c["loss_weight"], c["grad_rows"], c["grad_cols"], alpha,
                                     beta, dt)
            refs.append((w, o, g))
        what = f"view ({r}, {cc})"
        with torch.no_grad():
            gats_ref.assert_close(cal.model.get_weight(c["x"], view), refs[0][0], refs[1][0], what + " weights")
        gats_ref.assert_close(out, refs[0][1], refs[1][1], what + " logits")
        gats_ref.assert_close(probe.grad, refs[0][2], refs[1][2], what + " adjacency gradient")
        seen.append(graph)
        del view, graph, probe, out
    # the parent still has its own pattern, and nothing of the views stays with the calibrator
    assert cal.model.graph_for(op) is cal.model.graph and cal.model.graph.nnz == int(adj0.count_nonzero())
    assert len(cal.model._dense) <= cal.model.DENSE_SLOTS


def test_dense_adjacencies_are_told_apart_and_the_cache_is_bounded():
    """A dense tensor is recognised by identity and version: a changed tensor and a new tensor get their own
    pattern, and the calibrator keeps at most DENSE_SLOTS of them."""
    c = case("wide96")
    adj = c["adj"].to(DEV)
    cal = calibrator(c, adj)
    g0 = cal.model.graph_for(adj)
    assert g0 is cal.model.graph
    nnz0 = g0.nnz
    other = adj.clone()
    other[0, 5] = other[5, 0] = 1.0 - other[0, 5]
    g1 = cal.model.graph_for(other)
    assert g1 is not g0 and g1.nnz != nnz0 and cal.model.graph_for(other) is g1
    other[1, 7] = other[7, 1] = 1.0 - other[1, 7]          # in place: the version moves
    g2 = cal.model.graph_for(other)
    assert g2 is not g1 and g2.nnz != g1.nnz
    adj[0, 5] = adj[5, 0] = 1.0 - adj[0, 5]                # the construction tensor changed in place
    g3 = cal.model.graph_for(adj)
    assert g3 is not g0 and g3.nnz == g1.nnz
    for k in range(5):
        cal.model.graph_for(adj.clone())
    assert len(cal.model._dense) == cal.model.DENSE_SLOTS
    assert torch.isfinite(cal(c["x"], other)).all()


def test_training_changes_the_extractor_only_and_is_reproducible():
    c = case("iso120")
    states = []
    for epochs in (5, 5, 0):
        torch.manual_seed(0)
        base = base_model(c, wats_hip.SparseCompatibleGCN)
        before = {k: v.clone() for k, v in base.state_dict().items()}
        cal = wats_hip.DCGC(base, c["x"], c["y"], c["adj"], c["mask"], dropout=0.5, epochs=epochs)
        assert len(cal.model.history) == epochs and all(np.isfinite(cal.model.history))
        for k, v in base.state_dict().items():
            assert torch.equal(v, before[k]), k
        assert not any(p.requires_grad for p in cal.parameters())
        states.append({k: v.clone() for k, v in cal.model.extractor.state_dict().items()})
    assert set(states[0]) == {"0.weight", "0.bias", "3.weight", "3.bias", "6.weight", "6.bias"}
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k
    assert any(not torch.equal(states[0][k], states[2][k]) for k in states[0])
    assert torch.isfinite(cal(c["x"], c["adj"])).all()


def test_dense_adj_leaf_and_unsupported_base_models_raise():
    c = case("iso120")
    cal = calibrator(c, c["adj"])
    leaf = c["adj"].clone().to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError):
        cal(c["x"], leaf)

    class Other(nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = nn.Linear(16, 5)

        def forward(self, x, adj):
            return self.lin(x)

    with pytest.raises(NotImplementedError):
        wats_hip.DCGC(Other(), c["x"], c["y"], c["adj"], c["mask"], epochs=0)
