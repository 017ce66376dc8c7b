"""GPU tests of the edge-flip views (wats_hip/flips.py, csrc/flips.hip): the overlay's resolve kernel,
the forward and backward fix-ups, edge gradients and one attack step through a view, composition, and
the commit to a canonical CSR.

References are float64 numpy / dense torch of the flipped dense matrix, built by the reference's update
loop (calib_attack/calib_fga.py:901-904) as in test_edge_grad.py; the CSR commit is compared bit for
bit with the chained toggle_edges result.  Bounds: REL_TOL (1e-5, max|got - ref| / max|ref|) for one
kernel call or one propagation, 1e-4 for the two-layer model -- the bounds test_edge_grad.py uses."""
import copy
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import REL_TOL

pytestmark = pytest.mark.gpu

import wats_hip  # noqa: E402
from wats_hip import EdgeProbe, FlippedAdjacency, RowNormalizedAdjacency, propagate, toggle_edges  # noqa: E402
from wats_hip._lib import ptr  # noqa: E402
from wats_hip.graphgen import random_graph, rmat_graph  # noqa: E402

MODEL_TOL = 1e-4
F_VALUES = [1, 3, 4, 5, 64, 65, 130]
HUB_N = 3000


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def _np(t):
    return t.detach().cpu().numpy()


def _assert_close(got, ref, tol, what):
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    scale = np.max(np.abs(ref))
    assert scale > 0, f"{what}: the reference is all zero: the case checks nothing"
    err = np.max(np.abs(got - ref)) / scale
    print(f"{what}: max err / max|ref| = {err:.3e} (bound {tol:g})")
    assert err <= tol, f"{what}: max err / max|ref| = {err:.3e} > {tol:g}"


def _dense_flip(dense, rows, cols, symmetric):
    """calib_fga.py:901-904 on the dense float32 matrix, one pair after the other."""
    a = dense.copy()
    for r, c in zip(rows, cols):
        v = np.float32(-2) * a[r, c] + np.float32(1)
        a[r, c] += v
        if symmetric:
            a[c, r] += v
    return a


def _norm64(dense):
    """adj / deg of model.py:43-45 in float64, and deg."""
    deg = dense.astype(np.float64).sum(1)
    deg[deg == 0] = 1
    return dense.astype(np.float64) / deg[:, None], deg


class Graph:
    def __init__(self, A, valued):
        A = sp.csr_matrix(A)
        A.sort_indices()
        self.A, self.n, self.valued = A, A.shape[0], valued
        self.dense = A.toarray().astype(np.float32)
        self.op = RowNormalizedAdjacency(self.n, torch.from_numpy(A.indptr.astype(np.int64)),
                                         torch.from_numpy(A.indices.astype(np.int32)),
                                         torch.from_numpy(A.data.astype(np.float32)) if valued else None)
        self.counts = np.diff(A.indptr)


@pytest.fixture(scope="module")
def graphs():
    g = rmat_graph(400, 3000)
    assert g.values is None
    binary = Graph(g.to_scipy(), valued=False)
    g = random_graph(300, 0.03, directed=True, weighted=True, self_loop_frac=0.1, isolated_frac=0.05)
    weighted = Graph(g.to_scipy(), valued=True)
    assert (weighted.counts == 0).any() and weighted.dense.diagonal().any()
    # a star (node 0 - every node) plus a ring over the other nodes: row 0 has HUB_N - 1 entries,
    # more than one pass of a workgroup's sub-groups
    ring = np.arange(1, HUB_N)
    src = np.concatenate([np.zeros(HUB_N - 1, np.int64), ring, ring, np.roll(ring, -1)])
    dst = np.concatenate([ring, np.zeros(HUB_N - 1, np.int64), np.roll(ring, -1), ring])
    hub = Graph(sp.csr_matrix((np.ones(src.size, np.float32), (src, dst)), shape=(HUB_N, HUB_N)), valued=False)
    assert hub.counts[0] == HUB_N - 1 and hub.A.nnz == 4 * (HUB_N - 1)
    return dict(binary=binary, weighted=weighted, hub=hub)


def _present_absent(G, rng, n_present, n_absent):
    present = np.argwhere(np.triu(G.dense != 0, 1))
    absent = np.argwhere(np.triu((G.dense + G.dense.T) == 0, 1))
    sel = np.concatenate([present[rng.choice(len(present), n_present, replace=False)],
                          absent[rng.choice(len(absent), n_absent, replace=False)]])
    return [int(v) for v in sel[:, 0]], [int(v) for v in sel[:, 1]]


def _case(graphs, name):
    """(graph, rows, cols, symmetric, touched rows, extra checks) of a named flip call."""
    rng = np.random.default_rng(11)
    if name == "one_present":                   # P = 1, one touched row, an entry removed
        G = graphs["binary"]
        r, c = _present_absent(G, rng, 1, 0)
        return G, r, c, False
    if name == "one_absent_symmetric":          # P = 1, two touched rows, entries added
        G = graphs["binary"]
        r, c = _present_absent(G, rng, 0, 1)
        return G, r, c, True
    if name == "row_loses_every_entry":
        G = graphs["binary"]
        r0 = int(np.flatnonzero(G.counts == G.counts[G.counts > 0].min())[0])
        cs = [int(c) for c in np.flatnonzero(G.dense[r0])]
        return G, [r0] * len(cs), cs, False
    if name == "hub_64_symmetric":              # P = 64, 65 touched rows, the hub among them
        G = graphs["hub"]
        cs = [int(c) for c in rng.choice(np.arange(1, HUB_N), 64, replace=False)]
        return G, [0] * 64, cs, True
    if name == "hub_65_one_row":                # P = 65, one touched row: the hub loses 65 of its entries
        G = graphs["hub"]
        cs = [int(c) for c in rng.choice(np.arange(1, HUB_N), 65, replace=False)]
        return G, [0] * 65, cs, False
    if name == "weighted_mixed":                # weights change without leaving; an empty row gains an entry
        G = graphs["weighted"]
        r, c = _present_absent(G, rng, 5, 5)
        empty = [int(i) for i in np.flatnonzero((G.counts == 0) & (G.dense.sum(0) == 0))[:2]]
        taken = set(r) | set(c)
        partner = [int(i) for i in np.flatnonzero(G.counts > 0) if int(i) not in taken][:2]
        return G, r + empty, c + partner, True
    raise AssertionError(name)


CASES = ["one_present", "one_absent_symmetric", "row_loses_every_entry", "hub_64_symmetric", "hub_65_one_row",
         "weighted_mixed"]
TOUCHED = {"one_present": 1, "one_absent_symmetric": 2, "row_loses_every_entry": 1, "hub_64_symmetric": 65,
           "hub_65_one_row": 1, "weighted_mixed": None}


def _randn(n, F, seed):
    return torch.randn(n, F, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))


# ----------------------------------------------------------------- 1. resolve
@pytest.mark.parametrize("kind,valued", [("binary", False), ("weighted", True), ("weighted", False), ("hub", False)])
def test_resolve_vs_scipy(graphs, kind, valued):
    G = graphs[kind]
    A, n = G.A, G.n
    rng = np.random.default_rng(3)
    rows_with = np.flatnonzero(G.counts > 0)
    pos = set()
    for r in {0, n - 1, int(rows_with[0]), int(rows_with[-1]), int(np.argmax(G.counts))} | set(
            int(v) for v in rng.choice(rows_with, 8, replace=False)):
        cols = A.indices[A.indptr[r]:A.indptr[r + 1]]
        pos |= {(r, 0), (r, n - 1), (r, int(rng.integers(0, n)))}
        if len(cols):
            pos |= {(r, int(cols[0])), (r, int(cols[-1])), (r, int(cols[len(cols) // 2]))}     # present
            pos |= {(r, int(c)) for c in (cols[0] - 1, cols[-1] + 1) if 0 <= c < n}            # mostly absent
    empty = np.flatnonzero(G.counts == 0)
    if len(empty):
        pos |= {(int(empty[0]), 0), (int(empty[0]), n - 1), (int(empty[-1]), 5)}
    pos = sorted(pos)
    rows, cols = np.array([p[0] for p in pos]), np.array([p[1] for p in pos])
    t_rows, counts = np.unique(rows, return_counts=True)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    P, T = len(pos), len(t_rows)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    d_t, d_seg, d_cols = dev(t_rows, np.int32), dev(seg, np.int64), dev(cols, np.int32)
    op = G.op
    values = op.values if valued else None
    if valued:
        assert values is not None
    outs = []
    for _ in range(2):
        a_old = torch.full((P,), -7.0, device="cuda")
        base_pos = torch.full((P,), -7, dtype=torch.int64, device="cuda")
        row_sum = torch.full((T,), -7.0, dtype=torch.float64, device="cuda")
        rc = wats_hip._lib.load().wg_flip_resolve(n, ptr(op.indptr), ptr(op.indices), ptr(values), T, ptr(d_t),
                                                  ptr(d_seg), P, ptr(d_cols), ptr(a_old), ptr(base_pos), ptr(row_sum),
                                                  torch.cuda.current_stream().cuda_stream)
        wats_hip._lib.check(rc, "flip_resolve")
        outs.append((a_old, base_pos, row_sum))
    a_old, base_pos, row_sum = outs[0]
    assert all(torch.equal(u, v) for u, v in zip(outs[0], outs[1])), "two runs differ"
    data = A.data.astype(np.float32) if valued else np.ones(A.nnz, np.float32)
    ref_old, ref_pos = np.zeros(P, np.float32), np.full(P, -1, np.int64)
    for i, (r, c) in enumerate(pos):
        s, e = A.indptr[r], A.indptr[r + 1]
        k = s + np.searchsorted(A.indices[s:e], c)
        if k < e and A.indices[k] == c:
            ref_old[i], ref_pos[i] = data[k], k
    assert (ref_pos >= 0).sum() >= 10 and (ref_pos < 0).sum() >= 10
    assert np.array_equal(_np(a_old).view(np.uint32), ref_old.view(np.uint32))
    assert np.array_equal(_np(base_pos), ref_pos)
    ref_sum = np.array([data[A.indptr[r]:A.indptr[r + 1]].astype(np.float64).sum() for r in t_rows])
    if valued:   # a float64 sum of at most 30 float32 values in another order: a few ulp of float64
        assert np.allclose(_np(row_sum), ref_sum, rtol=1e-13, atol=0)
    else:
        assert np.array_equal(_np(row_sum), ref_sum)


# ----------------------------------------------------------------- 2. forward
@pytest.mark.parametrize("name", CASES)
def test_forward_of_a_view_vs_float64(graphs, name):
    G, rows, cols, symmetric = _case(graphs, name)
    n, op = G.n, G.op
    flipped = _dense_flip(G.dense, rows, cols, symmetric)
    norm, deg = _norm64(flipped)
    view = op.with_flips(rows, cols, symmetric=symmetric)
    assert isinstance(view, FlippedAdjacency) and isinstance(view, RowNormalizedAdjacency) and view.base is op
    changed = np.flatnonzero((flipped != G.dense).any(1))
    touched = torch.zeros(n, dtype=torch.bool, device="cuda")
    touched[torch.from_numpy(changed).cuda()] = True
    assert view.n_touched == len(changed) and view.n_positions == int((flipped != G.dense).sum())
    if TOUCHED[name] is not None:
        assert len(changed) == TOUCHED[name]
    assert view.nnz == int((flipped != 0).sum())
    real = view.materialize()
    if G.valued:
        _assert_close(_np(view.deg), deg, REL_TOL, f"{name}: deg")
    else:
        assert torch.equal(view.deg, real.deg)
        assert np.array_equal(_np(view.deg), deg.astype(np.float32))
    assert torch.equal(view.inv_deg, 1.0 / view.deg)
    for F in F_VALUES + ["offset"]:
        if F == "offset":   # F = 64 would take the 16-byte loads; a base off a 16-byte boundary must not
            buf = torch.zeros(n * 64 + 4, device="cuda")
            x = buf[1:1 + n * 64].view(n, 64)
            x.copy_(_randn(n, 64, 99))
            assert x.is_contiguous() and x.data_ptr() % 16 == 4
        else:
            x = _randn(n, F, F)
        y = view.fwd.apply(x)
        ref = norm @ _np(x).astype(np.float64)
        _assert_close(_np(y), ref, REL_TOL, f"{name}: forward F={F}")
        if np.abs(ref[changed]).max() > 0:      # the recomputed rows on their own scale
            _assert_close(_np(y)[changed], ref[changed], REL_TOL, f"{name}: forward F={F}, touched rows")
        assert torch.equal(y, view.fwd.apply(x)), "two runs differ"
        y0 = op.fwd.apply(x)
        assert torch.equal(y[~touched], y0[~touched]), "an untouched row changed"
        assert not torch.equal(y[touched], y0[touched])
        lost = np.flatnonzero((flipped != 0).sum(1) == 0)
        assert torch.equal(y[torch.from_numpy(lost).cuda()], torch.zeros(len(lost), x.shape[1], device="cuda"))
        if name == "row_loses_every_entry":
            assert rows[0] in lost
    if name == "weighted_mixed":
        assert ((G.dense == 0).all(1) & (flipped != 0).any(1)).any(), "no empty row gained an entry"
        both = (G.dense != 0) & (flipped != 0) & (G.dense != flipped)
        assert both.any(), "no weighted entry was modified without leaving"


# ----------------------------------------------------------------- 3. backward, edge gradients, one attack step
@pytest.mark.parametrize("name", CASES)
def test_backward_of_a_view_vs_float64(graphs, name):
    G, rows, cols, symmetric = _case(graphs, name)
    norm, _ = _norm64(_dense_flip(G.dense, rows, cols, symmetric))
    view = G.op.with_flips(rows, cols, symmetric=symmetric)
    for F in F_VALUES:
        g = _randn(G.n, F, 100 + F)
        gx = view.bwd.apply(g)
        _assert_close(_np(gx), norm.T @ _np(g).astype(np.float64), REL_TOL, f"{name}: backward F={F}")
        assert torch.equal(gx, view.bwd.apply(g)), "two runs differ"


def _dense_propagate64(adj64, x64):
    deg = adj64.sum(dim=1, keepdim=True)
    deg = torch.where(deg == 0, torch.ones_like(deg), deg)
    return (adj64 / deg) @ x64


@pytest.mark.parametrize("name", ["row_loses_every_entry", "one_absent_symmetric", "weighted_mixed"])
@pytest.mark.parametrize("F", [1, 20])
def test_probe_gradient_through_a_view_vs_dense_autograd(graphs, name, F):
    G, rows, cols, symmetric = _case(graphs, name)
    n = G.n
    flipped = torch.from_numpy(_dense_flip(G.dense, rows, cols, symmetric)).cuda()
    view = G.op.with_flips(rows, cols, symmetric=symmetric)
    ids = torch.arange(n, dtype=torch.int32)
    probe = EdgeProbe(ids.repeat_interleave(n), ids.repeat(n))
    x = _randn(n, F, 7).requires_grad_(True)
    gy = _randn(n, F, 8)
    y = propagate(view, x, probe)
    (y * gy).sum().backward()
    adj64 = flipped.double().requires_grad_(True)
    x64 = x.detach().double().requires_grad_(True)
    y64 = _dense_propagate64(adj64, x64)
    (y64 * gy.double()).sum().backward()
    _assert_close(_np(y), _np(y64), REL_TOL, f"{name}: propagate F={F}")
    _assert_close(_np(x.grad), _np(x64.grad), REL_TOL, f"{name}: x.grad F={F}")
    _assert_close(_np(probe.grad), _np(adj64.grad).reshape(-1), REL_TOL, f"{name}: probe.grad F={F}")


@pytest.fixture(scope="module")
def model400():
    from models import CompatibleGCN
    n = 400
    g = rmat_graph(n, 3000, seed=7)
    A = (g.to_scipy() + sp.eye(n)).toarray().astype(np.float32)
    adj = torch.tensor(A, device="cuda")
    torch.manual_seed(0)
    x = torch.randn(n, 33, device="cuda")
    ref32 = CompatibleGCN(33, 7, nhid=64).cuda().eval()
    model = wats_hip.SparseCompatibleGCN(33, nclass=7, nhid=64).cuda().eval()
    model.load_state_dict(ref32.state_dict())
    ref64 = copy.deepcopy(ref32).double().eval()
    t = int(np.argsort(A.sum(1))[n // 2])       # a node of median degree
    present = int(np.flatnonzero((A[t] != 0) & (np.arange(n) != t))[0])
    absent = int(np.flatnonzero(A[t] == 0)[0])
    rows, cols = [t, t], [present, absent]      # the target loses an edge and gains one
    flipped = torch.from_numpy(_dense_flip(A, rows, cols, True)).cuda()
    view = model.operator(adj).with_flips(rows, cols, symmetric=True)
    return dict(n=n, adj=adj, x=x, model=model, ref64=ref64, t=t, view=view, flipped=flipped)


def _attack_losses(out_t):
    """The three scalars the attack differentiates per step (calib_fga.py:868-890)."""
    c = int(out_t.argmax(dim=1))
    loss = torch.log_softmax(out_t, dim=1)[0, c]
    p_max, p_smax = torch.topk(torch.softmax(out_t, dim=1), 2, dim=1)[0][0]
    return [("loss", loss), ("p_max", p_max), ("p_smax", p_smax)]


def _check_attack_step(m, forward, forward64, what):
    n, t, view = m["n"], m["t"], m["view"]
    probe = EdgeProbe.for_target(n, t)
    out = forward(probe)
    adj64 = m["flipped"].double().requires_grad_(True)
    out64 = forward64(adj64)
    _assert_close(_np(out), _np(out64), MODEL_TOL, f"{what}: outputs")
    first = None
    for (name, s), (_, s64) in zip(_attack_losses(out[[t]]), _attack_losses(out64[[t]])):
        got = torch.autograd.grad(s, probe.delta, retain_graph=True)[0]
        ref = torch.autograd.grad(s64, adj64, retain_graph=True)[0]
        _assert_close(_np(got), _np(torch.cat([ref[t], ref[:, t]])), MODEL_TOL, f"{what}: d {name} / d adj[t,:], [:,t]")
        first = first or (got, ref, s)
    got, ref, s = first
    s.backward()
    assert torch.equal(probe.grad, got)
    scores = wats_hip.target_flip_scores(probe, view, t)
    ref_scores = (ref[t] + ref[:, t]) * (1 - 2 * adj64.detach()[t])
    _assert_close(_np(scores), _np(ref_scores), MODEL_TOL, f"{what}: flip scores")
    assert int(scores.argmax()) == int(ref_scores.argmax())
    assert torch.equal(view.dense_row(t), m["flipped"][t])


def test_attack_step_through_a_view_vs_dense_compatible_gcn(model400):
    m = model400
    _check_attack_step(m, lambda probe: m["model"](m["x"], m["view"], probe=probe),
                       lambda adj64: m["ref64"](m["x"].double(), adj64), "gcn on a view")


def test_attack_step_through_a_view_under_wats(model400):
    m = model400
    n = m["n"]
    gen = torch.Generator().manual_seed(3)
    feats = torch.rand(n, 1, generator=gen)
    labels = torch.randint(0, 7, (n,), generator=gen)
    val = torch.zeros(n, dtype=torch.bool)
    val[::3] = True
    w = wats_hip.WATS(m["model"], m["x"], labels, m["adj"], val, wavelet_feats=feats, verbose=False).eval()
    T = w.temperatures().detach().double()

    def forward64(adj64):
        return torch.log_softmax(m["ref64"](m["x"].double(), adj64) / T.unsqueeze(1), dim=1)

    _check_attack_step(m, lambda probe: w(m["x"], m["view"], probe=probe), forward64, "WATS on a view")


# ----------------------------------------------------------------- 4. composition
def _csr_equal(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("kind", ["binary", "weighted"])
@pytest.mark.parametrize("symmetric", [True, False])
def test_composed_views_equal_chained_flipped_operators(graphs, kind, symmetric):
    G = graphs[kind]
    rng = np.random.default_rng(5)
    ra, ca = _present_absent(G, rng, 4, 4)
    rb, cb = _present_absent(G, rng, 3, 3)
    rb, cb = rb + [ca[0], ra[1], ra[4]], cb + [ra[0], ca[1], ca[5]]    # a pair flipped back; rows touched again
    keep = {(min(r, c), max(r, c)): (r, c) for r, c in zip(rb, cb) if r != c}
    rb, cb = [p[0] for p in keep.values()], [p[1] for p in keep.values()]
    view = G.op.with_flips(ra, ca, symmetric=symmetric).with_flips(rb, cb, symmetric=symmetric)
    real = G.op.flipped(ra, ca, symmetric=symmetric).flipped(rb, cb, symmetric=symmetric)
    assert view.base is G.op and view.nnz == real.nnz
    assert _csr_equal(view.csr(), (real.indptr, real.indices, real.values))
    assert torch.equal(view.indptr, real.indptr) and torch.equal(view.indices, real.indices)
    if G.valued:
        _assert_close(_np(view.deg), _np(real.deg), REL_TOL, "composed deg")
    else:
        assert torch.equal(view.deg, real.deg)
    x = _randn(G.n, 33, 0)
    _assert_close(_np(view.fwd.apply(x)), _np(real.fwd.apply(x).double()), REL_TOL, "composed forward")
    _assert_close(_np(view.bwd.apply(x)), _np(real.bwd.apply(x).double()), REL_TOL, "composed backward")
    assert torch.equal(propagate(view.materialize(), x), propagate(real, x))
    assert torch.equal(propagate(G.op.with_flips(ra, ca, symmetric).flipped(rb, cb, symmetric), x), propagate(real, x))


@pytest.mark.parametrize("kind", ["binary", "weighted"])
def test_a_pair_flipped_twice_leaves_an_empty_overlay(graphs, kind):
    G = graphs[kind]
    r, c = _present_absent(G, np.random.default_rng(6), 3, 3)
    for symmetric in (True, False):
        view = G.op.with_flips(r, c, symmetric).with_flips(r, c, symmetric)
        if not G.valued:   # 1 - 2 a is its own inverse on {0, 1}; a weight w goes w -> 1 - w -> w only up to rounding
            assert view.n_positions == 0 and view.nnz == G.op.nnz and view.ov_rows.numel() == 0
            x = _randn(G.n, 17, 1)
            assert torch.equal(view.fwd.apply(x), G.op.fwd.apply(x))
            assert torch.equal(view.bwd.apply(x), G.op.bwd.apply(x))
            assert torch.equal(view.deg, G.op.deg)
            assert _csr_equal(view.csr()[:2], (G.op.indptr, G.op.indices))
        again = view.with_flips([], [])
        assert isinstance(again, FlippedAdjacency) and again.n_positions == view.n_positions


def test_with_flips_rejects_what_toggle_edges_rejects(graphs):
    op, n = graphs["binary"].op, graphs["binary"].n
    view = op.with_flips([1], [2])
    for target in (op, view):
        for rows, cols in (([3], [3]), ([1, 5, 1], [2, 6, 2]), ([1, 2], [2, 1]), ([0], [n]), ([-1], [0])):
            with pytest.raises(ValueError):
                target.with_flips(rows, cols)
        with pytest.raises(ValueError):
            target.with_flips([1, 2], [3])


# ----------------------------------------------------------------- 5. commit
def _random_pairs(n, P, rng):
    """P distinct unordered off-diagonal pairs, each in a random orientation."""
    keys = rng.choice(n * n, 4 * P + 16, replace=False)
    r, c = keys // n, keys % n
    _, first = np.unique(np.minimum(r, c) * n + np.maximum(r, c), return_index=True)
    sel = np.sort(first[(r != c)[first]])[:P]
    assert len(sel) == P
    return [int(v) for v in r[sel]], [int(v) for v in c[sel]]


@pytest.mark.parametrize("kind", ["binary", "weighted"])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("P", [1, 10, 2000])
def test_csr_of_a_view_equals_chained_toggle_edges(graphs, kind, symmetric, P):
    G = graphs[kind]
    op = G.op
    rows, cols = _random_pairs(G.n, P, np.random.default_rng(P))
    half = P // 2
    calls = [(rows[:half], cols[:half]), (rows[half:], cols[half:])] if half else [(rows, cols)]
    view, ref = op, (op.indptr, op.indices, op.values)
    for r, c in calls:
        view = view.with_flips(r, c, symmetric=symmetric)
        ref = toggle_edges(G.n, *ref, r, c, symmetric=symmetric)
    got = view.csr()
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
    assert _csr_equal(got, ref)
    assert view.nnz == ref[1].numel() and view.csr() is got
    again = op.with_flips(*calls[0], symmetric=symmetric)
    for r, c in calls[1:]:
        again = again.with_flips(r, c, symmetric=symmetric)
    assert _csr_equal(again.csr(), got), "two runs differ"
    g = view.to_graph()
    assert g.n == G.n and g.nnz == view.nnz
    if not G.valued and symmetric:      # the R-MAT graph is symmetric: every flipped entry is 0 or 1
        assert g.values is None
    if G.valued:
        assert torch.equal(g.values, ref[2])


def test_csr_patch_edge_positions(graphs):
    """Inserts before the first and after the last column of a row, a deletion that empties a row, and both
    beside untouched rows."""
    G = graphs["binary"]
    n = G.n
    r = next(int(i) for i in range(1, n - 1) if G.counts[i] >= 2 and G.dense[i, 0] == 0 and G.dense[i, n - 1] == 0)
    r0 = int(np.flatnonzero((G.counts == G.counts[G.counts > 0].min()) & (np.arange(n) != r))[0])
    cs = [int(c) for c in np.flatnonzero(G.dense[r0]) if c != r]
    rows, cols = [r, r] + [r0] * len(cs), [0, n - 1] + cs
    view = G.op.with_flips(rows, cols, symmetric=False)
    indptr, indices, values = view.csr()
    assert _csr_equal((indptr, indices, values), toggle_edges(n, G.op.indptr, G.op.indices, None, rows, cols, False))
    s, e = int(indptr[r]), int(indptr[r + 1])
    assert int(indices[s]) == 0 and int(indices[e - 1]) == n - 1 and e - s == G.counts[r] + 2
    if len(cs) == G.counts[r0]:
        assert int(indptr[r0]) == int(indptr[r0 + 1])


def test_csr_patch_on_a_graph_without_entries():
    n = 50
    op = RowNormalizedAdjacency(n, torch.zeros(n + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None)
    rows, cols = [4, 49, 0], [1, 0, 30]
    for symmetric in (True, False):
        view = op.with_flips(rows, cols, symmetric=symmetric)
        ref = toggle_edges(n, op.indptr, op.indices, None, rows, cols, symmetric)
        assert _csr_equal(view.csr(), ref) and view.nnz == (6 if symmetric else 3)
        assert view.to_graph().values is None
        assert torch.equal(view.deg, view.materialize().deg)


def test_committed_view_feeds_the_wavelet_features_and_a_real_operator(graphs):
    G = graphs["binary"]
    rows, cols = _present_absent(G, np.random.default_rng(9), 6, 6)
    view = G.op.with_flips(rows, cols, symmetric=True)
    g = view.to_graph()
    assert g.values is None
    ref = toggle_edges(G.n, G.op.indptr, G.op.indices, None, rows, cols, True)
    assert bool((ref[2] == 1).all())
    g_ref = wats_hip.DeviceCSR(G.n, ref[0], ref[1], None)
    H = wats_hip.graph_wavelet_features(g, k=8, s=0.8)
    H_ref = wats_hip.graph_wavelet_features(g_ref, k=8, s=0.8)
    assert torch.equal(H, H_ref) and float(H.abs().max()) > 0
    x = _randn(G.n, 33, 2)
    real = G.op.flipped(rows, cols, symmetric=True)
    assert torch.equal(propagate(view.materialize(), x), propagate(real, x))
    assert torch.equal(propagate(view.flipped([], []), x), propagate(real, x))


# ----------------------------------------------------------------- 6. reproducibility: every test above runs its
# kernel twice and compares with torch.equal ("two runs differ"); an empty overlay launches nothing
def test_entries_with_nothing_to_do_launch_nothing():
    lib = wats_hip._lib.load()
    buf = torch.zeros(8, dtype=torch.int64, device="cuda")
    nnz = ctypes.c_int64(-1)
    assert lib.wg_flip_resolve(4, ptr(buf), None, None, 0, None, None, 0, None, None, None, None, None) == 0
    assert lib.wg_flip_rows(4, ptr(buf), None, None, 0, None, None, 0, None, None, None, None, 3, None, None, None) == 0
    assert lib.wg_flip_cols(4, 0, None, None, 0, None, None, None, None, 3, None, None, None) == 0
    out = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    assert lib.wg_csr_patch(4, 0, ptr(buf), None, None, 0, None, None, 0, None, None, None, ptr(out), None, None, 0,
                            ctypes.byref(nnz), torch.cuda.current_stream().cuda_stream) == 0
    assert nnz.value == 0 and out.tolist() == [0, 0, 0, 0, 0]
