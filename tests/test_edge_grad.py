"""GPU tests of the edge gradients of the sparse base model: the SDDMM kernel
(wg_sddmm / wg_rowdot, csrc/sddmm.hip), EdgeProbe through one propagation and
through the two-layer model (alone and under WATS), the edge flip, and the
unchanged behaviour without a probe.

References are float64 numpy / dense torch autograd computed here (the quantity
the reference attack takes, calib_attack/calib_fga.py:864-881).  A whole vector
is compared by max|got - ref| / max|ref|: an edge gradient is a difference of
two dot products, so its small entries cancel and carry no relative accuracy of
their own.  Bounds: REL_TOL (1e-5) for one kernel call or one propagation,
1e-4 for the two-layer model (the bound test_sparse_gcn_matches_dense_compatible_gcn
uses for parameter gradients)."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import REL_TOL

pytestmark = pytest.mark.gpu

import wats_hip  # noqa: E402
from wats_hip import EdgeProbe, RowNormalizedAdjacency, propagate  # noqa: E402
from wats_hip.graphgen import random_graph, rmat_graph  # noqa: E402

MODEL_TOL = 1e-4
F_VALUES = [1, 3, 4, 5, 64, 65, 256, 260]
P_VALUES = [1, 63, 64, 65, 1000]
N_A, N_B = 50, 70


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def _np(t):
    return t.detach().cpu().numpy()


def _rel_err(got, ref):
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    scale = np.max(np.abs(ref))
    assert scale > 0, "the reference is all zero: the case checks nothing"
    return np.max(np.abs(got - ref)) / scale


def _assert_close(got, ref, tol, what):
    err = _rel_err(got, ref)
    print(f"{what}: max err / max|ref| = {err:.3e} (bound {tol:g})")
    assert err <= tol, f"{what}: max err / max|ref| = {err:.3e} > {tol:g}"


# ----------------------------------------------------------------- 1. the kernel
def _pairs(rng, P):
    rows = rng.integers(0, N_A, P).astype(np.int32)
    cols = rng.integers(0, N_B, P).astype(np.int32)
    rows[0] = cols[0] = 3                       # r == c
    if P >= 3:
        rows[2], cols[2] = rows[1], cols[1]     # a repeated pair
    return rows, cols


def _sddmm_ref(rows, cols, A, B, term=None, scale=None):
    out = np.einsum("pf,pf->p", A.astype(np.float64)[rows], B.astype(np.float64)[cols])
    if term is not None:
        out = out - term.astype(np.float64)[rows]
    if scale is not None:
        out = out * scale.astype(np.float64)[rows]
    return out


@pytest.mark.parametrize("F", F_VALUES)
def test_sddmm_and_rowdot_vs_numpy_float64(F):
    rng = np.random.default_rng(F)
    A = rng.standard_normal((N_A, F)).astype(np.float32)
    B = rng.standard_normal((N_B, F)).astype(np.float32)
    term = rng.standard_normal(N_A).astype(np.float32)
    scale = rng.uniform(0.05, 2.0, N_A).astype(np.float32)
    dA, dB, dterm, dscale = (torch.from_numpy(v).cuda() for v in (A, B, term, scale))
    for P in P_VALUES:
        rows, cols = _pairs(rng, P)
        drows, dcols = torch.from_numpy(rows).cuda(), torch.from_numpy(cols).cuda()
        for with_row in (False, True):
            kw = dict(row_term=dterm, row_scale=dscale) if with_row else {}
            got = wats_hip.sddmm(drows, dcols, dA, dB, **kw)
            again = wats_hip.sddmm(drows, dcols, dA, dB, **kw)
            ref = _sddmm_ref(rows, cols, A, B, *((term, scale) if with_row else ()))
            assert got.shape == (P,) and got.dtype == torch.float32
            _assert_close(_np(got), ref, REL_TOL, f"sddmm F={F} P={P} row={with_row}")
            assert torch.equal(got, again), "two runs differ"
        # only one of the two row arguments
        _assert_close(_np(wats_hip.sddmm(drows, dcols, dA, dB, row_term=dterm)),
                      _sddmm_ref(rows, cols, A, B, term=term), REL_TOL, f"sddmm F={F} P={P} term only")
        _assert_close(_np(wats_hip.sddmm(drows, dcols, dA, dB, row_scale=dscale)),
                      _sddmm_ref(rows, cols, A, B, scale=scale), REL_TOL, f"sddmm F={F} P={P} scale only")
    B2 = rng.standard_normal((N_A, F)).astype(np.float32)
    dB2 = torch.from_numpy(B2).cuda()
    for n in (1, 3, 4, 5, N_A):                 # the last sub-group of a wave, and of the launch
        got = wats_hip.rowdot(dA[:n], dB2[:n])
        ref = np.einsum("pf,pf->p", A[:n].astype(np.float64), B2[:n].astype(np.float64))
        _assert_close(_np(got), ref, REL_TOL, f"rowdot F={F} n={n}")
        assert torch.equal(got, wats_hip.rowdot(dA[:n], dB2[:n]))
    for r, c in ((N_A, 0), (0, N_B), (-1, 0)):  # the wrapper refuses ids the kernel would read out of bounds
        with pytest.raises(ValueError):
            wats_hip.sddmm(torch.tensor([r], dtype=torch.int32), torch.tensor([c], dtype=torch.int32), dA, dB)


@pytest.mark.parametrize("shift_a,shift_b", [(1, 0), (0, 1), (1, 1), (2, 3)])
def test_sddmm_misaligned_bases_take_the_dword_path(shift_a, shift_b):
    """F = 8 would take the 16-byte loads; a base pointer off a 16-byte boundary (a slice offset by
    whole floats) must not."""
    F = 8
    rng = np.random.default_rng(10 * shift_a + shift_b)
    A = rng.standard_normal((N_A, F)).astype(np.float32)
    B = rng.standard_normal((N_B, F)).astype(np.float32)
    bufA = torch.zeros(N_A * F + 4, device="cuda")
    bufB = torch.zeros(N_B * F + 4, device="cuda")
    dA = bufA[shift_a:shift_a + N_A * F].view(N_A, F)
    dB = bufB[shift_b:shift_b + N_B * F].view(N_B, F)
    dA.copy_(torch.from_numpy(A))
    dB.copy_(torch.from_numpy(B))
    assert dA.is_contiguous() and dA.data_ptr() % 16 == 4 * shift_a and dB.data_ptr() % 16 == (4 * shift_b) % 16
    rows, cols = _pairs(rng, 65)
    drows, dcols = torch.from_numpy(rows).cuda(), torch.from_numpy(cols).cuda()
    got = wats_hip.sddmm(drows, dcols, dA, dB)
    _assert_close(_np(got), _sddmm_ref(rows, cols, A, B), REL_TOL, f"sddmm misaligned {shift_a},{shift_b}")
    assert torch.equal(got, wats_hip.sddmm(drows, dcols, dA, dB))
    if shift_a == shift_b:
        got = wats_hip.rowdot(dA, dB[:N_A])
        ref = np.einsum("pf,pf->p", A.astype(np.float64), B[:N_A].astype(np.float64))
        _assert_close(_np(got), ref, REL_TOL, "rowdot misaligned")


def test_sddmm_row_offsets_beyond_2_31_elements():
    """A row that starts past 2^31 elements (n_a * F > 2^31, as 169 343 x 1 433 features are):
    32-bit row offsets would read another row."""
    F = 1024
    n_a = (1 << 21) + 8                          # n_a * F = 2^31 + 8192 elements (8 GiB)
    A = torch.empty((n_a, F), dtype=torch.float32, device="cuda")
    rows = torch.tensor([n_a - 1, 0, n_a - 3, 5, (1 << 21) + 1, (1 << 20)], dtype=torch.int32)
    gen = torch.Generator().manual_seed(0)
    rowvals = torch.randn(rows.numel(), F, generator=gen)
    B = torch.randn(N_B, F, generator=gen)
    A[rows.long().cuda()] = rowvals.cuda()
    cols = torch.tensor([0, 1, 2, 3, 69, 69], dtype=torch.int32)
    got = wats_hip.sddmm(rows.cuda(), cols.cuda(), A, B.cuda())
    ref = np.einsum("pf,pf->p", rowvals.numpy().astype(np.float64), B.numpy().astype(np.float64)[cols.numpy()])
    _assert_close(_np(got), ref, REL_TOL, "sddmm rows past 2^31 elements")


# ----------------------------------------------------------------- 2. one propagation
@pytest.fixture(scope="module")
def graph300():
    g = random_graph(300, 0.03, directed=True, weighted=True, self_loop_frac=0.1, isolated_frac=0.05)
    dense = torch.tensor(g.to_scipy().toarray(), dtype=torch.float32, device="cuda")
    assert (dense.sum(1) == 0).any() and (dense.sum(0) == 0).any() and dense.diagonal().any()
    n = g.n
    ids = torch.arange(n, dtype=torch.int32)
    return dense, RowNormalizedAdjacency.from_dense(dense), ids.repeat_interleave(n), ids.repeat(n)


def _dense_propagate64(adj64, x64):
    """model.py:43-47 in float64 with a differentiable adjacency."""
    deg = adj64.sum(dim=1, keepdim=True)
    deg = torch.where(deg == 0, torch.ones_like(deg), deg)
    return (adj64 / deg) @ x64


@pytest.mark.parametrize("F", [1, 7, 64, 130])
def test_probe_gradient_of_one_propagation_vs_dense_autograd(graph300, F):
    dense, op, rows, cols = graph300
    n = dense.shape[0]
    gen = torch.Generator("cuda").manual_seed(F)
    x = torch.randn(n, F, device="cuda", generator=gen, requires_grad=True)
    gy = torch.randn(n, F, device="cuda", generator=gen)      # every row, zero-degree rows included
    probe = EdgeProbe(rows, cols)
    assert len(probe) == n * n and probe.grad is None and probe.delta.dtype == torch.float32
    y = propagate(op, x, probe)
    (y * gy).sum().backward()

    adj64 = dense.double().requires_grad_(True)
    x64 = x.detach().double().requires_grad_(True)
    y64 = _dense_propagate64(adj64, x64)
    (y64 * gy.double()).sum().backward()
    _assert_close(_np(y), _np(y64), REL_TOL, f"propagate F={F}")
    _assert_close(_np(probe.grad), _np(adj64.grad).reshape(-1), REL_TOL, f"probe.grad F={F}")
    _assert_close(_np(x.grad), _np(x64.grad), REL_TOL, f"x.grad F={F}")
    # rows without entries: deg = 1 and y = 0, so the gradient there is g_i . x_j
    empty = (dense.sum(1) == 0).nonzero().flatten()
    got_empty = probe.grad.view(n, n)[empty]
    assert got_empty.abs().max() > 0
    _assert_close(_np(got_empty), _np(gy[empty].double() @ x.detach().double().t()), REL_TOL, f"empty rows F={F}")


def test_probe_subset_with_repeats_and_accumulation(graph300):
    """A probe names any positions, a position may repeat, and two backward passes add up."""
    dense, op, _, _ = graph300
    n = dense.shape[0]
    rng = np.random.default_rng(5)
    rows = rng.integers(0, n, 777).astype(np.int32)
    cols = rng.integers(0, n, 777).astype(np.int32)
    rows[10], cols[10] = rows[11], cols[11]
    x = torch.randn(n, 20, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    gy = torch.randn(n, 20, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    probe = EdgeProbe(rows, cols)
    for _ in range(2):
        (propagate(op, x, probe) * gy).sum().backward()
    adj64 = dense.double().requires_grad_(True)
    (_dense_propagate64(adj64, x.double()) * gy.double()).sum().backward()
    ref = 2 * _np(adj64.grad)[rows, cols]
    _assert_close(_np(probe.grad), ref, REL_TOL, "subset probe, two backward passes")
    with pytest.raises(ValueError):
        propagate(op, x, EdgeProbe([0, n], [0, 0]))


# ----------------------------------------------------------------- 3. the two-layer model
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
    return dict(n=n, adj=adj, x=x, model=model, ref64=ref64, t=t)


def _attack_losses(out_t):
    """The three scalars the attack differentiates per step (calib_fga.py:868-890)."""
    c = int(out_t.argmax(dim=1))
    loss = torch.log_softmax(out_t, dim=1)[0, c]
    p_max, p_smax = torch.topk(torch.softmax(out_t, dim=1), 2, dim=1)[0][0]
    return [("loss", loss), ("p_max", p_max), ("p_smax", p_smax)]


def _check_attack_step(m, forward, forward64, what):
    """forward(probe) / forward64(adj_leaf) -> (n, C) outputs of the model under test / the dense float64 one."""
    n, t, adj = m["n"], m["t"], m["adj"]
    probe = EdgeProbe.for_target(n, t)
    assert probe.rows.dtype == torch.int32 and len(probe) == 2 * n
    assert probe.rows[:n].eq(t).all() and probe.cols[:n].eq(torch.arange(n, device="cuda")).all()
    assert probe.cols[n:].eq(t).all() and probe.rows[n:].eq(torch.arange(n, device="cuda")).all()
    out = forward(probe)
    adj64 = adj.double().requires_grad_(True)
    out64 = forward64(adj64)
    _assert_close(_np(out), _np(out64), MODEL_TOL, f"{what}: outputs")
    scalars, scalars64 = _attack_losses(out[[t]]), _attack_losses(out64[[t]])
    grads = []
    for (name, s), (_, s64) in zip(scalars, scalars64):     # three gradients of one graph
        got = torch.autograd.grad(s, probe.delta, retain_graph=True)[0]
        ref = torch.autograd.grad(s64, adj64, retain_graph=True)[0]
        _assert_close(_np(got), _np(torch.cat([ref[t], ref[:, t]])), MODEL_TOL, f"{what}: d {name} / d adj[t,:], [:,t]")
        grads.append((got, ref))
    assert probe.grad is None
    scalars[0][1].backward()
    assert torch.equal(probe.grad, grads[0][0]), "backward() and autograd.grad() differ"
    op = m["model"].operator(adj)
    scores = wats_hip.target_flip_scores(probe, op, t)
    ref = grads[0][1]
    ref_scores = (ref[t] + ref[:, t]) * (1 - 2 * adj64.detach()[t])
    assert scores.shape == (n,)
    _assert_close(_np(scores), _np(ref_scores), MODEL_TOL, f"{what}: flip scores")
    assert int(scores.argmax()) == int(ref_scores.argmax())
    again = wats_hip.target_scores_from_grad(grads[0][0], op, t)
    assert torch.equal(scores, again)
    with pytest.raises(ValueError):
        wats_hip.target_flip_scores(probe, op, (t + 1) % n)


def test_two_layer_model_target_gradients_vs_dense_compatible_gcn(model400):
    m = model400
    _check_attack_step(m, lambda probe: m["model"](m["x"], m["adj"], probe=probe),
                       lambda adj64: m["ref64"](m["x"].double(), adj64), "gcn")


def test_wats_forwards_probe_to_the_sparse_base_model(model400):
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

    _check_attack_step(m, lambda probe: w(m["x"], m["adj"], probe=probe), forward64, "WATS")
    with torch.no_grad():
        assert torch.equal(w(m["x"], m["adj"]), w(m["x"], m["adj"], probe=None))
        # the operator in place of the dense adjacency (graphs whose dense form does not fit)
        assert torch.equal(w(m["x"], m["adj"]), w(m["x"], m["model"].operator(m["adj"])))


# ----------------------------------------------------------------- 4. the flip
@pytest.mark.parametrize("kind", ["weighted_directed", "binary_symmetric"])
@pytest.mark.parametrize("symmetric", [True, False])
def test_flipped_operator_equals_operator_of_flipped_dense(kind, symmetric):
    if kind == "binary_symmetric":
        g = rmat_graph(400, 3000, seed=2)
    else:
        g = random_graph(300, 0.03, seed=4, directed=True, weighted=True, self_loop_frac=0.1, isolated_frac=0.05)
    dense = torch.tensor(g.to_scipy().toarray(), dtype=torch.float32, device="cuda")
    n = g.n
    rng = np.random.default_rng(0)
    present = np.argwhere(np.triu(_np(dense) != 0, 1))
    absent = np.argwhere(np.triu(_np(dense + dense.t()) == 0, 1))
    sel = np.concatenate([present[rng.choice(len(present), 5, replace=False)],
                          absent[rng.choice(len(absent), 5, replace=False)]])
    counts = (_np(dense) != 0).sum(1)
    r0 = int(np.flatnonzero(counts == counts[counts > 0].min())[0])  # and every entry of a shortest row
    extra = [(r0, int(c)) for c in np.flatnonzero(_np(dense[r0])) if c != r0]
    pairs = {(min(a, b), max(a, b)): (int(a), int(b)) for a, b in list(map(tuple, sel)) + extra}
    rows, cols = zip(*pairs.values())
    flipped = dense.clone()
    for r, c in zip(rows, cols):                                    # calib_fga.py:901-904
        v = -2 * flipped[r, c] + 1
        flipped[r, c] += v
        if symmetric:
            flipped[c, r] += v
    op = RowNormalizedAdjacency.from_dense(dense)
    a = op.flipped(list(rows), list(cols), symmetric=symmetric)
    b = RowNormalizedAdjacency.from_dense(flipped)
    assert a.nnz == b.nnz
    assert torch.equal(a.indptr, b.indptr) and torch.equal(a.indices, b.indices) and torch.equal(a.values, b.values)
    assert torch.equal(a.deg, b.deg)
    x = torch.randn(n, 33, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    assert torch.equal(propagate(a, x), propagate(b, x))
    assert not torch.equal(propagate(a, x), propagate(op, x))
    with pytest.raises(ValueError):
        op.flipped([1], [1])
    with pytest.raises(ValueError):
        op.flipped([1, 2], [2, 1])


def test_operator_keeps_its_csr_and_degree(graph300):
    dense, op, _, _ = graph300
    A = sp.csr_matrix(_np(dense))
    A.sort_indices()
    assert np.array_equal(_np(op.indptr), A.indptr) and op.indptr.dtype == torch.int64
    assert np.array_equal(_np(op.indices), A.indices) and op.indices.dtype == torch.int32
    assert np.array_equal(_np(op.values), A.data)
    deg = _np(dense).astype(np.float64).sum(1).astype(np.float32)
    deg[deg == 0] = 1
    assert op.deg.dtype == torch.float32 and np.array_equal(_np(op.deg), deg)
    g = rmat_graph(500, 4000, seed=1)              # no values: deg is the row length
    op1 = RowNormalizedAdjacency(g.n, torch.from_numpy(g.indptr), torch.from_numpy(g.indices), None)
    d1 = np.diff(g.indptr).astype(np.float32)
    d1[d1 == 0] = 1
    assert op1.values is None and np.array_equal(_np(op1.deg), d1)


# ----------------------------------------------------------------- 5. no probe: as before
def test_without_probe_nothing_changes(graph300, model400):
    dense, op, _, _ = graph300
    n = dense.shape[0]
    x = torch.randn(n, 17, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    gy = torch.randn(n, 17, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    y0, gx0 = op.fwd.apply(x), op.bwd.apply(gy)         # the SpMM pair propagate has always run
    probe = EdgeProbe([0, 1], [1, 0])
    for kw in ({}, {"probe": None}, {"probe": probe}):
        xi = x.clone().requires_grad_(True)
        y = propagate(op, xi, **kw)
        (y * gy).sum().backward()
        assert torch.equal(y, y0) and torch.equal(xi.grad, gx0), kw
    assert probe.grad is not None and probe.grad.shape == (2,)

    m = model400
    outs, grads = [], []
    for kw in ({}, {"probe": None}, {"probe": EdgeProbe.for_target(m["n"], m["t"])}):
        xi = m["x"].clone().requires_grad_(True)
        out = m["model"](xi, m["adj"], **kw)
        out.square().sum().backward()
        outs.append(out.detach())
        grads.append(xi.grad)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    for kw in ({}, {"probe": EdgeProbe.for_target(m["n"], m["t"])}):
        with pytest.raises(NotImplementedError):
            m["model"](m["x"], m["adj"].clone().requires_grad_(True), **kw)
