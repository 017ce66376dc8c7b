"""A NaN row of X0 stays inside its K-hop ball.

The reference (scipy CSR @ dense, WATS.py:29-37) multiplies stored entries only, so a non-finite row of
X0 reaches exactly the rows within K hops of it and every other row of S and H keeps the bits of the
finite run (test_oracle_confines_nan pins that on the CPU).  A kernel that gathers something it should
not and hides it with a multiplication by 0, a masked lane or a shuffle across teams is right for
finite data and leaks the NaN.  The rows allowed to differ are computed here on the CPU, by K rounds
of breadth-first search on the symmetrised pattern, never read off the output.

The hybrid step is the documented exception (DESIGN.md "Parity"): a dense block
multiplies stored zeros by u, so 0 x NaN reaches the block's other rows by construction.  Its finite
form is asserted instead: one row of X0 set to 1e6 changes no row outside its ball, bitwise.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import test_handle_reuse as R
from oracle import wats_oracle as O

import wats_hip  # noqa: E402

NAN_ROW = 2000   # G0: the end of the 64-node path (caller ids 2000 .. 2063)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def ball(A, row, K):
    """rows within K hops of `row` on the symmetrised pattern (K rounds of breadth-first search)"""
    P = ((A != 0) + (A != 0).T).tocsr()
    seen = np.zeros(A.shape[0], bool)
    seen[row] = True
    frontier = np.array([row])
    for _ in range(K):
        nxt = np.unique(np.concatenate([P.indices[P.indptr[r]:P.indptr[r + 1]] for r in frontier] + [np.zeros(0, np.int64)]))
        nxt = nxt[~seen[nxt.astype(np.int64)]].astype(np.int64)
        seen[nxt] = True
        frontier = nxt
        if frontier.size == 0:
            break
    return seen


def test_oracle_confines_nan():
    """the reference behaviour the GPU tests hold to: the oracle makes exactly rows 2000 .. 2000 + K
    non-finite and leaves every other row of S and H bitwise equal to the finite run"""
    A = R.graph_g0()
    for K in (1, 3, 16):
        inside = ball(A, NAN_ROW, K)
        assert np.array_equal(np.flatnonzero(inside), np.arange(NAN_ROW, NAN_ROW + K + 1))
        for F in (1, 8):
            X = np.random.default_rng(10 * K + F).standard_normal((A.shape[0], F)).astype(np.float32)
            fin = O.graph_wavelet_features(A, k=K, s=0.8, X0=X, return_all=True)
            Xn = X.copy()
            Xn[NAN_ROW] = np.nan
            with np.errstate(invalid="ignore"):
                nan = O.graph_wavelet_features(A, k=K, s=0.8, X0=Xn, return_all=True)
            for key in ("S", "H"):
                assert np.array_equal(nan[key][~inside], fin[key][~inside])
                assert not np.isfinite(nan[key][inside]).any()


def _confined(L, A, F, K, row, what, bad=float("nan")):
    """the run with X0[row] = bad against the finite run on the same handle"""
    n = A.shape[0]
    inside = torch.from_numpy(ball(A, row, K)).cuda()
    assert 0 < int(inside.sum()) < n // 2, f"{what}: the ball ({int(inside.sum())} rows) leaves nothing to compare"
    Xh = np.random.default_rng(100 * K + F).standard_normal((n, F)).astype(np.float32)
    S0, H0 = R.checked_call(L, Xh, K)
    Xb = Xh.copy()
    Xb[row] = bad
    S1, H1 = R.checked_call(L, Xb, K)
    assert not L.chain_status()
    assert bool(torch.isfinite(S0).all() and torch.isfinite(H0).all()), what
    for name, a, b in (("S", S1, S0), ("H", H1, H0)):
        out = ~inside
        diff = (a[out] != b[out]).any(dim=1) | ~torch.isfinite(a[out]).all(dim=1)
        rows = out.nonzero().flatten()[diff]
        assert rows.numel() == 0, f"{what}: {name} changed in {rows.numel()} rows outside the ball, first {rows[:8].tolist()}"
        if bad != bad:
            assert not bool(torch.isfinite(a[inside]).any()), f"{what}: a finite {name} entry inside the ball"


pytest_gpu = pytest.mark.gpu


@pytest_gpu
@pytest.mark.parametrize("F", [4, 40, 64])
def test_team_kernel_confines_nan(gpu, F):
    """the team kernel, K = 1, 3, 16, straight-line and generic kernels, folded first launch and a
    permute-in pass"""
    A = R.graph_g0()
    for spec in (1, 0):
        for fold in (1, 0):
            L = R.make_handle(A, dict(team_spec=spec, fold=fold))
            for K in (1, 3, 16):
                _confined(L, A, F, K, NAN_ROW, f"team F={F} K={K} spec={spec} fold={fold}")
            assert "team:" in L.describe(F) and f"spec={spec}" in L.describe(F), L.describe(F)
            L.close()


@pytest_gpu
@pytest.mark.parametrize("knobs,F,names", [
    (dict(team=0, block_iter=16, chunk_iter=8), 40, ["split rows"]),
    ({}, 6, ["team:"]),
    (dict(lds=1, chain=0), 1, ["lds1:"]),
    (dict(lds=2, chain=0), 1, ["lds1:", "windows"]),
    (dict(lds=4, chain=0), 1, ["lds1:", "hub teams"]),
    ({}, 1, ["chain1:", "(solo:"]),
    (dict(chain_wg=4), 1, ["chain1:", "4 workers"]),
], ids=["wg-split-rows", "F6", "lds1", "lds2", "lds4", "chain-solo", "chain-wg4"])
def test_other_kernels_confine_nan(gpu, knobs, F, names):
    """the workgroup kernel with split rows, a padded width, and F = 1 through the LDS row teams, chunk
    windows, hub teams, the one-workgroup chain and 4 chain workers"""
    A = R.graph_g0()
    L = R.make_handle(A, knobs)
    for K in (1, 3, 16):
        _confined(L, A, F, K, NAN_ROW, f"{knobs} F={F} K={K}")
    desc = L.describe(R.padded_width(F))
    for nm in names:
        assert nm in desc, desc
    L.close()


@pytest_gpu
def test_valued_path_confines_nan(gpu):
    """G0 with random positive weights (CSR values gathered), F = 12"""
    A = R.graph_g0().copy()
    A.data = np.random.default_rng(5).uniform(0.1, 2.0, A.nnz).astype(np.float32)
    L = R.make_handle(A)
    for K in (1, 3, 16):
        _confined(L, A, 12, K, NAN_ROW, f"valued F=12 K={K}")
    assert "team:" not in L.describe(12)
    L.close()


@pytest_gpu
@pytest.mark.parametrize("F", [4, 40, 64, 1])
def test_nan_at_a_hub_leaf(gpu, F):
    """NaN at a leaf of the 1300-neighbour hub, K = 1: the ball is the leaf and its neighbours (the hub),
    and every other leaf of that hub shares waves with it"""
    A = R.graph_g0()
    deg = np.diff(A.indptr)
    hub = int(np.argmax(deg))
    assert deg[hub] >= 1250
    nb = A.indices[A.indptr[hub]:A.indptr[hub + 1]]
    leaf = int(nb[deg[nb] == 1][0])
    assert np.array_equal(np.flatnonzero(ball(A, leaf, 1)), np.sort([leaf, hub]))
    for knobs in ({}, dict(team_spec=0), dict(fold=0), dict(team=0, block_iter=16, chunk_iter=8)) if F > 1 else \
            (dict(lds=1, chain=0), dict(lds=2, chain=0), dict(lds=4, chain=0), {}, dict(chain_wg=4)):
        L = R.make_handle(A, knobs)
        _confined(L, A, F, 1, leaf, f"hub leaf {knobs} F={F}")
        L.close()


@pytest_gpu
@pytest.mark.parametrize("F", [7, 64, 500])
def test_propagate_confines_nan(gpu, F):
    """adj_norm @ x on G0 plus self loops: a one-hop ball, forward and backward"""
    A = (R.graph_g0() + sp.identity(R.graph_g0().shape[0], dtype=np.float32, format="csr")).tocsr()
    n = A.shape[0]
    op = wats_hip.RowNormalizedAdjacency.from_scipy(A)
    inside = torch.from_numpy(ball(A, NAN_ROW, 1)).cuda()
    assert int(inside.sum()) == 2
    gen = torch.Generator("cuda").manual_seed(F)
    x, gy = torch.randn(n, F, device="cuda", generator=gen), torch.randn(n, F, device="cuda", generator=gen)

    def run(xx, gg):
        xx = xx.clone().requires_grad_(True)
        y = wats_hip.propagate(op, xx)
        y.backward(gg)
        torch.cuda.synchronize()
        return y.detach(), xx.grad

    y0, g0 = run(x, gy)
    xn, gn = x.clone(), gy.clone()
    xn[NAN_ROW] = float("nan")
    gn[NAN_ROW] = float("nan")
    y1, g1 = run(xn, gn)
    for name, a, b in (("y", y1, y0), ("grad", g1, g0)):
        assert torch.equal(a[~inside], b[~inside]), f"propagate F={F}: {name} changed outside the ball"
        assert not bool(torch.isfinite(a[inside]).any()), f"propagate F={F}: finite {name} inside the ball"


@pytest_gpu
@pytest.mark.parametrize("F", [48, 64])
def test_hybrid_step_confines_a_finite_change(gpu, F):
    """The hybrid step (dense blocks on the matrix cores) multiplies stored zeros by u, so a NaN reaches
    a block's other rows by construction: non-finite X0 differs from the reference there (DESIGN.md
    "Parity").  The finite form holds: one row of X0 set to 1e6 changes no row outside its ball."""
    A = R.graph_hybrid()
    deg = np.diff(A.indptr)
    row = int(np.flatnonzero(deg == deg[deg > 0].min())[0])
    for extra in (dict(hyb_conc=0), dict(hyb_conc=2), dict(team=0)):
        L = R.make_handle(A, dict(tiles=1, tile_th=8, tile_max=3, **extra))
        for K in (1, 2):
            _confined(L, A, F, K, row, f"hybrid {extra} F={F} K={K}", bad=1e6)
        assert "tiles:" in L.describe(F), L.describe(F)
        L.close()
