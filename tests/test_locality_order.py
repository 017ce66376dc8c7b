"""Rows of equal length ordered by their hottest neighbours (prologue.hip;
WG_FLAG_CALLER_TIES restores the caller's order).  The order may not change what is computed: its
invariants, S and H against the oracle and against the caller-order handle, and the chain eager,
captured and replayed bitwise equal."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import assert_parity
from oracle import wats_oracle as O

pytestmark = pytest.mark.gpu

import wats_hip  # noqa: E402
from wats_hip import NormalizedLaplacian  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def _np(t):
    return t.detach().cpu().numpy()


def _sym(n, src, dst):
    A = sp.coo_matrix((np.ones(len(src), np.float32), (src, dst)), shape=(n, n)).tocsr()
    A = ((A + A.T) > 0).astype(np.float32).tocsr()
    A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    return A


def hub_graph(n=2003, hubs=(600, 500, 400), seed=0):
    """Hubs at caller rows 5, 6, 7 whose leaves interleave in caller order (leaf i belongs to hub
    i % 3), every 7th leaf tied to a second hub, a few leaf-leaf edges, and isolated rows: many rows
    of equal length with different hottest neighbours."""
    rng = np.random.default_rng(seed)
    hub_rows = np.array([5, 6, 7])[:len(hubs)]
    iso = set(range(40, n, 37))
    leaves = np.array([i for i in range(n) if i not in iso and i not in set(hub_rows.tolist())])
    src, dst = [], []
    left = list(hubs)
    for j, i in enumerate(leaves):
        h = j % len(hubs)
        if left[h] > 0:
            src.append(hub_rows[h]); dst.append(i); left[h] -= 1
            if j % 7 == 0:
                h2 = (h + 1 + j // 7 % max(1, len(hubs) - 1)) % len(hubs)
                if left[h2] > 0:
                    src.append(hub_rows[h2]); dst.append(i); left[h2] -= 1
        else:  # no hub left for this leaf: a chain to an earlier leaf
            src.append(leaves[j - 1 - int(rng.integers(0, 5))]); dst.append(i)
    extra = rng.choice(leaves, size=(120, 2))
    src += extra[:, 0].tolist(); dst += extra[:, 1].tolist()
    return _sym(n, np.array(src), np.array(dst))


def _handle(A, **kw):
    return NormalizedLaplacian.from_csr(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, n=A.shape[0], **kw)


def _perm(L):
    """internal row -> caller row"""
    ids = torch.arange(L.n, dtype=torch.float32, device=L.device).reshape(-1, 1)
    return _np(L.permute(ids, to_internal=True)).ravel().astype(np.int64)


@pytest.fixture(scope="module")
def hub_case():
    A = hub_graph()
    X = np.random.default_rng(3).standard_normal((A.shape[0], 40)).astype(np.float32)
    ref = O.graph_wavelet_features(A, k=16, s=0.8, X0=X, return_all=True)
    return A, X, ref


def test_order_invariants(hub_case):
    A = hub_case[0]
    n = A.shape[0]
    Lc = _handle(A, neighbour_ties=False)
    Ln = _handle(A)
    assert Lc.info == Ln.info, "the tie order changed the handle's info"
    pc, pn = _perm(Lc), _perm(Ln)
    assert np.array_equal(np.sort(pn), np.arange(n)) and np.array_equal(np.sort(pc), np.arange(n))
    deg = np.diff(A.indptr)
    colcnt = np.bincount(A.indices, minlength=n)
    pure = (deg == 0) & (colcnt == 0)
    # the parent's order: descending length, closed-form rows last, ties in caller order
    key = deg * 2 + (~pure)
    assert np.array_equal(pc, np.argsort(-key, kind="stable"))
    assert np.all(np.diff(deg[pn]) <= 0), "lengths must not increase"
    n_closed = int(Ln.info["n_closed_form"])
    assert n_closed == int(pure.sum()) and n_closed > 0
    assert pure[pn[n - n_closed:]].all() and not pure[pn[:n - n_closed]].any(), "closed-form rows come last"
    # the tie key: rank0 (position under the parent's order) of the hottest and second-hottest neighbour
    rank0 = np.empty(n, np.int64)
    rank0[pc] = np.arange(n)
    m = np.full((n, 2), n, np.int64)
    for r in range(n):
        nb = np.sort(rank0[A.indices[A.indptr[r]:A.indptr[r + 1]]])[:2]
        m[r, :len(nb)] = nb
    full = np.stack([-key[pn], m[pn, 0], m[pn, 1], pn], axis=1)
    assert np.array_equal(np.lexsort(full.T[::-1]), np.arange(n)), "rows are not in (length, tie key, caller) order"
    ties = np.diff(key[pn]) == 0
    assert ties.sum() > 1000 and (np.diff(pn)[ties] < 0).any(), "the graph has no tie that the key reorders"
    assert not np.array_equal(pn, pc)
    # deterministic for a given graph
    L2 = _handle(A)
    assert np.array_equal(_perm(L2), pn)
    for L in (Lc, Ln, L2):
        L.close()


def test_new_order_matches_oracle_and_caller_ties(hub_case):
    A, X, ref = hub_case
    out = {}
    for ties in (True, False):
        L = _handle(A, neighbour_ties=ties)
        H, S = wats_hip.graph_wavelet_features(L, k=16, s=0.8, X0=torch.from_numpy(X), return_S=True)
        assert "team:" in L.describe(40), "the team kernel did not run"
        out[ties] = (_np(S), _np(H))
        assert_parity(out[ties][0], ref["S"], what=f"neighbour_ties={ties} S")
        assert_parity(out[ties][1], ref["H"], what=f"neighbour_ties={ties} H")
        L.close()
    assert_parity(out[True][0], out[False][0], what="new order vs caller ties S")
    assert_parity(out[True][1], out[False][1], what="new order vs caller ties H")


def test_eager_captured_replayed_bitwise(hub_case):
    """The neighbour-ordered ties through the handle's own hipGraph
    (tuning key graph=1: the same buffers three calls in a row): eager, eager, captured + replayed,
    replayed give the same bits."""
    A, X, ref = hub_case
    L = _handle(A)
    L.tune(graph=1)
    lib = wats_hip._lib.load()
    Xd = torch.from_numpy(X).cuda()
    S = torch.zeros_like(Xd)
    H = torch.zeros_like(Xd)
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for _ in range(4):
        S.zero_()
        H.zero_()
        assert lib.wg_wavelet_features(L.handle, Xd.data_ptr(), 40, 16, 0.8, S.data_ptr(), H.data_ptr(), st) == 0
        torch.cuda.synchronize()
        outs.append((S.clone(), H.clone()))
    d = L.describe(40)
    assert "team:" in d and "long_rows=1" in d, d  # the team kernel, the 600-entry hub as part waves
    for S_i, H_i in outs[1:]:
        assert torch.equal(S_i, outs[0][0]) and torch.equal(H_i, outs[0][1])
    assert_parity(_np(outs[-1][0]), ref["S"], what="replayed S")
    assert_parity(_np(outs[-1][1]), ref["H"], what="replayed H")
    L.close()
