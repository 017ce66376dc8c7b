"""The team step's straight-line kernels, one per chain mode (tuning key team_spec):
the launches a Clenshaw-u chain makes after its first run kernels whose launch-uniform flags are fixed
at compile time and whose operand loads are issued behind the wave's first ids.  They may not change
a bit: S and H with team_spec 1 and 0 (the generic kernel for every launch) are compared with
torch.equal on one handle, and both against the oracle at test_gpu_parity's tolerances.

The graph of spec_graph() was run through the step planner on the CPU (plan_team_waves, the entry
tests/c/plan_check.cpp checks, at team_iter 96 with the rows in descending length).  At F = 40 (G = 6
sub-groups, 24 chunks of 4 ids per sub-group, 576 ids per part wave) it gives 306 waves:
  * 5 part waves: the 1300-neighbour hub as parts of 24, 24 and 7 chunks per sub-group (the last short,
    an odd count), the 700-neighbour hub as 24 and 6;
  * 3 / 1 / 1 team waves of LN 6 / 3 / 2 (the rows of 570, 420, 300 / 260, 200 / 150, 110 ids);
  * 296 team waves of LN 1 with 1 .. 24 chunks per sub-group, 211 odd and 90 even counts in all, 204
    of them single-chunk waves (rows of 1 .. 4 ids);
  * 216 closed-form rows (isolated nodes, finished by the first launch).
F = 4 / 8 / 64 (G = 64 / 32 / 4) move the same rows between these kinds: 32 / 60 / 458 waves, LN up to
16, no long row at F = 4 and 8, four long rows in 10 part waves (up to 4 parts) at F = 64.  With
team_iter 32 (192 ids per part wave at F = 40) the hubs are 7 and 4 parts: a last arriver that sums
more than its first batch of four."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import assert_parity
from oracle import wats_oracle as O

pytestmark = pytest.mark.gpu

import wats_hip  # noqa: E402
from wats_hip import NormalizedLaplacian  # noqa: E402
from wats_hip.graphgen import random_graph  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def _np(t):
    return t.detach().cpu().numpy()


def spec_graph(n=2000, seed=0):
    """Unweighted, symmetric: hubs of about 1300 and 700 neighbours, rows of 570 .. 110 ids, rows of
    5 .. 96, many rows of 1 .. 4, about 200 isolated nodes."""
    rng = np.random.default_rng(seed)
    iso = np.arange(7, n, 10)
    rest = np.setdiff1d(np.arange(n), iso)
    big = [1300, 700, 570, 420, 300, 260, 200, 150, 110]
    mid = np.linspace(5, 96, 48).astype(int).tolist()
    centres = rest[:len(big) + len(mid)]
    leaves = rest[len(big) + len(mid):]
    src, dst = [], []
    for c, d in zip(centres, big + mid):
        nb = rng.choice(leaves, size=d, replace=False)
        src += [c] * d
        dst += nb.tolist()
    A = sp.coo_matrix((np.ones(len(src), np.float32), (src, dst)), shape=(n, n)).tocsr()
    A = ((A + A.T) > 0).astype(np.float32).tocsr()
    A.sort_indices()
    return A


def _handle(A, **kw):
    return NormalizedLaplacian.from_csr(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, n=A.shape[0], **kw)


_REF = {}


def _case(A, key, K, F):
    """X0 and the oracle's S / H, computed once per (graph, K, F)"""
    if (key, K, F) not in _REF:
        X = np.random.default_rng(100 * K + F).standard_normal((A.shape[0], F)).astype(np.float32)
        _REF[(key, K, F)] = (X, O.graph_wavelet_features(A, k=K, s=0.8, X0=X, return_all=True))
    return _REF[(key, K, F)]


def _both(L, A, key, K, F):
    """the chain with team_spec 1 and 0 on one handle: equal bits, and the oracle's values"""
    X, ref = _case(A, key, K, F)
    out = {}
    for spec in (1, 0):
        L.tune(team_spec=spec)
        H, S = wats_hip.graph_wavelet_features(L, k=K, s=0.8, X0=torch.from_numpy(X), return_S=True)
        torch.cuda.synchronize()
        out[spec] = (S.clone(), H.clone())
        line = [ln for ln in L.describe(F).splitlines() if ln.startswith("team:")]
        assert line and f"spec={spec}" in line[0], L.describe(F)
    assert torch.equal(out[1][0], out[0][0]), f"K={K} F={F}: team_spec changed S"
    assert torch.equal(out[1][1], out[0][1]), f"K={K} F={F}: team_spec changed H"
    assert_parity(_np(out[1][0]), ref["S"], what=f"team_spec K={K} F={F} S")
    assert_parity(_np(out[1][1]), ref["H"], what=f"team_spec K={K} F={F} H")
    return line[0]


@pytest.fixture(scope="module")
def graph():
    A = spec_graph()
    deg = np.diff(A.indptr)
    assert deg.max() >= 1250 and ((deg >= 650) & (deg <= 750)).sum() == 1
    assert ((deg >= 100) & (deg <= 576)).sum() >= 7 and ((deg >= 5) & (deg <= 96)).sum() >= 40
    assert ((deg >= 1) & (deg <= 4)).sum() >= 1000 and (deg == 0).sum() >= 200
    return A


@pytest.mark.parametrize("F", [4, 8, 40, 64])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 16])
def test_spec_equals_generic(graph, K, F):
    """K = 1: the first launch is the final one; 2: no step in between; 3: the step without a
    previous row only; 4, 16: every mode.  F = 4, 8, 40, 64: 1, 2, 10 and 16 lanes per row."""
    L = _handle(graph)
    line = _both(L, graph, "sym", K, F)
    kv = dict(t.split("=") for t in line.split()[1:])
    if F == 40:  # both hubs as part waves (3 + 2 partial slots)
        assert int(kv["long_rows"]) == 2 and int(kv["part_slots"]) == 5 and int(kv["max_parts"]) == 3, line
    assert int(kv["pending_arrivals"]) == 0, line
    L.close()


@pytest.mark.parametrize("K", [3, 16])
def test_spec_isolated_rows_in_the_chain(K):
    """A directed graph: rows flagged isolated that still enter the chain (their diagonal term reads
    the row's own u in the epilogue)."""
    g = random_graph(1500, 0.004, seed=5, directed=True, weighted=False, self_loop_frac=0.05, isolated_frac=0.05)
    L = NormalizedLaplacian.from_graph(g)
    _both(L, g.to_scipy(), "dir", K, 40)
    L.close()


def test_spec_follows_fold_and_tie_order(graph):
    """fold 0 (a permute-in pass, then the same modes from the first step on) and the caller's tie
    order (another row order, so other waves)."""
    L = _handle(graph)
    L.tune(fold=0)
    _both(L, graph, "sym", 16, 40)
    L.close()
    L = _handle(graph, neighbour_ties=False)
    _both(L, graph, "sym", 16, 40)
    L.close()


def test_spec_many_parts(graph):
    """team_iter 32: the hubs as 7 and 4 part waves, so a last arriver goes round its loop after the
    first four parts, once with a part that does not exist."""
    L = _handle(graph)
    L.tune(team_iter=32)
    line = _both(L, graph, "sym", 16, 40)
    kv = dict(t.split("=") for t in line.split()[1:])
    assert int(kv["max_parts"]) == 7 and int(kv["npot_rows"]) >= 1, line
    L.close()
