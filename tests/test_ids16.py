"""16-bit column ids for the team step's turns whose columns all fit (tuning key ids16, DESIGN.md 4.1
"Round 10"): the chain's straight-line kernels read a wave's leading turns whose real ids are all
<= 65534 as one 16-B chunk of eight 16-bit ids, the rest as before.  The gathers, their order and the
sums are the same, so S and H may not change a bit: ids16 1 and 0 are compared with torch.equal on one
handle (a tune rebuilds the plan), and ids16 1 against the oracle at test_gpu_parity's tolerances.

Internal column ids are the rows' ranks by descending length, so ids past 65534 are the shortest rows.
big_graph() has about 71 000 active rows: a hub of 1300 neighbours, 400 of them leaves (degree 1: their
only neighbour is column 0, and as the hub's last entries they are high ids in the trailing turns of its
last part), centres of 5 .. 570 neighbours, a ring of degree-2 nodes, and 2 000 leaf-leaf pairs, whose
only neighbour is a high column.  The two edge graphs hold only low ids: 65 535 active rows (a symmetric
ring lattice: the highest id is 65 534), and 65 536 of which the last, the one shorter row, is nobody's
neighbour (directed: column 65 535 does not occur, and must not be mistaken for the pad)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import assert_parity
from oracle import wats_oracle as O
from test_team_spec import spec_graph

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


def _sym(src, dst, n):
    A = sp.coo_matrix((np.ones(len(src), np.float32), (src, dst)), shape=(n, n)).tocsr()
    A = ((A + A.T) > 0).astype(np.float32).tocsr()
    A.sort_indices()
    return A


def big_graph():
    rng = np.random.default_rng(7)
    n_ring, n_hub_leaves, n_pairs = 66600, 400, 2000
    centres = [900, 570, 420, 300, 200, 110] + np.linspace(5, 96, 24).astype(int).tolist()  # ring neighbours each
    ring = np.arange(n_ring)
    src, dst = [ring], [np.roll(ring, -1)]
    nxt = n_ring
    for d in centres:  # centre 0 is the hub
        src.append(np.full(d, nxt))
        dst.append(rng.choice(ring, size=d, replace=False))
        nxt += 1
    hub = n_ring
    leaves = np.arange(nxt, nxt + n_hub_leaves)
    src.append(np.full(n_hub_leaves, hub))
    dst.append(leaves)
    nxt += n_hub_leaves
    src.append(np.arange(nxt, nxt + n_pairs))
    dst.append(np.arange(nxt + n_pairs, nxt + 2 * n_pairs))
    nxt += 2 * n_pairs
    return _sym(np.concatenate(src), np.concatenate(dst), nxt + 50)  # 50 isolated nodes


def lattice_graph(n):
    """every node next to i +- 1, 2, 3: rows of 6 ids, one full turn each"""
    i = np.arange(n)
    return _sym(np.concatenate([i, i, i]), np.concatenate([(i + 1) % n, (i + 2) % n, (i + 3) % n]), n)


def directed_edge_graph(n=65536):
    """rows 0 .. n-2: 6 out-neighbours among the nodes 0 .. n-2; row n-1: 5, and no in-neighbour, so the
    shortest row, rank n-1 = 65 535, is no row's column"""
    m = n - 1
    i = np.arange(m)
    src = [np.repeat(i, 6), np.full(5, m)]
    dst = [((i[:, None] + np.arange(1, 7)[None, :]) % m).ravel(), np.arange(5)]
    A = sp.coo_matrix((np.ones(6 * m + 5, np.float32), (np.concatenate(src), np.concatenate(dst))), shape=(n, n)).tocsr()
    A.sort_indices()
    return A


def _handle(A, **kw):
    return NormalizedLaplacian.from_csr(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, n=A.shape[0], **kw)


_GRAPHS, _REF = {}, {}


def _graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = {"big": big_graph, "lat": lambda: lattice_graph(65535), "dir": directed_edge_graph,
                         "small": lambda: spec_graph(n=3000)}[name]()
    return _GRAPHS[name]


def _case(name, K, F):
    """X0 and the oracle's S / H, computed once per (graph, K, F)"""
    if (name, K, F) not in _REF:
        A = _graph(name)
        X = np.random.default_rng(100 * K + F).standard_normal((A.shape[0], F)).astype(np.float32)
        _REF[(name, K, F)] = (X, O.graph_wavelet_features(A, k=K, s=0.8, X0=X, return_all=True))
    return _REF[(name, K, F)]


def _ids16_line(L, F):
    line = [ln for ln in L.describe(F).splitlines() if ln.startswith("ids16:")]
    assert len(line) == 1, L.describe(F)
    return {k: int(v) for k, v in (t.split("=") for t in line[0].split()[1:])}


def _run(L, X, K):
    H, S = wats_hip.graph_wavelet_features(L, k=K, s=0.8, X0=torch.from_numpy(X), return_S=True)
    torch.cuda.synchronize()
    return S.clone(), H.clone()


def _both(L, name, K, F):
    """the chain with ids16 1 and 0 on one handle: equal bits, the oracle's values; returns both ids16: lines"""
    X, ref = _case(name, K, F)
    out, info = {}, {}
    for v in (1, 0):
        L.tune(ids16=v)
        out[v] = _run(L, X, K)
        info[v] = _ids16_line(L, F)
        assert info[v]["on"] == v
    assert torch.equal(out[1][0], out[0][0]), f"{name} K={K} F={F}: ids16 changed S"
    assert torch.equal(out[1][1], out[0][1]), f"{name} K={K} F={F}: ids16 changed H"
    assert_parity(_np(out[1][0]), ref["S"], what=f"ids16 {name} K={K} F={F} S")
    assert_parity(_np(out[1][1]), ref["H"], what=f"ids16 {name} K={K} F={F} H")
    assert info[0]["turns16"] == 0 and info[0]["ids16_bytes"] == 0 and info[0]["turns"] == info[1]["turns"]
    assert info[0]["ids32_bytes"] == info[1]["ids32_bytes"] > 0
    return info[1], out[1]


@pytest.mark.parametrize("ties", [True, False])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_high_and_low_ids(K, ties):
    """K = 4: every mode; K = 1 and 2: the final launch has no previous row and runs the generic kernel on the
    32-bit ids (at K = 2 behind one straight-line step).  Both tie orders: other ranks for the rows of equal
    length, so other high columns."""
    A = _graph("big")
    deg = np.diff(A.indptr)
    assert deg.max() == 1300 and (deg > 0).sum() >= 70000 and (deg == 1).sum() == 4400
    L = _handle(A, neighbour_ties=ties)
    info, _ = _both(L, "big", K, 40)
    assert 0 < info["turns16"] < info["turns"], info  # converted and kept turns both exist
    assert info["ids16_bytes"] == 16 * ((info["ids32_bytes"] // 16 + 1) // 2), info
    L.close()


@pytest.mark.parametrize("name", ["lat", "dir"])
def test_every_id_low_at_the_edge(name):
    """65 535 and 65 536 active rows and no column past 65 534: every full turn is converted"""
    A = _graph(name)
    assert (np.diff(A.indptr) > 0).sum() == (65535 if name == "lat" else 65536)
    L = _handle(A)
    info, _ = _both(L, name, 4, 8)
    assert info["turns16"] == info["turns"] > 0, info
    L.close()


def test_column_65535_is_high():
    """65 536 rows of a symmetric lattice: column 65 535 occurs in six rows, and their waves keep 32-bit ids"""
    n = 65536
    i = np.arange(n)
    A = _sym(np.concatenate([i, i, i]), np.concatenate([(i + 1) % n, (i + 2) % n, (i + 3) % n]), n)
    _GRAPHS["lat1"] = A
    L = _handle(A)
    info, _ = _both(L, "lat1", 4, 8)
    assert info["turns"] - 6 <= info["turns16"] < info["turns"], info
    L.close()


@pytest.mark.parametrize("F", [4, 36, 64])
def test_widths(F):
    """1, 9 and 16 lanes per row (64, 7 and 4 sub-groups per wave) on the 3 000-row graph of test_team_spec"""
    L = _handle(_graph("small"))
    info, _ = _both(L, "small", 16, F)
    assert info["turns16"] == info["turns"] > 0, info
    L.close()


def test_generic_kernels_ignore_the_key():
    """team_spec 0: every launch on the generic kernel, which reads the 32-bit ids whatever the wave table
    carries in its upper bits"""
    X, _ = _case("big", 4, 40)
    L = _handle(_graph("big"))
    want = _run(L, X, 4)  # the defaults
    assert _ids16_line(L, 40)["turns16"] > 0
    L.tune(team_spec=0)
    got = _run(L, X, 4)
    assert _ids16_line(L, 40)["turns16"] > 0  # built, not read
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    L.tune(ids16=0)
    got = _run(L, X, 4)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    L.close()


def test_rebuild_after_tune():
    """ids16 off and on again on one handle: each tune drops the plans, the next call builds them again and
    gives the first call's bits; a second call on the rebuilt plan reuses it"""
    X, _ = _case("small", 16, 40)
    L = _handle(_graph("small"))
    first = _run(L, X, 16)
    line = _ids16_line(L, 40)
    assert line["on"] == 1 and line["turns16"] > 0
    L.tune(ids16=0)
    off = _run(L, X, 16)
    assert _ids16_line(L, 40)["ids16_bytes"] == 0
    L.tune(ids16=1)
    on = _run(L, X, 16)
    again = _run(L, X, 16)
    assert _ids16_line(L, 40) == line
    for got in (off, on, again):
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])
    L.close()
