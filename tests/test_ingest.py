"""GPU tests of the device-side edge-list ingestion (wg_coo_to_csr, csrc/ingest.hip;
wats_hip.edge_index_to_csr).

Two yardsticks: the reference's dense pipeline on the device followed by
``dense_to_csr``, and the numpy restatement of the semantics in
tests/ingest_ref.py.  Results are compared bit for bit -- indptr, indices and
values, absent values counting as ones -- except for floating weights, where
the bound is one float32 rounding plus the float64 reordering bound of the
reference's own sum:  |got - ref| <= 2^-24 |ref| + terms * 2^-52 * sum|w|."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from ingest_ref import dense_pipeline, ingest_ref, ingest_ref_terms

pytestmark = pytest.mark.gpu

import wats_hip  # noqa: E402
from wats_hip import NormalizedLaplacian, RowNormalizedAdjacency, edge_index_to_csr  # noqa: E402
from wats_hip.graphgen import random_graph  # noqa: E402

MODES = list(itertools.product(("one", "sum"), (False, True), ("keep", "remove", "one")))


def _id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def _edge_index(src, dst, dtype=torch.int64):
    return torch.from_numpy(np.stack([np.asarray(src), np.asarray(dst)]).astype(np.int64)).to(dtype).cuda()


def _assert_csr(g, indptr, indices, values, what=""):
    """g (a DeviceCSR) equals the CSR (indptr, indices, values) bit for bit."""
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    values = np.asarray(values, dtype=np.float32)
    assert g.indptr.dtype == torch.int64 and g.indices.dtype == torch.int32
    assert g.indptr.shape == (g.n + 1,) and g.nnz == int(indptr[-1]) == g.indices.numel(), what
    assert np.array_equal(g.indptr.cpu().numpy(), indptr), f"{what}: indptr"
    assert np.array_equal(g.indices.cpu().numpy(), indices), f"{what}: indices"
    got = np.ones(g.nnz, np.float32) if g.values is None else g.values.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == values.shape
    assert np.array_equal(got.view(np.uint32), values.view(np.uint32)), f"{what}: values"


def _check_against_ref(src, dst, n, w, mode, dtype=torch.int64, what=""):
    duplicates, symmetric, self_loops = mode
    g = edge_index_to_csr(_edge_index(src, dst, dtype), n, None if w is None else torch.from_numpy(w),
                          duplicates=duplicates, symmetric=symmetric, self_loops=self_loops)
    assert (g.values is None) == (duplicates == "one")
    _assert_csr(g, *ingest_ref(src, dst, n, w, *mode), what=f"{what} {mode}")
    return g


def _int_weights(rng, n_edges):
    return rng.integers(-3, 4, size=n_edges).astype(np.float32)


# ------------------------------------------------------------ the dense path on the device
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("duplicates,symmetric,self_loops", MODES)
def test_matches_dense_path(duplicates, symmetric, self_loops, dtype):
    n, n_edges = 67, 400
    rng = np.random.default_rng(2)
    src, dst = rng.integers(0, n, n_edges), rng.integers(0, n, n_edges)
    w = _int_weights(rng, n_edges) if duplicates == "sum" else None
    assert np.count_nonzero(src == dst) > 0 and len(set(zip(src.tolist(), dst.tolist()))) < n_edges
    g = edge_index_to_csr(_edge_index(src, dst, dtype), n, None if w is None else torch.from_numpy(w),
                          duplicates=duplicates, symmetric=symmetric, self_loops=self_loops)
    adj = dense_pipeline(src, dst, n, w, duplicates, symmetric, self_loops, device="cuda")
    indptr, indices, values = wats_hip.dense_to_csr(adj)
    _assert_csr(g, indptr.cpu().numpy(), indices.cpu().numpy(), values.cpu().numpy(), what="dense path")
    assert torch.equal(g.to_dense(), adj)
    A = g.to_scipy()
    assert A.has_canonical_format and np.array_equal(A.toarray(), adj.cpu().numpy())


# ------------------------------------------------------------ against ingest_ref
@pytest.mark.parametrize("mode", MODES, ids=_id)
@pytest.mark.parametrize("n,loops", [(0, 0), (1, 0), (1, 3), (5, 0)])
def test_degenerate_sizes(n, loops, mode):
    src = dst = np.zeros(loops, np.int64)
    w = np.array([2.0, -0.5, 1.0], np.float32)[:loops] if mode[0] == "sum" else None
    g = _check_against_ref(src, dst, n, w, mode, what=f"n={n} E={loops}")
    if loops == 0:
        assert g.nnz == (n if mode[2] == "one" else 0)
        if mode[2] == "one":
            assert np.array_equal(g.indices.cpu().numpy(), np.arange(n))       # the identity


KEY_MODES = [("one", False, "keep"), ("sum", True, "remove"), ("one", True, "one")]


@pytest.mark.parametrize("n,mode", [(n, m) for n in (2, 256, 257, 65_536, 65_537, 1_048_577) for m in KEY_MODES
                                    if not (n > 65_537 and m[2] == "one")],    # a 10^6-entry python reference
                         ids=_id)
def test_key_width_boundaries(n, mode):
    rng = np.random.default_rng(n)
    ids = np.array([0, 1, n - 2, n - 1])
    src, dst = ids[rng.integers(0, 4, 64)], ids[rng.integers(0, 4, 64)]
    w = _int_weights(rng, 64) if mode[0] == "sum" else None
    for dtype in (torch.int32, torch.int64):
        _check_against_ref(src, dst, n, w, mode, dtype, what=f"n={n}")


@pytest.mark.parametrize("duplicates", ["one", "sum"])
@pytest.mark.parametrize("n_edges", [255, 256, 257, 1025])
def test_block_boundaries(n_edges, duplicates):
    """All edges in two rows and six columns: the runs of equal keys straddle workgroups of 256."""
    n = 50
    rng = np.random.default_rng(n_edges)
    src = np.where(rng.integers(0, 2, n_edges) == 0, 3, 7)
    dst = rng.integers(10, 16, n_edges)
    w = _int_weights(rng, n_edges) if duplicates == "sum" else None
    for symmetric in (False, True):
        _check_against_ref(src, dst, n, w, (duplicates, symmetric, "keep"), what=f"E={n_edges}")


def test_gap_rows():
    n = 1000
    rng = np.random.default_rng(5)
    src = np.where(rng.integers(0, 2, 300) == 0, 3, 998)
    dst = rng.integers(0, n, 300)
    g = _check_against_ref(src, dst, n, None, ("one", False, "keep"), what="gap rows")
    indptr = g.indptr.cpu().numpy()
    in3 = len(set(dst[src == 3].tolist()))
    want = np.concatenate([np.zeros(4), np.full(995, in3), np.full(2, g.nnz)]).astype(np.int64)
    assert np.array_equal(indptr, want)           # every entry: rows in a gap point at the next entry


def test_long_run():
    n = 300
    rng = np.random.default_rng(6)
    src = np.concatenate([rng.integers(18, n, 200), np.full(5000, 17)])     # the others stay out of row 17
    dst = np.concatenate([rng.integers(0, n, 200), np.full(5000, 123)])
    order = rng.permutation(src.size)
    src, dst = src[order], dst[order]
    g = _check_against_ref(src, dst, n, np.ones(src.size, np.float32), ("sum", False, "keep"), what="long run")
    assert g.to_scipy()[17, 123] == 5000.0
    g1 = _check_against_ref(src, dst, n, None, ("one", False, "keep"), what="long run")
    assert g1.to_scipy()[17, 123] == 1.0 and g1.indptr[18] - g1.indptr[17] == 1


def test_cancellation_drops_entries():
    n = 6
    src, dst = np.array([1, 2, 1, 0]), np.array([4, 3, 4, 5])
    w = np.array([2.5, 1.0, -2.5, 7.0], np.float32)
    g = _check_against_ref(src, dst, n, w, ("sum", False, "keep"), what="cancel")
    assert g.nnz == 2 and g.to_scipy()[1, 4] == 0
    src, dst = np.array([1, 4, 0]), np.array([4, 1, 5])
    w = np.array([1.0, -1.0, 7.0], np.float32)
    g = _check_against_ref(src, dst, n, w, ("sum", True, "keep"), what="cancel symmetric")
    assert g.nnz == 2 and np.array_equal(g.indptr.cpu().numpy(), [0, 1, 1, 1, 1, 1, 2])


def test_input_forms():
    n = 90
    rng = np.random.default_rng(7)
    ei = np.stack([rng.integers(0, n, 500), rng.integers(0, n, 500)])
    ei[:, -1] = n - 1                                  # num_nodes=None finds n
    ref = ingest_ref(ei[0], ei[1], n, None, "one", True, "one")
    kw = dict(convention="attack")
    _assert_csr(edge_index_to_csr(torch.from_numpy(ei), n, **kw), *ref, what="CPU tensor")
    _assert_csr(edge_index_to_csr(ei, n, **kw), *ref, what="numpy")
    _assert_csr(edge_index_to_csr(ei.astype(np.int32), n, **kw), *ref, what="numpy int32")
    _assert_csr(edge_index_to_csr(torch.from_numpy(ei).cuda(), **kw), *ref, what="num_nodes=None")
    wide = torch.zeros(2, 1000, dtype=torch.int64, device="cuda")
    wide[:, ::2] = torch.from_numpy(ei).cuda()
    view = wide[:, ::2]
    assert not view.is_contiguous()
    _assert_csr(edge_index_to_csr(view, n, **kw), *ref, what="non-contiguous")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        g = edge_index_to_csr(torch.from_numpy(ei).cuda(), n, **kw)
    stream.synchronize()
    _assert_csr(g, *ref, what="side stream")


def test_float_weights_reproducible_and_bounded():
    n, n_edges = 500, 20_000
    rng = np.random.default_rng(8)
    src, dst = rng.integers(0, n, n_edges), rng.integers(0, n, n_edges)
    w = rng.standard_normal(n_edges).astype(np.float32)
    ei, wt = _edge_index(src, dst), torch.from_numpy(w).cuda()
    a = edge_index_to_csr(ei, n, wt, duplicates="sum", symmetric=True)
    b = edge_index_to_csr(ei, n, wt, duplicates="sum", symmetric=True)
    assert torch.equal(a.indptr, b.indptr) and torch.equal(a.indices, b.indices)
    assert torch.equal(a.values.view(torch.int32), b.values.view(torch.int32))
    indptr, indices, values, terms, mags = ingest_ref_terms(src, dst, n, w, "sum", True, "keep")
    assert np.array_equal(a.indptr.cpu().numpy(), indptr) and np.array_equal(a.indices.cpu().numpy(), indices)
    got, ref = a.values.cpu().numpy().astype(np.float64), values.astype(np.float64)
    bound = 2.0**-24 * np.abs(ref) + terms * 2.0**-52 * mags
    worst = np.max(np.abs(got - ref) - bound)
    print(f"float weights: max |got - ref| = {np.max(np.abs(got - ref)):.3e}, max excess over the bound {worst:.3e}, "
          f"longest run {terms.max()}")
    assert terms.max() > 2 and np.all(np.abs(got - ref) <= bound)


@pytest.mark.parametrize("bad_id", [-1, 40], ids=["minus_one", "n"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_ids_out_of_range(bad_id, dtype):
    n = 40
    rng = np.random.default_rng(9)
    src, dst = rng.integers(0, n, 300), rng.integers(0, n, 300)
    bad_src = src.copy()
    bad_src[[5, 250]] = bad_id
    for s, d in ((bad_src, dst), (dst, bad_src)):
        with pytest.raises(ValueError, match=r"2 ids outside \[0, 40\)"):
            edge_index_to_csr(_edge_index(s, d, dtype), n, convention="attack")
    _check_against_ref(src, dst, n, None, ("one", True, "one"), dtype, what="after a refused call")
    assert torch.ones(4, device="cuda").sum().item() == 4.0        # the process is intact


# ------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def graph300():
    g = random_graph(300, 0.03, seed=11, directed=True)
    rows = np.repeat(np.arange(g.n), np.diff(g.indptr))
    return g.n, rows.astype(np.int64), g.indices.astype(np.int64)


def test_wavelet_features_match_from_scipy(graph300):
    n, src, dst = graph300
    g = edge_index_to_csr(_edge_index(src, dst), n, symmetric=True, self_loops="remove")
    H, S = wats_hip.graph_wavelet_features(g, k=3, return_S=True)
    H2, S2 = wats_hip.graph_wavelet_features(NormalizedLaplacian.from_scipy(g.to_scipy()), k=3, return_S=True)
    assert torch.equal(H, H2) and torch.equal(S, S2)
    L = NormalizedLaplacian.from_edge_index(_edge_index(src, dst), n, symmetric=True, self_loops="remove")
    H3, S3 = wats_hip.graph_wavelet_features(L, k=3, return_S=True)
    assert torch.equal(H, H3) and torch.equal(S, S3)
    assert float(S.abs().max()) > 0


def test_sparse_gcn_matches_from_scipy(graph300):
    n, src, dst = graph300
    torch.manual_seed(0)
    model = wats_hip.SparseCompatibleGCN(16, nclass=5).cuda().eval()
    x = torch.randn(n, 16, device="cuda")
    op = RowNormalizedAdjacency.from_edge_index(_edge_index(src, dst), n, convention="attack")
    g = edge_index_to_csr(_edge_index(src, dst), n, convention="attack")
    ref_op = RowNormalizedAdjacency.from_scipy(g.to_scipy())
    with torch.no_grad():
        out, ref = model(x, op), model(x, ref_op)
    assert torch.equal(out, ref) and float(out.abs().max()) > 0
    op2 = RowNormalizedAdjacency.from_graph(edge_index_to_csr(_edge_index(src, dst), n, convention="attack"))
    with torch.no_grad():
        assert torch.equal(model(x, op2), ref)


def test_conventions_match_the_reference_pipelines(graph300):
    n, src, dst = graph300
    ei = _edge_index(src, dst)
    # ugca_calib_attack.py:42-47
    adj = torch.zeros(n, n, device="cuda")
    adj[ei[0], ei[1]] = 1.0
    adj = adj + adj.t()
    adj = torch.clamp(adj, 0, 1)
    adj.fill_diagonal_(1.0)
    indptr, indices, values = (t.cpu().numpy() for t in wats_hip.dense_to_csr(adj))
    _assert_csr(edge_index_to_csr(ei, n, convention="attack"), indptr, indices, values, what="attack")
    # calibration/utils.py:19-25
    adj = torch.zeros(n, n, device="cuda")
    adj[ei[0], ei[1]] = 1.0
    indptr, indices, values = (t.cpu().numpy() for t in wats_hip.dense_to_csr(adj))
    _assert_csr(edge_index_to_csr(ei, n, convention="harness"), indptr, indices, values, what="harness")
    assert (sp.csr_matrix(adj.cpu().numpy()) != edge_index_to_csr(ei, n, convention="harness").to_scipy()).nnz == 0
