"""CPU tests of the edge-gradient feature: the argument validation of wg_sddmm /
wg_rowdot (it runs before any device call) and toggle_edges, the attack's edge
flip (reference calib_attack/calib_fga.py:901-904), against the dense update
followed by scipy's CSR conversion."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import wats_hip
from wats_hip import _lib
from wats_hip.graphgen import random_graph

ONE = ctypes.c_void_p(16)   # a non-NULL pointer; validation must fail before anything reads it


def test_sddmm_rejects_bad_arguments_without_gpu_work():
    lib = _lib.load()
    bad = [
        # n_pairs, rows, cols, F, A, n_a, B, n_b, row_term, row_scale, out
        ((-1, ONE, ONE, 4, ONE, 5, ONE, 5, None, None, ONE), b"negative size"),
        ((3, ONE, ONE, 4, ONE, -5, ONE, 5, None, None, ONE), b"negative size"),
        ((3, ONE, ONE, 4, ONE, 5, ONE, -5, None, None, ONE), b"negative size"),
        ((3, ONE, ONE, 0, ONE, 5, ONE, 5, None, None, ONE), b"F must be >= 1"),
        ((3, ONE, ONE, -2, ONE, 5, ONE, 5, None, None, ONE), b"F must be >= 1"),
        ((3, None, ONE, 4, ONE, 5, ONE, 5, None, None, ONE), b"NULL"),
        ((3, ONE, None, 4, ONE, 5, ONE, 5, None, None, ONE), b"NULL"),
        ((3, ONE, ONE, 4, None, 5, ONE, 5, None, None, ONE), b"NULL"),
        ((3, ONE, ONE, 4, ONE, 5, None, 5, None, None, ONE), b"NULL"),
        ((3, ONE, ONE, 4, ONE, 5, ONE, 5, None, None, None), b"NULL"),
        ((3, ONE, ONE, 4, ONE, 0, ONE, 5, None, None, ONE), b"empty operand"),
    ]
    for args, msg in bad:
        assert lib.wg_sddmm(*args, None) == -1, args
        err = lib.wg_last_error()
        assert err.startswith(b"wg_sddmm") and msg in err, (args, err)
    # nothing to do: WG_OK, no launch, no pointer read
    assert lib.wg_sddmm(0, None, None, 4, None, 0, None, 0, None, None, None, None) == 0
    with pytest.raises(_lib.WaveletError, match="wg_sddmm"):
        _lib.check(lib.wg_sddmm(-1, None, None, 1, None, 0, None, 0, None, None, None, None), "sddmm")


def test_rowdot_rejects_bad_arguments_without_gpu_work():
    lib = _lib.load()
    bad = [
        ((-1, 4, ONE, ONE, ONE), b"negative size"),
        ((3, 0, ONE, ONE, ONE), b"F must be >= 1"),
        ((3, 4, None, ONE, ONE), b"NULL"),
        ((3, 4, ONE, None, ONE), b"NULL"),
        ((3, 4, ONE, ONE, None), b"NULL"),
    ]
    for args, msg in bad:
        assert lib.wg_rowdot(*args, None) == -1, args
        err = lib.wg_last_error()
        assert err.startswith(b"wg_rowdot") and msg in err, (args, err)
    assert lib.wg_rowdot(0, 4, None, None, None, None) == 0


# ----------------------------------------------------------------- toggle_edges
def _graphs():
    g = random_graph(40, 0.12, seed=1, directed=False, weighted=False)
    binary = g.to_scipy().astype(np.float32).toarray()
    assert (binary == binary.T).all() and not binary.diagonal().any() and set(np.unique(binary)) == {0.0, 1.0}
    g = random_graph(40, 0.12, seed=2, directed=True, weighted=True, self_loop_frac=0.3)
    weighted = g.to_scipy().astype(np.float32).toarray()
    assert (weighted != weighted.T).any() and weighted.diagonal().any()
    weighted[7] = 0
    weighted[7, [2, 9, 30]] = 1       # entries equal to 1 (a flip removes them), in a row without a self loop
    return {"binary_symmetric": binary, "weighted_directed_selfloops": weighted}


GRAPHS = _graphs()


def _pairs(dense, kind):
    """(rows, cols) by what the flip does to this graph."""
    n = dense.shape[0]
    off = ~np.eye(n, dtype=bool)
    if kind == "removes":           # a stored 1 becomes 1 + (1 - 2) = 0 and is dropped
        r, c = np.argwhere((dense == 1) & off)[0]
        return [int(r)], [int(c)]
    if kind == "adds":              # an absent entry becomes 1
        r, c = np.argwhere((dense == 0) & (dense.T == 0) & off)[0]
        return [int(r)], [int(c)]
    if kind == "empties_row":       # every entry of a row of ones without a self loop
        r = next(i for i in range(n) if dense[i].any() and np.all(dense[i][dense[i] != 0] == 1) and not dense[i, i])
        cs = np.flatnonzero(dense[r])
        return [int(r)] * len(cs), [int(c) for c in cs]
    if kind == "mixed":             # present and absent positions, weights other than 1 among them
        rs, cs = np.argwhere(np.triu(off))[::37].T
        return [int(v) for v in rs], [int(v) for v in cs]
    raise AssertionError(kind)


def _dense_flip(dense, rows, cols, symmetric):
    """calib_fga.py:901-904 on the dense float32 matrix, one pair after the other."""
    a = dense.copy()
    for r, c in zip(rows, cols):
        v = np.float32(-2) * a[r, c] + np.float32(1)
        a[r, c] += v
        if symmetric:
            a[c, r] += v
    return a


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("kind", ["removes", "adds", "empties_row", "mixed"])
@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_toggle_edges_matches_dense_flip_then_scipy(graph, kind, symmetric):
    dense = GRAPHS[graph]
    rows, cols = _pairs(dense, kind)
    A = sp.csr_matrix(dense)
    A.sort_indices()
    out = wats_hip.toggle_edges(dense.shape[0], torch.from_numpy(A.indptr.astype(np.int64)),
                                torch.from_numpy(A.indices.astype(np.int32)), torch.from_numpy(A.data), rows, cols,
                                symmetric=symmetric)
    flipped = _dense_flip(dense, rows, cols, symmetric)
    ref = sp.csr_matrix(flipped)
    ref.sort_indices()
    assert out[0].dtype == torch.int64 and out[1].dtype == torch.int32 and out[2].dtype == torch.float32
    np.testing.assert_array_equal(out[0].numpy(), ref.indptr)
    np.testing.assert_array_equal(out[1].numpy(), ref.indices)
    np.testing.assert_array_equal(out[2].numpy().view(np.uint32), ref.data.astype(np.float32).view(np.uint32))
    if kind == "empties_row":
        r = rows[0]
        assert ref.indptr[r + 1] == ref.indptr[r] and A.indptr[r + 1] > A.indptr[r]
    if kind == "removes":
        assert flipped[rows[0], cols[0]] == 0 and dense[rows[0], cols[0]] == 1
    if kind == "adds":
        assert flipped[rows[0], cols[0]] == 1 and ref.nnz > A.nnz


def test_toggle_edges_unweighted_input_and_empty_graph():
    """values=None means all ones; a graph without entries gains the flipped edge."""
    dense = GRAPHS["binary_symmetric"]
    A = sp.csr_matrix(dense)
    A.sort_indices()
    args = (torch.from_numpy(A.indptr.astype(np.int64)), torch.from_numpy(A.indices.astype(np.int32)))
    a = wats_hip.toggle_edges(40, *args, None, [3], [17])
    b = wats_hip.toggle_edges(40, *args, torch.from_numpy(A.data), [3], [17])
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    e = wats_hip.toggle_edges(5, torch.zeros(6, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, [4], [1])
    assert e[0].tolist() == [0, 0, 1, 1, 1, 2] and e[1].tolist() == [4, 1] and e[2].tolist() == [1.0, 1.0]


@pytest.mark.parametrize("rows,cols", [([3], [3]), ([1, 5, 1], [2, 6, 2]), ([1, 2], [2, 1])])
def test_toggle_edges_rejects_self_loops_and_repeated_pairs(rows, cols):
    A = sp.csr_matrix(GRAPHS["binary_symmetric"])
    with pytest.raises(ValueError):
        wats_hip.toggle_edges(40, torch.from_numpy(A.indptr.astype(np.int64)),
                              torch.from_numpy(A.indices.astype(np.int32)), torch.from_numpy(A.data), rows, cols)


def test_toggle_edges_rejects_out_of_range_pairs():
    A = sp.csr_matrix(GRAPHS["binary_symmetric"])
    with pytest.raises(ValueError):
        wats_hip.toggle_edges(40, torch.from_numpy(A.indptr.astype(np.int64)),
                              torch.from_numpy(A.indices.astype(np.int32)), torch.from_numpy(A.data), [0], [40])
