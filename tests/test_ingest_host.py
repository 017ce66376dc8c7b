"""CPU tests of the edge-list ingestion: the numpy restatement of its semantics
(tests/ingest_ref.py) against the reference's dense pipeline in torch, and the
argument checks of wg_coo_capacity / wg_coo_to_csr, which run before any
device work."""
import ctypes
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from ingest_ref import dense_pipeline, ingest_ref

import wats_hip
from wats_hip import _lib

MODES = list(itertools.product(("one", "sum"), (False, True), ("keep", "remove", "one")))
INT32_MAX = 2**31 - 1


def random_edges(n, n_edges, seed, weighted):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, size=n_edges)
    dst = rng.integers(0, n, size=n_edges)
    src[: n_edges // 10] = dst[: n_edges // 10]            # loops
    src[-n_edges // 5:] = src[: n_edges // 5]              # duplicates
    dst[-n_edges // 5:] = dst[: n_edges // 5]
    # small integers (zero-sum pairs included): every order of summation is exact
    w = rng.integers(-3, 4, size=n_edges).astype(np.float32) if weighted else None
    return src, dst, w


@pytest.mark.parametrize("duplicates,symmetric,self_loops", MODES)
def test_ingest_ref_matches_dense_pipeline(duplicates, symmetric, self_loops):
    n, n_edges = 40, 300
    src, dst, w = random_edges(n, n_edges, seed=1, weighted=duplicates == "sum")
    indptr, indices, values = ingest_ref(src, dst, n, w, duplicates, symmetric, self_loops)
    ref = sp.csr_matrix(dense_pipeline(src, dst, n, w, duplicates, symmetric, self_loops).numpy())
    ref.sort_indices()
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and values.dtype == np.float32
    assert np.array_equal(indptr, ref.indptr)
    assert np.array_equal(indices, ref.indices)
    assert np.array_equal(values, ref.data)
    assert ref.nnz < n_edges * (2 if symmetric else 1) + n, "the case has duplicates"


@pytest.mark.parametrize("flags", [f for f in range(16) if (f & 12) != 12])
def test_coo_capacity(flags):
    lib = _lib.load()
    n, n_edges = 1000, 12345
    cap = ctypes.c_int64(-1)
    assert lib.wg_coo_capacity(n, n_edges, flags, ctypes.byref(cap)) == 0
    want = n_edges * (2 if flags & _lib.WG_COO_SYMMETRIC else 1) + (n if flags & _lib.WG_COO_LOOPS_ONE else 0)
    assert cap.value == want
    assert lib.wg_coo_capacity(0, 0, flags, ctypes.byref(cap)) == 0 and cap.value == 0


def test_coo_capacity_limits():
    lib = _lib.load()
    cap = ctypes.c_int64(-1)
    sym, loops_one = _lib.WG_COO_SYMMETRIC, _lib.WG_COO_LOOPS_ONE
    assert lib.wg_coo_capacity(10, INT32_MAX, 0, ctypes.byref(cap)) == 0 and cap.value == INT32_MAX
    for n, n_edges, flags in [(10, INT32_MAX + 1, 0), (10, 2**30, sym), (INT32_MAX + 1, 0, 0),
                              (INT32_MAX, 1, loops_one), (10, 2**62, sym)]:
        assert lib.wg_coo_capacity(n, n_edges, flags, ctypes.byref(cap)) == -4, (n, n_edges, flags)
        assert b"exceed" in lib.wg_last_error()
    assert lib.wg_coo_capacity(-1, 0, 0, ctypes.byref(cap)) == -1
    assert lib.wg_coo_capacity(10, 10, 12, ctypes.byref(cap)) == -1
    assert lib.wg_coo_capacity(10, 10, 0, None) == -1


def test_coo_to_csr_rejects_bad_arguments_before_device_work():
    """Never-dereferenced dummy addresses stand for the device buffers: every call fails in validation."""
    lib = _lib.load()
    nnz = ctypes.c_int64(0)
    buf = 4096   # a non-NULL address; never read or written
    ok = dict(n=10, n_edges=5, src=buf, dst=buf, id_bytes=8, weights=None, flags=0, indptr=buf, indices=buf,
              values=None, capacity=5, nnz_host=ctypes.byref(nnz), stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.wg_coo_to_csr(a["n"], a["n_edges"], a["src"], a["dst"], a["id_bytes"], a["weights"], a["flags"],
                                 a["indptr"], a["indices"], a["values"], a["capacity"], a["nnz_host"], a["stream"])

    cases = [
        (dict(n=-1), b"negative"),
        (dict(id_bytes=3), b"id_bytes"),
        (dict(flags=_lib.WG_COO_LOOPS_REMOVE | _lib.WG_COO_LOOPS_ONE), b"exclude"),
        (dict(weights=buf), b"weights need WG_COO_SUM"),
        (dict(capacity=4), b"capacity"),
        (dict(flags=_lib.WG_COO_SYMMETRIC, capacity=9), b"capacity"),
        (dict(indptr=None), b"NULL indptr"),
        (dict(nnz_host=None), b"NULL indptr"),
        (dict(src=None), b"NULL src"),
        (dict(indices=None), b"NULL indices"),
        (dict(flags=_lib.WG_COO_SUM), b"values"),
        (dict(flags=32), b"unknown flag"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, kw
        assert msg in lib.wg_last_error(), (kw, lib.wg_last_error())
    with pytest.raises(_lib.WaveletError):
        _lib.check(call(n=-1), "coo_to_csr")


def test_edge_index_to_csr_rejects_bad_input():
    """Shapes, modes and dtypes are checked before the GPU is asked for."""
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    w = torch.ones(3)
    bad = [
        (dict(edge_index=ei.t().contiguous()), "shape"),
        (dict(edge_index=ei[0]), "shape"),
        (dict(edge_index=ei.to(torch.float32)), "int32 or int64"),
        (dict(edge_index=ei.numpy().astype(np.float64)), "int32 or int64"),
        (dict(edge_index=ei, duplicates="max"), "duplicates"),
        (dict(edge_index=ei, self_loops="drop"), "self_loops"),
        (dict(edge_index=ei, convention="pyg"), "convention"),
        (dict(edge_index=ei, weights=w), "weights need"),
        (dict(edge_index=ei, weights=w, convention="attack"), "weights need"),
        (dict(edge_index=[[0, 1], [1, 0]]), "tensor or a numpy array"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            wats_hip.edge_index_to_csr(**kw)
