"""CPU tests of the edge-flip views: the argument checks of wg_flip_resolve / wg_flip_rows / wg_flip_cols /
wg_csr_patch, which run before any device work, and the Python surface without a GPU."""
import ctypes
import importlib

import pytest
import torch

import wats_hip
from wats_hip import _lib

ONE = 4096              # a non-NULL address; validation must fail before anything reads it
INT32_MAX = 2**31 - 1
INVALID, UNSUPPORTED = -1, -4


def _resolve(lib, **kw):
    a = dict(n=10, indptr=ONE, indices=ONE, values=None, T=2, t_rows=ONE, seg=ONE, P=3, cols=ONE, a_old=ONE,
             base_pos=ONE, row_sum=ONE)
    a.update(kw)
    return lib.wg_flip_resolve(a["n"], a["indptr"], a["indices"], a["values"], a["T"], a["t_rows"], a["seg"], a["P"],
                               a["cols"], a["a_old"], a["base_pos"], a["row_sum"], None)


def _rows(lib, **kw):
    a = dict(n=10, indptr=ONE, indices=ONE, values=None, T=2, t_rows=ONE, seg=ONE, P=3, cols=ONE, a_new=ONE,
             base_pos=ONE, deg_new=ONE, F=4, x=ONE, y=ONE)
    a.update(kw)
    return lib.wg_flip_rows(a["n"], a["indptr"], a["indices"], a["values"], a["T"], a["t_rows"], a["seg"], a["P"],
                            a["cols"], a["a_new"], a["base_pos"], a["deg_new"], a["F"], a["x"], a["y"], None)


def _cols(lib, **kw):
    a = dict(n=10, C=2, c_cols=ONE, cseg=ONE, P=3, rows=ONE, a_new=ONE, a_old=ONE, deg_new=ONE, F=4, g=ONE, gx=ONE)
    a.update(kw)
    return lib.wg_flip_cols(a["n"], a["C"], a["c_cols"], a["cseg"], a["P"], a["rows"], a["a_new"], a["a_old"],
                            a["deg_new"], a["F"], a["g"], a["gx"], None)


_NNZ = ctypes.c_int64(0)


def _patch(lib, **kw):
    a = dict(n=10, nnz=20, indptr=ONE, indices=ONE, values=None, T=2, t_rows=ONE, seg=ONE, P=3, cols=ONE, a_new=ONE,
             base_pos=ONE, out_indptr=ONE, out_indices=ONE, out_values=ONE, capacity=23, nnz_host=ctypes.byref(_NNZ))
    a.update(kw)
    return lib.wg_csr_patch(a["n"], a["nnz"], a["indptr"], a["indices"], a["values"], a["T"], a["t_rows"], a["seg"],
                            a["P"], a["cols"], a["a_new"], a["base_pos"], a["out_indptr"], a["out_indices"],
                            a["out_values"], a["capacity"], a["nnz_host"], None)


SHARED = [   # the overlay's shape, checked alike by the three entries that take it
    (dict(n=-1), INVALID, b"negative size"),
    (dict(P=-1), INVALID, b"negative size"),
    (dict(T=-1), INVALID, b"negative size"),
    (dict(n=INT32_MAX + 1), UNSUPPORTED, b"exceeds int32"),
    (dict(T=4), INVALID, b"touched rows"),
    (dict(T=0), INVALID, b"touched rows"),
    (dict(indptr=None), INVALID, b"NULL indptr"),
    (dict(t_rows=None), INVALID, b"NULL t_rows"),
    (dict(seg=None), INVALID, b"NULL t_rows"),
    (dict(cols=None), INVALID, b"NULL t_rows"),
]


@pytest.mark.parametrize("call,name,extra", [
    (_resolve, b"wg_flip_resolve", [(dict(a_old=None), INVALID, b"NULL a_old"), (dict(base_pos=None), INVALID, b"NULL a_old"),
                                    (dict(row_sum=None), INVALID, b"NULL a_old")]),
    (_rows, b"wg_flip_rows", [(dict(F=0), INVALID, b"F must be >= 1"), (dict(y=None), INVALID, b"NULL a_new"),
                              (dict(x=None), INVALID, b"NULL a_new"), (dict(a_new=None), INVALID, b"NULL a_new"),
                              (dict(deg_new=None), INVALID, b"NULL a_new")]),
    (_patch, b"wg_csr_patch", [(dict(nnz=-1), INVALID, b"negative size"),
                               (dict(nnz=INT32_MAX - 2), UNSUPPORTED, b"exceeds int32"),
                               (dict(nnz=INT32_MAX + 5), UNSUPPORTED, b"exceeds int32"),
                               (dict(n=INT32_MAX, T=2), UNSUPPORTED, b"exceeds int32"),
                               (dict(capacity=22), INVALID, b"capacity"),
                               (dict(out_indptr=None), INVALID, b"NULL indptr"),
                               (dict(nnz_host=None), INVALID, b"NULL indptr"),
                               (dict(indices=None), INVALID, b"NULL indices"),
                               (dict(a_new=None), INVALID, b"NULL a_new"),
                               (dict(out_indices=None), INVALID, b"NULL out_indices"),
                               (dict(out_values=None), INVALID, b"NULL out_indices")]),
])
def test_flip_entries_reject_bad_arguments_before_device_work(call, name, extra):
    lib = _lib.load()
    for kw, code, msg in SHARED + extra:
        assert call(lib, **kw) == code, (name, kw)
        err = lib.wg_last_error()
        assert err.startswith(name) and msg in err, (kw, err)
    with pytest.raises(_lib.WaveletError, match=name.decode()):
        _lib.check(call(lib, n=-1), "flip")


def test_flip_cols_rejects_bad_arguments_before_device_work():
    lib = _lib.load()
    cases = [
        (dict(n=-1), INVALID, b"negative size"),
        (dict(P=-1), INVALID, b"negative size"),
        (dict(C=-1), INVALID, b"negative size"),
        (dict(n=INT32_MAX + 1), UNSUPPORTED, b"exceeds int32"),
        (dict(C=4), INVALID, b"columns for"),
        (dict(C=0), INVALID, b"columns for"),
        (dict(F=0), INVALID, b"F must be >= 1"),
        (dict(gx=None), INVALID, b"NULL"),
        (dict(g=None), INVALID, b"NULL"),
        (dict(cseg=None), INVALID, b"NULL"),
        (dict(deg_new=None), INVALID, b"NULL"),
    ]
    for kw, code, msg in cases:
        assert _cols(lib, **kw) == code, kw
        err = lib.wg_last_error()
        assert err.startswith(b"wg_flip_cols") and msg in err, (kw, err)


def test_flips_module_imports_without_a_gpu():
    mod = importlib.import_module("wats_hip.flips")
    assert wats_hip.FlippedAdjacency is mod.FlippedAdjacency
    assert issubclass(mod.FlippedAdjacency, wats_hip.RowNormalizedAdjacency)
    for name in ("with_flips", "csr", "to_graph", "materialize", "flipped", "dense_row", "compose"):
        assert callable(getattr(mod.FlippedAdjacency, name))
    assert callable(wats_hip.RowNormalizedAdjacency.with_flips)


def test_with_flips_without_a_gpu_raises_the_package_error(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    op = object.__new__(wats_hip.RowNormalizedAdjacency)    # no operator can be built without a GPU: only the method is called
    op.n, op.device = 5, None
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        op.with_flips([0], [1])
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        wats_hip.FlippedAdjacency.compose(op, None, [0], [1])
