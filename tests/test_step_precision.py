"""Every Chebyshev step kernel against the float64 oracle in ROW units (tests/cheb_ref.py).

conftest.assert_parity scales an error by the column's maximum, which on a power-law graph is a hub's entry: the
leaves are invisible, and a step that loses the third bf16 piece of u or sums a row in float32 passes it
(tests/test_step_precision_host.py shows both).  Here every row is measured against its own absolute sum,
  c = max |got - truth| / unit,   unit_i = 2^-24 (|ck x0_i| + |cacc| sum_j |L_ij| |b1_j| + |b2_i|)   (one step)
                                  unit_i = 2^-24 max_k (2 |L| |T_k| + |T_k|)_i                       (a chain)
with no row left out, and the bounds come from the documented arithmetic, never from a kernel:
  valued step, wg_spmm                     c <= 2   float64 sums rounded once + the stored value's rounding
  value-free step (u = b dinv gathered)    c <= 6   final rounding, u, dinv_j, dinv_i, two inside the float32 L_hat
  hybrid step                              c <= max(6, c of the plain float32 CSR product on the same inputs)
  chains                                   c <= 2 max(c of the forward / Clenshaw / value-free Clenshaw models)
  H                                        |H - S / (|S|_1 + 1e-8)| <= 1.5 * 2^-24 |H| for the S that was returned
(a) one step through wg_clenshaw_step, (b) F = 1 through wg_cheb_step, wg_cheb_step_u and the one-launch chains,
(c) wg_spmm and its transpose, (d) whole chains through wg_wavelet_features, (e) H wherever it is returned.  Every
case names its kernel in describe() and prints each c beside its bound.  All vectors of the per-step entry points
are in the handle's internal order: L.permute carries them there and back, truth stays in the caller's order.
"""
import ctypes
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cheb_ref as C
import test_handle_reuse as R

pytestmark = pytest.mark.gpu

import wats_hip  # noqa: E402
from wats_hip._lib import check, ptr  # noqa: E402

UIN, UPREV, UOUT, FINAL, ACTIVE = 1, 2, 4, 8, 16
CK, CACC, SCALE = 0.3, 2.0, 0.8
KINDS = ("normal", "positive")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def _lib():
    return wats_hip._lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _in(L, x):
    """caller order (numpy) -> internal order (device)"""
    return None if x is None else L.permute(_dev(x), to_internal=True)


def _out(L, t):
    torch.cuda.synchronize()
    return L.permute(t, to_internal=False).cpu().numpy()


def _graph(gname):
    return {"g0": R.graph_g0, "valued": R.graph_valued, "hybrid": R.graph_hybrid}[gname]()


class Record:
    """every measurement printed beside its bound; the assertion after the last one, so a failing case shows all"""

    def __init__(self):
        self.bad = []

    def add(self, what, c, bound, extra=""):
        print(f"{what}: c={c:.3f} bound={bound:.3f}{' ' + extra if extra else ''}")
        if not c <= bound:
            self.bad.append(f"{what}: c {c:.3f} > bound {bound:.3f}")

    def h(self, what, H, S):
        e = C.h_error(H, S)
        print(f"{what}: H err={e:.3f} x 2^-24 |H| bound={C.H_BOUND / C.EPS:.1f}")
        if not e * C.EPS <= C.H_BOUND:
            self.bad.append(f"{what}: H is {e:.3f} x 2^-24 |H| from S / (|S|_1 + 1e-8), bound {C.H_BOUND / C.EPS:.1f}")

    def check(self):
        assert not self.bad, "\n".join(self.bad)


def _names(desc, names, absent=()):
    for nm in names:
        assert nm in desc, f"'{nm}' not in\n{desc}"
    for nm in absent:
        assert nm not in desc, f"'{nm}' in\n{desc}"
    R.pending_zero(desc)


# ------------------------------------------------------------------------------- references, once per module
_STEP, _CHAIN = {}, {}


def step_inputs(gname, F, kind):
    key = (gname, F, kind)
    if key not in _STEP:
        n = _graph(gname).shape[0]
        _STEP[key] = dict(inputs=tuple(C.signal(n, F, kind, 100 * F + i) for i in range(3)), truth={})
    return _STEP[key]


def step_truth(gname, F, kind, b2_null=False):
    """(b1, b2, x0), (y, unit) and the hybrid bound's model (iv), computed once"""
    case = step_inputs(gname, F, kind)
    b1, b2, x0 = case["inputs"]
    if b2_null:
        b2 = None
    if b2_null not in case["truth"]:
        A = _graph(gname)
        y, unit = C.truth_step(A, b1, b2, x0, CK, CACC)
        case["truth"][b2_null] = (y, unit, C.hybrid_step_bound(A, b1, b2, x0, CK, CACC, truth=(y, unit)))
    return (b1, b2, x0), case["truth"][b2_null]


def chain_truth(gname, F, kind, K):
    key = (gname, F, kind, K)
    if key not in _CHAIN:
        A = _graph(gname)
        X = C.signal(A.shape[0], F, kind, 1000 * F + K)
        tr = C.truth_chain(A, X, K, SCALE)
        _CHAIN[key] = (X, tr, C.chain_bound(A, X, K, SCALE, truth=tr))
    return _CHAIN[key]


# ------------------------------------------------------------------------------- (a) one step, wg_clenshaw_step
def clenshaw_step(L, A, b1, b2, x0, flags):
    """out = ck x0 + cacc (L_hat b1) - b2 through the C ABI, in and out in the caller's order as float64: with UIN /
    UPREV b1 / b2 go in as fl32(b dinv), with UOUT the result comes back as u and is divided by dinv here"""
    dinv = C.operator(A).dinv
    if flags & UIN:
        b1 = C.f32(C.f64(b1) * dinv)
    if flags & UPREV and b2 is not None:
        b2 = C.f32(C.f64(b2) * dinv)
    F = b1.shape[1]
    out = R.nan_like(A.shape[0], F)
    t1, t2, t0 = _in(L, b1), _in(L, b2), _in(L, x0)   # named: a temporary's memory would be reused by the next one
    check(_lib().wg_clenshaw_step(L.handle, F, ptr(t1), ptr(t2), ptr(t0), ptr(out), CK, CACC, flags, _stream()),
          "clenshaw_step")
    got = C.f64(_out(L, out))
    return got / dinv if flags & UOUT else got


def closed_form_rows(A):
    """the purely isolated rows (no entry in the row or the column, the diagonal aside): wg_wavelet_features keeps
    them out of the step kernel, and so does a step with WG_CLEN_ACTIVE"""
    P = sp.csr_matrix(A).copy()
    P.setdiag(0)
    P.eliminate_zeros()
    return (np.diff(P.indptr) == 0) & (np.diff(P.tocsc().indptr) == 0)


def run_steps(rec, L, gname, F, tag, flag_sets, hybrid=False):
    """both signals x the flag sets, and b2 = NULL once; every value-free step on all rows and once more on the
    chain's rows (WG_CLEN_ACTIVE); returns the number of value-free launches"""
    A = _graph(gname)
    closed = closed_form_rows(A)
    launches = 0
    for kind in KINDS:
        for flags, b2_null in [(f, False) for f in flag_sets] + [(flag_sets[-1], True)]:
            if b2_null and kind != "normal":
                continue
            (b1, b2, x0), (y, unit, (hb, c4)) = step_truth(gname, F, kind, b2_null)
            got = clenshaw_step(L, A, b1, b2, x0, flags)
            what = f"{tag} F={F} {kind} flags={flags}{' b2=NULL' if b2_null else ''}"
            if not flags & UIN:
                rec.add(what + " (valued)", C.c_of(got, y, unit, what), C.BOUND_VALUED)
                continue
            bound, extra = (hb, f"(model (iv) {c4:.2f})") if hybrid else (C.BOUND_VALUE_FREE, "")
            rec.add(what, C.c_of(got, y, unit, what), bound, extra)
            # the same step on the rows of wg_wavelet_features' chain (its plan is the one describe() shows): the
            # purely isolated rows are not written and keep the NaN, every other row is held to the same bound
            act = clenshaw_step(L, A, b1, b2, x0, flags | ACTIVE)
            assert np.isnan(act[closed]).all() and np.isfinite(act[~closed]).all(), f"{what}: rows WG_CLEN_ACTIVE wrote"
            rec.add(what + " active rows", C.c_of(act[~closed], y[~closed], unit[~closed], what), bound, extra)
            launches += 2
    return launches


UFLAGS = [0, FINAL, UIN | UPREV | UOUT, FINAL | UIN | UPREV]   # the last one also runs with b2 = NULL


@pytest.mark.parametrize("F", [4, 40, 64])
@pytest.mark.parametrize("spec", [1, 0])
def test_step_team_kernel(spec, F):
    """the independent-wave kernel, straight-line (team_spec 1) and generic: 1, 10 and 16 lanes per row, both hubs
    as part waves at F = 40 / 64; flags 0 and FINAL alone read the CSR values on the workgroup kernel"""
    L = R.make_handle(R.graph_g0(), dict(team_spec=spec))
    rec = Record()
    run_steps(rec, L, "g0", F, f"team spec={spec}", UFLAGS)
    _names(L.describe(F), ["team:", f"spec={spec}"])
    L.close()
    rec.check()


def test_step_vec2_width():
    """F = 6: a width the chain pads to 8; one step at 6 columns runs the 8-byte form of the workgroup kernel"""
    L = R.make_handle(R.graph_g0())
    rec = Record()
    run_steps(rec, L, "g0", 6, "F=6", UFLAGS)
    _names(L.describe(6), ["VEC=2"], absent=["team:"])
    L.close()
    rec.check()


def test_step_workgroup_kernel_split_rows():
    """team = 0: the workgroup kernel, the hubs split over chunks with in-kernel arrival counters"""
    L = R.make_handle(R.graph_g0(), dict(team=0, block_iter=16, chunk_iter=8))
    rec = Record()
    run_steps(rec, L, "g0", 40, "wg split rows", UFLAGS)
    _names(L.describe(40), ["split rows"], absent=["team:"])
    L.close()
    rec.check()


def test_step_valued_path():
    """a weighted directed graph (self loops, isolated rows): CSR values gathered; the value-free flags are refused"""
    A = R.graph_valued()
    L = R.make_handle(A)
    rec = Record()
    run_steps(rec, L, "valued", 12, "valued", [0, FINAL])
    _names(L.describe(12), ["team rows"], absent=["team:", "tiles:"])
    x = R.nan_like(A.shape[0], 12)
    assert _lib().wg_clenshaw_step(L.handle, 12, ptr(x), ptr(x), ptr(x), ptr(x), CK, CACC, UIN, _stream()) == -1
    L.close()
    rec.check()


HYBRID = [
    (dict(tile_th=1, tile_rows=64, hyb_conc=0), [16, 48, 64]),
    (dict(tile_th=1, tile_rows=128, hyb_conc=2), [16, 48, 64]),
    (dict(tile_th=16, tile_rows=64, hyb_conc=2), [16, 48, 64]),
    (dict(tile_th=16, tile_rows=128, hyb_conc=0), [16, 48, 64]),
    (dict(tile_th=1, tile_rows=128, hyb_conc=0, tile_mfma=32), [64]),
    (dict(tile_th=16, tile_rows=128, hyb_conc=2, tile_mfma=32), [64]),
]


@pytest.mark.parametrize("knobs,widths", HYBRID, ids=["-".join(f"{k[5:] if k.startswith('tile_') else k}{v}"
                                                              for k, v in kn.items()) for kn, _ in HYBRID])
def test_step_hybrid(knobs, widths):
    """dense blocks on the matrix cores (three bf16 pieces of u, float32 MFMA sums joined in float64) plus the
    gathered tail: every touched block dense (tile_th 1) and the default-like 16, 64- and 128-row blocks, the tail
    after the blocks (hyb_conc 0) and beside them (2), the 32x32x16 MFMA shape at width 64"""
    L = R.make_handle(R.graph_hybrid(), dict(tiles=1, **knobs))
    rec = Record()
    for F in widths:
        before = sum(_forms(L, F).values()) if "tiles:" in L.describe(F) else 0
        n = run_steps(rec, L, "hybrid", F, f"hybrid {knobs}", [UIN | UPREV | UOUT, FINAL | UIN | UPREV], hybrid=True)
        _names(L.describe(F), ["tiles:"])
        forms = _forms(L, F)
        assert sum(forms.values()) - before == n, f"{n} value-free steps, hybrid forms {forms} (before: {before})"
        if knobs["hyb_conc"] == 0:
            assert forms["fused"] == 0 and forms["two_stream"] == 0, forms
    L.close()
    rec.check()


def _forms(L, F):
    """launches per form of the hybrid step, summed over the handle's tile plans (all rows, the chain's rows)"""
    lines = [x for x in L.describe(F).splitlines() if x.startswith("hybrid forms:")]
    assert lines, L.describe(F)
    total = {}
    for line in lines:
        for k, v in (t.split("=") for t in line.split(":", 1)[1].split()):
            total[k] = total.get(k, 0) + int(v)
    return total


# ------------------------------------------------------------------------------- (b) F = 1
@pytest.mark.parametrize("gname", ["g0", "valued"])
def test_f1_cheb_step_fused(gname):
    """wg_cheb_step at F = 1 (the scalar form of the workgroup kernel on the CSR values), k = 1 and k = 2, with the
    heat sum and the normalisation fused: T_k, S and H of one launch"""
    A = _graph(gname)
    L = R.make_handle(A)
    n = A.shape[0]
    rec = Record()
    for kind in KINDS:
        b1, b2, s_old = step_inputs(gname, 1, kind)["inputs"]
        for k, ak in ((1, math.exp(-SCALE)), (2, math.exp(-2 * SCALE))):
            t_k, S, H = R.nan_like(n, 1), (R.nan_like(n, 1) if k == 1 else _in(L, s_old)), R.nan_like(n, 1)
            L.step(k, _in(L, b1), None if k == 1 else _in(L, b2), t_k, S=S, H=H, alpha0=1.0, alpha_k=ak)
            what = f"wg_cheb_step {gname} F=1 k={k} {kind}"
            y, unit = C.truth_step(A, b1, None, None, 0.0, 1.0) if k == 1 else C.truth_step(A, b1, b2, None, 0.0, 2.0)
            rec.add(what + " T_k", C.c_of(_out(L, t_k), y, unit, what), C.BOUND_VALUED)
            ys, us = C.truth_step(A, b1, None, b1, 1.0, ak) if k == 1 else \
                C.truth_step(A, b1, ak * C.f64(b2), s_old, 1.0, 2.0 * ak)
            Sg = _out(L, S)
            rec.add(what + " S", C.c_of(Sg, ys, us, what), C.BOUND_VALUED)
            rec.h(what, _out(L, H), Sg)
    _names(L.describe(1), ["VEC=1"])
    L.close()
    rec.check()


@pytest.mark.parametrize("lds,names", [(1, ["lds1:"]), (2, ["lds1:", "windows"]), (4, ["lds1:", "hub teams"])],
                         ids=["lds1-teams", "lds2-windows", "lds4-hubs"])
def test_f1_cheb_step_u(lds, names):
    """wg_cheb_step_u: the LDS row teams, the chunk windows and the hub teams gather u_{k-1} = fl32(T_{k-1} dinv);
    k = 1 and k = 3 with T_k, u_k and S returned"""
    A = R.graph_g0()
    L = R.make_handle(A, dict(lds=lds, chain=0))
    n = A.shape[0]
    dinv = C.operator(A).dinv
    ulen = ctypes.c_int64(0)
    check(_lib().wg_cheb_u_len(L.handle, ctypes.byref(ulen)), "cheb_u_len")
    assert ulen.value >= n, f"the LDS kernel does not apply: u_len {ulen.value}"
    rec = Record()
    for kind in KINDS:
        b1, b2, s_old = step_inputs("g0", 1, kind)["inputs"]
        for k, ak in ((1, math.exp(-SCALE)), (3, math.exp(-3 * SCALE))):
            u_in = torch.zeros(ulen.value, 1, device="cuda")
            u_in[:n] = _in(L, C.f32(C.f64(b1) * dinv))
            t_k, u_k = R.nan_like(n, 1), R.nan_like(ulen.value, 1)
            S = R.nan_like(n, 1) if k == 1 else _in(L, s_old)
            t1, t2 = _in(L, b1), (None if k == 1 else _in(L, b2))
            check(_lib().wg_cheb_step_u(L.handle, k, ptr(u_in), ptr(t1), ptr(t2), ptr(t_k), ptr(u_k), ptr(S), 1.0, ak,
                                        _stream()), "cheb_step_u")
            what = f"wg_cheb_step_u lds={lds} k={k} {kind}"
            y, unit = C.truth_step(A, b1, None, None, 0.0, 1.0) if k == 1 else C.truth_step(A, b1, b2, None, 0.0, 2.0)
            rec.add(what + " T_k", C.c_of(_out(L, t_k), y, unit, what), C.BOUND_VALUE_FREE)
            rec.add(what + " u_k", C.c_of(C.f64(_out(L, u_k[:n].contiguous())) / dinv, y, unit, what), C.BOUND_VALUE_FREE)
            ys, us = C.truth_step(A, b1, None, b1, 1.0, ak) if k == 1 else \
                C.truth_step(A, b1, ak * C.f64(b2), s_old, 1.0, 2.0 * ak)
            rec.add(what + " S", C.c_of(_out(L, S), ys, us, what), C.BOUND_VALUE_FREE)
    _names(L.describe(1), names, absent=["chain1:"])
    L.close()
    rec.check()


F1_CHAINS = [({}, ["chain1:", "(solo:"]), (dict(chain_wg=4), ["chain1:", "4 workers"])]


@pytest.mark.parametrize("knobs,names", F1_CHAINS, ids=["chain-solo", "chain-wg4"])
def test_f1_one_launch_chain_single_product(knobs, names):
    """the one-launch chains at K = 1: S = X0 + exp(-s) L_hat X0 is one value-free product (K = 2, the product and
    its successor, is among the chains below)"""
    A = R.graph_g0()
    L = R.make_handle(A, knobs)
    rec = Record()
    for kind in KINDS:
        X = step_inputs("g0", 1, kind)["inputs"][0]
        S, H = R.checked_call(L, X, 1)
        assert not L.chain_status()
        y, unit = C.truth_step(A, X, None, X, 1.0, math.exp(-SCALE))
        what = f"one-launch chain {knobs} K=1 {kind}"
        rec.add(what, C.c_of(R._np(S), y, unit, what), C.BOUND_VALUE_FREE)
        rec.h(what, R._np(H), R._np(S))
    _names(L.describe(1), names)
    L.close()
    rec.check()


# ------------------------------------------------------------------------------- (c) wg_spmm
def _spmm_graph(name):
    if name == "g0+I":
        A = R.graph_g0()
        return (A + sp.identity(A.shape[0], dtype=np.float32, format="csr")).tocsr()
    return R.graph_valued()


@pytest.mark.parametrize("F", [7, 64])
@pytest.mark.parametrize("name", ["g0+I", "valued"])
def test_spmm_rownorm_and_transpose(name, F):
    """y = adj_norm x and adj_norm^T x (the WG_FLAG_TRANSPOSE handle): truth a_ij / deg_i as a float64 quotient, unit
    2^-24 sum_j |a_ij / deg_i| |x_j|; F = 7 runs the scalar form, 64 the 16-byte one.

    deg_i is the reference's float32 degree (model.py:43, correctly rounded): the stored float32 value is then one
    rounding from the truth and c <= 2 holds (measured 1.10 .. 1.71).  Against the quotient by the FLOAT64 row sum
    the documented arithmetic has a third rounding, the degree's own: cheb_ref.model_spmm gives 2.04 (normal) and
    2.20 (positive) on the weighted graph at F = 64, forward, and the kernel gives the same figures to every digit
    printed; on the unweighted graph the degree is an integer and both truths coincide.  That second figure is
    printed and held to 3 units (degree, quotient, result)."""
    A = _spmm_graph(name)
    op = wats_hip.RowNormalizedAdjacency.from_scipy(A)
    rec = Record()
    for transpose, side in ((False, op.fwd), (True, op.bwd)):
        M, M64 = C.rownorm(A, transpose), C.rownorm(A, transpose, float32_degree=False)
        for kind in KINDS:
            x = C.signal(A.shape[0], F, kind, 7 * F + transpose)
            y, unit = C.truth_step(M, x, None, None, 0.0, 1.0)
            got = side.apply(_dev(x))
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            what = f"wg_spmm {name}{' transposed' if transpose else ''} F={F} {kind}"
            rec.add(what, C.c_of(got, y, unit, what), C.BOUND_VALUED)
            y64, unit64 = C.truth_step(M64, x, None, None, 0.0, 1.0)
            rec.add(what + " vs the float64 degree", C.c_of(got, y64, unit64, what), C.BOUND_VALUED + 1.0,
                    f"(model {C.c_of(C.model_spmm(A, x, transpose), y64, unit64):.3f})")
        desc = _lib().wg_laplacian_describe(side.h, F).decode()
        assert f"VEC={4 if F % 4 == 0 else 1}" in desc and ("team rows" in desc or "block rows" in desc), desc
    rec.check()


# ------------------------------------------------------------------------------- (d) whole chains
CHAINS = [
    ("g0", dict(team_spec=1), [4, 40, 64], ["team:", "spec=1"], []),
    ("g0", dict(team_spec=0), [4, 40, 64], ["team:", "spec=0"], []),
    ("g0", {}, [6], ["team:"], []),
    ("g0", dict(team=0, block_iter=16, chunk_iter=8), [40], ["split rows"], ["team:"]),
    ("g0", dict(clenshaw=0), [40], ["block rows"], ["team:"]),
    ("valued", {}, [12, 1], ["team rows"], ["team:", "tiles:", "lds1:", "chain1:"]),
    ("g0", dict(lds=1, chain=0), [1], ["lds1:"], ["chain1:"]),
    ("g0", dict(lds=2, chain=0), [1], ["lds1:", "windows"], ["chain1:"]),
    ("g0", dict(lds=4, chain=0), [1], ["lds1:", "hub teams"], ["chain1:"]),
    ("g0", {}, [1], ["chain1:", "(solo:"], []),
    ("g0", dict(chain_wg=4), [1], ["chain1:", "4 workers"], []),
] + [("hybrid", dict(tiles=1, **kn), w, ["tiles:"], []) for kn, w in HYBRID]
CHAIN_IDS = ["team-spec1", "team-spec0", "F6-padded", "wg-split-rows", "forward-recurrence", "valued", "lds1-teams",
             "lds2-windows", "lds4-hubs", "chain-solo", "chain-wg4"] + \
            ["hybrid-" + "-".join(f"{k[5:] if k.startswith('tile_') else k}{v}" for k, v in kn.items()) for kn, _ in HYBRID]


@pytest.mark.parametrize("gname,knobs,widths,names,absent", CHAINS, ids=CHAIN_IDS)
def test_chain(gname, knobs, widths, names, absent):
    """wg_wavelet_features, K = 3 and 16 (and 2 at F = 1: a product and its successor), s = 0.8, for every family
    above: S in chain units against twice the documented models' own c, H against the S returned"""
    A = _graph(gname)
    L = R.make_handle(A, knobs)
    rec = Record()
    for F in widths:
        for K in ([2] if F == 1 else []) + [3, 16]:
            for kind in KINDS:
                X, tr, (bound, cs) = chain_truth(gname, F, kind, K)
                S, H = R.checked_call(L, X, K)
                assert not L.chain_status()
                what = f"chain {gname} {knobs} F={F} K={K} {kind}"
                rec.add(what, C.c_of(R._np(S), tr["S"], tr["unit"], what), bound,
                        "(models " + " ".join(f"{k} {v:.2f}" for k, v in cs.items()) + ")")
                rec.h(what, R._np(H), R._np(S))
        _names(L.describe(R.padded_width(F)), names, absent)
    L.close()
    rec.check()
