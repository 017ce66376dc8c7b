"""The row-unit method of tests/test_step_precision.py, pinned without a GPU (tests/cheb_ref.py).

On G0 (test_handle_reuse.graph_g0: hubs of 1300 and 700 neighbours beside leaves) and on the 4000-node R-MAT graph
of test_tiles.py, at F = 8, with a normal signal and a positive one (|N(0,1)| + 0.5):
  * the arithmetic DESIGN.md documents (float64 sums rounded once; value-free on u = fl32(b dinv); the hybrid step's
    short float32 chains joined in float64; the three chain recurrences) stays within the bounds the GPU test uses;
  * a step that splits u into two bf16 pieces instead of three is at least 10 x above them, in one step and through
    a K = 16 chain, and a step that sums a row in float32 is above the single-step bound on the positive signal.
So the GPU test fails on a kernel that is wrong in either way, which the column-norm parity of conftest.assert_parity
(1e-5 of the column's maximum) lets through: the last test here shows both mutants passing it.
"""
import numpy as np
import pytest

import cheb_ref as C
import test_handle_reuse as R
from conftest import assert_parity

F = 8
CK, CACC = 0.3, 2.0
GRAPHS = {"g0": R.graph_g0, "rmat": R.graph_hybrid}
KINDS = ("normal", "positive")

_STEP, _CHAIN = {}, {}


def step_case(gname, kind):
    """inputs, truth and units of one step, once per (graph, signal)"""
    if (gname, kind) not in _STEP:
        A = GRAPHS[gname]()
        b1, b2, x0 = (C.signal(A.shape[0], F, kind, seed) for seed in (11, 12, 13))
        y, unit = C.truth_step(A, b1, b2, x0, CK, CACC)
        _STEP[(gname, kind)] = (A, (b1, b2, x0, CK, CACC), y, unit)
    return _STEP[(gname, kind)]


def chain_case(gname, kind, K):
    if (gname, kind, K) not in _CHAIN:
        A = GRAPHS[gname]()
        X = C.signal(A.shape[0], F, kind, 21)
        _CHAIN[(gname, kind, K)] = (A, X, C.truth_chain(A, X, K, 0.8))
    return _CHAIN[(gname, kind, K)]


def test_graphs_are_the_ones_the_figures_were_taken_on():
    A = R.graph_g0()
    assert A.shape[0] == 2064 and A.nnz == 12948 and sorted(np.diff(A.indptr))[-2:] == [700, 1300]
    B = R.graph_hybrid()
    assert B.shape[0] == 4000 and bool(np.all(B.data == 1.0)) and (B != B.T).nnz == 0


def test_bf16_pieces():
    """three pieces hold a float32 exactly, two lose at most 2^-16 of it (truncation, so never more than the value)"""
    u = np.concatenate([C.signal(4096, 1, "normal", 3).ravel() * s for s in (1.0, 1e-20, 1e20)] + [[0.0, 1.0, -1.5]])
    u = u.astype(np.float32)
    assert np.array_equal(C.bf16_pieces(u, 3), u.astype(np.float64))
    two = C.bf16_pieces(u, 2)
    assert np.all(np.abs(two - u) <= 2.0 ** -15 * np.abs(u)) and np.any(two != u)


def test_truth_is_the_oracle():
    """truth_chain restates nothing: S, H and every T_k are the oracle's, and a step of it is the recurrence"""
    from oracle import wats_oracle as O
    A, X, tr = chain_case("g0", "normal", 3)
    ref = O.graph_wavelet_features(A, k=3, s=0.8, X0=X, return_all=True)
    assert np.array_equal(tr["S"], ref["S"]) and np.array_equal(tr["H"], ref["H"])
    assert all(np.array_equal(a, b) for a, b in zip(tr["T"], ref["T"]))
    y, unit = C.truth_step(A, tr["T"][2], tr["T"][1], None, 0.0, 2.0)
    assert np.array_equal(y, tr["T"][3]) and np.all(unit >= 0)
    # an isolated row: L_hat_ii = -1, so its unit is |b1_i| cacc + |b2_i|, never 0 for a non-zero input
    iso = np.flatnonzero(np.diff(A.indptr) == 0)
    assert iso.size and np.all(unit[iso] > 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_documented_step_arithmetic_is_within_the_bounds(gname, kind):
    A, args, y, unit = step_case(gname, kind)
    tag = f"{gname} {kind}"
    C.report(f"{tag} valued model", C.c_of(C.model_step_valued(A, *args), y, unit), C.BOUND_VALUED)
    C.report(f"{tag} value-free model", C.c_of(C.model_step_u(A, *args), y, unit), C.BOUND_VALUE_FREE)
    C.report(f"{tag} value-free model, u out", C.c_of(C.model_step_u(A, *args, u_out=True), y, unit), C.BOUND_VALUE_FREE)
    bound, c4 = C.hybrid_step_bound(A, *args, truth=(y, unit))
    C.report(f"{tag} hybrid model", C.c_of(C.model_step_hybrid(A, *args), y, unit), bound, f"(model (iv) {c4:.2f})")
    # b2 = NULL and the heat sum's coefficients
    y0, unit0 = C.truth_step(A, args[0], None, args[2], 1.0, np.exp(-0.8))
    C.report(f"{tag} value-free model, b2 NULL", C.c_of(C.model_step_u(A, args[0], None, args[2], 1.0, np.exp(-0.8)),
                                                         y0, unit0), C.BOUND_VALUE_FREE)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_two_piece_split_is_rejected_in_one_step(gname, kind):
    A, args, y, unit = step_case(gname, kind)
    bound, c4 = C.hybrid_step_bound(A, *args, truth=(y, unit))
    c = C.c_of(C.mutant_step_two_pieces(A, *args), y, unit)
    print(f"{gname} {kind} two bf16 pieces: c={c:.1f} bound={bound:.2f} (model (iv) {c4:.2f})")
    assert c >= 10.0 * bound, f"{gname} {kind}: the two-piece split is at {c:.1f}, less than 10 x the bound {bound:.2f}"


@pytest.mark.parametrize("gname", list(GRAPHS))
def test_float32_row_sums_are_rejected_on_the_positive_signal(gname):
    A, args, y, unit = step_case(gname, "positive")
    c = C.c_of(C.mutant_step_f32_sums(A, *args), y, unit)
    c4 = C.c_of(C.model_step_f32(A, *args), y, unit)
    print(f"{gname} positive float32 row sums: value-free c={c:.1f}, plain float32 product (iv) c={c4:.1f}, "
          f"bound={C.BOUND_VALUE_FREE}")
    assert c > C.BOUND_VALUE_FREE and c4 > C.BOUND_VALUE_FREE


@pytest.mark.parametrize("K", [3, 16])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_chain_models_and_the_two_piece_split_through_a_chain(gname, kind, K):
    """the three documented recurrences give the chain bound, and the two-piece split through the same chain is
    above it.  (Not 10 x as in one step: the bound is twice the forward recurrence's c, about 11 at K = 16, where
    the heat sum's weights exp(-0.8 k) leave the split at 44 to 190 units; at K = 3 it is 18 x to 36 x.)"""
    A, X, tr = chain_case(gname, kind, K)
    bound, cs = C.chain_bound(A, X, K, 0.8, truth=tr)
    for name, c in cs.items():
        C.report(f"{gname} {kind} K={K} model {name}", c, bound)
    assert 0.5 <= max(cs.values()), cs   # a rounding of the final sum alone is half a unit somewhere
    c = C.c_of(C.model_clenshaw_u(A, X, K, 0.8, pieces=2), tr["S"], tr["unit"])
    print(f"{gname} {kind} K={K} two bf16 pieces through the chain: c={c:.1f} bound={bound:.2f}")
    factor = 10.0 if K == 3 else 1.0   # K = 16: rejected, which is what the GPU test needs
    assert c > factor * bound, f"{gname} {kind} K={K}: the two-piece chain is at {c:.1f}, bound {bound:.2f}"


@pytest.mark.parametrize("transpose", [False, True])
def test_spmm_model_and_the_degree_rounding(transpose):
    """wg_spmm's documented arithmetic (float32 degree, float32 quotient, float64 sums) is within 2 units of the
    float64 quotient by that float32 degree, and within 3 of the quotient by the float64 row sum: the degree's own
    rounding is a third unit (2.04 and 2.20 on this graph at F = 64, forward), which is why the GPU test's truth
    divides by the reference's float32 degree"""
    A = R.graph_valued()
    worst = 0.0
    for kind in KINDS:
        x = C.signal(A.shape[0], 64, kind, 7 * 64 + transpose)
        got = C.model_spmm(A, x, transpose)
        c32 = C.c_of(got, *C.truth_step(C.rownorm(A, transpose), x, None, None, 0.0, 1.0))
        c64 = C.c_of(got, *C.truth_step(C.rownorm(A, transpose, float32_degree=False), x, None, None, 0.0, 1.0))
        print(f"spmm model transposed={transpose} {kind}: c={c32:.3f} (float32 degree) {c64:.3f} (float64 row sum)")
        assert c32 <= C.BOUND_VALUED and c64 <= C.BOUND_VALUED + 1.0
        worst = max(worst, c64)
    if not transpose:
        assert worst > C.BOUND_VALUED   # the third rounding is real, not a margin


def test_column_norm_parity_lets_both_mutants_through():
    """why the row units exist: conftest.assert_parity (1e-5 of the column maximum) accepts the two-piece step and
    the float32 row sums on the R-MAT graph, positive signal"""
    A, args, y, unit = step_case("rmat", "positive")
    assert_parity(C.mutant_step_two_pieces(A, *args), y, what="two pieces")
    assert_parity(C.mutant_step_f32_sums(A, *args), y, what="float32 sums")
