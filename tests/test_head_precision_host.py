"""CPU tests of tests/head_ref.py, the yardstick of tests/test_head_precision.py (no GPU, no library).

  * the float32 model of csrc/head.hip (correctly rounded exp and log) stays inside every bound, c <= 1, on every input
    of the GPU test: the bounds are met by the documented arithmetic before a kernel is asked to meet them;
  * each wrong kernel (one property of the model replaced) leaves its bound on at least one of those inputs;
  * conftest.assert_parity at the tolerances of test_fused_head_forward_backward_vs_torch passes two of them: parameter
    gradients accumulated in float32 across the rows, and a wrong gradient for a nearly dead hidden unit.  That is the
    gap the per-element units close.
Every measurement is printed beside its bound (pytest -s).
"""
import numpy as np
import pytest

import head_ref as R
from conftest import assert_parity

CASES = R.cases()


def run_model(I, fwd=None, bwd=None, g=None):
    """(out, grads, c of out, {c of the gradients}) of the float32 model with the given mutant switches; the backward
    takes the (mutant) forward's own out as lp, as the kernel's does"""
    out = R.model_forward(I["logits"], I["t"], **(fwd or {}))
    c_out = R.rejected(lambda: R.forward_c(I["logits"], I["t"], out))
    lp = out if np.isfinite(out).all() else R.model_forward(I["logits"], I["t"])
    grads = R.model_backward(I, I["t"], I["pre"], lp, g=g, **(bwd or {}))
    return out, lp, grads, c_out


def grads_rejected(I, lp, grads, g=None, names=R.GRADS):
    truth = R.backward_truth(I, I["t"], I["pre"], lp, g)
    return {k: R.rejected(lambda k=k: R.backward_c(I, I["t"], I["pre"], lp, grads, names=(k,), truth=truth))
            for k in names}


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_model_stays_inside_every_bound(case):
    I = R.case_inputs(case)
    t = I["t"]
    if case[0] >= 4095 and case[2] > 1:
        assert t.min() < -90 and t.max() > 70, (t.min(), t.max())      # the temperature extremes are reached
    out = R.model_forward(I["logits"], t)
    R.C.report(f"{R.case_id(case)} out", R.forward_c(I["logits"], t, out), R.BOUND)
    grads = R.model_backward(I, t, I["pre"], out)
    truth = R.backward_truth(I, t, I["pre"], out)
    for k, c in R.backward_c(I, t, I["pre"], out, grads, truth=truth).items():
        R.C.report(f"{R.case_id(case)} {k}", c, R.BOUND)
    if I["dead"] is not None:       # a dead unit's unit is 0: its gradients are exactly 0
        assert not truth["W1"][1][I["dead"]].any() and not grads["W1"][I["dead"]].any()
        assert grads["b1"][I["dead"]] == 0 and grads["W2"][I["dead"]] == 0
    if I["zero"] is not None:       # pre == 0 exactly on the units without a bias
        assert not I["pre"][I["zero"], :min(2, case[2])].any()


def some_case_rejects(what, cases, measure):
    """measure(I) -> (rejected, text); at least one of `cases` has to reject"""
    hits = []
    for case in cases:
        bad, text = measure(R.case_inputs(case))
        print(f"mutant {what}: {R.case_id(case)}: {text} bound={R.BOUND:.3f} -> {'REJECTED' if bad else 'passes'}")
        hits.append(bad)
    assert any(hits), f"no input rejects the mutant: {what}"


def worst(results):
    bad = any(b for b, _ in results.values())
    return bad, " ".join(f"{k}: {text}" for k, (_, text) in results.items())


def test_mutant_float32_accumulation_across_rows():
    def measure(I):
        _, lp, grads, _ = run_model(I, bwd=dict(acc32=True))
        return worst(grads_rejected(I, lp, grads, names=R.PARAMS))
    some_case_rejects("parameter gradients accumulated in float32", [(4097, 7, 16, 1, 1, "nll"),
                                                                     (4097, 65, 16, 7, 1, "nll"),
                                                                     (4097, 7, 64, 29, 1, "randn")], measure)


def test_mutant_maximum_over_the_first_64_columns():
    """rejected at scale 30 and C > 64; at scale 1 the same wrong kernel stays inside the bound (printed): its exps
    then stay finite and the maximum cancels"""
    def measure(I):
        return run_model(I, fwd=dict(first64=True))[3]
    some_case_rejects("maximum over the first 64 columns", [(5, 65, 16, 7, 30, "randn"), (4097, 129, 16, 1, 30, "randn"),
                                                           (4097, 260, 16, 1, 30, "randn")], measure)
    for Cw in (65, 129, 260):
        bad, text = measure(R.case_inputs((4097, Cw, 16, 1, 1, "randn")))
        print(f"  the same at scale 1, C = {Cw}: {text} ({'rejected' if bad else 'not rejected'})")


def test_mutant_last_partial_chunk_dropped():
    def measure(I):
        return run_model(I, fwd=dict(drop_tail=True))[3]
    some_case_rejects("last partial chunk of columns dropped", [(5, 65, 16, 7, 1, "randn"), (4097, 65, 16, 1, 1, "randn")],
                      measure)


def test_mutant_lanes_beyond_hid_contribute():
    """t_save is held to the model bit for bit: the mutant's t differs"""
    def measure(I):
        t, _ = R.model_t(I, extra_lanes=True)
        differ = int(np.count_nonzero(t.view(np.int32) != I["t"].view(np.int32)))
        return differ > 0, f"{differ} of {t.size} rows differ from the model's t"
    some_case_rejects("lanes >= hid contribute to t", [(5, 7, 15, 2, 1, "randn"), (5, 7, 1, 1, 1, "randn"),
                                                      (5, 7, 63, 5, 1, "randn")], measure)
    t, _ = R.model_t(R.case_inputs((5, 7, 64, 29, 1, "randn")), extra_lanes=True)      # hid = 64 has no such lane
    assert np.array_equal(t, R.case_inputs((5, 7, 64, 29, 1, "randn"))["t"])


def test_mutant_neighbours_temperature():
    def measure(I):
        return run_model(I, fwd=dict(neighbour_T=True))[3]
    some_case_rejects("a row uses its neighbour's T", [(2, 7, 16, 1, 1, "randn"), (5, 7, 16, 7, 1, "randn")], measure)


def one_row(I, r):
    g = np.zeros_like(I["g"])
    g[r] = I["g"][r]
    return g


def test_mutant_row_after_the_grid_wrap_skipped():
    case = (4097, 7, 16, 1, 1, "randn")

    def forward(I):
        return run_model(I, fwd=dict(skip_rows=(4096,)))[3]

    def backward(I):
        g = one_row(I, 4096)
        _, lp, grads, _ = run_model(I, bwd=dict(skip_rows=(4096,)), g=g)
        return worst(grads_rejected(I, lp, grads, g=g))
    some_case_rejects("row 4096 skipped, forward", [case], forward)
    some_case_rejects("row 4096 skipped, backward with grad_out in that row alone", [case], backward)
    I = R.case_inputs(case)
    _, lp, grads, _ = run_model(I, g=one_row(I, 4096))      # and the model itself holds the one row's unit
    for k, (bad, text) in grads_rejected(I, lp, grads, g=one_row(I, 4096)).items():
        print(f"model, grad_out in row 4096 alone: {k}: {text}")
        assert not bad


def test_mutant_relu_pattern_at_zero():
    def measure(I):
        _, lp, grads, _ = run_model(I, bwd=dict(ge=True))
        return worst(grads_rejected(I, lp, grads, names=R.PARAMS))
    some_case_rejects("[pre >= 0] for [pre > 0]", [(5, 7, 16, 7, 1, "randn"), (3, 7, 16, 1, 1, "randn"),
                                                   (4097, 65, 17, 3, 1, "randn")], measure)


def test_mutant_g_logits_without_the_temperature():
    def measure(I):
        _, lp, grads, _ = run_model(I, bwd=dict(no_inv_T=True))
        return worst(grads_rejected(I, lp, grads, names=("g_logits",)))
    some_case_rejects("1 / T left off g_logits", [(5, 7, 16, 7, 1, "randn"), (1, 7, 16, 1, 1, "randn")], measure)


def test_the_backward_constant():
    """dt with the double 1.1 that head.hip held against the forward's 1.1f: printed in units of dt's unit, which has
    no term for it any more"""
    I = R.case_inputs((4097, 7, 16, 1, 1, "randn"))
    out = R.model_forward(I["logits"], I["t"])
    truth = R.backward_truth(I, I["t"], I["pre"], out)
    for flag in (False, True):
        c = R.backward_c(I, I["t"], I["pre"], out, R.model_backward(I, I["t"], I["pre"], out, double_11=flag),
                         truth=truth, names=R.PARAMS)
        print(f"double 1.1 in the backward = {flag}: " + " ".join(f"{k}: c={v:.3f}" for k, v in c.items()))
        assert flag or max(c.values()) <= R.BOUND


def parity_as_the_old_tests(grads, truth):
    for k in R.GRADS:
        assert_parity(grads[k].reshape(-1, 1), truth[k][0].reshape(-1, 1), tol=2e-5, what=f"d{k}")


def test_assert_parity_passes_two_wrong_kernels():
    """the gap: one maximum per gradient, at 2e-5 of its largest entry"""
    case = (4097, 7, 16, 1, 1, "nll")
    I = R.case_inputs(case)
    _, lp, grads, _ = run_model(I, bwd=dict(acc32=True))
    truth = R.backward_truth(I, I["t"], I["pre"], lp)
    parity_as_the_old_tests(grads, truth)
    res = grads_rejected(I, lp, grads, names=R.PARAMS)
    print("float32 accumulation: assert_parity passes; " + worst(res)[1])
    assert worst(res)[0]

    case = (4097, 7, 16, 7, 1, "randn")
    I = R.case_inputs(case)
    near = I["near"]
    assert 0 < np.count_nonzero(I["pre"][:, near] > 0) < 0.05 * case[0]
    _, lp, grads, _ = run_model(I)
    truth = R.backward_truth(I, I["t"], I["pre"], lp)
    for k in ("W1", "b1", "W2"):        # the nearly dead unit's gradient doubled
        grads[k] = grads[k].copy()
        grads[k][near] *= 2
    parity_as_the_old_tests(grads, truth)
    res = grads_rejected(I, lp, grads, names=("W1", "b1", "W2"))
    print("nearly dead unit's gradient doubled: assert_parity passes; " + worst(res)[1])
    assert all(bad for bad, _ in res.values())
