"""CPU tests of the evaluation step's arithmetic: the numpy model of csrc/calib.hip (tests/calib_eval_ref.py) against
the reference's own fixtures (tests/golden/evaluation, tools/gen_golden_evaluation.py) and against
oracle/ece_oracle.py, the binning identity that lets one table serve np.digitize and sklearn's calibration_curve, the
fragility condition the GPU tests' seeds rely on, and the mutants the fixtures must catch.

Bounds.  A fixture quantity is held within that fixture's recorded f32_vs_f64 (the reference's own float32
arithmetic is that far from the float64 evaluation of the same float32 p) plus 2^-40 (the fixed point: at most
2^-41 per bin mean, weights summing to at most 1, plus float64 rounding).  Against ece_oracle on float64 copies the
bound is 2^-40 alone.
"""
import numpy as np
import pytest

import calib_eval_ref as R
from oracle import ece_oracle as O

FIX = 2.0 ** -40
CASES = R.load_fixture_cases()
unflatten = R.unflatten_curves


def fixture_failures(mutant=None):
    """The names of the fixtures whose triple or per-class ECE the model (with one mutation) misses."""
    bad = []
    for name, c in CASES.items():
        f = c["f32_vs_f64"]
        m10 = R.model_report(c["outputs"], c["labels"], c["rows"], c["kind"], 10, mutant=mutant)
        mb = R.model_report(c["outputs"], c["labels"], c["rows"], c["kind"], c["n_bins"], mutant=mutant)
        acc, conf, ece = c["triple"]
        ok = (abs(m10["acc"] - acc) <= f["acc"] + FIX and abs(m10["conf"] - conf) <= f["conf"] + FIX
              and abs(m10["ece"] - ece) <= f["ece"] + FIX
              and np.max(np.abs(mb["ece_class"] - c["per_class"])) <= f["per_class"] + FIX)
        if not ok:
            bad.append(name)
    return bad


def test_fixture_set_covers_the_cases_of_the_issue():
    assert 8 <= len(CASES) <= 12
    kinds = {c["kind"] for c in CASES.values()}
    assert kinds == {"probs", "exp"}
    assert {c["rows_form"] for c in CASES.values()} == {"mask", "index"}
    assert all(c["n"] <= 2000 and c["C"] <= 10 for c in CASES.values())
    assert any(np.max(np.exp(c["outputs"].astype(np.float64))) > 1 for c in CASES.values() if c["kind"] == "exp")
    c = CASES["absent_class_bad_labels_n400_c6"]
    assert 4 not in c["labels"] and -1 in c["labels"] and 6 in c["labels"]
    t = R.bin_table(CASES["bins_of_3_and_4_c3"]["outputs"], CASES["bins_of_3_and_4_c3"]["labels"])
    assert 3 in t[0, :10, 0] and 4 in t[0, :10, 0]
    p = CASES["exact_zero_one_c4"]["outputs"]
    assert (p == 0).any() and (p == 1).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_matches_reference_fixture(name):
    c = CASES[name]
    f = c["f32_vs_f64"]
    m = R.model_report(c["outputs"], c["labels"], c["rows"], c["kind"], 10)
    acc, conf, ece = c["triple"]
    print(name, "acc", abs(m["acc"] - acc), "conf", abs(m["conf"] - conf), "ece", abs(m["ece"] - ece), "allowed", f)
    assert m["n"] == c["n"]
    assert abs(m["acc"] - acc) <= f["acc"] + FIX
    assert abs(m["conf"] - conf) <= f["conf"] + FIX
    assert abs(m["ece"] - ece) <= f["ece"] + FIX
    mb = R.model_report(c["outputs"], c["labels"], c["rows"], c["kind"], c["n_bins"])
    assert np.max(np.abs(mb["ece_class"] - c["per_class"])) <= f["per_class"] + FIX
    if c["curves"]:
        got = R.curves_from_table(mb["table"], c["C"])
        for (t, q), (t_ref, q_ref) in zip(got, unflatten(c)):
            assert t.shape == t_ref.shape
            assert np.max(np.abs(t - t_ref), initial=0) <= f["curves"] + FIX
            assert np.max(np.abs(q - q_ref), initial=0) <= f["curves"] + FIX


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_matches_oracle_on_float64_copies(name):
    c = CASES[name]
    p = R.probabilities(c["outputs"], c["kind"])
    idx = R.row_list(c["rows"], len(p))
    p64, y = p[idx].astype(np.float64), c["labels"][idx]
    m = R.model_report(c["outputs"], c["labels"], c["rows"], c["kind"], c["n_bins"])
    want = np.array([O.calculate_ece(p64, y, k, logits=False, n_bins=c["n_bins"]) for k in range(c["C"])])
    assert np.max(np.abs(m["ece_class"] - want)) <= FIX


@pytest.mark.parametrize("n_bins", [1, 2, 3, 7, 10, 15, 20, 64])
def test_digitize_and_calibration_curve_rules_agree_on_every_edge_neighbour(n_bins):
    """np.digitize(p, edges, right=True) - 1 (utils/ece.py:40) and sklearn's searchsorted(edges[1:-1], p) give the
    same bin for every float32 p in (0, 1], checked one float32 ulp either side of every edge; they differ only at
    p == 0 (no bin against bin 0)."""
    edges = np.linspace(0, 1, n_bins + 1)
    e32 = edges.astype(np.float32)
    vals = np.unique(np.concatenate([e32, np.nextafter(e32, np.float32(2)), np.nextafter(e32, np.float32(-1)),
                                     np.float32([1e-45, 2.0 ** -17, 0.5, 1.0])]))
    vals = vals[(vals > 0) & (vals <= 1)].astype(np.float64)
    assert len(vals) >= 3 * n_bins - 1
    a = np.digitize(vals, edges, right=True) - 1
    b = np.searchsorted(edges[1:-1], vals)
    assert np.array_equal(a, b)
    assert np.digitize(0.0, edges, right=True) - 1 == -1 and np.searchsorted(edges[1:-1], 0.0) == 0
    # the model's slots are digitize's bins
    t = R.bin_table(vals.astype(np.float32)[:, None], np.zeros(len(vals), np.int64), n_bins=n_bins)
    assert np.array_equal(t[0, :n_bins, 0], np.bincount(a, minlength=n_bins).astype(np.uint64))


def test_fixed_point_is_exact_from_2_pow_minus_17_and_within_half_a_quantum_below():
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.random(4000).astype(np.float32), np.float32([2.0 ** -17, 1.0]),
                        np.nextafter(np.float32(2.0 ** -17), np.float32(1), dtype=np.float32)[None]])
    big = p[p >= np.float32(2.0 ** -17)].astype(np.float64)
    assert np.array_equal(np.rint(big * R.Q40) / R.Q40, big)
    small = (rng.random(4000) * 2.0 ** -17).astype(np.float32).astype(np.float64)
    assert np.max(np.abs(np.rint(small * R.Q40) / R.Q40 - small)) <= 2.0 ** -41
    assert (1 << 23) * R.Q40 < 2 ** 63 + 1      # 2^23 rows of p <= 1


@pytest.mark.parametrize("kind", ["exp", "logits"])
@pytest.mark.parametrize("seed", R.GPU_SEEDS)
def test_gpu_seeds_have_no_fragile_element(kind, seed):
    """An element is fragile when its longdouble p lies within 2^-50 (relative) of a float32 rounding midpoint or its
    rounded p is an edge: a float64 evaluation may then bin it elsewhere.  The GPU tests compare tables exactly, so the
    inputs they use (calib_eval_ref.gpu_logits) must have none: a cap of 0.  (One column under "logits" is p = s / s,
    1 in any arithmetic.)"""
    for C in R.GPU_WIDTHS:
        if kind == "logits" and C == 1:
            continue
        assert not R.fragile(R.gpu_logits(C, seed), kind, R.GPU_BINS).any()


def test_fragility_condition_sees_a_midpoint_and_an_edge():
    a, b = np.float32(0.3), np.nextafter(np.float32(0.3), np.float32(1))
    mid = (np.longdouble(a) + np.longdouble(b)) / 2
    x = np.log(mid).astype(np.float64)
    # exp of the float32 nearest to log(mid) is ~1e-8 away from the midpoint: not fragile; an exact edge is
    assert not R.fragile(np.float32([[x]]), "exp").any()
    assert R.fragile(np.float32([[0.0]]), "exp").all()          # exp(0) = 1 is an edge
    assert R.fragile(np.float32([[0.0, 0.0]]), "logits").all()  # softmax = 0.5 is an edge


def test_unmutated_model_passes_every_fixture():
    assert fixture_failures() == []


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_fails_a_fixture(mutant):
    bad = fixture_failures(mutant)
    print(mutant, "caught by", bad)
    assert bad, f"mutant {mutant} passes every fixture"


def test_scalar_truth_on_a_small_case():
    p = np.float32([[0.5, 0.25, 0.25], [0.0, 1.0, 0.0], [np.nan, 0.5, 0.5], [0.2, 0.3, 0.5]])
    y = np.array([0, 0, 1, 3])
    val, mag = R.scalar_truth(p, y, None, "probs")
    assert list(val[:3]) == [4, 3, 1]
    assert float(val[3]) == 0.5 + 1.0 + 0.5
    assert float(val[5]) == 1 and abs(float(val[4]) - np.log(2)) < 1e-15     # row 1: p_label == 0, row 3: no class
    assert abs(float(val[6]) - ((0.25 + 0.0625 + 0.0625) + 2.0 + (0.04 + 0.09 + 0.25))) < 1e-7
