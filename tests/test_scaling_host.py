"""CPU tests of the node-wise calibrators' yardstick (tests/scaling_ref.py) against the fixtures generated from the
reference's own TS / VS / MS / ETS classes (tools/gen_golden_scaling.py, tests/golden/scaling): the float64
restatement reproduces them within the manifest's f32_vs_f64 and stops where the reference stopped; its analytic
gradients agree with float64 dense autograd; its Adam agrees with torch.optim.Adam; every mutant falls outside."""
import hashlib
import os

import numpy as np
import pytest
import torch

import scaling_ref as R
from conftest import GOLDEN

TIGHT = 1e-12


def dist(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


@pytest.fixture(scope="module", params=R.CASES)
def case(request):
    d, meta, files = R.load_case(request.param)
    z = R.base_logits(R.case_base(d), d["x"], d["adj"])
    return request.param, d, meta, z


@pytest.fixture(scope="module")
def runs(case):
    """the restatement's training runs, once per case"""
    _, d, _, z = case
    return {c: R.train(c, z, d["y"], R.case_rows(d)) for c in ("ts", "vs", "ms")}


def restated_params(c, d, z, runs):
    if c != "ets":
        return runs[c]["params"]
    rows = R.case_rows(d)
    tau = runs["ts"]["params"][0]
    w = R.ets_fit(*R.ets_label_probs(z[rows], d["y"][rows], tau), z.shape[1])
    return [tau] + [np.asarray(v) for v in w]


def test_fixture_files_match_the_manifest(case):
    name, d, _, _ = case
    _, _, files = R.load_case(name)
    with open(os.path.join(GOLDEN, "scaling", name + ".npz"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == files["sha256"]
    assert sorted(d.keys()) == files["keys"]
    assert not any(v.dtype == object for v in d.values())


@pytest.mark.parametrize("c", R.CALIBRATORS)
def test_restatement_reproduces_the_reference(case, runs, c):
    name, d, meta, z = case
    f = meta["f32_vs_f64"]
    r = runs["ts" if c == "ets" else c]
    assert r["epochs_run"] == int(d[f"epochs_{c}"])
    assert (r["stop_epoch"] if r["stop_epoch"] is not None else -1) == int(d[f"stop_{c}"])
    slack = 1e-9     # the float64 restatement itself moves by a few 2^-53 between BLAS builds
    assert dist(r["loss"], d[f"loss_{c}"]) <= f[f"loss_{c}"] + slack
    params = restated_params(c, d, z, runs)
    assert max(dist(a, b) for a, b in zip(params, R.case_params(d, c))) <= f[f"params_{c}"] + slack
    assert dist(R.forward(c, z, params), d[f"out_{c}"]) <= f[f"out_{c}"] + slack
    grad = R.adjacency_gradient(c, R.case_base(d), params, d["x"], d["adj"], d["loss_weight"], d["grad_rows"],
                                d["grad_cols"])
    assert dist(grad, d[f"grad_{c}"]) <= f[f"grad_{c}"] + slack
    if c == "ets":
        assert dist(params[1:], d["w_ets"]) <= f["w_ets"] + slack


def test_every_stopping_comparison_is_far_from_a_tie(case, runs):
    """the condition on the fixtures: rounding cannot move a stopping epoch"""
    _, d, meta, _ = case
    for c in ("ts", "vs", "ms"):
        for losses in (d[f"loss_{c}"], runs[c]["loss"]):
            best, gaps = np.inf, []
            for v in losses:
                if np.isfinite(best):
                    gaps.append(abs(v - best))
                best = min(best, v)
            assert min(gaps) > 100 * meta["f32_vs_f64"][f"loss_{c}"]


@pytest.mark.parametrize("mode,normalize", [("ts", False), ("vs", False), ("ms", False), ("ms", True), ("ets", False)])
def test_analytic_gradients_agree_with_float64_autograd(mode, normalize):
    rng = np.random.default_rng(7)
    n, C = 37, 6
    z = rng.standard_normal((n, C)) * 3
    g = rng.standard_normal((n, C))
    params = {"ts": [np.array([0.7])], "vs": [rng.standard_normal(C)],
              "ms": [rng.standard_normal((C, C)), rng.standard_normal(C)],
              "ets": [np.array([0.4]), np.array([0.6]), np.array([0.3]), np.array([0.1])]}[mode]
    gz, gp, (gz_abs, gp_abs) = R.backward(mode, z, params, g, normalize)
    zt = torch.tensor(z, requires_grad=True)
    pt = [torch.tensor(np.asarray(q, np.float64), requires_grad=True) for q in params]
    out = R.torch_forward(mode, zt, pt, normalize)
    assert dist(out.detach().numpy(), R.forward(mode, z, params, normalize)) <= TIGHT * np.abs(z).sum(axis=1).max() * 10
    (out * torch.tensor(g)).sum().backward()
    assert np.all(np.abs(gz - zt.grad.numpy()) <= TIGHT * gz_abs + 1e-300)
    for a, t, ab in zip(gp, pt, gp_abs):
        assert np.all(np.abs(a.reshape(t.shape) - t.grad.numpy()) <= TIGHT * ab.reshape(t.shape) + 1e-300)


def test_epoch_matches_autograd_of_the_reference_loss():
    """the epoch's loss and gradients (L1 term, 1 / n) against autograd of MS.py:68-69 restated in float64"""
    rng = np.random.default_rng(3)
    n, C = 29, 5
    z, y = rng.standard_normal((n, C)) * 2, rng.integers(0, C, n)
    W, b = np.ones((C, C)) + 0.1 * rng.standard_normal((C, C)), rng.standard_normal(C)
    W[1, 1] = 1.0                        # sign(0) = 0
    q = R.epoch("ms", z, y, [W, b])
    Wt, bt = torch.tensor(W, requires_grad=True), torch.tensor(b, requires_grad=True)
    out = R.torch_forward("ms", torch.tensor(z), [Wt, bt])
    loss = torch.nn.functional.nll_loss(out, torch.tensor(y)) + 1 * torch.sum(torch.abs(Wt - torch.eye(C)))
    loss.backward()
    assert abs(q["loss"] - float(loss)) <= TIGHT * q["loss_abs"]
    assert np.all(np.abs(q["grads"][0] - Wt.grad.numpy()) <= TIGHT * q["grads_abs"][0])
    assert np.all(np.abs(q["grads"][1] - bt.grad.numpy()) <= TIGHT * q["grads_abs"][1])
    assert q["correct"] == int((out.argmax(dim=1).numpy() == y).sum())


def test_adam_restatement_agrees_with_torch():
    rng = np.random.default_rng(5)
    theta = torch.tensor(rng.standard_normal(12), requires_grad=True)
    opt = torch.optim.Adam([theta], lr=R.LR, weight_decay=R.WD)
    t, m, v = theta.detach().numpy().copy(), np.zeros(12), np.zeros(12)
    for step in range(1, 251):
        g = rng.standard_normal(12) * 10.0 ** rng.integers(-4, 2)
        theta.grad = torch.tensor(g)
        opt.step()
        t, m, v = R.adam_step(t, g, m, v, step)
        assert dist(t, theta.detach().numpy()) <= TIGHT * max(1.0, np.abs(t).max())


# ------------------------------------------------------------------------------------------------------ mutants
def trained_out(c, d, z, mutant):
    r = R.train(c, z, d["y"], R.case_rows(d), mutant=mutant)
    return r, R.forward(c, z, r["params"], mutant=mutant if mutant in ("ts_divide", "ms_no_shift") else None)


def test_mutant_ts_divide(case):
    _, d, meta, z = case
    _, out = trained_out("ts", d, z, "ts_divide")
    assert dist(out, d["out_ts"]) > 100 * meta["f32_vs_f64"]["out_ts"]


def test_mutant_ms_identity_init_and_no_shift(case):
    _, d, meta, z = case
    for mutant in ("ms_identity_init", "ms_no_shift"):
        r, out = trained_out("ms", d, z, mutant)
        n = min(len(r["loss"]), len(d["loss_ms"]))
        assert dist(r["loss"][:n], d["loss_ms"][:n]) > 100 * meta["f32_vs_f64"]["loss_ms"], mutant
        assert dist(out, d["out_ms"]) > 100 * meta["f32_vs_f64"]["out_ms"], mutant


def test_mutant_decoupled_weight_decay(case):
    _, d, meta, z = case
    for c in ("ts", "vs", "ms"):
        r, _ = trained_out(c, d, z, "decoupled_wd")
        assert max(dist(a, b) for a, b in zip(r["params"], R.case_params(d, c))) > 10 * meta["f32_vs_f64"][f"params_{c}"]


def test_mutant_sign_of_zero(case):
    _, d, meta, z = case
    r, _ = trained_out("ms", d, z, "sign0_is_1")
    n = min(len(r["loss"]), len(d["loss_ms"]))
    assert dist(r["loss"][:n], d["loss_ms"][:n]) > 100 * meta["f32_vs_f64"]["loss_ms"]


def test_mutant_ets_conventions(runs):
    """both temperature conventions, on the case whose weights are not at the start (1, 0, 0)"""
    d, meta, _ = R.load_case("wide96")
    z = R.base_logits(R.case_base(d), d["x"], d["adj"])
    rows, f = R.case_rows(d), meta["f32_vs_f64"]
    tau = R.case_params(d, "ets")[0]
    w = R.ets_fit(*R.ets_label_probs(z[rows], d["y"][rows], tau, mutant="ets_fit_softplus"), z.shape[1])
    assert f["w_ets"] > 0 and dist(w, d["w_ets"]) > 4 * f["w_ets"]
    out = R.forward("ets", z, R.case_params(d, "ets"), mutant="ets_forward_multiply")
    assert dist(out, d["out_ets"]) > 100 * f["out_ets"]


def test_mutant_float32_loss_accumulator():
    """outside the kernels' bound on the loss: 1e-12 of the sum of the absolute terms"""
    rng = np.random.default_rng(11)
    n, C = 4097, 7
    z, y = rng.standard_normal((n, C)) * 3, rng.integers(0, C, n)
    good = R.epoch("ts", z, y, [np.ones(1)])
    bad = R.epoch("ts", z, y, [np.ones(1)], mutant="f32_loss")
    assert abs(bad["loss"] - good["loss"]) > TIGHT * good["loss_abs"]


def test_one_rounding_bound_rejects_two_roundings():
    truth = np.array([[1.0 + 2.0 ** -24 + 2.0 ** -30]])
    assert R.one_rounding_ok(truth.astype(np.float32), truth, np.abs(truth)) <= 1.0
    with pytest.raises(AssertionError):
        R.one_rounding_ok(np.array([[1.0]], np.float32) - np.float32(2.0 ** -24), truth, np.abs(truth))
