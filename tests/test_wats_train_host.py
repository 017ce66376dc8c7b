"""CPU tests of WATS's training on the device: the float64 restatement (tests/wats_train_ref.py) against the fixtures of
the reference's own runs (tests/golden/wats_train) and against dense float64 torch autograd plus torch.optim.Adam, the
generator's seed conditions, the host argument checks of the C entry points, and the restatement's mutants."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import scaling_ref as SR
import wats_train_ref as R

TIGHT = 1e-12


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in R.CASES:
        d, meta = R.load_case(name)
        z64 = SR.base_logits(R.case_base(d), d["x"], d["adj"])
        out[name] = dict(d=d, meta=meta, z64=z64,
                         run=R.train(d["wavelet_feats"], z64, d["y"], R.case_rows(d), R.case_init(d)))
    return out


@pytest.mark.parametrize("case", R.CASES)
def test_fixture_files_match_the_manifest(case):
    man = R.load_manifest()
    path = os.path.join(R.GOLDEN, case + ".npz")
    assert os.path.getsize(path) < 200 * 1024
    with open(path, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == man["files"][case + ".npz"]["sha256"]
    d, _ = R.load_case(case)
    assert sorted(d) == man["files"][case + ".npz"]["keys"]
    assert man["gap_factor"] == 10.0 and man["generator"] == "tools/gen_golden_wats_train.py"


@pytest.mark.parametrize("case", R.CASES)
def test_restatement_reproduces_the_reference(case, runs):
    c = runs[case]
    d, f, r = c["d"], c["meta"]["f32_vs_f64"], c["run"]
    assert r["epochs_run"] == int(d["epochs"]) == len(d["loss"])
    assert (r["stop_epoch"] if r["stop_epoch"] is not None else -1) == int(d["stop"])
    assert R.dist(d["loss"], r["loss"]) <= f["loss"]
    assert max(R.dist(a, b) for a, b in zip(R.case_trained(d), r["params"])) <= f["params"]
    assert R.dist(d["out"], R.forward(d["wavelet_feats"], c["z64"], r["params"])) <= f["out"]


def test_the_two_cases_are_the_ones_the_generator_promises(runs):
    a, b = runs["stop120"], runs["full96"]
    assert int(a["d"]["stop"]) >= 0 and int(a["d"]["epochs"]) == int(a["d"]["stop"]) + 1 < 250
    assert a["d"]["val"].dtype == bool
    assert int(b["d"]["stop"]) == -1 and int(b["d"]["epochs"]) == 250
    val = b["d"]["val"]
    assert val.dtype == np.int64 and np.any(np.diff(val) < 0) and len(np.unique(val)) == len(val)


@pytest.mark.parametrize("case", R.CASES)
def test_every_stopping_comparison_is_far_from_a_tie(case, runs):
    c = runs[case]
    need = R.load_manifest()["gap_factor"] * c["meta"]["f32_vs_f64"]["loss"]
    for trace in (c["d"]["loss"], c["run"]["loss"]):
        gap, stop = R.stop_gaps(trace)
        assert gap > need and stop == int(c["d"]["stop"])
    assert c["meta"]["min_gap"] > need


def torch_epoch(H, z, y, params):
    """loss and gradients of WATS.py:124-130, :150 through dense float64 autograd"""
    t = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in R.as_params(params)]
    W1, b1, W2, b2 = t
    Ht, zt = torch.tensor(H, dtype=torch.float64), torch.tensor(z, dtype=torch.float64)
    temp = (torch.relu(Ht @ W1.T + b1) @ W2.reshape(-1, 1) + b2).squeeze(1)
    T = torch.log(torch.exp(temp) + torch.tensor(R.SHIFT, dtype=torch.float64))
    out = torch.log_softmax(zt / T.unsqueeze(1), dim=1)
    loss = torch.nn.functional.nll_loss(out, torch.tensor(y))
    loss.backward()
    return float(loss.detach()), [p.grad.numpy() for p in t], out.detach().numpy()


def random_problem(hid, F, C, n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((n, F))
    z = rng.standard_normal((n, C)) * scale
    y = rng.integers(0, C, n)
    params = [rng.standard_normal((hid, F)) * 0.7, rng.standard_normal(hid) * 0.5, rng.standard_normal(hid) * 0.5,
              rng.standard_normal(1) * 0.3]
    return H, z, y, params


@pytest.mark.parametrize("hid,F", [(16, 1), (16, 4)])
def test_epoch_agrees_with_float64_autograd(hid, F):
    for C, n, scale in ((7, 50, 1.0), (40, 33, 30.0), (1, 5, 1.0)):
        H, z, y, params = random_problem(hid, F, C, n, seed=hid + F + C, scale=scale)
        q = R.epoch(H, z, y, params)
        loss, grads, out = torch_epoch(H, z, y, params)
        assert R.kink_margin(q) > 1e-9
        assert abs(q["loss"] - loss) <= TIGHT * q["loss_abs"]
        for g, w, ab in zip(q["grads"], grads, q["grads_abs"]):
            assert np.all(np.abs(g - w.reshape(g.shape)) <= TIGHT * ab + 1e-300)
        assert q["correct"] == int((out.argmax(axis=1) == y).sum())
        assert R.dist(R.forward(H, z, params), out) <= TIGHT * (1 + np.abs(out).max())


@pytest.mark.parametrize("hid,F", [(16, 1), (16, 4)])
def test_training_agrees_with_torch_adam(hid, F):
    H, z, y, params = random_problem(hid, F, 7, 60, seed=3 * hid + F)
    rows = np.random.default_rng(1).permutation(60)[:25]
    r = R.train(H, z, y, rows, params, epochs=25, patience=4)
    t = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in R.as_params(params)]
    opt = torch.optim.Adam(t, lr=0.01, weight_decay=5e-4)
    Ht, zt, yt = (torch.tensor(a[rows]) for a in (H, z, y))
    best, left, losses = np.inf, 4, []
    for e in range(25):
        opt.zero_grad()
        temp = (torch.relu(Ht @ t[0].T + t[1]) @ t[2].reshape(-1, 1) + t[3]).squeeze(1)
        T = torch.log(torch.exp(temp) + torch.tensor(R.SHIFT, dtype=torch.float64))
        loss = torch.nn.functional.nll_loss(torch.log_softmax(zt / T.unsqueeze(1), dim=1), yt)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if losses[-1] < best:
            best, left = losses[-1], 4
        else:
            left -= 1
        if left <= 0:
            break
    assert r["epochs_run"] == len(losses)
    assert np.allclose(r["loss"], losses, rtol=0, atol=1e-12)
    for a, b in zip(r["params"], t):
        assert np.allclose(a, b.detach().numpy().reshape(a.shape), rtol=0, atol=1e-12)


def test_zero_preactivation_contributes_nothing_and_a_nan_reaches_the_loss():
    H, z, y, params = random_problem(16, 4, 7, 12, seed=9)
    params[1][:5] = 0.0                       # b1_j = 0 on five units
    H[3] = 0.0                                # and a zero feature row: pre_j == 0 exactly there
    q = R.epoch(H, z, y, params)
    assert np.all(q["pre"][3, :5] == 0.0)
    loss, grads, _ = torch_epoch(H, z, y, params)
    for g, w, ab in zip(q["grads"], grads, q["grads_abs"]):      # torch's threshold backward: 0 at 0
        assert np.all(np.abs(g - w.reshape(g.shape)) <= TIGHT * ab + 1e-300)
    without = R.epoch(np.delete(H, 3, 0), np.delete(z, 3, 0), np.delete(y, 3), params)
    assert np.allclose(q["grads"][1][:5] * 12, without["grads"][1][:5] * 11, rtol=1e-13, atol=0)
    H[7, 1] = np.nan
    q = R.epoch(H, z, y, params)
    assert np.isnan(q["loss"]) and np.isnan(q["grads"][3][0]) and np.all(np.isnan(q["grads"][2]))
    r = R.train(H, z, y, np.arange(12), params, patience=6)
    assert r["epochs_run"] == 6 and r["stop_epoch"] == 5 and r["best_loss"] == np.inf


# ------------------------------------------------------------------------------------------- the host's checks
def test_host_argument_checks_without_a_gpu():
    from wats_hip import _lib
    lib = _lib.load()
    INVALID, UNSUPPORTED = -1, -4
    assert lib.wg_wats_train_max_params() == 2048 and lib.wg_wats_train_chunk_rows() == 256
    nbytes = ctypes.c_int64(-1)
    sb = lambda F, hid, ep=250, rows=1000: lib.wg_wats_train_state_bytes(F, hid, ep, rows, ctypes.byref(nbytes))  # noqa: E731
    assert sb(1, 16) == 0
    P, chunks = 49, 4
    assert nbytes.value == 8 * (16 + 3 * P + 2 * 250 + chunks * (P + 2))
    assert sb(29, 64) == 0 and sb(1, 64) == 0                         # P = 1985, 193
    assert sb(30, 64) == UNSUPPORTED and b"2049" in lib.wg_last_error()
    assert sb(1, 65) == INVALID and sb(1, 0) == INVALID and sb(0, 16) == INVALID
    assert sb(1, 16, ep=0) == INVALID and sb(1, 16, rows=0) == INVALID
    assert sb(1, 16, rows=2 ** 31) == UNSUPPORTED
    assert lib.wg_wats_train_state_bytes(1, 16, 250, 1000, None) == INVALID

    # pointers are only compared with NULL before any device call: every call below fails on the host
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p).value

    def init(state=p, F=1, hid=16, C=5, ep=250, rows=1000, patience=10, W1=p, b1=p, W2=p, b2=p):
        return lib.wg_wats_train_state_init(state, F, hid, C, ep, rows, patience, 0.01, 5e-4, W1, b1, W2, b2, None)
    assert init(state=None) == INVALID and b"NULL" in lib.wg_last_error()
    for k in ("W1", "b1", "W2", "b2"):
        assert init(**{k: None}) == INVALID, k
    assert init(state=p + 4) == INVALID and init(patience=0) == INVALID
    assert init(hid=65) == INVALID and init(F=30, hid=64) == UNSUPPORTED
    assert init(C=0) == INVALID and init(C=257) == UNSUPPORTED

    def epoch(state=p, F=1, hid=16, C=5, ep=250, max_rows=1000, n=2000, n_rows=1000, H=p, logits=p, rows=p, labels=p,
              g=0):
        return lib.wg_wats_train_epoch(state, F, hid, C, ep, max_rows, n, n_rows, H, logits, rows, labels, g, None)
    assert epoch(F=30, hid=64) == UNSUPPORTED and b"2049" in lib.wg_last_error()
    assert epoch(hid=65) == INVALID
    assert epoch(n_rows=0) == INVALID
    assert epoch(n_rows=1001) == INVALID and b"sized for" in lib.wg_last_error()
    assert epoch(rows=None) == INVALID and b"no row list" in lib.wg_last_error()
    for k in ("state", "H", "logits", "labels"):
        assert epoch(**{k: None}) == INVALID and b"NULL" in lib.wg_last_error(), k
    assert epoch(C=257) == UNSUPPORTED and epoch(C=0) == INVALID
    assert epoch(n=2 ** 31, n_rows=10) == UNSUPPORTED
    assert epoch(g=-1) == INVALID and epoch(g=1025) == INVALID
    assert lib.wg_wats_train_state_read(None, 1, 16, 250, None, None, None, None, None, None) == INVALID
    assert lib.wg_wats_train_state_read(p, 30, 64, 250, None, None, None, None, None, None) == UNSUPPORTED


def test_the_header_names_the_queue_as_a_stream_and_points_to_the_test():
    from conftest import REPO
    from test_streams_host import header_prototypes
    protos = header_prototypes()
    for name in ("wg_wats_train_state_init", "wg_wats_train_state_read", "wg_wats_train_epoch"):
        args, doc = protos[name]
        assert args.rstrip().endswith("void* queue"), name
        assert "queue is a HIP stream" in doc and "captured" in doc and "tests/test_wats_train.py" in doc
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "tests/test_wats_train.py" in design.split("Streams and capture")[1]


# -------------------------------------------------------------------------------------------------- the mutants
def mutant_problem():
    H, z, y, params = random_problem(16, 4, 7, 80, seed=21, scale=3.0)
    rows = np.random.default_rng(2).permutation(80)[:30]
    return H, z, y, params, rows


def outside(got, want, ab):
    return bool(np.any(np.abs(np.asarray(got) - np.asarray(want)) > TIGHT * np.asarray(ab)))


@pytest.mark.parametrize("mutant", ["decoupled_wd", "no_bias_decay"])
def test_mutant_weight_decay(mutant):
    """one step from the same gradients: the parameters leave the test's 2 x 2^-24 bound"""
    H, z, y, params, rows = mutant_problem()
    params[1] += 3.0                                     # biases large enough for their decay to show in float32
    params[3] += 3.0
    good = R.train(H, z, y, rows, params, epochs=3)
    bad = R.train(H, z, y, rows, params, epochs=3, mutant=mutant)
    assert any(np.any(np.abs(a - b) > 2 * R.EPS32 * np.abs(a)) for a, b in zip(good["params"], bad["params"]))
    if mutant == "no_bias_decay":
        assert np.array_equal(good["loss"][:1], bad["loss"][:1])


def test_mutant_multiply_instead_of_divide():
    H, z, y, params, rows = mutant_problem()
    q, m = R.epoch(H[rows], z[rows], y[rows], params), R.epoch(H[rows], z[rows], y[rows], params, mutant="multiply_T")
    assert outside(m["loss"], q["loss"], q["loss_abs"])
    assert all(outside(a, b, ab) for a, b, ab in zip(m["grads"], q["grads"], q["grads_abs"]))


def test_mutant_relu_gradient_at_zero():
    H, z, y, params, rows = mutant_problem()
    params[1][:4] = 0.0
    H[rows[2]] = 0.0
    q = R.epoch(H[rows], z[rows], y[rows], params)
    m = R.epoch(H[rows], z[rows], y[rows], params, mutant="relu_grad_at_zero")
    assert q["loss"] == m["loss"]
    assert outside(m["grads"][1], q["grads"][1], q["grads_abs"][1])        # g_b1 of the zero units
    assert not outside(m["grads"][2], q["grads"][2], q["grads_abs"][2])


def test_mutant_best_loss_comparison():
    """two equal losses in a row: < counts the second one down, <= does not"""
    H, z, y, params, rows = mutant_problem()
    good = R.train(H, z, y, rows, params, epochs=40, patience=3, lr=0.0, wd=0.0)
    bad = R.train(H, z, y, rows, params, epochs=40, patience=3, lr=0.0, wd=0.0, mutant="best_le")
    assert good["stop_epoch"] == 3 and bad["stop_epoch"] is None and bad["epochs_run"] == 40


def test_mutant_mean_over_all_rows():
    H, z, y, params, rows = mutant_problem()
    q = R.epoch(H[rows], z[rows], y[rows], params)
    m = R.epoch(H[rows], z[rows], y[rows], params, mutant="mean_n_total", n_total=80)
    assert outside(m["loss"], q["loss"], q["loss_abs"])
    assert np.isclose(m["loss"] * 80, q["loss"] * 30)


def test_mutant_shift_constant():
    H, z, y, params, rows = mutant_problem()
    q = R.epoch(H[rows], z[rows], y[rows], params)
    m = R.epoch(H[rows], z[rows], y[rows], params, mutant="shift_double")
    assert outside(m["loss"], q["loss"], q["loss_abs"])
    assert outside(m["grads"][3], q["grads"][3], q["grads_abs"][3])


def test_the_mutant_list_is_the_one_tested():
    assert set(R.MUTANTS) == {"decoupled_wd", "no_bias_decay", "multiply_T", "relu_grad_at_zero", "best_le",
                              "mean_n_total", "shift_double"}
