"""GPU tests of the node-wise calibrators: the kernels of csrc/scale.hip against tests/scaling_ref.py, the training
epoch's state block, and the classes of wats_hip/scaling.py against the fixtures of the reference's own TS / VS / MS /
ETS (tests/golden/scaling).

Bounds.  out, g_logits and wg_scale_backward's parameter gradients are float64 values rounded once: 0.5 ulp of
float32 plus the float64 evaluation's error, 1e-12 of the sum of the absolute terms (scaling_ref.one_rounding_ok).
The epoch's loss and parameter gradients stay float64: 1e-12 of the same sums.  The correct count is exact.  Training
on the fixtures is held to the float64 restatement within the manifest's f32_vs_f64 (the device run is no farther from
the truth than the reference's own float32 run) and to the stopping epoch exactly; ETS's weights to the fixture within
4 x f32_vs_f64 (SLSQP's finite-difference step amplifies objective noise).  A class that loaded the fixture's
parameters is within f32_vs_f64 of the restatement on those parameters (output and edge gradient) and of the recorded
float32 output; its edge gradient is within 2 x f32_vs_f64 of the recorded float32 one (two float32 evaluations, each
within f32_vs_f64 of the float64 one: measured 1.22e-4 against a recorded 1.10e-4 for MS on plain120).  wg_ets_label_probs is held to the restatement's two float64 vectors at 1e-12 of each value.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import scaling_ref as R  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip import scaling as S  # noqa: E402
from wats_hip.metrics import calculate_average_ece  # noqa: E402

DEV = "cuda"
TIGHT = 1e-12
ROWS = (1, 2, 63, 64, 65, 257, 4097)
WIDTHS = {"ts": (2, 3, 7, 40, 41, 64, 65, 255, 256), "vs": (2, 3, 7, 40, 41, 64, 65, 255, 256),
          "ets": (2, 3, 7, 40, 41, 64, 65, 255, 256), "ms": (2, 3, 7, 16, 40, 47, 64)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()
    assert S.max_classes("ts") >= 256 and S.max_classes("vs") >= 256 and S.max_classes("ets") >= 256
    assert S.max_classes("ms") >= 64


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def host(t):
    return t.detach().cpu().numpy()


def dist(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def make_logits(n, C, scale, seed):
    """float32 logits at the given scale; row 0 constant, row 1 holding +-1e4 (where the shape has them)"""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((n, C)) * scale).astype(np.float32)
    if n >= 3:
        z[0] = np.float32(0.75 * scale)
        z[1, 0], z[1, -1] = 1e4, -1e4
    return z


def make_params(mode, C, seed):
    rng = np.random.default_rng(1000 + seed)
    f = lambda a: np.asarray(a, np.float32)   # noqa: E731
    if mode == "ts":
        return [f([0.3])]
    if mode == "vs":
        return [f(rng.standard_normal(C) * 0.5)]
    if mode == "ms":
        W = np.ones((C, C)) + 0.2 * rng.standard_normal((C, C))
        W[0, 0] = 1.0
        return [f(W), f(1 + 0.2 * rng.standard_normal(C))]
    return [f([0.4]), f([0.6]), f([0.3]), f([0.1])]


def row_list(kind, n, seed):
    rng = np.random.default_rng(2000 + seed)
    if kind == "absent":
        return None, np.arange(n)
    if kind == "mask":
        m = rng.random(n) < 0.5
        m[0] = True
        return torch.from_numpy(m), np.nonzero(m)[0]
    k = max(1, (2 * n) // 3)
    ids = rng.choice(n, size=k, replace=False)
    if kind == "sorted":
        ids = np.sort(ids)
    if kind == "repeats":
        ids = np.concatenate([ids, ids[: max(1, k // 3)], ids[:1]])
        rng.shuffle(ids)
    return torch.from_numpy(ids.astype(np.int64)), ids


def check_forward_backward(mode, n, C, scale, kind, normalize=False, seed=0):
    z = make_logits(n, C, scale, seed)
    params = make_params(mode, C, seed)
    rows, idx = row_list(kind, n, seed)
    g = np.random.default_rng(3000 + seed).standard_normal((len(idx), C)).astype(np.float32)
    zt = dev(z).requires_grad_(True)
    pt = [dev(p).requires_grad_(True) for p in params]
    out = S.scaled_log_probs(zt, mode, *pt, rows=rows, normalize=normalize)
    assert out.shape == (len(idx), C) and out.dtype == torch.float32
    truth, ab = R.forward(mode, z[idx], params, normalize, with_abs=True)
    what = f"{mode} n={n} C={C} scale={scale} rows={kind}"
    R.one_rounding_ok(host(out), truth, ab, what + " out")
    out.backward(dev(g))
    gz, gp, (gz_abs, gp_abs) = R.backward(mode, z[idx], params, g, normalize)
    full, full_abs = np.zeros((n, C)), np.zeros((n, C))
    np.add.at(full, idx, gz)                       # a repeated row collects every copy's gradient
    np.add.at(full_abs, idx, gz_abs)
    if kind == "repeats":
        # k copies, each rounded once, then k - 1 float32 additions by torch's index_add_: 2 k - 1 roundings, and
        # below the smallest normal float32 (2^-126) such an addition may flush to zero
        counts = np.bincount(idx, minlength=n)[:, None]
        err = np.abs(host(zt.grad) - full)
        bound = 2 * counts * (R.EPS32 * full_abs + 2.0 ** -126) + TIGHT * full_abs
        assert np.all(err <= bound), what + f" g_logits: {float((err / (bound + 1e-300)).max()):.3f} of the bound"
    else:
        R.one_rounding_ok(host(zt.grad), full, full_abs, what + " g_logits")
    for k, (a, t, abk) in enumerate(zip(gp, pt, gp_abs)):
        R.one_rounding_ok(host(t.grad), a.reshape(t.shape), abk.reshape(t.shape), what + f" parameter gradient {k}")


@pytest.mark.parametrize("mode,C", [(m, C) for m in ("ts", "vs", "ms", "ets") for C in WIDTHS[m]])
def test_kernels_hold_the_one_rounding_bound_at_every_shape(mode, C):
    for n in ROWS:
        for scale in (1.0, 30.0):
            check_forward_backward(mode, n, C, scale, kind="absent", seed=n + C)


@pytest.mark.parametrize("kind", ["sorted", "unsorted", "repeats", "mask"])
@pytest.mark.parametrize("mode,C,normalize", [("ts", 41, False), ("vs", 65, False), ("ms", 47, False),
                                              ("ms", 7, True), ("ets", 7, False)])
def test_row_lists_and_scales(mode, C, normalize, kind):
    for scale in (1.0, 30.0):
        check_forward_backward(mode, 257, C, scale, kind, normalize, seed=int(scale))


def one_epoch(mode, z, y, idx_t, params, normalize=False, n_workgroups=0, epochs=3, launches=1):
    n, C = z.shape
    n_rows = n if idx_t is None else idx_t.numel()
    st = S._TrainingState(S._mode(mode), C, epochs, n_rows, 10, normalize, torch.device(DEV, 0),
                          init=[dev(p) for p in params])
    zt, yt = dev(z), dev(y, torch.int64)
    for _ in range(launches):
        st.epoch(zt, idx_t, yt, n_workgroups)
    return st


# every n of the issue with a row list of its own, 4097 also with repeats
EPOCH_ROWS = ((1, "absent"), (2, "unsorted"), (63, "mask"), (64, "absent"), (65, "unsorted"), (257, "mask"),
              (4097, "absent"), (4097, "repeats"))


def check_epoch(mode, C, normalize, n, kind, scale):
    seed = n + C
    z = make_logits(n, C, scale, seed)
    y = np.random.default_rng(seed).integers(0, C, n)
    params = make_params(mode, C, seed)
    rows, idx = row_list(kind, n, seed)
    idx_t = None if rows is None else S._row_list(rows, n, DEV)
    st = one_epoch(mode, z, y, idx_t, params, normalize)
    q = R.epoch(mode, z[idx], y[idx], params, normalize)
    nll = R.epoch(mode, z[idx], y[idx], params, normalize, Lambda=0.0)      # the chunk partials hold the nll part
    new, info = st.read()
    what = f"{mode} C={C} n={n} {kind} scale={scale}"
    assert info[1] == 1 and info[2] == 1, what
    loss, acc = info[5], info[5 + 3]
    assert abs(loss - q["loss"]) <= TIGHT * q["loss_abs"], f"{what}: loss {loss!r} vs {q['loss']!r}"
    assert acc == q["correct"] / len(idx), what           # the count is exact
    part = host(st.partials(len(idx)))
    assert part[:, 1].sum() == q["correct"], what
    flat = np.concatenate([np.ravel(v) for v in nll["grads"]])
    flat_abs = np.concatenate([np.ravel(v) for v in nll["grads_abs"]])
    got = part[:, 2:].sum(axis=0) / len(idx)
    assert np.all(np.abs(got - flat) <= TIGHT * flat_abs + 1e-300), what + " parameter gradients"
    # the Adam step from the full gradients (L1 term included)
    for k, p in enumerate(params):
        want, _, _ = R.adam_step(p, q["grads"][k], np.zeros_like(p, np.float64), np.zeros_like(p, np.float64), 1)
        assert np.all(np.abs(host(new[k]) - want.astype(np.float32)) <= 2 * R.EPS32 * np.abs(want) + 1e-30), what


@pytest.mark.parametrize("mode,C,normalize", [(m, C, False) for m in ("ts", "vs", "ms") for C in WIDTHS[m]]
                         + [("ms", 16, True), ("ms", 47, True)])
def test_epoch_quantities(mode, C, normalize):
    """the epoch's loss, parameter gradients (1e-12 of the absolute sums) and correct count (exact) at every n and C
    of the issue, both scales"""
    for n, kind in EPOCH_ROWS:
        for scale in (1.0, 30.0):
            check_epoch(mode, C, normalize, n, kind, scale)


@pytest.mark.parametrize("C", WIDTHS["ets"])
def test_ets_label_probs_match_the_restatement(C):
    """wg_ets_label_probs against scaling_ref.ets_label_probs, both float64: exp(x) errs by |x| 2^-53 relative, and
    |x| stays below 745 before the result underflows, so 1e-12 of the value (an underflowed entry is exactly 0)"""
    for n in ROWS:
        for k, kind in enumerate(("absent", "sorted", "unsorted", "repeats", "mask")):
            for scale, tau in ((1.0, 0.7), (30.0, 3.25), (1.0, -1.5)):       # the RAW tau divides, whatever its sign
                seed = n + C + k
                z = make_logits(n, C, scale, seed)
                y = np.random.default_rng(seed).integers(0, C, n)
                if n >= 3:
                    y[1] = (0, C - 1)[k % 2]                                 # the label on a +-1e4 column
                if C > 64:
                    y[n // 2] = C - 1                                        # a label past the first 64 lanes
                rows, idx = row_list(kind, n, seed)
                p0, p1 = S.ets_label_probs(dev(z), dev(y, torch.int64), dev([tau]), rows=rows)
                w0, w1 = R.ets_label_probs(z[idx], y[idx], np.float32(tau))
                what = f"C={C} n={n} rows={kind} scale={scale} tau={tau}"
                assert p0.dtype == torch.float64 and p0.shape == (len(idx),), what
                for got, want, name in ((host(p0), w0, "p0y"), (host(p1), w1, "p1y")):
                    assert np.all(np.isfinite(got)), what
                    assert np.all(np.abs(got - want) <= TIGHT * np.abs(want)), f"{what} {name}"
    # the softplus of tau as the divisor is another vector altogether
    m0, _ = R.ets_label_probs(z[idx], y[idx], np.float32(tau), mutant="ets_fit_softplus")
    assert not np.allclose(m0, w0, rtol=1e-6, atol=0)


@pytest.mark.parametrize("mode,C", [("ts", 41), ("vs", 65), ("ms", 47)])
def test_state_bits_do_not_depend_on_the_grid(mode, C):
    n = 4097
    z = make_logits(n, C, 1.0, 5)
    y = np.random.default_rng(5).integers(0, C, n)
    params = make_params(mode, C, 5)
    blocks = [one_epoch(mode, z, y, None, params, n_workgroups=g, launches=3).block.clone() for g in (1, 2, 7, 0)]
    for b in blocks[1:]:
        assert torch.equal(b.view(torch.int64), blocks[0].view(torch.int64))


# ------------------------------------------------------------------------------------------ training, fixtures
_cases = {}


def case(name):
    if name not in _cases:
        d, meta, _ = R.load_case(name)
        P = R.case_base(d)
        z64 = R.base_logits(P, d["x"], d["adj"])
        rows = R.case_rows(d)
        _cases[name] = dict(d=d, meta=meta, z64=z64, rows=rows,
                            runs={c: R.train(c, z64, d["y"], rows) for c in ("ts", "vs", "ms")})
    return _cases[name]


def base_of(c, dropout=0.0):
    d = c["d"]
    P = R.case_base(d)
    base = wats_hip.SparseCompatibleGCN(d["x"].shape[1], nclass=P["gc2.weight"].shape[0],
                                        nhid=P["gc1.weight"].shape[0], dropout=dropout)
    base.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    return base.to(DEV).eval()


def tensors(c):
    d = c["d"]
    return (torch.from_numpy(d["x"]).to(DEV), torch.from_numpy(d["y"]).to(DEV), torch.from_numpy(d["adj"]).to(DEV),
            torch.from_numpy(d["val"]).to(DEV))


CLASSES = {"ts": S.TemperatureScaling, "vs": S.VectorScaling, "ms": S.MatrixScaling, "ets": S.ETS}


def build(c, name, **kw):
    x, y, adj, val = tensors(c)
    kw.setdefault("verbose", False)
    kw.setdefault("frozen_logits", True)
    if name == "ets":
        vm = torch.from_numpy(c["d"]["val_mask"]).to(DEV)
        return S.ETS(base_of(c), x, y, adj, val, **kw).fit([~vm, val, ~vm])
    return CLASSES[name](base_model=base_of(c), x=x, y=y, adj=adj, val_idx=val, **kw)


@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("cal", ["ts", "vs", "ms"])
def test_training_reaches_the_restatement_within_the_references_own_error(name, cal):
    c = case(name)
    f, want = c["meta"]["f32_vs_f64"], c["runs"][cal]
    model = build(c, cal)
    run = model.training_run
    assert run.epochs_run == want["epochs_run"] == int(c["d"][f"epochs_{cal}"])
    assert run.stop_epoch == want["stop_epoch"]
    d_loss = dist(run.loss, want["loss"])
    d_par = max(dist(host(a), b) for a, b in zip(run.params, want["params"]))
    print(f"{name} {cal}: loss distance {d_loss:.3e} (allowed {f['loss_' + cal]:.3e}), parameters {d_par:.3e} "
          f"(allowed {f['params_' + cal]:.3e})")
    assert d_loss <= f["loss_" + cal]
    assert d_par <= f["params_" + cal]
    assert np.array_equal(run.acc, want["acc"])


@pytest.mark.parametrize("name", R.CASES)
def test_ets_weights(name):
    c = case(name)
    f = c["meta"]["f32_vs_f64"]["w_ets"]
    model = build(c, "ets")
    w = np.array([float(v.detach()) for v in (model.w1, model.w2, model.w3)])
    measured = R.load_manifest().get("measured", {}).get("w_ets", {})
    assert name in measured, "record the device run's distance in the manifest (tests/golden/scaling/manifest.json)"
    print(f"{name}: ETS w {w.tolist()} vs {c['d']['w_ets'].tolist()}: distance {dist(w, c['d']['w_ets']):.3e} "
          f"(allowed {4 * f:.3e})")
    assert model.w1.dtype == torch.float64 and model.w1.dim() == 0        # as ETS.py:45 leaves them
    assert dist(w, c["d"]["w_ets"]) <= 4 * f


def test_both_training_modes_agree_bitwise_without_dropout():
    c = case("plain120")
    for cal in ("ts", "ms"):
        a, b = build(c, cal, frozen_logits=True), build(c, cal, frozen_logits=False)
        assert a.training_run.epochs_run == b.training_run.epochs_run
        assert np.array_equal(a.training_run.loss, b.training_run.loss)
        for p, q in zip(a.training_run.params, b.training_run.params):
            assert torch.equal(p, q)


def test_live_dropout_reaches_the_logits_in_the_default_mode():
    """TS.py:60: self.train() puts the base model into train mode, so p > 0 changes the epochs' logits"""
    c = case("plain120")
    x, y, adj, val = tensors(c)
    torch.manual_seed(0)
    live = S.TemperatureScaling(base_of(c, dropout=0.5), x, y, adj, val, verbose=False, epochs=12)
    frozen = S.TemperatureScaling(base_of(c, dropout=0.5), x, y, adj, val, verbose=False, epochs=12,
                                  frozen_logits=True)
    assert not np.array_equal(live.training_run.loss, frozen.training_run.loss)
    assert np.array_equal(frozen.training_run.loss, c["runs"]["ts"]["loss"][:12]) or \
        dist(frozen.training_run.loss, c["runs"]["ts"]["loss"][:12]) <= c["meta"]["f32_vs_f64"]["loss_ts"]


@pytest.mark.parametrize("mode", ["ts", "vs", "ms"])
def test_callable_logits_follow_the_restatement(mode):
    c = case("wide96")
    d = c["d"]
    z = c["z64"].astype(np.float32)
    seq = [z + np.random.default_rng(100 + e).standard_normal(z.shape).astype(np.float32) for e in range(130)]
    want = R.train(mode, lambda e: seq[e], d["y"], c["rows"], epochs=130)
    calls = []

    def logits(e):
        calls.append(e)
        return dev(seq[e])
    run = S.train_scaling(mode, logits, torch.from_numpy(d["y"]), torch.from_numpy(d["val"]), epochs=130)
    assert run.epochs_run == want["epochs_run"] and run.stop_epoch == want["stop_epoch"]
    assert want["stop_epoch"] is not None and len(calls) < 130         # the host stopped calling
    assert np.allclose(run.loss, want["loss"], rtol=1e-9, atol=1e-9)
    for a, b in zip(run.params, want["params"]):
        assert np.allclose(host(a), b, rtol=1e-6, atol=1e-7)


def test_nan_row_is_contained_and_patience_counts_down():
    c = case("plain120")
    d = c["d"]
    z = c["z64"].astype(np.float32)
    bad = int(c["rows"][3])
    zn = z.copy()
    zn[bad, 1] = np.nan
    run = S.train_scaling("ts", dev(zn), torch.from_numpy(d["y"]), torch.from_numpy(d["val"]), patience=7)
    assert run.epochs_run == 7 and run.stop_epoch == 6 and run.patience_left == 0
    assert np.all(np.isnan(run.loss)) and run.best_loss == np.inf
    for mode in ("ts", "vs", "ms", "ets"):
        p = [dev(q) for q in make_params(mode, z.shape[1], 1)]
        a, b = S.scaled_log_probs(dev(z), mode, *p), S.scaled_log_probs(dev(zn), mode, *p)
        keep = torch.arange(z.shape[0], device=DEV) != bad
        assert torch.equal(a[keep], b[keep]) and bool(torch.isnan(b[bad]).any())


def test_launches_past_stopped_leave_the_state_alone():
    c = case("plain120")
    d = c["d"]
    z, y = dev(c["z64"].astype(np.float32)), dev(d["y"], torch.int64)
    rows = S._row_list(torch.from_numpy(d["val"]), z.shape[0], DEV)
    for mode, epochs in (("ms", 250), ("ts", 5)):                        # out of patience; out of epochs
        st = S._TrainingState(S._mode(mode), z.shape[1], epochs, rows.numel(), 10, False, torch.device(DEV, 0))
        for _ in range(epochs):
            st.epoch(z, rows, y)
        assert st.stopped()
        before = st.block.clone()
        for g in (0, 1, 3):
            st.epoch(z, rows, y, g)
        torch.cuda.synchronize()
        assert torch.equal(before.view(torch.int64), st.block.view(torch.int64))


# --------------------------------------------------------------------------------------------------- the classes
@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("cal", R.CALIBRATORS)
def test_classes_reproduce_the_fixture(name, cal):
    c = case(name)
    d, f = c["d"], c["meta"]["f32_vs_f64"]
    model = build(c, cal, epochs=2)                    # the parameters come from the fixture
    pre = f"p__{cal}__"
    state = {k[len(pre):]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith(pre)}
    assert set(model.state_dict().keys()) == set(state.keys())
    model.load_state_dict(state)
    model.eval()
    x, _, adj, _ = tensors(c)
    probe = wats_hip.EdgeProbe(d["grad_rows"], d["grad_cols"])
    out = model(x, adj, probe=probe)
    truth = R.forward(cal, c["z64"], R.case_params(d, cal))
    print(f"{name} {cal}: out to the restatement {dist(host(out), truth):.3e}, to the fixture "
          f"{dist(host(out), d['out_' + cal]):.3e} (f32_vs_f64 {f['out_' + cal]:.3e})")
    assert dist(host(out), truth) <= f["out_" + cal]
    assert dist(host(out), d["out_" + cal]) <= f["out_" + cal]
    (out * torch.from_numpy(d["loss_weight"]).to(DEV)).sum().backward()
    g_truth = R.adjacency_gradient(cal, R.case_base(d), R.case_params(d, cal), d["x"], d["adj"], d["loss_weight"],
                                   d["grad_rows"], d["grad_cols"])
    print(f"  edge gradient to the restatement {dist(host(probe.grad), g_truth):.3e} "
          f"(f32_vs_f64 {f['grad_' + cal]:.3e})")
    assert dist(host(probe.grad), g_truth) <= f["grad_" + cal]
    print(f"  edge gradient to the fixture {dist(host(probe.grad), d['grad_' + cal]):.3e}")
    # two float32 evaluations, each within f32_vs_f64 of the float64 one (the device's: asserted above; the
    # reference's: the manifest's definition), are within twice that of each other
    assert dist(host(probe.grad), d["grad_" + cal]) <= 2 * f["grad_" + cal]


def test_harness_blocks_end_in_ece():
    """benchmark_calibration_methods.py:198-257 with its keywords, scored as the harness scores (ECE on the test
    nodes); on overconfident logits every calibrator lowers the validation nll it was trained on"""
    c = case("plain120")
    d = c["d"]
    x, y, adj, val = tensors(c)
    test_mask = ~torch.from_numpy(d["val_mask"]).to(DEV)
    base = base_of(c)
    ncls = int(y.max()) + 1
    with torch.no_grad():
        base_nll = float(torch.nn.functional.nll_loss(torch.log_softmax(base(x, adj), dim=1)[val], y[val]))
    with contextlib.redirect_stdout(io.StringIO()) as log:
        models = {
            "ts": wats_hip.TemperatureScaling(base_model=base, x=x, y=y, adj=adj, val_idx=val),
            "vs": wats_hip.VectorScaling(base_model=base, x=x, y=y, adj=adj, val_idx=val),
            "ms": wats_hip.MatrixScaling(base_model=base, x=x, y=y, adj=adj, val_idx=val),
            "ets": wats_hip.ETS(base, x, y, adj, val).fit([test_mask, val, test_mask]),
        }
    assert "loss_calibration" in log.getvalue() and "Early stopping at epoch 110" in log.getvalue()
    for name, m in models.items():
        m.eval()
        with torch.no_grad():
            out = m(x, adj)
            probs = torch.softmax(out, dim=1) if name == "ms" else torch.exp(out)
            ece = calculate_average_ece(probs[test_mask], y[test_mask], ncls, logits=False)
            nll = float(torch.nn.functional.nll_loss(torch.log(probs)[val], y[val]))
        print(f"{name}: ECE {ece:.4f}, validation nll {nll:.4f} (base {base_nll:.4f})")
        assert 0.0 <= ece <= 1.0 and np.isfinite(nll)
        if name in ("ts", "vs"):               # trained on this very nll (MS: on its raw output plus the L1 term;
            assert nll < base_nll              # ETS: its two temperature conventions are kept as found)
    assert wats_hip.TS is wats_hip.TemperatureScaling and wats_hip.VS is wats_hip.VectorScaling
    assert wats_hip.MS is wats_hip.MatrixScaling
    assert isinstance(wats_hip.calibrate_with_temperature_scaling(base, x, y, adj, val, verbose=False, epochs=2),
                      wats_hip.TemperatureScaling)
    assert isinstance(wats_hip.calibrate_with_vector_scaling(base, x, y, adj, val, verbose=False, epochs=2),
                      wats_hip.VectorScaling)
    assert isinstance(wats_hip.calibrate_with_matrix_scaling(base, x, y, adj, val, verbose=False, epochs=2),
                      wats_hip.MatrixScaling)


def test_limits_and_bad_arguments():
    z = torch.zeros(4, 65, device=DEV)
    with pytest.raises(NotImplementedError):
        S.scaled_log_probs(z, "ms", torch.ones(65, 65, device=DEV), torch.ones(65, device=DEV))
    with pytest.raises(NotImplementedError):
        S.scaled_log_probs(torch.zeros(4, 257, device=DEV), "ts", torch.ones(1, device=DEV))
    with pytest.raises(IndexError):
        S.scaled_log_probs(z, "ts", torch.ones(1, device=DEV), rows=torch.tensor([4]))
    with pytest.raises(ValueError):
        S.scaled_log_probs(z, "vs", torch.ones(64, device=DEV))
    with pytest.raises(ValueError):
        S.train_scaling("ets", z, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(IndexError):
        S.train_scaling("ts", z, torch.full((4,), 65, dtype=torch.int64))


def test_calib_fga_local_evaluation_picks_the_same_flips():
    c = case("plain120")
    d = c["d"]
    x, y, adj, _ = tensors(c)
    model = build(c, "ts")
    flips = {}
    for local in (True, False):
        atk = wats_hip.Calib_FGA(model, device=DEV, local_eval=local)
        kw = dict(n_perturb=[], best_conf=[], runtime=[])
        with contextlib.redirect_stdout(io.StringIO()):
            try:
                atk.flip_beam_hybridloss_attack(x, adj, int(d["target"]), 3, "under", res_gt=y, **kw)
            except ValueError as e:
                assert "Final label" in str(e)
        assert (atk._local is not None) == local
        flips[local] = (list(atk.flips), [s["label"] for s in atk.trace])
    assert flips[True] == flips[False] and len(flips[True][0]) >= 1
    with pytest.raises(NotImplementedError):
        wats_hip.Calib_IGA(model, device=DEV).attack(x, adj, int(d["target"]), 2, "under", res_gt=y)
