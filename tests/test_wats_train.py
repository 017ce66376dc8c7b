"""GPU tests of WATS's training on the device: the epoch kernel of csrc/watstrain.hip against tests/wats_train_ref.py,
its state block, wats_hip.train_wats_head and WATS(fused_training=True) against the fixtures of the reference's own
runs (tests/golden/wats_train), and the stream / capture promise of the three `queue`-taking entry points.

Bounds.  The epoch's loss and chunk-summed parameter gradients stay float64: 1e-12 of the sums of their absolute terms
(wats_train_ref's docstring derives them), two float64 orders of the same sum.  The correct count is exact.  The
parameters after the step are float64 values rounded once on the way out: 2 x 2^-24 |want|.  Training on the fixtures
is held to the float64 restatement within the manifest's f32_vs_f64 (the device run is float64, so it is no farther
from the restatement than the reference's own float32 run was) and to the stopping epoch and the accuracy trace
exactly; the eval-mode output to the recorded one within 4 x f32_vs_f64["out"] (two float32 passes, the HIP features
and the head, sit between them).

Measured on the MI355X (tests/golden/wats_train/manifest.json "measured"): see test_training_on_the_fixtures.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import scaling_ref as SR  # noqa: E402
import wats_train_ref as R  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip import head as HD  # noqa: E402
from wats_hip import scaling as S  # noqa: E402

DEV = "cuda"
TIGHT = 1e-12
SHAPES = ((1, 1), (16, 1), (16, 4), (15, 2), (17, 3), (16, 40), (64, 29))        # (hid, F); the last: P = 1985
WIDTHS = (1, 2, 7, 40, 65, 256)
# every n_rows of the issue with a row list of its own, 4097 also with repeats
EPOCH_ROWS = ((1, "absent"), (2, "unsorted"), (255, "mask"), (256, "absent"), (257, "unsorted"), (4097, "absent"),
              (4097, "repeats"))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()
    assert HD.max_train_params() == 2048


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def host(t):
    return t.detach().cpu().numpy()


def make_logits(n, C, scale, seed):
    """float32 logits at the given scale; row 0 constant, row 1 holding +-1e4 (where the shape has them)"""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((n, C)) * scale).astype(np.float32)
    if n >= 3:
        z[0] = np.float32(0.75 * scale)
        z[1, 0], z[1, -1] = 1e4, -1e4
    return z


def make_head(hid, F, seed):
    rng = np.random.default_rng(1000 + seed)
    f = lambda a: np.asarray(a, np.float32)   # noqa: E731
    return [f(rng.standard_normal((hid, F)) * 0.7), f(rng.standard_normal(hid) * 0.5),
            f(rng.standard_normal(hid) * 0.5), f(rng.standard_normal(1) * 0.3)]


def row_list(kind, n_rows, seed):
    """(n_total, what the caller passes as rows, the listed ids) with exactly n_rows listed rows"""
    rng = np.random.default_rng(2000 + seed)
    if kind == "absent":
        return n_rows, None, np.arange(n_rows)
    n = n_rows + n_rows // 2 + 3
    if kind == "repeats":
        k = max(1, (2 * n_rows) // 3)
        ids = rng.choice(n, size=k, replace=False)
        ids = np.concatenate([ids, rng.choice(ids, size=n_rows - k)])
        rng.shuffle(ids)
        return n, torch.from_numpy(ids.astype(np.int64)), ids
    ids = rng.choice(n, size=n_rows, replace=False)
    if kind == "mask":
        m = np.zeros(n, dtype=bool)
        m[ids] = True
        return n, torch.from_numpy(m), np.nonzero(m)[0]
    return n, torch.from_numpy(ids.astype(np.int64)), ids


def new_state(H, z, idx_t, params, epochs=3, patience=10):
    n, C = z.shape
    hid, F = params[0].shape
    n_rows = n if idx_t is None else idx_t.numel()
    return HD._HeadTrainingState(F, hid, C, epochs, n_rows, patience, torch.device(DEV, 0), [dev(p) for p in params],
                                 R.LR, R.WD)


def within(got, want, ab):
    return np.all(np.abs(np.asarray(got) - np.asarray(want)) <= TIGHT * np.asarray(ab) + 1e-300)


def check_epoch(hid, F, C, n_rows, kind, scale):
    seed = n_rows + C + hid + F
    n, rows, idx = row_list(kind, n_rows, seed)
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((n, F)).astype(np.float32)
    z = make_logits(n, C, scale, seed)
    y = rng.integers(0, C, n)
    params = make_head(hid, F, seed)
    idx_t = None if rows is None else S._row_list(rows, n, DEV)
    what = f"hid={hid} F={F} C={C} rows={n_rows} {kind} scale={scale}"
    q = R.epoch(H[idx], z[idx], y[idx], params)
    assert len(idx) == n_rows and R.kink_margin(q) >= 1e-9, what + ": a pre-activation at the kink"
    st = new_state(H, z, idx_t, params)
    st.epoch(dev(H), dev(z), idx_t, dev(y, torch.int64))
    new, info = st.read()
    assert info[0] == 0 and info[1] == 1 and info[2] == 1, what
    loss, acc = info[5], info[5 + 3]
    assert abs(loss - q["loss"]) <= TIGHT * q["loss_abs"], f"{what}: loss {loss!r} vs {q['loss']!r}"
    assert acc == q["correct"] / n_rows, what                              # the count is exact
    part = host(st.partials(n_rows))
    assert part.shape == (-(-n_rows // 256), 2 + hid * F + 2 * hid + 1)
    assert part[:, 1].sum() == q["correct"], what
    flat = np.concatenate([np.ravel(v) for v in q["grads"]])
    flat_abs = np.concatenate([np.ravel(v) for v in q["grads_abs"]])
    assert within(part[:, 2:].sum(axis=0) / n_rows, flat, flat_abs), what + " parameter gradients"
    for k, p in enumerate(R.as_params(params)):
        want, _, _ = SR.adam_step(p, q["grads"][k], np.zeros_like(p), np.zeros_like(p), 1)
        got = host(new[k]).reshape(want.shape)
        assert np.all(np.abs(got - want.astype(np.float32)) <= 2 * R.EPS32 * np.abs(want) + 1e-30), f"{what} tensor {k}"


@pytest.mark.parametrize("hid,F", SHAPES)
def test_epoch_quantities(hid, F):
    """the epoch's loss, parameter gradients (1e-12 of the absolute sums), correct count (exact) and the parameters
    after the step at every shape, width, row count and both scales of the issue"""
    for C in WIDTHS:
        for n_rows, kind in EPOCH_ROWS:
            for scale in (1.0, 30.0):
                check_epoch(hid, F, C, n_rows, kind, scale)


def test_zero_preactivations_contribute_nothing_and_a_nan_reaches_the_loss():
    hid, F, C, n = 16, 4, 7, 300
    rng = np.random.default_rng(4)
    H = rng.standard_normal((n, F)).astype(np.float32)
    z, y, params = make_logits(n, C, 1.0, 4), rng.integers(0, C, n), make_head(hid, F, 4)
    params[1][:5] = 0.0
    H[3] = H[260] = 0.0                                   # pre_j == 0 exactly on five units, in both chunks
    q = R.epoch(H, z, y, params)
    assert np.all(q["pre"][[3, 260], :5] == 0.0)
    mutant = R.epoch(H, z, y, params, mutant="relu_grad_at_zero")
    st = new_state(H, z, None, params)
    st.epoch(dev(H), dev(z), None, dev(y, torch.int64))
    _, info = st.read()
    got = host(st.partials(n))[:, 2:].sum(axis=0) / n
    flat = np.concatenate([np.ravel(v) for v in q["grads"]])
    flat_abs = np.concatenate([np.ravel(v) for v in q["grads_abs"]])
    assert within(got, flat, flat_abs) and abs(info[5] - q["loss"]) <= TIGHT * q["loss_abs"]
    assert not within(got, np.concatenate([np.ravel(v) for v in mutant["grads"]]), flat_abs)
    # one NaN feature: its row's units are all NaN, so they are inactive (gW1, gb1 stay finite) and t carries it on
    H[7, 1] = np.nan
    q = R.epoch(H, z, y, params)
    st = new_state(H, z, None, params)
    st.epoch(dev(H), dev(z), None, dev(y, torch.int64))
    _, info = st.read()
    part = host(st.partials(n))
    got = part[:, 2:].sum(axis=0) / n
    flat = np.concatenate([np.ravel(v) for v in q["grads"]])
    flat_abs = np.concatenate([np.ravel(v) for v in q["grads_abs"]])
    assert np.isnan(info[5]) and np.isnan(q["loss"])
    assert info[4] == np.inf and info[3] == 9                               # no best loss, patience counted down
    assert np.array_equal(np.isnan(got), np.isnan(flat)) and np.isnan(flat[-1]) and np.isfinite(flat[0])
    fin = np.isfinite(flat) & np.isfinite(flat_abs)
    assert within(got[fin], flat[fin], flat_abs[fin])
    assert part[:, 1].sum() == q["correct"]
    assert np.isfinite(part[1]).all()                                       # the NaN stays in its chunk's partial


def test_state_bits_do_not_depend_on_the_grid():
    n, C, hid, F = 4097, 41, 16, 4
    rng = np.random.default_rng(5)
    H = rng.standard_normal((n, F)).astype(np.float32)
    z, y, params = make_logits(n, C, 1.0, 5), rng.integers(0, C, n), make_head(hid, F, 5)
    Ht, zt, yt = dev(H), dev(z), dev(y, torch.int64)
    blocks = []
    for g in (1, 2, 7, 0):
        st = new_state(H, z, None, params)
        for _ in range(3):
            st.epoch(Ht, zt, None, yt, g)
        blocks.append(st.block.clone())
    assert blocks[0][2].item() == 3
    for b in blocks[1:]:
        assert torch.equal(b.view(torch.int64), blocks[0].view(torch.int64))


# ------------------------------------------------------------------------------------------ training, fixtures
_cases = {}


def case(name):
    if name not in _cases:
        d, meta = R.load_case(name)
        z64 = SR.base_logits(R.case_base(d), d["x"], d["adj"])
        _cases[name] = dict(d=d, meta=meta, z64=z64, rows=R.case_rows(d),
                            run=R.train(d["wavelet_feats"], z64, d["y"], R.case_rows(d), R.case_init(d)))
    return _cases[name]


def base_of(c, dropout=0.0):
    P = R.case_base(c["d"])
    base = wats_hip.SparseCompatibleGCN(c["d"]["x"].shape[1], nclass=P["gc2.weight"].shape[0],
                                        nhid=P["gc1.weight"].shape[0], dropout=dropout)
    base.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    return base.to(DEV).eval()


def tensors(c):
    d = c["d"]
    return (torch.from_numpy(d["x"]).to(DEV), torch.from_numpy(d["y"]).to(DEV), torch.from_numpy(d["adj"]).to(DEV),
            torch.from_numpy(d["val"]).to(DEV))


def build(c, load_init=True, dropout=0.0, **kw):
    kw.setdefault("verbose", False)
    kw.setdefault("fused_training", True)
    model = wats_hip.WATS(base_of(c, dropout), *tensors(c), train=False, **kw)
    if load_init:
        model.net.load_state_dict({k: torch.from_numpy(c["d"]["init__net." + k]) for k in
                                   ("0.weight", "0.bias", "2.weight", "2.bias")})
    return model.calib_train()


@pytest.mark.parametrize("name", R.CASES)
def test_training_on_the_fixtures(name):
    """Measured on the MI355X: recorded per case under "measured" in the manifest."""
    c = case(name)
    d, f, want = c["d"], c["meta"]["f32_vs_f64"], c["run"]
    model = build(c, frozen_logits=True)
    run = model.training_run
    assert not model.training and not model.base_model.training
    assert run.epochs_run == want["epochs_run"] == int(d["epochs"])
    assert run.stop_epoch == want["stop_epoch"] and (run.stop_epoch if run.stop_epoch is not None else -1) == int(d["stop"])
    d_loss = R.dist(run.loss, want["loss"])
    d_par = max(R.dist(host(a).reshape(b.shape), b) for a, b in zip(run.params, want["params"]))
    with torch.no_grad():
        out = model(*tensors(c)[::2])
    d_out = R.dist(host(out), d["out"])
    print(f"{name}: loss distance {d_loss:.3e} (allowed {f['loss']:.3e}), parameters {d_par:.3e} (allowed "
          f"{f['params']:.3e}), eval output to the fixture {d_out:.3e} (allowed {4 * f['out']:.3e})")
    assert np.array_equal(run.acc, want["acc"])
    assert d_loss <= f["loss"]
    assert d_par <= f["params"]
    for p, v in zip(model.net.parameters(), run.params):                  # copied into the module
        assert torch.equal(p.detach(), v.reshape(p.shape))
    measured = R.load_manifest().get("measured", {}).get("out", {})
    assert name in measured, "record the device run's distance in the manifest (tests/golden/wats_train/manifest.json)"
    assert d_out <= 4 * f["out"]


def test_training_with_wide_features_follows_the_restatement():
    """F = 4, generic H, a callable sequence of logits: 30 epochs against the restatement"""
    n, C, hid, F = 300, 7, 16, 4
    rng = np.random.default_rng(11)
    H = rng.standard_normal((n, F)).astype(np.float32)
    y = rng.integers(0, C, n)
    rows = rng.permutation(n)[:120]
    base = make_logits(n, C, 2.0, 11)
    seq = [base + np.random.default_rng(100 + e).standard_normal(base.shape).astype(np.float32) * 0.3 for e in range(30)]
    net = torch.nn.Sequential(torch.nn.Linear(F, hid), torch.nn.ReLU(), torch.nn.Linear(hid, 1)).to(DEV)
    before = [p.detach().clone() for p in net.parameters()]
    init = [host(p) for p in net.parameters()]
    want = R.train(H, lambda e: seq[e], y, rows, init, epochs=30, patience=30)
    run = wats_hip.train_wats_head(dev(H), lambda e: dev(seq[e]), torch.from_numpy(y), torch.from_numpy(rows), net,
                                   epochs=30, patience=30)
    assert run.epochs_run == want["epochs_run"] == 30 and run.stop_epoch is None
    assert np.allclose(run.loss, want["loss"], rtol=1e-9, atol=1e-12)
    assert np.array_equal(run.acc, want["acc"])
    for a, b in zip(run.params, want["params"]):
        assert np.all(np.abs(host(a).reshape(b.shape) - b) <= 2 * R.EPS32 * np.abs(b) + 1e-9)
    for p, q in zip(net.parameters(), before):                              # net is not written
        assert torch.equal(p.detach(), q)


def test_patience_runs_out_at_a_known_epoch():
    """Two phases: the logits agree with the labels ever more sharply for 12 epochs, then turn to noise.  The loss
    falls by far more than 1e-3 per epoch, then sits far above the best: patience 5 runs out in epoch 16."""
    n, C, hid, F = 300, 7, 16, 4
    rng = np.random.default_rng(12)
    H = rng.standard_normal((n, F)).astype(np.float32)
    good = rng.standard_normal((n, C)).astype(np.float32)
    y = good.argmax(axis=1)
    noise = rng.standard_normal((n, C)).astype(np.float32)
    seq = [good * np.float32(0.5 + 0.25 * e) if e < 12 else noise for e in range(40)]
    rows = np.sort(rng.permutation(n)[:150])
    init = make_head(hid, F, 12)
    net = torch.nn.Sequential(torch.nn.Linear(F, hid), torch.nn.ReLU(), torch.nn.Linear(hid, 1))
    net.load_state_dict({"0.weight": torch.from_numpy(init[0]), "0.bias": torch.from_numpy(init[1]),
                         "2.weight": torch.from_numpy(init[2].reshape(1, hid)), "2.bias": torch.from_numpy(init[3])})
    want = R.train(H, lambda e: seq[e], y, rows, init, epochs=40, patience=5)
    gap, stop = R.stop_gaps(want["loss"], patience=5)
    assert gap > 1e-3 and stop == want["stop_epoch"] == 16
    calls = []

    def logits(e):
        calls.append(e)
        return dev(seq[e])
    run = wats_hip.train_wats_head(dev(H), logits, torch.from_numpy(y), torch.from_numpy(rows), net, epochs=40,
                                   patience=5)
    assert run.epochs_run == 17 and run.stop_epoch == 16 and run.patience_left == 0
    assert len(calls) == 20                                                 # the host looked after 10 and 20 epochs
    assert np.allclose(run.loss, want["loss"], rtol=1e-9, atol=1e-12)
    assert abs(run.best_loss - want["best_loss"]) <= 1e-9 * want["best_loss"]


def test_both_training_modes_agree_bitwise_without_dropout():
    c = case("stop120")
    a, b = build(c, frozen_logits=True), build(c, frozen_logits=False)
    assert a.training_run.epochs_run == b.training_run.epochs_run == int(c["d"]["epochs"])
    assert np.array_equal(a.training_run.loss, b.training_run.loss)
    for p, q in zip(a.training_run.params, b.training_run.params):
        assert torch.equal(p, q)
    assert not b.training and not b.base_model.training                     # the module ends in eval mode


def test_live_dropout_reaches_the_logits_in_the_default_mode():
    """WATS.py:147: self.train() puts the base model into train mode, so p > 0 changes the epochs' logits"""
    c = case("stop120")
    torch.manual_seed(0)
    live = build(c, dropout=0.5, epochs=12)
    frozen = build(c, dropout=0.5, epochs=12, frozen_logits=True)
    assert live.training_run.epochs_run == frozen.training_run.epochs_run == 12
    assert not np.array_equal(live.training_run.loss, frozen.training_run.loss)
    assert R.dist(frozen.training_run.loss, c["run"]["loss"][:12]) <= c["meta"]["f32_vs_f64"]["loss"]


def test_the_torch_loop_is_unchanged_by_the_extras(capsys):
    c = case("stop120")
    models = []
    for kw in (dict(), dict(fused_training=False, frozen_logits=False, epochs=250, train=True)):
        torch.manual_seed(3)
        models.append(wats_hip.WATS(base_of(c), *tensors(c), verbose=False, **kw))
    torch.manual_seed(3)
    late = wats_hip.WATS(base_of(c), *tensors(c), verbose=False, train=False)
    assert not hasattr(late, "training_run")
    late.calib_train()
    for other in (models[1], late):
        for (ka, va), (kb, vb) in zip(models[0].state_dict().items(), other.state_dict().items()):
            assert ka == kb and torch.equal(va, vb), ka
    assert not hasattr(models[0], "training_run")
    torch.manual_seed(3)
    short = wats_hip.WATS(base_of(c), *tensors(c), verbose=True, epochs=2)
    text = capsys.readouterr().out
    assert "epoch: 1 " in text and "epoch: 2 " not in text and short is not None


def test_verbose_prints_the_references_lines_after_the_run(capsys):
    c = case("stop120")
    model = build(c, frozen_logits=True, verbose=True)
    text = capsys.readouterr().out
    stop = int(c["d"]["stop"])
    assert f"epoch: {stop} loss_calibration: " in text and f"Early stopping at epoch {stop}, best loss: " in text
    assert text.count("loss_calibration") == model.training_run.epochs_run


# ------------------------------------------------------------------------------------------------------ the state
def fixture_problem(name="stop120"):
    c = case(name)
    d = c["d"]
    z = dev(c["z64"].astype(np.float32))
    rows = S._row_list(torch.from_numpy(d["val"]), z.shape[0], DEV)
    return c, dev(d["wavelet_feats"]), z, rows, dev(d["y"], torch.int64), [np.asarray(p, np.float32) for p in R.case_init(d)]


def test_launches_past_stopped_leave_the_state_alone():
    c, H, z, rows, y, init = fixture_problem()
    for epochs in (250, 5):                                                 # out of patience; out of epochs
        st = HD._HeadTrainingState(H.shape[1], 16, z.shape[1], epochs, rows.numel(), 10, torch.device(DEV, 0),
                                   [dev(p) for p in init], R.LR, R.WD)
        for _ in range(epochs):
            st.epoch(H, z, rows, y)
        assert st.stopped() and st.block[1].item() == (1 if epochs == 250 else 2)
        before = st.block.clone()
        for g in (0, 1, 3):
            st.epoch(H, z, rows, y, g)
        torch.cuda.synchronize()
        assert torch.equal(before.view(torch.int64), st.block.view(torch.int64))


def test_a_nan_row_stops_the_run_after_patience_epochs():
    c, H, z, rows, y, init = fixture_problem()
    zn = z.clone()
    zn[int(rows[3]), 1] = float("nan")
    net = torch.nn.Sequential(torch.nn.Linear(H.shape[1], 16), torch.nn.ReLU(), torch.nn.Linear(16, 1))
    run = wats_hip.train_wats_head(H, zn, y, rows, net, patience=7)
    assert run.epochs_run == 7 and run.stop_epoch == 6 and run.patience_left == 0
    assert np.all(np.isnan(run.loss)) and run.best_loss == np.inf
    clean = wats_hip.train_wats_head(H, z, y, rows, net, patience=7, epochs=7)
    assert clean.epochs_run == 7 and np.all(np.isfinite(clean.loss))


def test_limits_and_bad_arguments():
    c, H, z, rows, y, init = fixture_problem()
    net = torch.nn.Sequential(torch.nn.Linear(H.shape[1], 16), torch.nn.ReLU(), torch.nn.Linear(16, 1))
    with pytest.raises(IndexError):
        wats_hip.train_wats_head(H, z, torch.full_like(y, z.shape[1]), rows, net)
    with pytest.raises(IndexError):
        wats_hip.train_wats_head(H, z, y, torch.tensor([z.shape[0]]), net)
    with pytest.raises(ValueError):
        wats_hip.train_wats_head(H[:-1], z, y, rows, net)
    with pytest.raises(ValueError):
        wats_hip.train_wats_head(torch.cat([H, H], dim=1), z, y, rows, net)
    wide = torch.nn.Sequential(torch.nn.Linear(30, 64), torch.nn.ReLU(), torch.nn.Linear(64, 1))
    with pytest.raises(NotImplementedError):
        wats_hip.train_wats_head(torch.zeros(z.shape[0], 30, device=DEV), z, y, rows, wide)
    with pytest.raises(NotImplementedError):
        wats_hip.train_wats_head(H, torch.zeros(z.shape[0], 257, device=DEV), y, rows, net)


# ---------------------------------------------------------------------------------------------- streams, capture
def test_captured_epochs_replay_as_further_epochs():
    """Five epoch launches captured on a side stream: a replay after state_init gives the block bits of five eager
    launches on the default stream, a second replay those of ten.  Three chunks, so the arrival counter is used."""
    n, C, hid, F = 700, 7, 16, 4
    rng = np.random.default_rng(13)
    H = rng.standard_normal((n, F)).astype(np.float32)
    z, y, params = make_logits(n, C, 1.0, 13), rng.integers(0, C, n), make_head(hid, F, 13)
    Ht, zt, yt = dev(H), dev(z), dev(y, torch.int64)
    eager = new_state(H, z, None, params, epochs=12, patience=100)
    want = {}
    for e in range(1, 11):
        eager.epoch(Ht, zt, None, yt)
        if e in (5, 10):
            want[e] = eager.block.clone()
    torch.cuda.synchronize()
    assert want[5][2].item() == 5 and want[10][2].item() == 10
    assert not torch.equal(want[5].view(torch.int64), want[10].view(torch.int64))

    st = new_state(H, z, None, params, epochs=12, patience=100)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        st.epoch(Ht, zt, None, yt)                       # warm
        with torch.cuda.graph(graph, stream=side):
            for _ in range(5):
                st.epoch(Ht, zt, None, yt)
    torch.cuda.synchronize()
    st.reset()                                           # eager, on the default stream
    torch.cuda.synchronize()
    for e in (5, 10):
        with torch.cuda.stream(side):
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(st.block.view(torch.int64), want[e].view(torch.int64)), f"after {e} replayed epochs"
    # state_init and state_read on the side stream: ordered behind the epochs there
    with torch.cuda.stream(side):
        st.reset()
        graph.replay()
        _, info = st.read()
    assert info[1] == 5 and np.array_equal(info[5:10], host(want[5])[16 + 3 * st.n_params:][:5])
