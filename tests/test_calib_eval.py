"""GPU tests of the evaluation step: csrc/calib.hip (wg_calib_bins, wg_calib_ece) against the numpy model of its
documented arithmetic (tests/calib_eval_ref.py), oracle/ece_oracle.py and the reference's fixtures
(tests/golden/evaluation), and the functions of wats_hip/metrics.py built on it.

Bounds.
* table: the model's integers, exactly; the same bits for n_workgroups 1, 2, 7, 0 and across two runs.
* float64 scalars: within n_rows * 2^-52 of the sum of the absolute terms of the np.longdouble truth (a tree or
  sequential float64 sum, plus a few ulps of exp / log); counts are exact.  Bit-equal across grids.
* ece_class / ece_top: within 2^-40 of ece_oracle on float64 copies of the float32 p (at most 2^-41 of quantisation
  per bin mean, the weights sum to at most 1, plus float64 rounding).
* fixtures: within the fixture's f32_vs_f64 plus 2^-40.
* kind="exp" / "logits" inputs come from calib_eval_ref.gpu_logits, whose seeds tests/test_calib_eval_host.py holds
  free of fragile elements, so their tables are compared exactly too.
"""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import calib_eval_ref as R  # noqa: E402
import scaling_ref  # noqa: E402
import wats_hip  # noqa: E402
from oracle import ece_oracle as O  # noqa: E402
from wats_hip import _lib  # noqa: E402
from wats_hip import metrics as M  # noqa: E402

DEV = "cuda"
FIX = 2.0 ** -40
CASES = R.load_fixture_cases()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = _lib.load()
    assert lib.wg_calib_chunk_rows() == 256 and R.GPU_ROWS == 2 * 256 + 1
    assert lib.wg_calib_max_rows() == 1 << 23 and lib.wg_calib_max_classes() == 256 and lib.wg_calib_max_bins() == 64


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def launch(out, labels, rows, kind, n_bins, n_workgroups=0, min_count=4):
    """Both entries on buffers prefilled with 0xFF; out (G, n, C).  Returns table, scalars, ece_class, ece_top."""
    lib = _lib.load()
    out = np.asarray(out, np.float32)
    G, n, C = out.shape
    idx = None if rows is None else R.row_list(rows, n)
    n_rows = n if idx is None else len(idx)
    d_out, d_lab = dev(out, torch.float32), dev(labels, torch.int64)
    d_rows = None if idx is None else dev(idx, torch.int64)
    d_edges = dev(np.linspace(0, 1, n_bins + 1), torch.float64)
    cells = (C + 1) * (n_bins + 2) * 3
    nbytes = ctypes.c_int64(0)
    _lib.check(lib.wg_calib_workspace(G, C, n_bins, n_rows, ctypes.byref(nbytes)))
    ff = lambda k: torch.full((max(1, k),), -1, dtype=torch.int64, device=DEV)   # noqa: E731  (0xFF bytes)
    ws, table, scal, ec, et = ff(nbytes.value // 8), ff(G * cells), ff(G * 8), ff(G * C), ff(G)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.wg_calib_bins(G, n, C, M.KINDS[kind], d_out.data_ptr(), d_lab.data_ptr(), n_rows,
                                 None if d_rows is None else d_rows.data_ptr(), n_bins, d_edges.data_ptr(), n_workgroups,
                                 ws.data_ptr(), table.data_ptr(), scal.data_ptr(), stream), "calib_bins")
    _lib.check(lib.wg_calib_ece(G, C, n_bins, n_rows, min_count, table.data_ptr(), ec.data_ptr(), et.data_ptr(), stream),
               "calib_ece")
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device error: nothing more may start on this GPU in this session
        pytest.exit(f"device error after wg_calib_bins / wg_calib_ece: {e}", returncode=3)
    host = lambda t, k: t.cpu().numpy()[:k]   # noqa: E731
    return (host(table, G * cells).view(np.uint64).reshape(G, C + 1, n_bins + 2, 3),
            host(scal, G * 8).view(np.float64).reshape(G, 8), host(ec, G * C).view(np.float64).reshape(G, C),
            host(et, G).view(np.float64).reshape(G))


def special_probs(C, seed, n=R.GPU_ROWS):
    """float32 probabilities with every special value: each edge of 10 / 15 / 64 bins and one ulp either side, 0, 1,
    p > 1, negative p, NaN and +-inf rows; labels include -1 and C"""
    rng = np.random.default_rng(100 + seed)
    z = rng.standard_normal((n, C)) * 2.0
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    e = np.unique(np.concatenate([np.linspace(0, 1, b + 1) for b in (10, 15, 64)])).astype(np.float32)
    vals = np.unique(np.concatenate([e, np.nextafter(e, np.float32(2)), np.nextafter(e, np.float32(-1)),
                                     np.float32([1.5, 7.5, -0.25, 2.0 ** -17, 1e-30, 1e-45])]))
    where = rng.permutation(n * C)[:len(vals)] if n * C >= 4 * len(vals) else np.arange(0)
    p.reshape(-1)[where] = vals[:len(where)]
    if n >= 64:
        p[5, :] = np.nan
        p[17, C // 2] = np.nan
        p[23, 0] = np.inf
        p[29, C - 1] = -np.inf
        p[31, :] = 0.0
        p[37, :] = 0.0
        p[37, C - 1] = 1.0
        p[41, :] = np.float32(1.0 / 3)       # a tie: the first column is the top label
    y = rng.integers(0, C, n)
    y[::50] = -1
    y[7::50] = C
    return p, y


def row_forms(n, seed):
    rng = np.random.default_rng(200 + seed)
    idx = rng.permutation(n)[:max(1, (2 * n) // 3)]
    if len(idx) > 4:
        idx[4] = idx[1]
    return {"none": None, "mask": rng.random(n) < 0.6, "index": idx}


def check_against_model(out, labels, rows, kind, n_bins, what):
    """One launch of G sets against the model: table exactly, scalars within the float64 bound, ECE against the
    oracle.  Returns the launch's outputs."""
    table, scal, ec, et = launch(out, labels, rows, kind, n_bins)
    for g in range(out.shape[0]):
        p = R.probabilities(out[g], kind)
        idx = R.row_list(rows, out.shape[1])
        n_rows = len(idx)
        assert np.array_equal(table[g], R.bin_table(p, labels, idx, n_bins)), f"{what} set {g}: table"
        val, mag = R.scalar_truth(out[g], labels, idx, kind)
        err = np.abs(scal[g, :7].astype(R.LD) - val)
        bound = n_rows * R.LD(2.0 ** -52) * mag
        print(f"{what} set {g}: scalars err {[float(e) for e in err]} bound {[float(b) for b in bound]}")
        assert np.all(err <= bound), f"{what} set {g}: scalars {scal[g]} against {val}"
        assert scal[g, 7] == 0
        p64, y = p[idx].astype(np.float64), np.asarray(labels)[idx]
        if n_rows:
            want = np.array([O.calculate_ece(p64, y, c, logits=False, n_bins=n_bins) for c in range(out.shape[2])])
            assert np.max(np.abs(ec[g] - want)) <= FIX, f"{what} set {g}: ece_class"
            with np.errstate(all="ignore"):
                top = np.max(p64, axis=1)
            hit = (np.argmax(p[idx], axis=1) == y).astype(np.int64)
            want_top = O.calculate_ece(top[:, None], 1 - hit, 0, logits=False, n_bins=n_bins)
            assert abs(et[g] - want_top) <= FIX, f"{what} set {g}: ece_top"
        else:
            assert not ec[g].any() and et[g] == 0
    return table, scal, ec, et


# C with the bin count it runs at: every width and every bin count, both sides of the LDS limit
# ((C + 1) (n_bins + 2) 3 <= 5120 words: 40 / 64 bins, 65 / 15 bins and 256 / any go to the global table)
SHAPES = [(1, 1), (2, 10), (7, 64), (40, 10), (40, 64), (41, 15), (64, 15), (65, 15), (65, 64), (256, 1), (256, 10)]


@pytest.mark.parametrize("C,n_bins", SHAPES)
def test_probs_table_scalars_and_ece(C, n_bins):
    p, y = special_probs(C, seed=C + n_bins)
    forms = row_forms(len(p), C)
    for name, rows in forms.items():
        check_against_model(p[None], y, rows, "probs", n_bins, f"C={C} bins={n_bins} rows={name}")


@pytest.mark.parametrize("kind", ["exp", "logits"])
@pytest.mark.parametrize("C,n_bins", [(1, 10), (2, 1), (7, 15), (40, 10), (41, 64), (64, 10), (65, 10), (256, 15)])
def test_exp_and_logits_table_scalars_and_ece(kind, C, n_bins):
    z = R.gpu_logits(C, R.GPU_SEEDS[0])
    y = np.random.default_rng(C).integers(-1, C + 1, len(z))
    rows = row_forms(len(z), C)["index" if C % 2 else "mask"]
    check_against_model(z[None], y, rows, kind, n_bins, f"{kind} C={C} bins={n_bins}")


@pytest.mark.parametrize("kind", ["probs", "exp", "logits"])
def test_nonfinite_rows_of_every_kind(kind):
    C = 7
    z = R.gpu_logits(C, R.GPU_SEEDS[1]) if kind != "probs" else special_probs(C, 3)[0]
    z = z.copy()
    z[3, 2] = np.nan
    z[9, :] = np.inf
    z[11, 1] = -np.inf
    z[13, 4] = np.inf
    y = np.random.default_rng(1).integers(0, C, len(z))
    _, scal, _, _ = check_against_model(z[None], y, None, kind, 10, f"nonfinite {kind}")
    assert scal[0, 0] == len(z) and scal[0, 1] < scal[0, 0]


@pytest.mark.parametrize("n_rows", [0, 1, 3, 4, 255, 256, 257, 513])
def test_row_counts_around_the_chunk(n_rows):
    C = 7
    for kind, data in (("probs", special_probs(C, 9)[0]), ("logits", R.gpu_logits(C, R.GPU_SEEDS[2]))):
        y = np.random.default_rng(n_rows).integers(0, C, len(data))
        rows = np.random.default_rng(n_rows + 1).permutation(len(data))[:n_rows]
        check_against_model(data[None], y, rows, kind, 10, f"{kind} n_rows={n_rows}")
        check_against_model(data[None, :n_rows], y[:n_rows], None, kind, 10, f"{kind} n={n_rows}, no list")


@pytest.mark.parametrize("G", [1, 2, 3])
def test_sets_share_labels_and_rows(G):
    C = 41
    out = np.stack([R.gpu_logits(C, s) for s in R.GPU_SEEDS[:G]])
    y = np.random.default_rng(G).integers(0, C, out.shape[1])
    rows = row_forms(out.shape[1], G)["index"]
    for kind in ("exp", "logits"):
        table, scal, ec, et = check_against_model(out, y, rows, kind, 15, f"G={G} {kind}")
        one = launch(out[G - 1:], y, rows, kind, 15)
        assert np.array_equal(table[G - 1], one[0][0]) and np.array_equal(scal[G - 1].view(np.uint64),
                                                                          one[1][0].view(np.uint64))


@pytest.mark.parametrize("kind,C,n_bins", [("probs", 40, 10), ("logits", 65, 64), ("exp", 256, 10)])
def test_bits_do_not_depend_on_the_grid_or_the_run(kind, C, n_bins):
    data = special_probs(C, 4)[0] if kind == "probs" else R.gpu_logits(C, R.GPU_SEEDS[0])
    y = np.random.default_rng(0).integers(0, C, len(data))
    rows = row_forms(len(data), 1)["index"]
    runs = [launch(np.stack([data, data[::-1]]), y, rows, kind, n_bins, n_workgroups=g) for g in (1, 2, 7, 0, 0)]
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_refused_rows_are_counted_not_read():
    C = 7
    p, y = special_probs(C, 2, n=64)
    rows = np.array([0, 5, 64, -1, 63, 1 << 40])
    table, scal, _, _ = launch(p[None], y, rows, "probs", 10)
    assert scal[0, 0] == 3 and scal[0, 7] == 3
    assert np.array_equal(table[0], R.bin_table(p, y, np.array([0, 5, 63]), 10))
    with pytest.raises(IndexError):
        wats_hip.calibration_report(dev(p, torch.float32), dev(y, torch.int64), rows=dev(rows, torch.int64))


def test_bad_arguments_raise():
    p, y = special_probs(7, 1, n=64)
    dp, dy = dev(p, torch.float32), dev(y, torch.int64)
    rep = wats_hip.calibration_report
    with pytest.raises(ValueError):
        rep(dp[0], dy)                                            # outputs not 2-D / 3-D
    with pytest.raises(ValueError):
        rep(dp, dy[:-1])                                          # labels of another length
    with pytest.raises(ValueError):
        rep(dp, dy.float())
    with pytest.raises(ValueError):
        rep(dp, dy, rows=torch.ones(63, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        rep(dp, dy, rows=torch.zeros(4, device=DEV))              # a float index
    with pytest.raises(ValueError):
        rep(dp, dy, kind="softmax")
    with pytest.raises(ValueError):
        rep(dp, dy, n_classes=8)
    with pytest.raises(ValueError):
        rep([dp, dp[:, :3]], dy)
    with pytest.raises(wats_hip.WaveletError):
        rep(dp, dy, n_bins=65)
    with pytest.raises(wats_hip.WaveletError):
        rep(dp, dy, n_bins=0)
    with pytest.raises(wats_hip.WaveletError):
        rep(torch.zeros((4, 257), device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV))
    with pytest.raises(wats_hip.WaveletError):                    # n_rows above 2^23: refused before any device call
        rep(dp, dy, rows=torch.zeros((1 << 23) + 1, dtype=torch.int64, device=DEV))
    lib = _lib.load()
    nbytes = ctypes.c_int64(0)
    assert lib.wg_calib_workspace(1, 7, 10, (1 << 23) + 1, ctypes.byref(nbytes)) != 0
    assert lib.wg_calib_bins(1, 64, 7, 3, dp.data_ptr(), dy.data_ptr(), 64, None, 10, dp.data_ptr(), 0, dp.data_ptr(),
                             dp.data_ptr(), dp.data_ptr(), None) != 0          # kind 3
    assert lib.wg_calib_bins(1, 64, 7, 0, dp.data_ptr(), dy.data_ptr(), 32, None, 10, dp.data_ptr(), 0, dp.data_ptr(),
                             dp.data_ptr(), dp.data_ptr(), None) != 0          # no list, but n_rows != n
    assert lib.wg_calib_bins(1, 64, 7, 0, dp.data_ptr(), dy.data_ptr(), 64, None, 10, dp.data_ptr(), 1025,
                             dp.data_ptr(), dp.data_ptr(), dp.data_ptr(), None) != 0          # n_workgroups
    assert lib.wg_calib_bins(1, 64, 7, 0, dp.data_ptr(), dy.data_ptr(), 64, None, 10, dp.data_ptr(), 0, None,
                             dp.data_ptr(), dp.data_ptr(), None) != 0          # no workspace
    assert lib.wg_calib_bins(0, 64, 7, 0, None, None, 64, None, 10, None, 0, None, None, None, None) == 0   # G == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_fixtures(name):
    """The reference's own triple, per-class ECE and sklearn's curves, through the public functions."""
    c = CASES[name]
    f = c["f32_vs_f64"]
    out, y, rows = dev(c["outputs"], torch.float32), dev(c["labels"], torch.int64), torch.from_numpy(c["rows"]).to(DEV)
    acc, conf, ece = c["triple"]
    with contextlib.redirect_stdout(io.StringIO()) as log:
        if c["kind"] == "exp":
            got = wats_hip.evaluate_calibration(lambda x, adj: out, None, y, None, rows, name)
        else:
            got = wats_hip.evaluate_calibration_probs(out, y, rows, name)
    print(name, "acc", abs(got[0] - acc), "conf", abs(got[1] - conf), "ece", abs(got[2] - ece), "allowed", f)
    assert log.getvalue().splitlines() == c["printed"]
    assert abs(got[0] - acc) <= f["acc"] + FIX
    assert abs(got[1] - conf) <= f["conf"] + FIX
    assert abs(got[2] - ece) <= f["ece"] + FIX
    r = wats_hip.calibration_report(out, y, rows=rows, kind=c["kind"], n_bins=c["n_bins"])
    assert r.n == c["n"] and r.nonfinite_rows == 0
    assert np.max(np.abs(r.ece_per_class - c["per_class"])) <= f["per_class"] + FIX
    sub, ysub = out[rows], y[rows]
    if c["curves"]:
        curves = wats_hip.reliability_curves(sub, ysub, c["C"], n_bins=c["n_bins"], kind=c["kind"])
        for (t, q), (t_ref, q_ref) in zip(curves, R.unflatten_curves(c)):
            assert t.shape == t_ref.shape
            assert np.max(np.abs(t - t_ref), initial=0) <= f["curves"] + FIX
            assert np.max(np.abs(q - q_ref), initial=0) <= f["curves"] + FIX
    else:
        assert r.outside > 0
        with pytest.raises(ValueError):
            wats_hip.reliability_curves(sub, ysub, c["C"], n_bins=c["n_bins"], kind=c["kind"])


def test_report_against_the_existing_torch_path_and_many_sets():
    C, n = 40, 3000
    rng = np.random.default_rng(8)
    y = dev(rng.integers(0, C, n), torch.int64)
    mask = dev(rng.random(n) < 0.3, torch.bool)
    sets = [torch.softmax(dev(rng.standard_normal((n, C)) * s, torch.float32), dim=1) for s in (1.0, 3.0)]
    old = [M.calculate_average_ece(p[mask], y[mask], C, logits=False) for p in sets]
    reports = wats_hip.calibration_report(sets, y, rows=mask)
    for r, o in zip(reports, old):
        assert abs(r.ece - o) <= 1e-12
        assert r.n == int(mask.sum()) and r.counts.shape == (C + 1, 10)
        assert int(r.counts[C].sum()) == r.n and 0.0 <= r.brier <= 2.0 and r.nll > 0
    assert wats_hip.calibration_report(torch.stack(sets), y, rows=mask)[1].ece == reports[1].ece
    assert wats_hip.calibration_report(sets[0], y, rows=mask).ece == reports[0].ece
    many = wats_hip.average_ece_many([p[mask] for p in sets], y[mask], C)
    assert many == [r.ece for r in reports]
    few = wats_hip.calibration_report(sets[0], y, rows=mask, n_classes=5)
    assert abs(few.ece - M.calculate_average_ece(sets[0][mask], y[mask], 5, logits=False)) <= 1e-12
    # 15 bins, an index list with a repeat
    idx = dev(np.array([5, 1, 1, 900, 17] * 40), torch.int64)
    r15 = wats_hip.calibration_report(sets[1], y, rows=idx, n_bins=15)
    assert abs(r15.ece - M.calculate_average_ece(sets[1][idx], y[idx], C, logits=False, n_bins=15)) <= 1e-12


def test_drop_in_over_a_calibrator_equals_the_report_of_its_output():
    d, _, _ = scaling_ref.load_case("plain120")
    P = scaling_ref.case_base(d)
    base = wats_hip.SparseCompatibleGCN(d["x"].shape[1], nclass=P["gc2.weight"].shape[0],
                                        nhid=P["gc1.weight"].shape[0], dropout=0.0)
    base.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    base = base.to(DEV).eval()
    x, y, adj = (torch.from_numpy(d[k]).to(DEV) for k in ("x", "y", "adj"))
    val = torch.from_numpy(d["val"]).to(DEV)
    test_mask = ~torch.from_numpy(d["val_mask"]).to(DEV)
    ts = wats_hip.TemperatureScaling(base_model=base, x=x, y=y, adj=adj, val_idx=val, verbose=False, epochs=5)
    with contextlib.redirect_stdout(io.StringIO()) as log:
        acc, conf, ece = wats_hip.evaluate_calibration(ts, x, y, adj, test_mask, "TS")
    assert log.getvalue().splitlines()[0] == "TS Results:" and len(log.getvalue().splitlines()) == 4
    ts.eval()
    with torch.no_grad():
        out = ts(x, adj)
    r = wats_hip.calibration_report(out, y, rows=test_mask, kind="exp")
    assert (acc, conf, ece) == (r.accuracy, r.avg_confidence, r.ece)
    # its output is log-probabilities: exp of them and the softmax of them agree up to float32 rounding of p
    quiet = wats_hip.evaluate_calibration(ts, x, y, adj, test_mask, verbose=False, kind="logits")
    assert abs(quiet[2] - ece) <= 1e-6 and quiet[0] == acc
    # the base model returns raw logits: the reference's exp misreads them, kind="logits" scores them
    raw = wats_hip.evaluate_calibration(base, x, y, adj, test_mask, verbose=False)
    good = wats_hip.evaluate_calibration(base, x, y, adj, test_mask, verbose=False, kind="logits")
    assert raw[0] == good[0] and 0.0 < good[1] <= 1.0 and raw[1] != good[1]
