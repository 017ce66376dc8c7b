"""GPU tests of the SimCalib similarity temperature (csrc/simcalib.hip, wats_hip/simcalib.py) against the dense
restatement of tests/simcalib_ref.py.

The bound on every value is measured in the test, as in tests/test_gats.py: err = max|kernel - ref64| must not
exceed max(2 * max|ref32 - ref64|, 4 * 2^-24 * max|ref64|) (gats_ref.error_bound), where ref32 / ref64 are the
restatement on the CPU in float32 / float64 from the same float32 inputs.  Both float32 paths carry the same 1 / tau
amplification of the similarities' rounding, so the factor needs no tau term.  For the calibrator the fixture that
the reference recorded is the float32 side, and the float64 side is the restatement from the fixture's inputs.
"""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import gats_ref  # noqa: E402
import simcalib_ref as R  # noqa: E402
import wats_hip  # noqa: E402
from models import CompatibleGCN  # noqa: E402
from wats_hip import simcalib  # noqa: E402

DEV = "cuda"
BIG = 1e30     # a clamp that never acts
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simcalib")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


NS, MS, DS = [1, 31, 129, 300], [1, 15, 33, 257], [1, 3, 16, 64, 65, 256]
LARGEST = (300, 257, 256)


def pairwise_cover():
    """A subset of NS x MS x DS (the largest shape, then product order) that holds every value pair of every two
    dimensions."""
    seen, out = set(), []
    for n, m, d in [LARGEST] + list(itertools.product(NS, MS, DS)):
        pairs = {("nm", n, m), ("nd", n, d), ("md", m, d)}
        if not pairs <= seen:
            seen |= pairs
            out.append((n, m, d))
    return out


SHAPES = pairwise_cover()


def make_inputs(n, m, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g).float()
    bank = F.normalize(torch.randn(m, d, generator=g).float(), p=2, dim=1)
    v = 1.0 / (0.1 + 0.9 * torch.rand(m, generator=g).float() + 1e-8)
    gt = torch.randn(n, generator=g).float()
    return x, bank, v, gt


def kernel(x, bank, v, gt, tau, t_min=-BIG, t_max=BIG):
    """(t, grad of sum(gt * t) w.r.t. x) of the HIP path."""
    xd = x.to(DEV).requires_grad_(True)
    t = wats_hip.similarity_temperature(xd, bank.to(DEV), v.to(DEV), tau, t_min, t_max)
    (t * gt.to(DEV)).sum().backward()
    return t.detach(), xd.grad


def references(x, bank, v, gt, tau, t_min=-BIG, t_max=BIG):
    r32 = R.temperature_and_grad(x, bank, v, gt, tau, t_min, t_max, torch.float32)
    r64 = R.temperature_and_grad(x, bank, v, gt, tau, t_min, t_max, torch.float64)
    return r32, r64


def check(x, bank, v, gt, tau, what, rows=None):
    """Forward and backward within the measured bound; ``rows``: compare these rows only (t and gx)."""
    (_, t32, g32), (_, t64, g64) = references(x, bank, v, gt, tau)
    t, gx = kernel(x, bank, v, gt, tau)
    sel = slice(None) if rows is None else rows
    gats_ref.assert_close(t[sel], t32[sel], t64[sel], f"{what} t")
    gats_ref.assert_close(gx[sel], g32[sel], g64[sel], f"{what} gx")
    return t, gx


@pytest.mark.parametrize("n,m,d", SHAPES)
def test_shapes(n, m, d):
    check(*make_inputs(n, m, d, 1000 * n + 10 * m + d), 0.1, f"n={n} m={m} d={d}")


def test_every_shape_value_and_pair_is_covered():
    for a, b, key in ((NS, MS, lambda s: (s[0], s[1])), (NS, DS, lambda s: (s[0], s[2])),
                      (MS, DS, lambda s: (s[1], s[2]))):
        assert {key(s) for s in SHAPES} == set(itertools.product(a, b))


def test_small_tau_with_only_negative_similarities():
    """tau = 0.01 on rows whose best similarity is far below 1: a shift by 1 / tau would underflow to 0 / 0."""
    x, bank, v, gt = make_inputs(129, 33, 16, 7)
    bank = F.normalize(bank + 2.0, p=2, dim=1)          # a bank with a strong common direction
    x = -bank.mean(0, keepdim=True) + 0.02 * x
    sim = F.normalize(x, dim=1) @ bank.t()
    assert float(sim.max()) < -0.5
    check(x, bank, v, gt, 0.01, "tau=0.01 negative")


def test_tau_one():
    check(*make_inputs(129, 33, 16, 8), 1.0, "tau=1")


def test_confidences_down_to_zero():
    """inv_conf from 1 to 1 / eps = 1e8 (a validation node of confidence 0)."""
    x, bank, _, gt = make_inputs(129, 33, 16, 9)
    v = torch.logspace(0, 8, 33).float()
    check(x, bank, v, gt, 0.1, "inv_conf 1..1e8")


def test_latent_row_equal_to_a_bank_row():
    """Similarity 1 up to rounding, above or below."""
    x, bank, v, gt = make_inputs(31, 33, 65, 10)
    x[5] = bank[3]
    x[6] = 2.5 * bank[4]
    x[7] = -bank[5]
    check(x, bank, v, gt, 0.1, "row == bank row")


def test_zero_and_tiny_rows():
    """F.normalize's clamp: a row of zeros weighs every bank row alike, and gx = ga / 1e-12 as torch gives it; so
    for a row of norm 1e-20.  Compared per row: their 1 / eps-scaled gradients do not set the scale of the others."""
    x, bank, v, gt = make_inputs(31, 33, 16, 11)
    x[3] = 0.0
    x[9] *= 1e-20 / float(x[9].norm())
    ordinary = [i for i in range(31) if i not in (3, 9)]
    t, gx = check(x, bank, v, gt, 0.1, "ordinary rows", rows=ordinary)
    (_, t32, g32), (_, t64, g64) = references(x, bank, v, gt, 0.1)
    for i in (3, 9):
        gats_ref.assert_close(t[i:i + 1], t32[i:i + 1], t64[i:i + 1], f"row {i} t")
        gats_ref.assert_close(gx[i], g32[i], g64[i], f"row {i} gx")
    mean = float(v.double().mean())
    assert abs(float(t[3]) - mean) <= 4 * 2.0 ** -24 * mean
    assert float(gx[3].abs().max()) > 1e6 * float(gx[ordinary].abs().max())     # the 1 / eps scale is real


def test_clamp_values_and_zero_gradient():
    """Temperatures on both sides of t_min and t_max; the gradient is exactly zero on the clamped rows."""
    x, bank, _, gt = make_inputs(129, 33, 64, 12)
    v = torch.full((33,), 1.0)
    v[:8], v[8:16] = 0.01, 8.0
    x[:20] = bank[:20] * 3.0 + 0.05 * x[:20]            # rows that sit on one bank row each
    raw = wats_hip.raw_similarity_temperature(x.to(DEV), bank.to(DEV), v.to(DEV), 0.1).cpu()
    low, high = raw < 0.1, raw > 5.0
    inside = ~(low | high)
    assert int(low.sum()) > 0 and int(high.sum()) > 0 and int(inside.sum()) > 0
    (raw32, t32, g32), (raw64, t64, g64) = references(x, bank, v, gt, 0.1, 0.1, 5.0)
    assert torch.equal(raw64 < 0.1, low) and torch.equal(raw64 > 5.0, high)      # no row sits on an edge
    t, gx = kernel(x, bank, v, gt, 0.1, 0.1, 5.0)
    assert torch.equal(t.cpu(), raw.clamp(0.1, 5.0))
    gats_ref.assert_close(t, t32, t64, "clamped t")
    gats_ref.assert_close(gx, g32, g64, "clamped gx")
    assert float(gx.cpu()[low | high].abs().max()) == 0.0
    assert bool((gx.cpu()[inside].abs().amax(1) > 0).all())


def test_two_calls_are_bit_identical():
    x, bank, v, gt = make_inputs(*LARGEST, 13)
    a, b = kernel(x, bank, v, gt, 0.1), kernel(x, bank, v, gt, 0.1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_nan_stays_in_its_row():
    x, bank, v, gt = make_inputs(129, 33, 65, 14)
    clean_t, clean_gx = kernel(x, bank, v, gt, 0.1)
    x[40, 2] = float("nan")
    t, gx = kernel(x, bank, v, gt, 0.1)
    others = [i for i in range(129) if i != 40]
    assert bool(torch.isnan(t[40])) and bool(torch.isnan(gx[40]).all())
    assert torch.equal(t[others], clean_t[others]) and torch.equal(gx[others], clean_gx[others])


def test_matches_the_dense_device_path():
    """similarity_temperature against clamp(softmax(compute_similarity_matrix(.) / tau) @ inv_conf) in float32 on
    the device: the same bound, with the dense device result as the float32 side."""
    x, bank, v, gt = make_inputs(300, 257, 64, 15)
    fv = bank * (0.5 + torch.rand(257, 1, generator=torch.Generator().manual_seed(1)))    # unnormalised rows
    bank_obj = wats_hip.SimilarityBank(fv, 1.0 / v - 1e-8, 1e-8, DEV)
    sim = wats_hip.SimCalib.compute_similarity_matrix(None, x.to(DEV), fv.to(DEV))
    dense = (torch.softmax(sim / 0.1, dim=1) @ bank_obj.inv_conf.unsqueeze(1)).squeeze(1).clamp(0.1, 5.0)
    t = wats_hip.similarity_temperature(x.to(DEV), bank_obj)
    ref64 = R.raw_temperature(x, bank_obj.bank.cpu(), bank_obj.inv_conf.cpu(), 0.1, torch.float64).clamp(0.1, 5.0)
    gats_ref.assert_close(t, dense, ref64, "dense device path")


def test_argument_errors():
    x, bank, v, _ = make_inputs(5, 4, 8, 16)
    with pytest.raises(ValueError, match="at least one"):
        wats_hip.similarity_temperature(x.to(DEV), bank[:0].to(DEV), v[:0].to(DEV))
    with pytest.raises(ValueError, match="at least one validation"):
        wats_hip.SimilarityBank(bank[:0], v[:0], device=DEV)
    with pytest.raises(ValueError, match="tau"):
        wats_hip.similarity_temperature(x.to(DEV), bank.to(DEV), v.to(DEV), tau=0.0)
    wide = simcalib.max_latent_width() + 1
    with pytest.raises(wats_hip.WaveletError, match="status -4"):
        wats_hip.similarity_temperature(torch.zeros(2, wide, device=DEV), torch.zeros(3, wide, device=DEV),
                                        torch.ones(3, device=DEV))
    assert wats_hip.similarity_temperature(x[:0].to(DEV), bank.to(DEV), v.to(DEV)).shape == (0,)


# ---------------------------------------------------------------------------------------------------------
# the calibrator on the fixtures the reference recorded
# ---------------------------------------------------------------------------------------------------------
_cases = {}


def case(name):
    """The fixture and its float64 restatement (state, log-probs, raw temperatures, adjacency gradient), once."""
    if name not in _cases:
        with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as d:
            c = {k: torch.from_numpy(np.asarray(d[k])) for k in d.files}
        params = (c["gc1_weight"], c["gc1_bias"], c["gc2_weight"], c["gc2_bias"])
        mask = c["val_mask"].bool()
        fv, conf = R.calibration_state(c["adj"], c["x"], params, mask, torch.float64)
        out, raw = R.forward(c["adj"], c["x"], params, fv, conf, float(c["epsilon"]), dtype=torch.float64)
        grad = R.adjacency_gradient(c["adj"], c["x"], params, fv, conf, c["loss_weight"], c["grad_rows"],
                                    c["grad_cols"], torch.float64)
        c["ref64"] = dict(features_val=fv, val_confidence=conf, out=out.detach(), raw_t=raw.detach(), grad=grad)
        c["params"], c["mask"] = params, mask
        _cases[name] = c
    return _cases[name]


def base_model(c, cls):
    nhid, nfeat = c["gc1_weight"].shape
    model = cls(nfeat=nfeat, nclass=c["gc2_weight"].shape[0], nhid=nhid)
    model.load_state_dict({"gc1.weight": c["gc1_weight"], "gc1.bias": c["gc1_bias"], "gc2.weight": c["gc2_weight"],
                           "gc2.bias": c["gc2_bias"]})
    return model.to(DEV)


@pytest.mark.parametrize("adj_kind", ["dense", "operator"])
@pytest.mark.parametrize("name", ["plain120", "clamp96"])
def test_calibrator_matches_the_reference(name, adj_kind):
    c = case(name)
    ref = c["ref64"]
    adj = c["adj"].to(DEV)
    if adj_kind == "operator":
        adj = wats_hip.RowNormalizedAdjacency.from_dense(adj)
    cal = wats_hip.SimCalib(base_model(c, wats_hip.SparseCompatibleGCN), c["x"], c["y"], adj, c["mask"])
    assert cal.calib_train() is cal and cal.fit() is cal
    what = f"{name} {adj_kind}"
    gats_ref.assert_close(cal.features_val, c["features_val"], ref["features_val"], what + " features_val")
    gats_ref.assert_close(cal.val_confidence, c["val_confidence"], ref["val_confidence"], what + " val_confidence")
    with torch.no_grad():
        raw = wats_hip.raw_similarity_temperature(cal.latent_feature_1(c["x"], adj), cal.bank, None, cal.tau)
    gats_ref.assert_close(raw, c["raw_t"], ref["raw_t"], what + " raw temperatures")
    probe = wats_hip.EdgeProbe(c["grad_rows"], c["grad_cols"])
    out = cal(c["x"], adj, probe=probe)
    gats_ref.assert_close(out, c["out"], ref["out"], what + " log-probs")
    (out * c["loss_weight"].to(DEV)).sum().backward()
    gats_ref.assert_close(probe.grad, c["grad"], ref["grad"], what + " adjacency gradient")


@pytest.mark.parametrize("name", ["plain120", "clamp96"])
def test_calibrator_on_a_dense_base_model(name):
    """The literal path: any base model with a gc1; outputs only."""
    c = case(name)
    ref = c["ref64"]
    cal = wats_hip.SimCalib(base_model(c, CompatibleGCN), c["x"], c["y"], c["adj"], c["mask"])
    gats_ref.assert_close(cal.features_val, c["features_val"], ref["features_val"], name + " literal features_val")
    gats_ref.assert_close(cal.val_confidence, c["val_confidence"], ref["val_confidence"],
                          name + " literal val_confidence")
    with torch.no_grad():
        out = cal(c["x"], c["adj"])
    gats_ref.assert_close(out, c["out"], ref["out"], name + " literal log-probs")


def test_dense_adj_leaf_still_raises():
    c = case("plain120")
    cal = wats_hip.SimCalib(base_model(c, wats_hip.SparseCompatibleGCN), c["x"], c["y"], c["adj"], c["mask"])
    leaf = c["adj"].clone().to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError):
        cal(c["x"], leaf)
