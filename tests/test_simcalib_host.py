"""CPU tests of the SimCalib yardsticks and of the host side of wats_hip.simcalib: the fixtures' hashes, the float32
restatement (tests/simcalib_ref.py) against the arrays the reference recorded, the clamp counts of the second
fixture, the backward formula that csrc/simcalib.hip implements against autograd, the ABI's argument checks, the
exported surface and the refusal to run without a GPU."""
import hashlib
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import simcalib_ref as R
import wats_hip
from wats_hip import simcalib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "simcalib")
CASES = ["plain120", "clamp96"]
EPS = 2.0 ** -24


def load_case(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as d:
        return {k: torch.from_numpy(np.asarray(d[k])) for k in d.files}


def params_of(c):
    return c["gc1_weight"], c["gc1_bias"], c["gc2_weight"], c["gc2_bias"]


def test_manifest_hashes_match():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        manifest = json.load(f)
    assert sorted(manifest["files"]) == sorted(c + ".npz" for c in CASES)
    for name, meta in manifest["files"].items():
        path = os.path.join(GOLDEN, name)
        assert os.path.getsize(path) < 200 * 1024
        with open(path, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == meta["sha256"], name
        with np.load(path, allow_pickle=False) as d:
            assert sorted(d.files) == meta["keys"]


@pytest.fixture(scope="module")
def restatement_differences():
    """simcalib_ref.fixture_differences of both fixtures, computed in one child process that starts torch on the
    CPU code paths the fixtures were generated on (torch's float32 CPU kernels differ in the last bit between
    instruction sets, and the settings that pin them are read at start-up only)."""
    paths = [os.path.join(GOLDEN, c + ".npz") for c in CASES]
    env = dict(os.environ, **R.PINNED_CPU_PATH)
    run = subprocess.run([sys.executable, os.path.join(HERE, "simcalib_ref.py")] + paths, env=env, check=True,
                         capture_output=True, text=True)
    got = json.loads(run.stdout.strip().splitlines()[-1])
    return {c: got[p] for c, p in zip(CASES, paths)}


@pytest.mark.parametrize("name", CASES)
def test_float32_restatement_reproduces_the_reference(name, restatement_differences):
    """The same torch ops in the same order on the same CPU code path: expected equal; the bound is
    4 * 2^-24 * max|ref|.  Measured: equal but for the adjacency gradient (the reference evaluates the first layer
    twice, so autograd adds the two paths' gradients in another order): 1.8e-7 of 1.4 and 2.4e-7 of 1.5.  On a CPU
    where MKL takes a path that the settings do not reach (measured on the AMD hosts of the GPU machines) the
    temperatures differ by 9.5e-7 in both fixtures, 0.91 and 0.63 of the bound."""
    for key, (err, scale) in restatement_differences[name].items():
        print(f"{name} {key}: max|restatement32 - reference| = {err:.3e}, max|reference| = {scale:.3e}")
        assert err <= 4 * EPS * scale, key


def test_fixtures_cover_both_sides_of_the_clamp():
    raw = load_case("clamp96")["raw_t"]
    assert int((raw > R.T_MAX).sum()) > 0 and int((raw <= R.T_MAX).sum()) > 0
    raw = load_case("plain120")["raw_t"]
    assert float(raw.min()) > R.T_MIN and float(raw.max()) < R.T_MAX
    c = load_case("plain120")
    i = int(c["isolated"][0])
    assert float(c["adj"][i].abs().sum()) == 0.0 and float(c["adj"][:, i].abs().sum()) == 0.0
    # the recorded positions hold present edges, absent ones and the target's whole row and column
    at = c["adj"][c["grad_rows"].long(), c["grad_cols"].long()]
    assert int((at != 0).sum()) > 0 and int((at == 0).sum()) > 0
    n, t = c["adj"].shape[0], int(c["target"])
    assert c["grad_rows"][-2 * n:-n].eq(t).all() and c["grad_cols"][-n:].eq(t).all()


def kernel_formula(x, bank, v, g, tau):
    """What wg_simcalib_backward computes, in float64 torch: ga, then F.normalize's Jacobian by cases."""
    x, bank, v, g = x.double(), bank.double(), v.double(), g.double()
    nrm = x.norm(dim=1, keepdim=True)
    a = x / nrm.clamp_min(1e-12)
    w = torch.softmax(a @ bank.t() / tau, dim=1)
    t = w @ v
    ga = (g / tau).unsqueeze(1) * ((w * (v.unsqueeze(0) - t.unsqueeze(1))) @ bank)
    normal = (ga - a * (a * ga).sum(1, keepdim=True)) / nrm
    return t, torch.where(nrm >= 1e-12, normal, ga / 1e-12)


@pytest.mark.parametrize("tau", [0.1, 0.01, 1.0])
def test_backward_formula_equals_autograd(tau):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(9, 5, generator=g, dtype=torch.float64)
    x[2] = 0.0                       # F.normalize's clamp: a = 0, gx = ga / eps
    x[3] *= 1e-20 / x[3].norm()      # below eps
    x[4] = 0.0
    x[4, 1] = 1e-12                  # exactly eps: clamp_min passes the gradient to the norm
    bank = torch.nn.functional.normalize(torch.randn(7, 5, generator=g, dtype=torch.float64), dim=1)
    v = 1.0 / (torch.rand(7, generator=g, dtype=torch.float64) + 1e-8)
    gt = torch.randn(9, generator=g, dtype=torch.float64)
    raw, _, grad = R.temperature_and_grad(x, bank, v, gt, tau, -1e30, 1e30, torch.float64)
    t, gx = kernel_formula(x, bank, v, gt, tau)
    assert float((t - raw).abs().max()) <= 1e-12 * float(raw.abs().max())
    assert float(x[4].norm()) == 1e-12
    # a row's gradient is a sum of terms of size |g| max|v| / (tau |x|) that cancel, each carrying the 1 / tau
    # amplification of its exponent: 100 float64 roundings of that size
    for i in range(9):
        scale = abs(float(gt[i])) * float(v.max()) / (tau * tau * max(float(x[i].norm()), 1e-12))
        assert float((gx[i] - grad[i]).abs().max()) <= 100 * 2.0 ** -53 * scale, i
    w_uniform = float(v.mean())
    assert abs(float(raw[2]) - w_uniform) <= 1e-12 * w_uniform      # a zero row weighs every bank row alike


def test_abi_checks_arguments_before_any_device_work():
    lib = wats_hip._lib.load()
    fwd, bwd = lib.wg_simcalib_forward, lib.wg_simcalib_backward
    p = 4096   # any non-NULL address: no call below reaches the device
    assert lib.wg_simcalib_max_d() == 256 == simcalib.max_latent_width()
    ok_f = [3, 2, 4, p, p, p, 0.1, p, p, None]
    ok_b = [3, 2, 4, p, p, p, 0.1, p, p, p + 4096, None]
    for f, ok, ptrs in ((fwd, ok_f, (3, 4, 5, 7, 8)), (bwd, ok_b, (3, 4, 5, 7, 8, 9))):
        for k in (0, 1, 2):
            for bad_size in (0, -1):
                bad = list(ok)
                bad[k] = bad_size
                assert f(*bad) == -1 and b"positive" in lib.wg_last_error(), (k, bad_size)
        for k in ptrs:
            bad = list(ok)
            bad[k] = None
            assert f(*bad) == -1 and b"NULL" in lib.wg_last_error(), k
        for tau in (0.0, -0.1, float("inf"), float("nan"), 1e-60):
            bad = list(ok)
            bad[6] = tau
            assert f(*bad) == -1 and b"tau" in lib.wg_last_error(), tau
        bad = list(ok)
        bad[2] = 257
        assert f(*bad) == -4 and b"exceeds" in lib.wg_last_error()
    bad = list(ok_b)
    bad[9] = p     # gx == x
    assert bwd(*bad) == -1 and b"alias" in lib.wg_last_error()


def test_exported_surface():
    for name in ("SimCalib", "SimilarityBank", "similarity_temperature", "raw_similarity_temperature"):
        assert getattr(wats_hip, name) is getattr(simcalib, name)
    assert simcalib.SimCalib.fit is simcalib.SimCalib.calib_train
    sig = inspect.signature(simcalib.SimCalib.__init__)
    assert list(sig.parameters)[:8] == ["self", "base_model", "features", "labels", "adj", "val_mask", "k", "epsilon"]
    assert sig.parameters["k"].default == 10 and sig.parameters["epsilon"].default == 1e-8
    assert sig.parameters["tau"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["tau"].default == 0.1
    st = inspect.signature(simcalib.similarity_temperature)
    assert [st.parameters[k].default for k in ("tau", "t_min", "t_max")] == [0.1, 0.1, 5.0]
    for name in ("forward", "latent_feature_1", "compute_similarity_matrix", "calib_train"):
        assert callable(getattr(simcalib.SimCalib, name))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU refusal")
def test_refuses_to_run_without_a_gpu():
    c = load_case("plain120")
    base = wats_hip.SparseCompatibleGCN(nfeat=16, nclass=5, nhid=32)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        simcalib.SimCalib(base, c["x"], c["y"], c["adj"], c["val_mask"].bool())
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        simcalib.SimilarityBank(c["features_val"], c["val_confidence"])
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        simcalib.similarity_temperature(torch.zeros(3, 4), torch.zeros(2, 4), torch.ones(2))
