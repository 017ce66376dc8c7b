"""CPU tests of the DCGC yardsticks and of the host side of wats_hip.dcgc: the fixtures' hashes, the float32
restatement (tests/dcgc_ref.py) against the arrays the reference recorded, the hashed dropout masks against the
values the header lists, the ABI's argument checks, the workspace rule, the exported surface and the refusal to run
without a GPU."""
import ctypes
import hashlib
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dcgc_ref as R
import wats_hip
from wats_hip import dcgc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "dcgc")
CASES = ["iso120", "wide96"]
EPS = 2.0 ** -24


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
    """dcgc_ref.fixture_differences of both fixtures in one child process that starts torch on the CPU code paths
    the fixtures were generated on (they are read at start-up only)."""
    paths = [os.path.join(GOLDEN, c + ".npz") for c in CASES]
    env = dict(os.environ, **R.PINNED_CPU_PATH)
    run = subprocess.run([sys.executable, os.path.join(HERE, "dcgc_ref.py")] + paths, env=env, check=True,
                         capture_output=True, text=True)
    got = json.loads(run.stdout.strip().splitlines()[-1])
    return {c: got[p] for c, p in zip(CASES, paths)}


@pytest.mark.parametrize("name", CASES)
def test_float32_restatement_reproduces_the_reference(name, restatement_differences):
    """The same torch ops on the same CPU code path: expected equal (measured: equal); the bound is
    4 * 2^-24 * max|ref|, as for the SimCalib fixtures."""
    for key, (err, scale) in restatement_differences[name].items():
        print(f"{name} {key}: max|restatement32 - reference| = {err:.3e}, max|reference| = {scale:.3e}")
        assert err <= 4 * EPS * scale, key


def test_fixtures_hold_what_the_tests_need():
    c = R.load_case(os.path.join(GOLDEN, "iso120.npz"))
    i = int(c["isolated"][0])
    adj = c["adj"]
    assert float(adj[i].abs().sum()) == 0.0 and float(adj[:, i].abs().sum()) == 0.0
    for name in CASES:
        c = R.load_case(os.path.join(GOLDEN, name + ".npz"))
        adj = c["adj"]
        n, C = adj.shape[0], c["gc2_weight"].shape[0]
        assert torch.equal(adj, adj.t()) and int(adj.diagonal().sum()) == n - len(c["isolated"])
        rows, cols = R.pattern(adj)
        assert c["weights"].shape == c["homo"].shape == rows.shape
        assert tuple(c["ext_w1"].shape) == (4 * C, 2 * C) and tuple(c["ext_w3"].shape) == (1, 2 * C)
        assert float((c["weights"] > 0).float().mean()) > 0.2
        at = adj[c["grad_rows"].long(), c["grad_cols"].long()]
        assert int((at != 0).sum()) >= rows.numel() and int((at == 0).sum()) >= rows.numel()
        t = int(c["target"])
        assert c["grad_rows"][-2 * n:-n].eq(t).all() and c["grad_cols"][-n:].eq(t).all()
        assert float(c["grad"].abs().max()) > 0


def test_hash_matches_the_header():
    """The example words of include/wats_hip.h, read from the header itself."""
    text = open(os.path.join(REPO, "include", "wats_hip.h")).read()
    block = text[text.index("Examples with seed = 7"):]
    words = [int(w, 16) for w in re.findall(r"0x[0-9a-f]{8}\b", block)[:8]]
    assert len(words) == 8
    pairs = [(0, 0), (1, 0), (0, 1), (123456, 77)]
    got = [int(R.hash_words(7, layer, e, j)) for layer in (1, 2) for e, j in pairs]
    assert got == words
    assert words[0] == 0xf75f04cb and words[7] == 0x3b9c8399
    # vectorised calls agree with scalar ones, and the masks are what the threshold says
    e, j = np.arange(50)[:, None], np.arange(9)[None, :]
    grid = R.hash_words(99, 2, e, j)
    assert grid[17, 4] == R.hash_words(99, 2, 17, 4)
    assert np.array_equal(R.keep_mask(99, 2, 50, 9, 0.25), grid >= np.uint32(2 ** 30))
    assert R.keep_mask(99, 2, 50, 9, 0.0).all()
    for layer in (1, 2):
        keep = R.keep_mask(12345, layer, 4000, 28, 0.5)
        assert keep.size >= 10 ** 5 and abs(float(keep.mean()) - 0.5) <= 0.02
    assert not np.array_equal(R.keep_mask(1, 1, 100, 8, 0.5), R.keep_mask(2, 1, 100, 8, 0.5))
    assert not np.array_equal(R.keep_mask(1, 1, 100, 8, 0.5), R.keep_mask(1, 2, 100, 8, 0.5))


def test_restatement_gradients_match_a_plain_autograd_run():
    """edge_mlp_and_grads and the documented value gradient against torch autograd on the dense form."""
    g = torch.Generator().manual_seed(0)
    n, C = 9, 3
    adj = (torch.rand(n, n, generator=g) < 0.4).float()
    rows, cols = R.pattern(adj)
    emb = torch.randn(n, C, generator=g)
    params = [torch.randn(s, generator=g) * 0.5 for s in ((4 * C, 2 * C), (4 * C,), (2 * C, 4 * C), (2 * C,),
                                                          (1, 2 * C), (1,))]
    masks = R.dropout_masks(rows.numel(), C, 0.5, 3, torch.float64)
    g_w = torch.randn(rows.numel(), generator=g)
    w, gp, ge = R.edge_mlp_and_grads(emb, params, rows, cols, g_w, masks, torch.float64)
    # the kernel's formulas in float64
    w1, b1, w2, b2, w3, b3 = (p.double() for p in params)
    f = torch.cat([emb.double()[rows], emb.double()[cols]], 1)
    z1 = f @ w1.t() + b1
    h1 = z1.clamp_min(0) * masks[0]
    z2 = h1 @ w2.t() + b2
    h2 = z2.clamp_min(0) * masks[1]
    z3 = (h2 @ w3.t()).reshape(-1) + b3
    d3 = g_w.double() * (z3 > 0)
    d2 = d3.unsqueeze(1) * w3 * masks[1] * (z2 > 0)
    d1 = (d2 @ w2) * masks[0] * (z1 > 0)
    gf = d1 @ w1
    ge2 = torch.zeros(n, C, dtype=torch.float64).index_add_(0, rows, gf[:, :C]).index_add_(0, cols, gf[:, C:])
    mine = [d1.t() @ f, d1.sum(0), d2.t() @ h1, d2.sum(0), (d3.unsqueeze(1) * h2).sum(0, keepdim=True), d3.sum().reshape(1)]
    for a, b in zip(mine + [ge2, z3.clamp_min(0)], gp + [ge, w]):
        assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1.0)


def test_abi_checks_arguments_before_any_device_work():
    lib = wats_hip._lib.load()
    cmax = lib.wg_edge_mlp_max_c()
    assert cmax == dcgc.max_classes() and cmax >= 41
    assert lib.wg_edge_mlp_tile() == dcgc.edge_mlp_tile() == 1024
    p = 4096   # any non-NULL address: no call below reaches the device
    fwd_ok = dict(n=4, nnz=6, indptr=p, indices=p, C=3, emb=p, W1=p, b1=p, W2=p, b2=p, w3=p, b3=p, p=0.0, seed=0,
                  ws=p, w=p, stream=None)
    bwd_ok = dict(n=4, nnz=6, indptr=p, indices=p, C=3, emb=p, W1=p, b1=p, W2=p, b2=p, w3=p, b3=p, p=0.0, seed=0,
                  g_w=p, t_indptr=p, t_indices=p, t_pos=p, gW1=p, gb1=p, gW2=p, gb2=p, gw3=p, gb3=p, g_emb=p + 4096,
                  ws=p, stream=None)
    for fn, ok in ((lib.wg_edge_mlp_forward, fwd_ok), (lib.wg_edge_mlp_backward, bwd_ok)):
        call = lambda **kw: fn(*[kw.get(k, v) for k, v in ok.items()])
        for kw in (dict(n=-1), dict(nnz=-1), dict(C=0), dict(C=-2)):
            assert call(**kw) == -1 and b"bad size" in lib.wg_last_error(), kw
        for bad_p in (1.0, -0.1, 1.5, float("nan")):
            assert call(p=bad_p) == -1 and b"[0, 1)" in lib.wg_last_error(), bad_p
        for k in ok:
            if ok[k] == p and not k.startswith("t_") and k != "g_emb":
                assert call(**{k: None}) == -1 and b"NULL" in lib.wg_last_error(), k
        assert call(C=cmax + 1) == -4 and b"exceeds" in lib.wg_last_error()
        assert call(n=2 ** 31) == -4
    bwd = lambda **kw: lib.wg_edge_mlp_backward(*[kw.get(k, v) for k, v in bwd_ok.items()])
    assert bwd(t_pos=None) == -1 and b"transposed" in lib.wg_last_error()
    assert bwd(g_emb=p) == -1 and b"alias" in lib.wg_last_error()
    # nothing to do in the forward: WG_OK with no pointer read
    assert lib.wg_edge_mlp_forward(*[dict(nnz=0, indptr=None, indices=None, emb=None, ws=None, w=None).get(k, v)
                                     for k, v in fwd_ok.items()]) == 0
    agg = lambda **kw: lib.wg_edge_aggregate(*[kw.get(k, v) for k, v in dict(
        n=4, nnz=6, indptr=p, indices=p, n_long=0, long_rows=None, val=p, map=None, rs=None, cs=None, C=3, x=p,
        out=p + 4096, stream=None).items()])
    assert agg(n=-1) == -1 and agg(x=None) == -1 and agg(val=None) == -1 and agg(n_long=1) == -1
    assert agg(out=p) == -1 and b"alias" in lib.wg_last_error()
    assert agg(n=0) == 0 and agg(C=0) == 0 and agg(n_long=5) == -1
    assert lib.wg_edge_aggregate_long_row() == 128
    pid = lambda **kw: lib.wg_edge_pair_inv_distance(*[kw.get(k, v) for k, v in dict(
        nnz=3, rows=p, cols=p, C=4, n=5, Q=p, alpha=0.5, out=p, stream=None).items()])
    assert pid(nnz=-1) == -1 and pid(rows=None) == -1 and pid(Q=None) == -1 and pid(nnz=0) == 0
    with pytest.raises(wats_hip.WaveletError, match="wg_edge_mlp_workspace"):
        dcgc.edge_mlp_workspace(5, 5, cmax + 1)


def test_workspace_rule():
    """No (E, k) buffer: doubling nnz adds at most 16 bytes per entry; the rest grows with n C and the parameter
    count only."""
    for C in (1, 3, 7, 40, 41, 48):
        for n in (1, 50, 100000):
            for nnz in (1, 2, 3, 5, 33, 63, 64, 511, 512, 513, 1023, 1024, 1025, 2049, 10 ** 5, 2.5e6):
                nnz = int(nnz)
                a, b = dcgc.edge_mlp_workspace(n, nnz, C), dcgc.edge_mlp_workspace(n, 2 * nnz, C)
                assert 0 <= b - a <= 16 * nnz, (C, n, nnz, b - a)
        P = 16 * C * C + 8 * C + 1
        assert dcgc.edge_mlp_workspace(1000, 0, C) <= 8 * 1000 * C + 256 * 8 * P + 64 * P + 65536


def test_exported_surface():
    for name in ("DCGC", "DecisiveEdge", "EdgeWeightGraph", "edge_mlp_weights", "weighted_propagate",
                 "homophily_weights"):
        assert getattr(wats_hip, name) is getattr(dcgc, name)
    sig = inspect.signature(dcgc.DCGC.__init__)
    assert list(sig.parameters)[:9] == ["self", "base_model", "features", "labels", "adj", "val_mask", "dropout",
                                        "alpha", "beta"]
    assert [sig.parameters[k].default for k in ("dropout", "alpha", "beta", "epochs", "verbose")] == [0.5, 0.5, 10, 250,
                                                                                                     False]
    for k in ("graph", "epochs", "verbose"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    fs = inspect.signature(dcgc.DCGC.forward)
    assert list(fs.parameters)[:4] == ["self", "x", "adj", "probe"]
    es = inspect.signature(dcgc.edge_mlp_weights)
    assert es.parameters["p"].default == 0.0 and es.parameters["seed"].default == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU refusal")
def test_refuses_to_run_without_a_gpu():
    c = R.load_case(os.path.join(GOLDEN, "iso120.npz"))
    base = wats_hip.SparseCompatibleGCN(nfeat=16, nclass=5, nhid=32)
    with pytest.raises(wats_hip.WaveletError, match="no ROCm GPU"):
        dcgc.DCGC(base, c["x"], c["y"], c["adj"], c["val_mask"].bool(), epochs=1)
    with pytest.raises(wats_hip.WaveletError, match="no ROCm GPU"):
        dcgc.EdgeWeightGraph(c["adj"])
    with pytest.raises(wats_hip.WaveletError, match="no ROCm GPU"):
        dcgc.edge_mlp_weights(None, c["x"], None)
    with pytest.raises(wats_hip.WaveletError, match="no ROCm GPU"):
        dcgc.weighted_propagate(None, c["weights"], c["x"])
    with pytest.raises(wats_hip.WaveletError, match="no ROCm GPU"):
        dcgc.homophily_weights(None, c["out"])
