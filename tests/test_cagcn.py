"""GPU tests of the CaGCN calibrator's graph convolution (csrc/symnorm.hip, wats_hip/cagcn.py) against the
float64 edge-list restatement (A) of tests/cagcn_ref.py.

The bound on every value is measured in the test: err = max|kernel - A_float64| must not exceed
max(2 * max|A_float32 - A_float64|, 4 * 2^-24 * max|A_float64|) (gats_ref.error_bound), both restatements on the
layer's own float32 dinv.  The references of the aggregation run on the CPU from edge lists that the tests build
themselves (numpy: duplicates merged, self loops replaced), so the ingestion, the edge direction and the transpose
are under test as well.  The references of the whole layers are (A), in float64 and in float32, wrapped in the
layers' own torch steps (float32, on the device, deterministic torch algorithms), as in tests/test_gats.py.
"""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import cagcn_ref as R  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip import cagcn  # noqa: E402
from wats_hip._lib import ptr  # noqa: E402

DEV = "cuda"
EPS = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


# the graphs of tests/test_gats.py; the star's hub has 701 entries: more than five turns of its workgroup's
# sub-groups at any width, and at least twice the threshold (asserted below)
GRAPHS = {
    "single": lambda: (np.zeros(0, np.int64), np.zeros(0, np.int64), 1),
    "lonely": lambda: (np.array([0, 0, 1]), np.array([1, 2, 2]), 3),
    "path": lambda: R.path_graph(3),
    "symmetric": lambda: R.random_graph(300, 6, False, 1),
    "directed": lambda: R.random_graph(300, 6, True, 2),
    "loops": lambda: R.random_graph(300, 6, True, 3, loops=40),
    "star": lambda: R.star_graph(700, 50),
    "wide16": lambda: R.random_graph(200, 12, True, 4),
    "wide32": lambda: R.random_graph(120, 20, True, 5),
    "wide64": lambda: R.random_graph(100, 40, True, 6),
}
WIDTHS = [1, 3, 7, 40, 41, 64, 260]
_cache = {}


def graph(name):
    """(SymNormGraph, src, dst, n): the device graph from the raw edge_index, the reference's edge list from numpy."""
    if name not in _cache:
        src, dst, n = GRAPHS[name]()
        ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
        rs, rd = R.with_self_loops(src, dst, n)
        _cache[name] = (wats_hip.SymNormGraph(ei, n, device=DEV), rs, rd, n)
    return _cache[name]


def inputs(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, C, generator=g).float(), torch.randn(C, generator=g).float(),
            torch.randn(n, C, generator=g).float())


def reference(src, dst, dinv, x, bias, G, relu, dtype):
    """(out, grad_x) of (A) on the CPU in `dtype` from the float32 inputs and the layer's float32 dinv."""
    xr = x.detach().clone().to(dtype).requires_grad_(True)     # a float32 x.to(float32) would be x itself
    out = R.sym_norm_edges(src, dst, xr, dinv, bias, relu, dtype)
    (out * G.to(dtype)).sum().backward()
    return out.detach(), xr.grad


def kernel(g, x, bias, G, relu):
    """(out, grad_x, grad_bias or None) of the HIP path."""
    xd = x.detach().clone().to(DEV).requires_grad_(True)
    bd = None if bias is None else bias.detach().clone().to(DEV).requires_grad_(True)
    out = wats_hip.sym_norm_aggregate(g, xd, bd, relu)
    (out * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), xd.grad, None if bd is None else bd.grad


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_aggregate_matches_the_float64_restatement(name, C):
    g, src, dst, n = graph(name)
    dinv = g.dinv.cpu()
    # in_degree^-1/2 in float32 by the device's pow (not correctly rounded: within two ulps of the float64 value);
    # both restatements below take this very vector, so its last bit does not enter the comparison
    exact = R.in_degree(dst, n).pow(-0.5)
    assert dinv.dtype == torch.float32 and float(((dinv.double() - exact) / exact).abs().max()) <= 4 * EPS
    x, bias, G = inputs(n, C, 100 + C)
    for with_bias in (False, True):
        for relu in (False, True):
            b = bias if with_bias else None
            out, gx, gb = kernel(g, x, b, G, relu)
            r64 = reference(src, dst, dinv, x, b, G, relu, torch.float64)
            r32 = reference(src, dst, dinv, x, b, G, relu, torch.float32)
            what = f"{name} C={C} bias={with_bias} relu={relu}"
            R.assert_close(out, r32[0], r64[0], what + " out")
            R.assert_close(gx, r32[1], r64[1], what + " grad_x")
            if with_bias:   # the column sum of the masked gradient, by the same torch reduction
                masked = G.to(DEV) * (out > 0) if relu else G.to(DEV)
                assert torch.equal(gb, masked.sum(0)), what + " grad_bias"


def test_bin_assignment_on_the_star():
    g, src, dst, n = graph("star")
    th = cagcn.symnorm_long_row_threshold()
    in_len, out_len = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    assert in_len[0] == 701 and in_len[0] >= 2 * th, "the hub takes several turns of its workgroup"
    assert g.long_rows.tolist() == [0]          # the forward: by in-degree
    assert g.t_long_rows.tolist() == [1]        # the backward: node 1 is long by out-degree only
    assert out_len[1] >= th > in_len[1] and out_len[0] < th
    assert "long rows=1" in g.describe() and "long transposed rows=1" in g.describe()
    for name in ("directed", "wide64"):         # no hubs: no workgroup rows in either direction
        h = graph(name)[0]
        assert h.long_rows.numel() == 0 and h.t_long_rows.numel() == 0
        assert int((h.indptr[1:] - h.indptr[:-1]).max()) < th and int((h.t_indptr[1:] - h.t_indptr[:-1]).max()) < th


def test_a_shared_attention_graph_is_read_not_changed():
    src, dst, n = GRAPHS["loops"]()
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    ag = wats_hip.AttentionGraph(ei, n, device=DEV)
    before = {k: v.clone() for k, v in vars(ag).items() if torch.is_tensor(v)}
    g = wats_hip.SymNormGraph(ag)
    assert g.ag is ag and g.indices is ag.indices
    assert all(torch.equal(getattr(ag, k), v) for k, v in before.items())
    ref = graph("loops")[0]
    assert torch.equal(g.dinv, ref.dinv) and torch.equal(g.indices, ref.indices)
    with pytest.raises(ValueError, match="self_loops"):
        wats_hip.SymNormGraph(wats_hip.AttentionGraph(torch.tensor([[0, 1], [1, 2]]), 3, self_loops=False, device=DEV))


@pytest.mark.parametrize("name", ["directed", "star"])
def test_relu_epilogue(name):
    g, src, dst, n = graph(name)
    C = 40
    x, bias, _ = inputs(n, C, 7)
    dinv = g.dinv.cpu()
    pre64 = R.sym_norm_edges(src, dst, x, dinv, bias, False, torch.float64)
    pre32 = R.sym_norm_edges(src, dst, x, dinv, bias, False, torch.float32)
    bound, _ = R.error_bound(pre32, pre64)
    below = pre64 <= -bound
    assert below.any() and (~below).any()
    # a gradient that arrives only where the pre-activation is negative by more than the bound
    G = torch.randn(n, C, generator=torch.Generator().manual_seed(8)).float() * below
    out, gx, gb = kernel(g, x, bias, G, True)
    assert (out.cpu()[below] == 0).all(), "exactly 0 where (A64 + bias) <= -bound"
    assert (out >= 0).all(), "never negative"
    assert (gx == 0).all() and (gb == 0).all(), "the ReLU passes no gradient there"


@pytest.mark.parametrize("name", ["directed", "star"])
def test_same_bits_twice_and_for_any_edge_order(name):
    g, src, dst, n = graph(name)
    x, bias, G = inputs(n, 40, 10)
    raw_src, raw_dst, _ = GRAPHS[name]()
    rng = np.random.default_rng(11)
    dup = rng.integers(0, len(raw_src), len(raw_src) // 3)            # a third of the edges twice
    s2, d2 = np.concatenate([raw_src, raw_src[dup]]), np.concatenate([raw_dst, raw_dst[dup]])
    perm = rng.permutation(len(s2))
    ei = torch.from_numpy(np.stack([s2[perm], d2[perm]]).astype(np.int64))
    other = wats_hip.SymNormGraph(ei, n, device=DEV)
    for relu in (False, True):
        first, again, shuffled = kernel(g, x, bias, G, relu), kernel(g, x, bias, G, relu), kernel(other, x, bias, G, relu)
        for u, v, w in zip(first, again, shuffled):
            assert torch.equal(u, v) and torch.equal(u, w)


@pytest.mark.parametrize("name,j", [("directed", 7), ("star", 5), ("star", 0)])
def test_a_nan_row_reaches_exactly_the_rows_that_list_it(name, j):
    g, src, dst, n = graph(name)
    x, bias, _ = inputs(n, 40, 12)
    hit = np.zeros(n, bool)
    hit[dst[src == j]] = True                  # j itself among them (its self loop)
    assert hit[j] and (name != "star" or hit[0]) and not hit.all()
    bad = x.clone()
    bad[j] = float("nan")
    hit_t = torch.from_numpy(hit)
    for relu in (False, True):
        clean = wats_hip.sym_norm_aggregate(g, x.to(DEV), bias.to(DEV), relu).cpu()
        out = wats_hip.sym_norm_aggregate(g, bad.to(DEV), bias.to(DEV), relu).cpu()
        assert torch.isnan(out[hit_t]).all(), f"relu={relu}: every column of a row that lists {j} is NaN"
        assert torch.equal(out[~hit_t], clean[~hit_t]), f"relu={relu}: every other row has the clean bits"


def raw_call(g, x, out, bias=None, relu=False, long_rows="own", transposed=False):
    lib = wats_hip._lib.load()
    indptr, indices = (g.t_indptr, g.t_indices) if transposed else (g.indptr, g.indices)
    if isinstance(long_rows, str):
        long_rows = g.t_long_rows if transposed else g.long_rows
    n_long = 0 if long_rows is None else int(long_rows.numel())
    rc = lib.wg_symnorm_aggregate(g.n, g.nnz, ptr(indptr), ptr(indices), n_long, ptr(long_rows) if n_long else None,
                                  ptr(g.dinv), x.shape[1], ptr(x), ptr(bias), int(relu), ptr(out),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def offset_view(t):
    """The same (n, C) values at a base one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("name", ["directed", "star"])
def test_misaligned_buffers_and_odd_widths_take_the_dword_path(name):
    g, _, _, n = graph(name)
    x, bias, _ = inputs(n, 40, 13)
    xd, bd = x.to(DEV), bias.to(DEV)
    assert xd.data_ptr() % 16 == 0
    aligned = wats_hip.sym_norm_aggregate(g, xd, bd, True)
    # the same sums in the same order, loaded dword by dword: the same bits
    assert torch.equal(wats_hip.sym_norm_aggregate(g, offset_view(xd), bd, True), aligned)
    out = offset_view(torch.zeros(n, 40))
    assert raw_call(g, xd, out, bd, True) == 0 and torch.equal(out, aligned)
    out = offset_view(torch.zeros(n, 40))
    assert raw_call(g, offset_view(xd), out, bd, True) == 0 and torch.equal(out, aligned)
    # C = 41 (never 16-byte rows): its first 40 columns are the C = 40 problem
    x41 = torch.cat([xd, torch.randn(n, 1, device=DEV)], 1).contiguous()
    b41 = torch.cat([bd, torch.ones(1, device=DEV)])
    assert torch.equal(wats_hip.sym_norm_aggregate(g, x41, b41, True)[:, :40], aligned)
    # narrower problems: a short row's sum is one chain in ascending position at any width (the same bits); a hub's
    # entries are dealt to as many sub-groups as the width leaves (another order: one rounding apart)
    short = torch.ones(n, dtype=torch.bool, device=DEV)
    short[g.long_rows.long()] = False
    for C in (3, 7):
        got = wats_hip.sym_norm_aggregate(g, xd[:, :C].contiguous(), bd[:C].contiguous(), True)
        assert torch.equal(got[short], aligned[:, :C][short])
        assert float((got - aligned[:, :C]).abs().max()) <= 4 * EPS * float(aligned.abs().max())


def test_direct_abi_calls():
    lib = wats_hip._lib.load()
    g, src, dst, n = graph("star")
    x, bias, G = inputs(n, 40, 14)
    xd, bd, Gd = x.to(DEV), bias.to(DEV), G.to(DEV)
    want = wats_hip.sym_norm_aggregate(g, xd, bd, False)
    out = torch.full_like(xd, float("nan"))
    assert raw_call(g, xd, out, bd) == 0 and torch.equal(out, want)
    # no list at all (n_long = 0, NULL): the hub is walked by one sub-group, in another order: right to the bound
    out = torch.full_like(xd, float("nan"))
    assert raw_call(g, xd, out, bd, long_rows=None) == 0
    dinv = g.dinv.cpu()
    r64 = R.sym_norm_edges(src, dst, x, dinv, bias, False, torch.float64)
    r32 = R.sym_norm_edges(src, dst, x, dinv, bias, False, torch.float32)
    R.assert_close(out, r32, r64, "unlisted hub")
    assert torch.equal(out[1:], want[1:])
    # a listed row that is not long stays with the sub-group kernel: the same bits; so does a list without the hub
    out = torch.full_like(xd, float("nan"))
    assert raw_call(g, xd, out, bd, long_rows=torch.tensor([0, 5, 9], dtype=torch.int32, device=DEV)) == 0
    assert torch.equal(out, want)
    out = torch.full_like(xd, float("nan"))
    assert raw_call(g, xd, out, bd, long_rows=torch.tensor([5], dtype=torch.int32, device=DEV)) == 0
    R.assert_close(out, r32, r64, "a list without the hub")
    # the backward entry: the transposed structure, no bias, no ReLU
    gx = torch.full_like(xd, float("nan"))
    assert raw_call(g, Gd, gx, transposed=True) == 0
    assert torch.equal(gx, kernel(g, x, None, G, False)[1])
    gx2 = torch.full_like(xd, float("nan"))
    assert raw_call(g, Gd, gx2, long_rows=None, transposed=True) == 0
    b64 = R.sym_norm_edges(dst, src, G, dinv, None, False, torch.float64)
    b32 = R.sym_norm_edges(dst, src, G, dinv, None, False, torch.float32)
    R.assert_close(gx2, b32, b64, "unlisted transposed hub")
    # argument errors and empty problems: no launch
    keep = out.clone()
    assert lib.wg_symnorm_aggregate(0, 0, None, None, 0, None, None, 40, None, None, 0, None, None) == 0
    assert lib.wg_symnorm_aggregate(n, g.nnz, ptr(g.indptr), ptr(g.indices), 0, None, ptr(g.dinv), 0, ptr(xd), None, 0,
                                    ptr(out), None) == 0
    assert lib.wg_symnorm_aggregate(n, g.nnz, ptr(g.indptr), ptr(g.indices), 0, None, ptr(g.dinv), 40, ptr(xd), None, 0,
                                    ptr(xd), None) == -1 and b"alias" in lib.wg_last_error()
    assert lib.wg_symnorm_aggregate(n, g.nnz, ptr(g.indptr), ptr(g.indices), 1, None, ptr(g.dinv), 40, ptr(xd), None, 0,
                                    ptr(out), None) == -1 and b"long_rows" in lib.wg_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, keep)
    empty = wats_hip.sym_norm_aggregate(g, torch.empty(n, 0, device=DEV))
    assert empty.shape == (n, 0)


# ---------------------------------------------------------------------------------------------------------
# the layer and the calibrator
# ---------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def deterministic_torch():
    """index_add_ on the device adds with float atomics by default: the float32 reference's own error, which
    sets the bound, would change from run to run."""
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before)


@pytest.mark.parametrize("name", ["directed", "star"])
@pytest.mark.parametrize("relu", [False, True])
def test_gcn_conv_gradients(name, relu):
    g, src, dst, n = graph(name)
    cin, cout = 40, 7
    gen = torch.Generator().manual_seed(15)
    x = torch.randn(n, cin, generator=gen).to(DEV)
    w = torch.randn(n, cout, generator=gen).to(DEV)
    torch.manual_seed(16)
    conv = wats_hip.GCNConv(cin, cout, g)
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == {"lin.weight": (cout, cin), "bias": (cout,)}
    with torch.no_grad():
        conv.bias.copy_(torch.randn(cout, generator=gen) * 0.5)
    xd = x.clone().requires_grad_(True)
    out = conv(xd, relu=relu)
    (out * w).sum().backward()
    got = {"lin.weight": conv.lin.weight.grad, "bias": conv.bias.grad, "x": xd.grad}

    def ref(dtype):
        p = {k: v.detach().clone().requires_grad_(True) for k, v in conv.state_dict().items()}
        xr = x.clone().requires_grad_(True)
        with deterministic_torch():
            o = R.gcn_conv(p["lin.weight"], p["bias"], src, dst, xr, g.dinv, relu, torch.float32, aggregate_dtype=dtype)
            (o * w).sum().backward()
        return o.detach(), {"lin.weight": p["lin.weight"].grad, "bias": p["bias"].grad, "x": xr.grad}

    o64, g64 = ref(torch.float64)
    o32, g32 = ref(torch.float32)
    R.assert_close(out, o32, o64, f"conv {name} relu={relu} out")
    for k in got:
        R.assert_close(got[k], g32[k], g64[k], f"conv {name} relu={relu} grad {k}")


class LogitModel(torch.nn.Module):
    """A base model that ignores the graph: forward(x, adj) as the calibrators call it."""

    def __init__(self, nfeat, nclass):
        super().__init__()
        self.lin = torch.nn.Linear(nfeat, nclass)

    def forward(self, x, adj=None, **kwargs):
        return self.lin(x)


SCALING = ("scaling_model.0.lin.weight", "scaling_model.0.bias", "scaling_model.1.lin.weight", "scaling_model.1.bias")
_cora = {}


def cora():
    """The Cora-shaped problem, built once: edges, a frozen base model with informative logits, a split and a
    fixed state of the scaling model."""
    if not _cora:
        src, dst, n, y = R.cora_like_edges()
        gen = torch.Generator().manual_seed(17)
        yt = torch.from_numpy(y)
        x = (F.one_hot(yt, 7).float() + 0.8 * torch.randn(n, 7, generator=gen)).to(DEV)
        base = LogitModel(7, 7)
        with torch.no_grad():
            base.lin.weight.copy_(2.0 * torch.eye(7) + 0.1 * torch.randn(7, 7, generator=gen))
            base.lin.bias.zero_()
        val = torch.zeros(n, dtype=torch.bool)
        val[torch.randperm(n, generator=gen)[:500]] = True
        state = {SCALING[0]: torch.randn(7, 7, generator=gen) * 0.5, SCALING[1]: torch.randn(7, generator=gen) * 0.1,
                 SCALING[2]: torch.randn(7, 7, generator=gen) * 0.5, SCALING[3]: torch.randn(7, generator=gen) * 0.1}
        ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64)).to(DEV)
        rs, rd = R.with_self_loops(src, dst, n)
        _cora.update(n=n, x=x, y=yt.to(DEV), val=val.to(DEV), base=base.to(DEV), ei=ei, rs=rs, rd=rd,
                     state={k: v.to(DEV) for k, v in state.items()}, graph=wats_hip.SymNormGraph(ei, n, device=DEV))
    return _cora


def calibrator(c, **kw):
    cal = wats_hip.CaGCN(c["base"], c["x"], c["y"], None, c["val"], graph=c["graph"], verbose=False, **kw)
    return cal


def set_state(cal, state):
    missing = cal.load_state_dict(state, strict=False)
    assert not missing.unexpected_keys and all(k.startswith("base_model.") for k in missing.missing_keys)


def test_cagcn_forward_on_a_cora_shaped_graph():
    c = cora()
    cal = calibrator(c, epochs=0)
    assert cal.history == [] and cal.n_classes == 7
    assert set(SCALING) <= set(cal.state_dict()), "the scaling model is part of the state dict"
    assert all(not p.requires_grad for p in c["base"].parameters())
    set_state(cal, c["state"])
    cal.eval()
    with torch.no_grad():
        out = cal(c["x"], None)
        logits = cal.base_predict(c["x"], None)
        with deterministic_torch():
            r64 = R.cagcn_forward(c["state"], c["rs"], c["rd"], logits, c["graph"].dinv, torch.float32, torch.float64)
            r32 = R.cagcn_forward(c["state"], c["rs"], c["rd"], logits, c["graph"].dinv, torch.float32, torch.float32)
    assert out.shape == (c["n"], 7)
    R.assert_close(out, r32, r64, "CaGCN forward")
    lse = torch.logsumexp(out.double(), dim=1).abs().max()
    print(f"CaGCN forward: max |logsumexp| = {float(lse):.3e} (bound {4 * EPS * 7:.3e})")
    assert float(lse) <= 4 * EPS * 7, "every row is a row of log-probabilities"
    # an adj that is not a dense tensor (here: none at all) needs graph=
    with pytest.raises(ValueError, match="graph="):
        wats_hip.CaGCN(c["base"], c["x"], c["y"], None, c["val"], verbose=False, epochs=0)


def reference_training(c, dtype, epochs, alpha=0.5):
    """calib_train's loop (CaGCN.py:118-139) on the restatement with the aggregation in `dtype`."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in c["state"].items()}
    opt = torch.optim.Adam([p[k] for k in SCALING], lr=0.01, weight_decay=5e-4)
    with torch.no_grad():
        logits = c["base"](c["x"], None)
    losses = []
    with deterministic_torch():
        for _ in range(epochs):
            opt.zero_grad()
            out = R.cagcn_forward(p, c["rs"], c["rd"], logits, c["graph"].dinv, torch.float32, dtype)
            loss = F.nll_loss(out[c["val"]], c["y"][c["val"]]) + \
                alpha * wats_hip.calibration_loss(out[c["val"]], c["y"][c["val"]])
            loss.backward()
            opt.step()
            losses.append(loss.item())
    return torch.tensor(losses, dtype=torch.float64)


def test_cagcn_training_follows_the_restatement():
    c = cora()
    cal = calibrator(c, epochs=0, dropout=0.0)
    set_state(cal, c["state"])
    cal.epochs = 5
    assert cal.fit() is cal
    got = torch.tensor(cal.history, dtype=torch.float64)
    l64, l32 = reference_training(c, torch.float64, 5), reference_training(c, torch.float32, 5)
    for e in range(5):
        print(f"epoch {e}: loss {got[e]:.9f} restatement float64 {l64[e]:.9f} float32 {l32[e]:.9f}")
    assert got.numel() == 5 and torch.isfinite(got).all()
    R.assert_close(got, l32, l64, "CaGCN training losses")


def test_cagcn_default_training_run_finishes():
    c = cora()
    torch.manual_seed(18)
    cal = calibrator(c)                                    # dropout 0.5, up to 100 epochs, patience 10
    h = cal.history
    assert 1 <= len(h) <= 100 and all(np.isfinite(h))
    if len(h) < 100:                                       # stopped by patience: ten epochs without a new best
        assert len(h) > 10 and min(h[:-10]) <= min(h[-10:])
    assert not cal.training
    assert all(torch.isfinite(p).all() for p in cal.parameters())
    assert isinstance(cal.scaling_model, torch.nn.ModuleList) and len(cal.scaling_model) == 2
    assert cal.dropout.p == 0.5


def test_cagcn_graph_selection():
    """graph= wins; else the construction adj's graph; another dense adj (or the same one changed in place) gets a
    graph of its own, kept while the tensor is unchanged."""
    src, dst, n = GRAPHS["loops"]()
    adj = torch.zeros(n, n)
    adj[torch.from_numpy(src), torch.from_numpy(dst)] = 1.0
    adj = adj.to(DEV)
    gen = torch.Generator().manual_seed(19)
    x = torch.randn(n, 5, generator=gen).to(DEV)
    y = torch.randint(0, 4, (n,), generator=gen).to(DEV)
    val = torch.arange(0, n, 3, device=DEV)
    base = LogitModel(5, 4).to(DEV)
    cal = wats_hip.CaGCN(base, x, y, adj, val, epochs=2, verbose=False).eval()
    ref = graph("loops")[0]
    assert torch.equal(cal.graph.indices, ref.indices) and cal.graph_for(adj) is cal.graph
    with torch.no_grad():
        out = cal(x, adj)
        fixed = wats_hip.CaGCN(base, x, y, adj, val, graph=ref, epochs=0, verbose=False).eval()
        set_state(fixed, {k: v for k, v in cal.state_dict().items() if k.startswith("scaling_model.")})
        assert torch.equal(fixed(x, adj), out) and torch.equal(fixed(x, None), out)
        other = adj.clone()
        other[3, 4] = 1.0 - other[3, 4]
        g2 = cal.graph_for(other)
        assert g2 is not cal.graph and cal.graph_for(other) is g2 and cal.graph_for(adj) is cal.graph
        assert g2.nnz != cal.graph.nnz
        assert not torch.equal(cal(x, other), out)
        assert fixed.graph_for(other) is ref
        other[3, 4] = 1.0 - other[3, 4]                    # changed in place: a new version, the old graph again
        g3 = cal.graph_for(other)
        assert g3 is not g2 and torch.equal(g3.indices, cal.graph.indices)
        assert torch.equal(cal(x, other), out)
    with pytest.raises(ValueError, match="graph="):
        cal(x, None)
    with pytest.raises(ValueError, match="square"):
        cal(x, adj[:, :5])


def test_attack_gradient_through_a_calibrated_sparse_gcn():
    """d NLL(target) / d adj at probe positions, through CaGCN over SparseCompatibleGCN, against float64 autograd
    through the dense chain (tests/models.py CompatibleGCN on a dense leaf, then the restatement on the fixed
    graph).  The bound is the two-layer model's of tests/test_edge_grad.py: max err / max|ref| <= 1e-4; the float32
    dense chain's own error is measured beside it."""
    import copy

    from models import CompatibleGCN
    from wats_hip.graphgen import rmat_graph
    n = 400
    A = (rmat_graph(n, 3000, seed=7).to_scipy() + sp.eye(n)).toarray().astype(np.float32)
    adj = torch.tensor(A, device=DEV)
    torch.manual_seed(0)
    x = torch.randn(n, 33, device=DEV)
    gen = torch.Generator().manual_seed(20)
    y = torch.randint(0, 7, (n,), generator=gen).to(DEV)
    val = torch.arange(0, n, 3, device=DEV)
    ref32 = CompatibleGCN(33, 7, nhid=64).to(DEV).eval()
    model = wats_hip.SparseCompatibleGCN(33, nclass=7, nhid=64).to(DEV).eval()
    model.load_state_dict(ref32.state_dict())
    ref64 = copy.deepcopy(ref32).double().eval()
    cal = wats_hip.CaGCN(model, x, y, adj, val, epochs=3, verbose=False).eval()
    # about 40 positions around a target with ten neighbours: both directions of ten present and ten absent pairs
    off = A - np.diag(np.diag(A))
    deg = (off != 0).sum(1)
    t = int(np.flatnonzero(deg >= 10)[np.argmin(deg[deg >= 10])])
    present = np.flatnonzero(off[t])[:10]
    absent = np.flatnonzero((off[t] == 0) & (off[:, t] == 0) & (np.arange(n) != t))[:10]
    others = np.concatenate([present, absent])
    rows = np.concatenate([np.full(len(others), t), others])
    cols = np.concatenate([others, np.full(len(others), t)])
    assert len(rows) == 40 and int((A[rows, cols] != 0).sum()) >= 10
    probe = wats_hip.EdgeProbe(rows, cols)
    out = cal(x, adj, probe=probe)
    label = int(y[t])
    (-out[t, label]).backward()
    got = probe.delta.grad
    assert got is not None and got.shape == (40,)

    r, c_ = np.nonzero(A)
    rs, rd = R.with_self_loops(r, c_, n)       # adj[r, c] != 0 is the edge r -> c
    state = {k: v.detach() for k, v in cal.state_dict().items() if k.startswith("scaling_model.")}

    def dense_chain(dtype, base):
        leaf = adj.to(dtype).requires_grad_(True)
        logits = base(x.to(dtype), leaf)
        o = R.cagcn_forward({k: v.to(dtype) for k, v in state.items()}, rs, rd, logits, cal.graph.dinv, dtype)
        (-o[t, label]).backward()
        return o.detach(), leaf.grad[torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV)]

    o64, g64 = dense_chain(torch.float64, ref64)
    with deterministic_torch():
        o32, g32 = dense_chain(torch.float32, ref32)
    scale = float(g64.abs().max())
    assert scale > 0
    err = float((got.double() - g64).abs().max()) / scale
    err32 = float((g32.double() - g64).abs().max()) / scale
    oerr = float((out.detach().double() - o64).abs().max()) / float(o64.abs().max())
    print(f"attack path: output err {oerr:.3e}; probe gradient err / max|ref| = {err:.3e} "
          f"(float32 dense chain {err32:.3e}, bound 1e-4)")
    assert oerr <= 1e-4
    assert torch.isfinite(got).all() and err <= 1e-4
    # both halves carry gradient: the present and the absent positions
    assert float(got[:10].abs().max()) > 0 and float(got[10:20].abs().max()) > 0
