"""GPU tests of the GATS attention layer (csrc/gats.hip, wats_hip/gats.py) against the float64 edge-list
restatement (A) of tests/gats_ref.py.

The bound on every value is measured in the test: err = max|kernel - A_float64| must not exceed
max(2 * max|A_float32 - A_float64|, 4 * 2^-24 * max|A_float64|) (gats_ref.error_bound).  The references of
the attention run on the CPU from edge lists that the tests build themselves (numpy: duplicates merged, self
loops replaced), so the layer's ingestion, its edge direction and its transpose map are under test as well.
The references of the whole layer are (A), in float64 and in float32, wrapped in the layer's own torch steps
(float32, on the layer's device, deterministic torch algorithms): the rounding of those steps is the same on
both sides of the comparison, in a scalar gradient that is a cancelling float32 sum it would otherwise drown
the attention's own error, and the bound does not move from run to run.  The layer's output is also compared
with the whole layer in float64 on the CPU, loosely: that pins the torch steps themselves.
"""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import gats_ref as R  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip import gats  # noqa: E402
from wats_hip._lib import ptr  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def lonely_graph():
    """Node 0 hears from nobody: its only in-edge is its self loop."""
    return np.array([0, 0, 1]), np.array([1, 2, 2]), 3


GRAPHS = {
    "single": lambda: (np.zeros(0, np.int64), np.zeros(0, np.int64), 1),
    "lonely": lonely_graph,
    "path": lambda: R.path_graph(3),
    "symmetric": lambda: R.random_graph(300, 6, False, 1),
    "directed": lambda: R.random_graph(300, 6, True, 2),
    "loops": lambda: R.random_graph(300, 6, True, 3, loops=40),
    "star": lambda: R.star_graph(700, 50),
    # mean row lengths of about 13, 21 and 34 with the self loop: sub-groups of 16, 32 and 64 lanes
    "wide16": lambda: R.random_graph(200, 12, True, 4),
    "wide32": lambda: R.random_graph(120, 20, True, 5),
    "wide64": lambda: R.random_graph(100, 40, True, 6),
}
_cache = {}


def graph(name):
    """(AttentionGraph, src, dst, n): the device graph from the raw edge_index, the reference's edge list from numpy."""
    if name not in _cache:
        src, dst, n = GRAPHS[name]()
        ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
        rs, rd = R.with_self_loops(src, dst, n)
        _cache[name] = (wats_hip.AttentionGraph(ei, n, device=DEV), rs, rd, n)
    return _cache[name]


def inputs(n, C, H, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(n, C, generator=g) * scale).float()
    t = torch.randn(n, H, generator=g).float()
    conf = torch.rand(n, generator=g).float()
    G = torch.randn(n, H, generator=g).float()
    return a, t, conf, G


def reference(src, dst, a, t, conf, G, dtype):
    """(sim, dconf, grad_a, grad_t) of (A) on the CPU in `dtype` from the float32 inputs."""
    ar, tr = a.to(dtype).requires_grad_(True), t.to(dtype).requires_grad_(True)
    sim, dconf = R.attention_edges(src, dst, ar, tr, conf, 0.2, dtype)
    (sim * G.to(dtype)).sum().backward()
    return sim.detach(), dconf.detach(), ar.grad, tr.grad


def kernel(g, a, t, conf, G):
    ad, td = a.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
    sim, dconf = wats_hip.edge_softmax_attention(g, ad, td, conf.to(DEV))
    assert not dconf.requires_grad
    (sim * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return sim.detach(), dconf.detach(), ad.grad, td.grad


def check_all(name, C, H, seed=0, scale=1.0, a_edit=None):
    g, src, dst, n = graph(name)
    a, t, conf, G = inputs(n, C, H, seed, scale)
    if a_edit is not None:
        a_edit(a)
    got = kernel(g, a, t, conf, G)
    r64 = reference(src, dst, a, t, conf, G, torch.float64)
    r32 = reference(src, dst, a, t, conf, G, torch.float32)
    for k, what in enumerate(("sim", "dconf", "grad_a", "grad_t")):
        R.assert_close(got[k], r32[k], r64[k], f"{name} C={C} H={H} {what}")
    return got


WIDTHS = [(name, 40, 8) for name in sorted(GRAPHS)] + [
    ("directed", 1, 1), ("directed", 3, 3), ("directed", 7, 8), ("directed", 41, 3), ("symmetric", 40, 1),
    ("symmetric", 3, 8), ("star", 41, 3), ("star", 7, 1), ("path", 1, 3),
    # more than one tile of 8 heads (sub-group and workgroup rows), the head limit
    ("directed", 7, 9), ("star", 7, 9), ("wide32", 40, 16), ("lonely", 3, 64),
    # node pass: 8 / 32 / 64 lanes per sub-group, and more items than lanes (C = 260: 65 + 1 items, two trips)
    ("directed", 20, 8), ("symmetric", 100, 16), ("path", 260, 3), ("star", 260, 1), ("wide16", 260, 9),
]


@pytest.mark.parametrize("name,C,H", WIDTHS)
def test_forward_and_backward_match_the_float64_restatement(name, C, H):
    check_all(name, C, H)


def test_hub_row_took_the_workgroup_kernels():
    g, src, dst, n = graph("star")
    th = gats.long_row_threshold()
    in_len = np.bincount(dst, minlength=n)
    out_len = np.bincount(src, minlength=n)
    assert in_len[0] == 701 and in_len[0] >= 2 * th, "the hub takes several turns of its workgroup"
    assert g.long_rows.tolist() == [0]                      # by in-degree: the forward and the edge pass
    assert g.t_long_rows.tolist() == [0, 1]                 # node 1 is long by out-degree only: the node pass
    assert out_len[1] >= th > in_len[1]
    assert "long rows=1" in g.describe() and "long nodes=2" in g.describe()
    assert graph("directed")[0].long_rows.numel() == 0


def test_large_logits_do_not_overflow():
    # unit-variance logits times 50: self dots of 40 * 50^2 = 1e5 and cross dots of about 1.6e4, the range that
    # logits of a trained model times 200 reach (times 200 here would give 1.6e6: every softmax a one-hot)
    got = check_all("symmetric", 40, 8, seed=4, scale=50.0)
    assert all(torch.isfinite(x).all() for x in got)
    check_all("star", 40, 8, seed=5, scale=50.0)


def test_zero_logits_take_the_slope_in_the_backward():
    def zero_one(a):
        a[7] = 0.0                                              # every d_7j and d_l7 is exactly 0
    check_all("directed", 40, 8, seed=6, a_edit=zero_one)
    check_all("symmetric", 7, 3, seed=7, a_edit=zero_one)


def test_all_negative_dots():
    """No self loops, edges only between a positive and a negative half: every d_ij < 0 (the leaky branch), and
    the nodes without in-edges give 0."""
    rng = np.random.default_rng(8)
    n, m = 60, 200
    src, dst = rng.integers(0, n // 2, m), rng.integers(n // 2, n, m)
    flip = rng.random(m) < 0.5
    src, dst = np.where(flip, dst, src), np.where(flip, src, dst)
    g = wats_hip.AttentionGraph(torch.from_numpy(np.stack([src, dst])), n, self_loops=False, device=DEV)
    key = np.unique(dst * n + src)
    rs, rd = key % n, key // n
    a, t, conf, G = inputs(n, 40, 8, 9)
    a = a.abs() + 0.1
    a[n // 2:] *= -1.0
    assert ((a[rs] * a[rd]).sum(1) < 0).all()
    got = kernel(g, a, t, conf, G)
    r64, r32 = reference(rs, rd, a, t, conf, G, torch.float64), reference(rs, rd, a, t, conf, G, torch.float32)
    for k, what in enumerate(("sim", "dconf", "grad_a", "grad_t")):
        R.assert_close(got[k], r32[k], r64[k], f"negative dots {what}")


@pytest.mark.parametrize("name", ["directed", "star"])
def test_same_bits_twice_and_for_any_edge_order(name):
    g, src, dst, n = graph(name)
    a, t, conf, G = inputs(n, 40, 8, 10)
    first = kernel(g, a, t, conf, G)
    again = kernel(g, a, t, conf, G)
    raw_src, raw_dst, _ = GRAPHS[name]()
    perm = np.random.default_rng(11).permutation(len(raw_src))
    ei = torch.from_numpy(np.stack([raw_src[perm], raw_dst[perm]]).astype(np.int64))
    shuffled = kernel(wats_hip.AttentionGraph(ei, n, device=DEV), a, t, conf, G)
    for u, v, w in zip(first, again, shuffled):
        assert torch.equal(u, v) and torch.equal(u, w)


def test_graph_inputs_agree():
    """edge_index, dense adjacency, (indptr, indices) and DeviceCSR describe the same graph."""
    src, dst, n = GRAPHS["loops"]()
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    dense = torch.zeros(n, n)
    dense[ei[0], ei[1]] = 1.0
    csr = wats_hip.edge_index_to_csr(ei, n, device=DEV)
    ref = graph("loops")[0]
    for other in (dense.to(DEV), (csr.indptr, csr.indices), csr):
        g = wats_hip.AttentionGraph(other, n, device=DEV)
        assert torch.equal(g.indptr, ref.indptr) and torch.equal(g.indices, ref.indices)
        assert torch.equal(g.t_pos, ref.t_pos) and torch.equal(g.deg_inv, ref.deg_inv)


def test_transpose_map():
    g, src, dst, n = graph("directed")
    # the CSR by destination is the reference's edge list sorted by (dst, src)
    e_src, e_dst = g.edge_list()
    assert e_src.cpu().tolist() == src.tolist() and e_dst.cpu().tolist() == dst.tolist()
    order = np.lexsort((dst, src))                      # by (src, dst): the transposed order
    assert g.t_pos.cpu().tolist() == order.tolist()
    assert g.t_indices.cpu().tolist() == dst[order].tolist()
    assert g.t_indptr.cpu().tolist() == np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).tolist()
    deg = np.bincount(src, minlength=n).astype(np.float32)
    assert torch.equal(g.deg_inv.cpu(), torch.from_numpy(np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0).astype(np.float32)))


@pytest.mark.parametrize("name", ["path", "star", "directed"])
@pytest.mark.parametrize("max_hop", [1, 2, 3])
def test_bfs_levels(name, max_hop):
    src, dst, n = GRAPHS[name]()
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    rng = np.random.default_rng(12)
    masks = [rng.random(n) < 0.1, np.zeros(n, bool), np.arange(n) == (1 if name == "star" else 0)]
    for mask in masks:
        want = R.bfs_levels(src, dst, mask, max_hop)
        got = wats_hip.shortest_path_length(ei.to(DEV), torch.from_numpy(mask), max_hop)
        assert got.dtype == torch.int64 and got.cpu().tolist() == want.tolist()
        assert graph(name)[0].bfs(torch.from_numpy(mask), max_hop).cpu().tolist() == want.tolist()
    assert set(np.unique(want).tolist()) <= set(range(max_hop)) | {R.INT64_MAX}


def test_direct_abi_calls():
    lib = wats_hip._lib.load()
    g, src, dst, n = graph("directed")
    a, t, conf, _ = (x.to(DEV) for x in inputs(n, 40, 8, 13))
    nul = [None] * 6
    assert lib.wg_gat_forward(0, 0, None, None, 0, None, 40, 8, None, None, None, 0.2, *nul, None) == 0
    assert lib.wg_gat_backward(0, 0, None, None, 0, None, None, None, None, 0, None, 40, 8, None, None, None, None,
                               None, None, 0.2, None, None, None, None) == 0
    sim = torch.empty(n, 8, device=DEV)
    dconf = torch.empty(n, device=DEV)
    args = lambda C, a_ptr: (n, g.nnz, ptr(g.indptr), ptr(g.indices), 0, None, C, 8, a_ptr, ptr(t), ptr(conf), 0.2,
                             ptr(sim), ptr(dconf), None, None, None, None)
    assert lib.wg_gat_forward(*args(0, ptr(a))) == -1 and b"C must be" in lib.wg_last_error()
    assert lib.wg_gat_forward(*args(40, None)) == -1 and b"NULL" in lib.wg_last_error()
    e_save = torch.empty(g.nnz, dtype=torch.float64, device=DEV)
    partial = list(args(40, ptr(a)))
    partial[14] = ptr(e_save)
    assert lib.wg_gat_forward(*partial) == -1 and b"together" in lib.wg_last_error()
    # the save group given as NULL: the same forward output
    with_save = g.forward(a, t, conf, 0.2, save=True)
    without = g.forward(a, t, conf, 0.2, save=False)
    assert without[2] is None and torch.equal(with_save[0], without[0]) and torch.equal(with_save[1], without[1])
    # a multi-turn row without the saved logits recomputes them: still the same bits
    star = graph("star")[0]
    a2, t2, conf2, _ = (x.to(DEV) for x in inputs(star.n, 41, 3, 14))
    u, v = star.forward(a2, t2, conf2, 0.2, save=True), star.forward(a2, t2, conf2, 0.2, save=False)
    assert torch.equal(u[0], v[0]) and torch.equal(u[1], v[1])
    # misaligned operands take the dword loads: same values to the bound
    buf = torch.empty(n * 40 + 1, device=DEV)
    a_off = buf[1:].view(n, 40)
    a_off.copy_(a)
    assert a_off.data_ptr() % 16 != 0
    off = g.forward(a_off, t, conf, 0.2)
    assert float((off[0] - without[0]).abs().max()) <= 4 * 2.0 ** -24 * float(without[0].abs().max())


# ---------------------------------------------------------------------------------------------------------
# the layer and the calibrator
# ---------------------------------------------------------------------------------------------------------
PARAMS = ("temp_lin.weight", "conf_coef", "bias", "train_a", "dist1_a")


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


def layer_reference_grads(state, src, dst, x, dist, weights, dtype):
    """Gradients of sum(out * weights) w.r.t. the five parameters through (A) in `dtype`, wrapped in the layer's
    own torch steps: float32, on the layer's device.  What differs from the layer is the attention alone."""
    p = {k: state[k].detach().clone().requires_grad_(True) for k in PARAMS}
    with deterministic_torch():
        out = R.layer_reference(p, src, dst, x, dist, 0.2, torch.float32, attention_dtype=dtype)
        (out * weights).sum().backward()
    return out.detach(), {k: p[k].grad for k in PARAMS}


@pytest.mark.parametrize("name", ["directed", "star"])
def test_layer_parameter_gradients(name):
    g, src, dst, n = graph(name)
    C, H = 40, 8
    gen = torch.Generator().manual_seed(15)
    x = (torch.randn(n, C, generator=gen) * 2.0).to(DEV)
    mask = torch.rand(n, generator=gen) < 0.2
    torch.manual_seed(16)
    layer = wats_hip.CalibAttentionLayer(C, 1, g, n, mask, heads=H, device=DEV)
    state = layer.state_dict()
    assert {k: tuple(v.shape) for k, v in state.items()} == {
        "temp_lin.weight": (H, C), "conf_coef": (), "bias": (1,), "train_a": (1,), "dist1_a": (1,),
        "dist_to_train": (n,)}
    raw_src, raw_dst, _ = GRAPHS[name]()
    assert state["dist_to_train"].cpu().tolist() == R.bfs_levels(raw_src, raw_dst, mask.numpy(), 2).tolist()
    with torch.no_grad():
        layer.conf_coef.fill_(0.3)
        layer.train_a.fill_(1.25)
        layer.dist1_a.fill_(0.8)
    w = torch.randn(n, 1, generator=gen).to(DEV)
    out = layer(x)
    assert out.shape == (n, 1)
    (out * w).sum().backward()
    state = layer.state_dict()
    o64, g64 = layer_reference_grads(state, src, dst, x, state["dist_to_train"], w, torch.float64)
    o32, g32 = layer_reference_grads(state, src, dst, x, state["dist_to_train"], w, torch.float32)
    R.assert_close(out, o32, o64, f"layer {name} out")
    # the layer's torch steps themselves, against the whole layer in float64 on the CPU.  Loose on purpose: it
    # pins what the steps compute, not their float32 rounding (dconf alone is a sum of up to 701 confidences
    # rounded to float32, scaled by conf_coef / deg: a few 1e-5 of the output at most)
    cpu64 = {k: state[k].detach().cpu().double() for k in PARAMS}
    full = R.layer_reference(cpu64, src, dst, x.cpu(), state["dist_to_train"].cpu(), 0.2, torch.float64)
    err = float((out.detach().double().cpu() - full).abs().max())
    print(f"layer {name} out vs float64 CPU layer: err={err:.3e} of {float(full.abs().max()):.3e}")
    assert err <= 1e-4 * float(full.abs().max())
    for k in PARAMS:
        grad = dict(layer.named_parameters())[k].grad
        R.assert_close(grad, g32[k], g64[k], f"layer {name} grad {k}")


def cora_like(seed=42, n=2708, nfeat=1433, ncls=7, avg_deg=3.9):
    """The Cora-shaped graph of tests/test_harness.py: SBM classes, sparse row-normalised features, the
    Planetoid split, a dense float32 adjacency without self loops."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, ncls, n)
    m = int(n * avg_deg / 2)
    src = rng.integers(0, n, m)
    same = rng.random(m) < 0.85
    by_cls = [np.flatnonzero(y == c) for c in range(ncls)]
    dst = np.where(same, [by_cls[y[s]][rng.integers(0, len(by_cls[y[s]]))] for s in src], rng.integers(0, n, m))
    keep = src != dst
    adj = np.zeros((n, n), np.float32)
    adj[src[keep], dst[keep]] = 1.0
    adj[dst[keep], src[keep]] = 1.0
    proto = rng.random((ncls, nfeat)) < 0.02
    x = ((rng.random((n, nfeat)) < 0.004) | (proto[y] & (rng.random((n, nfeat)) < 0.5))).astype(np.float32)
    x /= np.maximum(x.sum(1, keepdims=True), 1)
    train = np.zeros(n, bool)
    for c in range(ncls):
        train[np.flatnonzero(y == c)[:20]] = True
    rest = np.flatnonzero(~train)
    rng.shuffle(rest)
    val = np.zeros(n, bool)
    val[rest[:500]] = True
    t = torch.from_numpy
    return t(x), t(y.astype(np.int64)), t(adj), t(train), t(val)


def test_gats_calibrator_on_the_harness_graph():
    from models import CompatibleGCN
    torch.manual_seed(42)
    x, y, adj, train_mask, val_mask = (v.to(DEV) for v in cora_like())
    n = x.shape[0]
    base = CompatibleGCN(x.shape[1], 7, nhid=64, dropout=0.5).to(DEV)
    opt = torch.optim.Adam(base.parameters(), lr=0.01, weight_decay=5e-4)
    base.train()
    for _ in range(40):
        opt.zero_grad()
        F.nll_loss(F.log_softmax(base(x, adj)[train_mask], dim=1), y[train_mask]).backward()
        opt.step()
    base.eval()
    cal = wats_hip.GATSCalibrator(base, x, y, adj, val_mask, epochs=3, verbose=False)
    assert all(not p.requires_grad for p in base.parameters())
    cal.eval()
    with torch.no_grad():
        out = cal(x, adj)
        logits = base(x, adj)
        temp = cal.graph_temperature_scale(logits)
    assert out.shape == (n, 7) and torch.isfinite(out).all()
    assert float((out.exp().sum(1) - 1).abs().max()) <= 1e-5
    assert temp.shape == (n, 7) and float(temp.min()) > 0
    layer = cal.calib_attention
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == {
        "temp_lin.weight": (8, 7), "conf_coef": (), "bias": (1,), "train_a": (1,), "dist1_a": (1,),
        "dist_to_train": (n,)}
    assert set(layer.dist_to_train.unique().tolist()) <= {0, 1, R.INT64_MAX}
    # a second instance on the sparse form of the same graph, with the first one's state: the same bits
    ei = adj.nonzero().t().contiguous()
    other = wats_hip.GATS(base, x, y, adj, val_mask, graph=ei, epochs=1, verbose=False)
    other.load_state_dict(cal.state_dict())
    other.eval()
    with torch.no_grad():
        assert torch.equal(other(x, adj), out)
    # one training step's parameter gradients against (A)
    cal.zero_grad()
    F.nll_loss(cal(x, adj)[val_mask], y[val_mask]).backward()
    src, dst = R.with_self_loops(ei[0].cpu().numpy(), ei[1].cpu().numpy(), n)
    state = layer.state_dict()

    def ref(dtype):
        p = {k: state[k].detach().clone().requires_grad_(True) for k in PARAMS}
        with deterministic_torch():
            T = R.layer_reference(p, src, dst, logits, state["dist_to_train"], 0.2, torch.float32, attention_dtype=dtype)
            F.nll_loss(F.log_softmax(logits / T, dim=1)[val_mask], y[val_mask]).backward()
        return {k: p[k].grad for k in PARAMS}

    g64, g32 = ref(torch.float64), ref(torch.float32)
    for k in PARAMS:
        R.assert_close(dict(layer.named_parameters())[k].grad, g32[k], g64[k], f"calibrator grad {k}")
