"""CPU tests of the GATS layer's yardsticks (tests/gats_ref.py) and of the host side of wats_hip.gats: the
two restatements agree, a hand-checked path graph, the BFS restatement's quirks, the backward formulas that
csrc/gats.hip implements against autograd, the layer's state layout and its refusal to run without a GPU."""
import math

import numpy as np
import pytest
import torch

import gats_ref as R
import wats_hip
from wats_hip import gats


def inputs(n, C, H, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(n, C, generator=g) * scale).float()
    t = torch.randn(n, H, generator=g).float()
    conf = torch.rand(n, generator=g).float()
    return a, t, conf


GRAPHS = {
    "symmetric": lambda: R.random_graph(40, 5, False, 1),
    "directed": lambda: R.random_graph(37, 4, True, 2, loops=3),
    "sparse": lambda: R.random_graph(25, 1, True, 3),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_edge_list_and_dense_restatements_agree(name):
    src, dst, n = GRAPHS[name]()
    src, dst = R.with_self_loops(src, dst, n)
    a, t, conf = inputs(n, 7, 3, 5)
    out = []
    for fn in (R.attention_edges, R.attention_dense):
        a64, t64 = a.double().requires_grad_(True), t.double().requires_grad_(True)
        sim, dconf = fn(src, dst, a64, t64, conf)
        g = torch.Generator().manual_seed(9)
        (sim * torch.randn(sim.shape, generator=g, dtype=torch.float64)).sum().backward()
        out.append((sim.detach(), dconf.detach(), a64.grad, t64.grad))
    for u, v, what in zip(out[0], out[1], ("sim", "dconf", "grad_a", "grad_t")):
        assert float((u - v).abs().max()) <= 1e-12 * max(float(v.abs().max()), 1.0), what


def test_path_graph_by_hand():
    """0 - 1 - 2 with C = 2: the middle node hears from 0, 1 and 2."""
    src, dst, n = R.path_graph(3)
    src, dst = R.with_self_loops(src, dst, n)
    assert sorted(zip(dst.tolist(), src.tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2)]
    a = torch.tensor([[1.0, 0.0], [1.0, 1.0], [-2.0, 0.5]])
    t = torch.tensor([[1.0], [10.0], [100.0]])
    conf = torch.tensor([0.5, 0.25, 1.0])
    # d_10 = 1, d_11 = 2, d_12 = -2 + 0.5 = -1.5 -> e = 1, 2, 0.2 * -1.5 = -0.3
    w = [math.exp(1.0 - 2.0), math.exp(0.0), math.exp(-0.3 - 2.0)]
    p = [v / sum(w) for v in w]
    for fn in (R.attention_edges, R.attention_dense):
        sim, dconf = fn(src, dst, a, t, conf)
        assert abs(float(sim[1, 0]) - (p[0] * 1.0 + p[1] * 10.0 + p[2] * 100.0)) <= 1e-12
        assert abs(float(dconf[1]) - ((0.25 - 0.5) + 0.0 + (0.25 - 1.0))) <= 1e-15
        # node 0: d_00 = 1, d_01 = 1 -> p = 1/2 each
        assert abs(float(sim[0, 0]) - 5.5) <= 1e-12


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_bfs_restatement_on_a_path(depth):
    src, dst, n = R.path_graph(6)
    mask = np.zeros(n, bool)
    mask[0] = True
    dist = R.bfs_levels(src, dst, mask, depth)
    for i in range(n):
        assert dist[i] == (i if i < depth else R.INT64_MAX)   # nothing at distance >= max_hop is assigned
    assert set(R.bfs_levels(src, dst, mask, 2).tolist()) == {0, 1, R.INT64_MAX}
    assert (R.bfs_levels(src, dst, np.zeros(n, bool), depth) == R.INT64_MAX).all()
    # along the edges' direction only
    one_way = R.bfs_levels(np.array([1]), np.array([0]), np.array([True, False]), 3)
    assert one_way.tolist() == [0, R.INT64_MAX]


def test_backward_formulas_match_autograd():
    """q, m, r, s and the two sums of grad_a as include/wats_hip.h states them (what the kernels compute),
    in numpy per edge, against autograd through (A); one node has zero logits, so d == 0 takes the slope."""
    src, dst, n = R.random_graph(30, 4, True, 7, loops=2)
    src, dst = R.with_self_loops(src, dst, n)
    a, t, conf = inputs(n, 5, 3, 11)
    a[4] = 0.0
    a64, t64 = a.double().requires_grad_(True), t.double().requires_grad_(True)
    sim, _ = R.attention_edges(src, dst, a64, t64, conf)
    G = torch.randn(sim.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    (sim * G).sum().backward()
    an, tn, Gn = a.double().numpy(), t.double().numpy(), G.numpy()
    d = (an[dst] * an[src]).sum(1)
    e = np.where(d > 0, d, 0.2 * d)
    mx = np.full(n, -np.inf)
    np.maximum.at(mx, dst, e)
    ex = np.exp(e - mx[dst])
    den = np.zeros(n)
    np.add.at(den, dst, ex)
    p = ex / den[dst]
    q = (Gn[dst] * tn[src]).sum(1)
    m = np.zeros(n)
    np.add.at(m, dst, p * q)
    s = p * (q - m[dst]) * np.where(d > 0, 1.0, 0.2)
    grad_t = np.zeros_like(tn)
    np.add.at(grad_t, src, p[:, None] * Gn[dst])
    grad_a = np.zeros_like(an)
    np.add.at(grad_a, dst, s[:, None] * an[src])
    np.add.at(grad_a, src, s[:, None] * an[dst])
    assert (d == 0).any()
    assert np.abs(grad_t - t64.grad.numpy()).max() <= 1e-12
    assert np.abs(grad_a - a64.grad.numpy()).max() <= 1e-12


def test_layer_state_layout_is_the_reference():
    assert gats.STATE_LAYOUT == {
        "temp_lin.weight": ("heads", "in_channels"),
        "conf_coef": (),
        "bias": (1,),
        "train_a": (1,),
        "dist1_a": (1,),
        "dist_to_train": ("num_nodes",),
    }
    assert wats_hip.GATS is wats_hip.GATSCalibrator
    assert gats.GATSCalibrator.fit is gats.GATSCalibrator.calib_train
    assert gats.long_row_threshold() == 256


def test_abi_checks_arguments_before_any_device_work():
    lib = wats_hip._lib.load()
    nul = [None] * 6
    assert lib.wg_gat_forward(0, 0, None, None, 0, None, 4, 8, None, None, None, 0.2, *nul, None) == 0
    assert lib.wg_gat_forward(3, 3, None, None, 0, None, 0, 8, None, None, None, 0.2, *nul, None) == -1
    assert b"C must be" in lib.wg_last_error()
    assert lib.wg_gat_forward(3, 3, None, None, 0, None, 4, 65, None, None, None, 0.2, *nul, None) == -1
    assert b"Hh must be" in lib.wg_last_error()
    assert lib.wg_gat_forward(3, 3, None, None, 0, None, 4, 8, None, None, None, 0.2, *nul, None) == -1
    assert b"NULL" in lib.wg_last_error()
    assert lib.wg_bfs_levels(-1, None, None, None, 2, None, None) == -1
    assert lib.wg_csr_transpose_map(2, 1, None, None, None, None, None, None) == -1


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU refusal")
def test_layer_refuses_to_run_without_a_gpu():
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        gats.CalibAttentionLayer(4, 1, ei, 3, torch.tensor([True, False, False]))
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        gats.shortest_path_length(ei, torch.tensor([True, False, False]), 2)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        gats.AttentionGraph(ei, 3)
