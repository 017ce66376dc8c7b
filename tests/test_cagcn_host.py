"""CPU tests of the CaGCN layer's yardsticks (tests/cagcn_ref.py) and of the host side of wats_hip.cagcn: the
two restatements agree, a hand-checked path graph, the degree a directed edge is scaled by, the backward formula
that csrc/symnorm.hip implements against autograd, calibration_loss by hand, the ABI's argument checks, the
exported surface and the refusal to run without a GPU."""
import math

import numpy as np
import pytest
import torch

import cagcn_ref as R
import wats_hip
from wats_hip import cagcn

GRAPHS = {
    "symmetric": lambda: R.random_graph(40, 5, False, 1),
    "directed": lambda: R.random_graph(37, 4, True, 2, loops=3),
    "sparse": lambda: R.random_graph(25, 1, True, 3),
}


def features(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, C, generator=g).float(), torch.randn(C, generator=g).float()


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("relu", [False, True])
def test_edge_list_and_dense_restatements_agree(name, relu):
    src, dst, n = GRAPHS[name]()
    src, dst = R.with_self_loops(src, dst, n)
    x, bias = features(n, 7, 5)
    out = []
    for fn in (R.sym_norm_edges, R.sym_norm_dense):
        x64, b64 = x.double().requires_grad_(True), bias.double().requires_grad_(True)
        y = fn(src, dst, x64, bias=b64, relu=relu)
        g = torch.Generator().manual_seed(9)
        (y * torch.randn(y.shape, generator=g, dtype=torch.float64)).sum().backward()
        out.append((y.detach(), x64.grad, b64.grad))
    for u, v, what in zip(out[0], out[1], ("out", "grad_x", "grad_bias")):
        assert float((u - v).abs().max()) <= 1e-12 * max(float(v.abs().max()), 1.0), what


def test_path_graph_by_hand():
    """0 - 1 - 2: deg = [2, 3, 2] with the loops; x = I makes the output the matrix itself."""
    src, dst, n = R.path_graph(3)
    src, dst = R.with_self_loops(src, dst, n)
    assert R.in_degree(dst, n).tolist() == [2.0, 3.0, 2.0]
    eye = torch.eye(3, dtype=torch.float64)
    for fn in (R.sym_norm_edges, R.sym_norm_dense):
        a = fn(src, dst, eye)
        assert abs(float(a[0, 0]) - 1 / 2) <= 1e-15
        assert abs(float(a[1, 1]) - 1 / 3) <= 1e-15
        assert abs(float(a[0, 1]) - 1 / math.sqrt(6)) <= 1e-15
        assert abs(float(a[1, 0]) - 1 / math.sqrt(6)) <= 1e-15
        assert float(a[0, 2]) == 0.0 and float(a[2, 0]) == 0.0
        assert abs(float(a[2, 2]) - 1 / 2) <= 1e-15


def test_a_source_is_scaled_by_its_own_in_degree():
    """0 -> 1 and 0 -> 2: node 0 sends three messages (its loop among them) but hears only from itself, so its
    factor is 1 / sqrt(1), not 1 / sqrt(3); nodes 1 and 2 hear from 0 and from themselves: 1 / sqrt(2)."""
    src, dst = R.with_self_loops(np.array([0, 0]), np.array([1, 2]), 3)
    assert R.in_degree(dst, 3).tolist() == [1.0, 2.0, 2.0]
    eye = torch.eye(3, dtype=torch.float64)
    for fn in (R.sym_norm_edges, R.sym_norm_dense):
        a = fn(src, dst, eye)
        assert abs(float(a[1, 0]) - 1 / math.sqrt(2)) <= 1e-15      # dinv_1 * dinv_0 = 2^-1/2 * 1
        assert float(a[0, 0]) == 1.0 and float(a[0, 1]) == 0.0      # no message flows back
        assert abs(float(a[1, 1]) - 1 / 2) <= 1e-15


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_gradient_is_the_aggregate_over_the_reversed_edges(name):
    """What the kernel's backward launch computes: the same entry over the transposed structure with the same
    dinv, grad_x[j] = dinv_j sum_{i : j in In(i)} dinv_i g_i."""
    src, dst, n = GRAPHS[name]()
    src, dst = R.with_self_loops(src, dst, n)
    x, _ = features(n, 5, 11)
    dinv = R.in_degree(dst, n).pow(-0.5)
    x64 = x.double().requires_grad_(True)
    y = R.sym_norm_edges(src, dst, x64, dinv)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    (y * g).sum().backward()
    back = R.sym_norm_edges(dst, src, g, dinv)
    assert float((back - x64.grad).abs().max()) <= 1e-13


def test_calibration_loss_by_hand():
    prob = [[0.7, 0.2, 0.1], [0.1, 0.6, 0.3], [0.25, 0.25, 0.5]]
    labels = [0, 2, 2]
    # correct: 1 - 0.7 + 0.2; wrong: 0.6 - 0.3; correct: 1 - 0.5 + 0.25
    want = (0.5 + 0.3 + 0.75) / 3
    assert abs(R.calibration_loss_by_hand(prob, labels) - want) <= 1e-15
    got = wats_hip.calibration_loss(torch.tensor(prob, dtype=torch.float64).log(), torch.tensor(labels))
    assert abs(float(got) - want) <= 1e-12
    # differentiable, and a shift of a row's logits changes nothing
    z = torch.tensor(prob, dtype=torch.float64).log().requires_grad_(True)
    wats_hip.calibration_loss(z + 3.0, torch.tensor(labels)).backward()
    assert z.grad is not None and float(z.grad.sum(1).abs().max()) <= 1e-12


def test_abi_checks_arguments_before_any_device_work():
    lib = wats_hip._lib.load()
    f = lib.wg_symnorm_aggregate
    one = 16   # any non-NULL address: no call below reaches the device
    assert lib.wg_symnorm_long_row() == 128 == cagcn.symnorm_long_row_threshold()
    # nothing to do
    assert f(0, 0, None, None, 0, None, None, 4, None, None, 0, None, None) == 0
    assert f(3, 3, None, None, 0, None, None, 0, None, None, 0, None, None) == 0
    assert f(0, 0, None, None, 0, None, None, 0, None, None, 1, None, None) == 0
    # negative sizes
    for args in ((-1, 0, 0, 4), (3, -1, 0, 4), (3, 3, -1, 4), (3, 3, 0, -1)):
        n, nnz, n_long, C = args
        assert f(n, nnz, one, one, n_long, one, one, C, one, None, 0, one + 16, None) == -1, args
        assert b"negative" in lib.wg_last_error()
    # a NULL required pointer with work to do
    ok = [3, 3, one, one, 0, None, one, 4, one, None, 0, one + 16, None]
    for k in (2, 3, 6, 8, 11):
        bad = list(ok)
        bad[k] = None
        assert f(*bad) == -1 and b"NULL" in lib.wg_last_error(), k
    bad = list(ok)
    bad[4] = 1     # a long row announced, no list
    assert f(*bad) == -1 and b"long_rows" in lib.wg_last_error()
    bad = list(ok)
    bad[11] = one  # out == x
    assert f(*bad) == -1 and b"alias" in lib.wg_last_error()
    # nnz == 0 needs no indices; the bias may be NULL: both reach the launch, which a machine without a GPU refuses
    # with another status, so only the argument errors are pinned here


def test_exported_surface():
    for name in ("CaGCN", "GCNConv", "SymNormGraph", "sym_norm_aggregate", "calibration_loss"):
        assert getattr(wats_hip, name) is getattr(cagcn, name)
    assert cagcn.CaGCN.fit is cagcn.CaGCN.calib_train
    import inspect
    sig = inspect.signature(cagcn.CaGCN.__init__)
    assert list(sig.parameters)[:6] == ["self", "base_model", "x", "y", "adj", "val_idx"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("graph", "dropout", "verbose", "epochs"))
    assert sig.parameters["dropout"].default == 0.5 and sig.parameters["epochs"].default == 100
    ct = inspect.signature(cagcn.CaGCN.calib_train)
    assert ct.parameters["patience"].default == 10 and ct.parameters["alpha"].default == 0.5


def test_gcn_conv_has_the_reference_layers_parameter_names():
    graph = object.__new__(cagcn.SymNormGraph)     # the layer's parameters need no graph
    graph.device = torch.device("cpu")
    torch.manual_seed(0)
    conv = cagcn.GCNConv(5, 7, graph)
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == {"lin.weight": (7, 5), "bias": (7,)}
    assert float(conv.bias.detach().abs().max()) == 0.0
    bound = math.sqrt(6.0 / (5 + 7))               # Glorot
    assert 0.5 * bound < float(conv.lin.weight.detach().abs().max()) <= bound
    assert set(cagcn.GCNConv(5, 7, graph, bias=False).state_dict()) == {"lin.weight"}


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU refusal")
def test_refuses_to_run_without_a_gpu():
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        cagcn.SymNormGraph(ei, 3)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        cagcn.GCNConv(3, 3, ei)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        cagcn.CaGCN(torch.nn.Linear(3, 3), torch.zeros(3, 3), torch.tensor([0, 1, 2]), torch.eye(3),
                    torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="SymNormGraph"):
        cagcn.sym_norm_aggregate(ei, torch.zeros(3, 3))
