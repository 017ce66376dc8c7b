"""Plain-torch restatements of the CaGCN calibrator's graph convolution (reference calibration/CaGCN.py:68-70,
:104-112; PyG GCNConv / gcn_norm), written from the formulas without PyG.  Helpers of tests/test_cagcn_host.py,
tests/test_cagcn.py and tools/cagcn_probe.py; not a test.  PyG is not installed where this project is developed,
so no reference-generated fixture exists for this layer: these restatements are the yardstick.

Edges are (src, dst) pairs WITH the self loops (gats_ref.with_self_loops): a message flows src -> dst, node i
aggregates over In(i) = {src : dst == i}, deg_i = |In(i)| (the in-degree with the loop), dinv = deg^-1/2 and

    out_i = act( sum over j in In(i) of dinv_i dinv_j x_j  +  bias )

  sym_norm_edges    (A) edge list: index_select and index_add_, the dtype a parameter.  In float64 the yardstick.
  sym_norm_dense    (B) an (N, N) matrix D^-1/2 M D^-1/2 with M[i, j] = 1 for j in In(i), for small N.
  gcn_conv          the whole GCNConv: x W^T in the dtype of the torch steps, then (A).
  cagcn_forward     the whole CaGCN forward from logits (CaGCN.py:105-112, eval mode: no dropout) on top of gcn_conv.
  cora_like_edges   a Cora-shaped random graph (n = 2708, 7 classes) from a seed.
"""
import numpy as np
import torch

from gats_ref import assert_close, error_bound, path_graph, random_graph, star_graph, with_self_loops  # noqa: F401


def in_degree(dst, n, dtype=torch.float64, device=None):
    dst = torch.as_tensor(dst, device=device).long()
    return torch.zeros(n, dtype=dtype, device=dst.device).index_add_(0, dst, torch.ones(len(dst), dtype=dtype,
                                                                                     device=dst.device))


def sym_norm_edges(src, dst, x, dinv=None, bias=None, relu=False, dtype=torch.float64):
    """(A) in `dtype`, differentiable w.r.t. x and bias.  dinv: the per-node factor to use (cast to `dtype`; the
    tests pass the layer's float32 dinv so that both sides share it); None: deg^-1/2 computed in `dtype`."""
    src = torch.as_tensor(src, device=x.device).long()
    dst = torch.as_tensor(dst, device=x.device).long()
    n = x.shape[0]
    x = x.to(dtype)
    dinv = in_degree(dst, n, dtype, x.device).pow(-0.5) if dinv is None else dinv.to(device=x.device, dtype=dtype)
    w = dinv.index_select(0, dst) * dinv.index_select(0, src)
    out = torch.zeros(n, x.shape[1], dtype=dtype, device=x.device).index_add_(
        0, dst, w.unsqueeze(-1) * x.index_select(0, src))
    if bias is not None:
        out = out + bias.to(dtype)
    return torch.relu(out) if relu else out


def sym_norm_dense(src, dst, x, bias=None, relu=False, dtype=torch.float64):
    """(B): the same through the (N, N) matrix, deg from its row sums."""
    n = x.shape[0]
    m = torch.zeros(n, n, dtype=dtype, device=x.device)
    m[torch.as_tensor(dst).long(), torch.as_tensor(src).long()] = 1.0
    dinv = m.sum(1).pow(-0.5)
    out = (dinv.unsqueeze(1) * m * dinv.unsqueeze(0)) @ x.to(dtype)
    if bias is not None:
        out = out + bias.to(dtype)
    return torch.relu(out) if relu else out


def gcn_conv(weight, bias, src, dst, x, dinv=None, relu=False, dtype=torch.float64, aggregate_dtype=None):
    """GCNConv: x W^T in `dtype` (the layer's torch step), then (A) in `aggregate_dtype` (default `dtype`) on that
    product with the bias and the ReLU inside, cast back to `dtype`."""
    h = x.to(dtype) @ weight.to(dtype).t()
    out = sym_norm_edges(src, dst, h, dinv, None if bias is None else bias.to(dtype), relu, aggregate_dtype or dtype)
    return out.to(dtype)


def cagcn_forward(params, src, dst, logits, dinv=None, dtype=torch.float64, aggregate_dtype=None):
    """CaGCN.py:105-112 without dropout.  params: scaling_model.{0,1}.lin.weight / .bias."""
    logits = logits.to(dtype)
    t = gcn_conv(params["scaling_model.0.lin.weight"], params["scaling_model.0.bias"], src, dst, logits, dinv, True,
                 dtype, aggregate_dtype)
    t = gcn_conv(params["scaling_model.1.lin.weight"], params["scaling_model.1.bias"], src, dst, t, dinv, False,
                 dtype, aggregate_dtype)
    t = torch.log(torch.exp(t) + 1.1)
    return torch.log_softmax(logits * t, dim=1)


def calibration_loss_by_hand(prob, labels):
    """CaGCN.py:9-42 from a probability matrix, row by row in Python."""
    total = 0.0
    for row, y in zip(prob, labels):
        order = sorted(range(len(row)), key=lambda k: -row[k])
        p1, p2 = row[order[0]], row[order[1]]
        total += (1 - p1 + p2) if order[0] == y else (p1 - p2)
    return total / len(labels)


def cora_like_edges(seed=42, n=2708, ncls=7, avg_deg=3.9):
    """(src, dst, n, y): SBM classes, 85 % of the edges inside a class, symmetric, no self loops."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, ncls, n)
    m = int(n * avg_deg / 2)
    src = rng.integers(0, n, m)
    same = rng.random(m) < 0.85
    order = np.argsort(y, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(y, minlength=ncls))])
    pick = start[y[src]] + (rng.random(m) * (start[y[src] + 1] - start[y[src]])).astype(np.int64)
    dst = np.where(same, order[pick], rng.integers(0, n, m))
    keep = src != dst
    src, dst = src[keep], dst[keep]
    return np.concatenate([src, dst]), np.concatenate([dst, src]), n, y.astype(np.int64)
