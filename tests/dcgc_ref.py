"""Test-only dense restatement of the reference's DCGC (``calibration/DCGC.py``) and of the base model it wraps
(``src/gnn/model.py:37-53``) in plain torch, in a chosen dtype, on the CPU, plus the edge MLP's hashed dropout masks
(``include/wats_hip.h``) in numpy.  The product never imports this file.  Every function converts its inputs to
``dtype`` first, so the float64 run starts from the same float32 numbers as the float32 run and the kernels."""
import numpy as np
import torch
import torch.nn.functional as F

# the CPU code paths the fixtures were generated on (tools/gen_golden_dcgc.py); read when torch starts
PINNED_CPU_PATH = {"MKL_ENABLE_INSTRUCTIONS": "AVX2", "ATEN_CPU_CAPABILITY": "avx2"}
EXTRACTOR_KEYS = ("ext_w1", "ext_b1", "ext_w2", "ext_b2", "ext_w3", "ext_b3")
BASE_KEYS = ("gc1_weight", "gc1_bias", "gc2_weight", "gc2_bias")

_K1, _K2, _K3 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def hash_words(seed, layer, e, j):
    """The 32-bit word of unit ``j`` of layer ``layer`` of entry ``e`` (arrays broadcast), as the header states."""
    with np.errstate(over="ignore"):
        e, j = np.asarray(e, np.uint64), np.asarray(j, np.uint64)
        x = (np.uint64(seed) ^ (_K1 * np.uint64(layer))) + e * _K2 + j * _K3
        x ^= x >> np.uint64(30)
        x *= _K2
        x ^= x >> np.uint64(27)
        x *= _K3
        x ^= x >> np.uint64(31)
        return (x >> np.uint64(32)).astype(np.uint32)


def keep_mask(seed, layer, nnz, units, p):
    """(nnz, units) bool: the units the kernel keeps."""
    if p == 0:
        return np.ones((nnz, units), bool)
    thr = np.uint32(int(np.floor(p * 4294967296.0)))
    return hash_words(seed, layer, np.arange(nnz)[:, None], np.arange(units)[None, :]) >= thr


def dropout_masks(nnz, C, p, seed, dtype):
    """(D1 (nnz, 4C), D2 (nnz, 2C)) scaled by the kernel's float32 1 / (1 - p)."""
    scale = float(np.float32(1.0 / (1.0 - p)))
    return tuple(torch.from_numpy(keep_mask(seed, layer, nnz, units, p)).to(dtype) * scale
                 for layer, units in ((1, 4 * C), (2, 2 * C)))


def pattern(adj):
    """dense_to_sparse's pattern: (rows, cols) of ``adj != 0`` in row-major order."""
    idx = torch.nonzero(adj != 0)
    return idx[:, 0], idx[:, 1]


def edge_mlp(emb, params, rows, cols, masks=None, dtype=torch.float64):
    """DCGC.py:70-73, :78 at the entries: (w, z1, z2, z3).  ``params`` may require grad (they are used as given when
    already of ``dtype``); ``masks`` = (D1, D2) or None (eval mode)."""
    w1, b1, w2, b2, w3, b3 = (p.to(dtype) for p in params)
    emb = emb.to(dtype)
    f12 = torch.cat([emb[rows.long()], emb[cols.long()]], dim=-1)     # f1 = emb[r], f2 = emb[c]
    z1 = F.linear(f12, w1, b1)
    h1 = F.relu(z1)
    if masks is not None:
        h1 = h1 * masks[0].to(dtype)
    z2 = F.linear(h1, w2, b2)
    h2 = F.relu(z2)
    if masks is not None:
        h2 = h2 * masks[1].to(dtype)
    z3 = F.linear(h2, w3, b3).reshape(-1)
    return F.relu(z3), z1, z2, z3


def edge_mlp_and_grads(emb, params, rows, cols, g_w, masks=None, dtype=torch.float64):
    """(w, [six parameter gradients], g_emb) of sum(g_w * w) in ``dtype``."""
    leaves = [p.detach().clone().to(dtype).requires_grad_(True) for p in params]
    e = emb.detach().clone().to(dtype).requires_grad_(True)
    w = edge_mlp(e, leaves, rows, cols, masks, dtype)[0]
    if w.numel():
        (w * g_w.to(dtype)).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return w.detach(), [zero(p) for p in leaves], zero(e)


def kink_entries(emb, params, rows, cols, masks=None):
    """Entries with a pre-activation within 64 * 2^-24 * max|z| of its layer of zero (float64): a float32 run may
    take the other side of the ReLU there."""
    _, z1, z2, z3 = edge_mlp(emb, params, rows, cols, masks, torch.float64)
    bad = torch.zeros(rows.numel(), dtype=torch.bool)
    for z in (z1, z2, z3.unsqueeze(1)):
        if z.numel():
            bad |= (z.abs() < 64 * 2.0 ** -24 * float(z.abs().max())).any(dim=1)
    return bad


def row_normalize(adj):
    """model.py:43-45."""
    deg = adj.sum(dim=1, keepdim=True)
    deg = torch.where(deg == 0, torch.ones_like(deg), deg)
    return adj / deg


def gcn(adj, x, base, dtype=torch.float64):
    """model.py:37-53 in eval mode."""
    w1, b1, w2, b2 = (p.to(dtype) for p in base)
    an = row_normalize(adj.to(dtype))
    h = F.relu(F.linear(torch.mm(an, x.to(dtype)), w1, b1))
    return F.linear(torch.mm(an, h), w2, b2)


def propagate(rows, cols, n, w, x, dtype=torch.float64):
    """``adj_norm @ x`` for the adjacency whose stored entries are ``w`` (differentiable w.r.t. w and x)."""
    a = torch.zeros(n, n, dtype=dtype).index_put((rows.long(), cols.long()), w.to(dtype), accumulate=True)
    return torch.mm(row_normalize(a), x.to(dtype))


def forward(adj, x, base, ext, alpha=0.5, beta=10, dtype=torch.float64, pattern_adj=None):
    """DCGC.forward (DCGC.py:143-150) in eval mode: (w at the entries, homophily weights at the entries, logits).
    ``adj`` may require grad; the pattern comes from ``pattern_adj`` (default: ``adj`` detached)."""
    n = adj.shape[0]
    rows, cols = pattern(adj.detach() if pattern_adj is None else pattern_adj)
    emb = gcn(adj, x, base, dtype)                                            # DCGC.py:68
    w = edge_mlp(emb, ext, rows, cols, None, dtype)[0]                        # :70-73
    dec = torch.zeros(n, n, dtype=dtype).index_put((rows, cols), w).relu()    # :74-78
    with torch.no_grad():                                                     # :155-158
        pred = F.softmax(gcn(dec.detach(), x, base, dtype), dim=1)
    pred = torch.exp(beta * pred)                                             # :160-161
    pred = pred / torch.sum(pred, dim=1, keepdim=True)
    coef = 1 / (torch.norm(pred[rows] - pred[cols], dim=1) + alpha)           # :163-165
    homo = torch.zeros(n, n, dtype=dtype).index_put((rows, cols), coef)
    return w, coef, gcn(dec * homo, x, base, dtype)                           # :147-148


def adjacency_gradient(adj, x, base, ext, loss_weight, rows, cols, alpha=0.5, beta=10, dtype=torch.float64):
    """d sum(loss_weight * logits) / d adj at (rows, cols), the dense way of the attack."""
    a = adj.detach().clone().to(dtype).requires_grad_(True)
    out = forward(a, x, base, ext, alpha, beta, dtype)[2]
    (out * loss_weight.to(dtype)).sum().backward()
    return a.grad[rows.long(), cols.long()]


def load_case(path):
    with np.load(path, allow_pickle=False) as d:
        return {k: torch.from_numpy(np.asarray(d[k])) for k in d.files}


def case_parts(c):
    return tuple(c[k] for k in BASE_KEYS), tuple(c[k] for k in EXTRACTOR_KEYS)


def fixture_differences(path):
    """{key: [max|float32 restatement - recorded array|, max|recorded array|]} for one fixture file."""
    c = load_case(path)
    base, ext = case_parts(c)
    alpha, beta = float(c["alpha"]), float(c["beta"])
    w, homo, out = forward(c["adj"], c["x"], base, ext, alpha, beta, torch.float32)
    grad = adjacency_gradient(c["adj"], c["x"], base, ext, c["loss_weight"], c["grad_rows"], c["grad_cols"], alpha,
                              beta, torch.float32)
    got = dict(weights=w, homo=homo, out=out, grad=grad)
    return {k: [float((v.detach() - c[k]).abs().max()), float(c[k].abs().max())] for k, v in got.items()}


if __name__ == "__main__":
    # python tests/dcgc_ref.py <fixture.npz> ...: one JSON line {file: fixture_differences(file)}
    import json
    import sys
    print(json.dumps({p: fixture_differences(p) for p in sys.argv[1:]}))
