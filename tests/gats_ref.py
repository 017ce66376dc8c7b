"""Plain-torch restatements of the GATS attention layer (reference calibration/GATS.py:111-167), written from
its formulas without PyG.  Helpers of tests/test_gats_host.py and tests/test_gats.py; not a test.

Edges are (src, dst) pairs: a message flows src -> dst and the softmax groups by dst, so node i aggregates
over In(i) = {src : dst == i}.  `with_self_loops` is the layer's self-loop step (GATS.py:102-106).

  attention_edges   (A) edge list: index_select, scatter_reduce(amax), index_add_.  In float64 the yardstick.
  attention_dense   (B) an (N, N) mask, masked_fill(-inf), softmax(dim=1).  In float64 it pins (A).
  layer_reference   (A) wrapped in the layer's torch steps (GATS.py:114-131 before, :141-145 after).
  bfs_levels        shortest_path_length (GATS.py:25-49) in numpy, quirks included.
"""
import numpy as np
import torch
import torch.nn.functional as F

INT64_MAX = np.iinfo(np.int64).max


def with_self_loops(src, dst, n):
    """Duplicates merged, self loops removed, then one added per node; sorted by (dst, src)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    keep = src != dst
    src = np.concatenate([src[keep], np.arange(n)])
    dst = np.concatenate([dst[keep], np.arange(n)])
    key = np.unique(dst * n + src)
    return key % n, key // n


def attention_edges(src, dst, a, t, conf, slope=0.2, dtype=torch.float64):
    """(A): (sim (N, H), dconf (N,)) in `dtype`, differentiable w.r.t. a and t."""
    src, dst = torch.as_tensor(src, device=a.device).long(), torch.as_tensor(dst, device=a.device).long()
    a, t, conf = a.to(dtype), t.to(dtype), conf.to(dtype)
    n = a.shape[0]
    d = (a.index_select(0, dst) * a.index_select(0, src)).sum(-1)
    e = F.leaky_relu(d, slope)
    mx = torch.full((n,), -float("inf"), dtype=dtype, device=a.device)
    mx = mx.scatter_reduce(0, dst, e.detach(), "amax", include_self=True)
    ex = torch.exp(e - mx.index_select(0, dst))
    den = torch.zeros(n, dtype=dtype, device=a.device).index_add_(0, dst, ex)
    p = ex / den.index_select(0, dst)
    sim = torch.zeros(n, t.shape[1], dtype=dtype, device=a.device).index_add_(
        0, dst, p.unsqueeze(-1) * t.index_select(0, src))
    dconf = torch.zeros(n, dtype=dtype, device=a.device).index_add_(
        0, dst, conf.index_select(0, dst) - conf.index_select(0, src))
    return sim, dconf


def attention_dense(src, dst, a, t, conf, slope=0.2, dtype=torch.float64):
    """(B): the same through an (N, N) mask (mask[i, j]: j is a source of i), for small N."""
    a, t, conf = a.to(dtype), t.to(dtype), conf.to(dtype)
    n = a.shape[0]
    mask = torch.zeros(n, n, dtype=torch.bool, device=a.device)
    mask[torch.as_tensor(dst).long(), torch.as_tensor(src).long()] = True
    e = F.leaky_relu(a @ a.t(), slope).masked_fill(~mask, -float("inf"))
    p = torch.softmax(e, dim=1)
    m = mask.to(dtype)
    return p @ t, m.sum(1) * conf - m @ conf


def layer_reference(params, src, dst, x, dist_to_train, slope=0.2, dtype=torch.float64, attention_dtype=None):
    """The layer's output (N, 1) with (A) in the middle.  params: temp_lin.weight, conf_coef, bias, train_a,
    dist1_a (tensors of `dtype`, requiring grad where a gradient is wanted); src / dst with the self loops.
    The torch steps around the attention run in `dtype`, (A) in `attention_dtype` (default: `dtype`) on the
    `dtype` operands, its results cast back: with dtype = float32 these are the layer's own steps, and
    attention_dtype = float64 / float32 give the yardstick and its float32 error for the attention alone."""
    x = x.to(dtype)
    n = x.shape[0]
    src_t, dst_t = torch.as_tensor(src, device=x.device).long(), torch.as_tensor(dst, device=x.device).long()
    lo, hi = x.min(1, keepdim=True)[0], x.max(1, keepdim=True)[0]
    nx = (x - lo) / (hi - lo + 1e-8)
    temp = torch.sort(nx, -1)[0] @ params["temp_lin.weight"].t()
    a_cluster = torch.ones(n, dtype=dtype, device=x.device)
    a_cluster = torch.where(dist_to_train == 0, params["train_a"], a_cluster)
    a_cluster = torch.where(dist_to_train == 1, params["dist1_a"], a_cluster)
    conf = torch.softmax(x, dim=1).amax(-1)
    deg = torch.zeros(n, dtype=dtype, device=x.device).index_add_(0, src_t, torch.ones(len(src_t), dtype=dtype, device=x.device))
    deg_inv = torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))
    sim, dconf = attention_edges(src_t, dst_t, x / a_cluster.unsqueeze(-1), temp * a_cluster.unsqueeze(-1), conf,
                                 slope, attention_dtype or dtype)
    sim, dconf = sim.to(dtype), dconf.to(dtype)
    out = F.softplus(sim + params["conf_coef"] * dconf.unsqueeze(-1) * deg_inv.unsqueeze(-1))
    return (out.mean(1) + params["bias"]).unsqueeze(1)


def bfs_levels(src, dst, mask, max_hop):
    """GATS.py:25-49: only the levels 0 .. max_hop - 1 are assigned; the rest keeps the int64 maximum."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    cur = np.asarray(mask, bool).copy()
    dist = np.full(cur.shape[0], INT64_MAX, np.int64)
    seen = cur.copy()
    for hop in range(max_hop):
        dist[cur] = hop
        nxt = np.zeros_like(cur)
        nxt[dst[cur[src]]] = True
        cur = nxt & ~seen
        seen |= nxt
        if not cur.any():
            break
    return dist


def error_bound(ref32, ref64):
    """The tests' bound on max|kernel - A_float64|: twice the error of (A) in float32 (another exp), and at
    least 4 * 2^-24 * max|A_float64| (one rounding of p, one of the output, two ulps of exp) for the case
    where torch's float32 path happens to be exact."""
    ref64 = ref64.detach().double().cpu()
    err32 = float((ref32.detach().double().cpu() - ref64).abs().max()) if ref64.numel() else 0.0
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    return max(2.0 * err32, 4.0 * 2.0 ** -24 * scale), err32


def assert_close(got, ref32, ref64, what):
    bound, err32 = error_bound(ref32, ref64)
    got64 = got.detach().double().cpu()
    assert torch.isfinite(got64).all(), f"{what}: non-finite output"
    err = float((got64 - ref64.detach().double().cpu()).abs().max()) if got64.numel() else 0.0
    print(f"{what}: err={err:.3e} err32={err32:.3e} bound={bound:.3e}")
    assert err <= bound, f"{what}: err {err:.3e} > bound {bound:.3e} (err32 {err32:.3e})"


# ---------------------------------------------------------------------------------------------------------
# graphs as (src, dst, n) edge lists WITHOUT the self-loop step
# ---------------------------------------------------------------------------------------------------------
def path_graph(n=3):
    s = np.arange(n - 1)
    return np.concatenate([s, s + 1]), np.concatenate([s + 1, s]), n


def random_graph(n, mean_degree, directed, seed, loops=0):
    rng = np.random.default_rng(seed)
    m = int(n * mean_degree / (1 if directed else 2))
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    if loops:   # some self loops in the input: the layer replaces them
        l = rng.integers(0, n, loops)
        src, dst = np.concatenate([src, l]), np.concatenate([dst, l])
    if not directed:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    return src, dst, n


def star_graph(hub_in=700, short=50):
    """Node 0 has `hub_in` in-neighbours (1 .. hub_in, each of which hears only from the hub's first leaf and
    itself); `short` more nodes form a directed ring."""
    leaves = np.arange(1, hub_in + 1)
    ring = np.arange(hub_in + 1, hub_in + 1 + short)
    src = np.concatenate([leaves, np.full(hub_in - 1, 1), ring])
    dst = np.concatenate([np.zeros(hub_in, np.int64), leaves[1:], np.roll(ring, -1)])
    return src, dst, hub_in + 1 + short
