"""DCGC measurement at the ogbn-arxiv size (the benchmark's R-MAT graph, symmetric with self loops, C = 40 classes,
random float32 inputs): the edge MLP and the weighted base model on the HIP kernels (csrc/edgemlp.hip,
csrc/edgeagg.hip) against the torch restatement on the same device.

  edge MLP, forward + backward with g_emb / without g_emb
    (a) hip          ``wats_hip.edge_mlp_weights`` and its backward
    (b) torch_f32    the restatement of tests/dcgc_ref.py in float32 in edge chunks (``--chunk`` entries), each chunk's
                     forward and backward before the next, parameter gradients accumulated: only (chunk, k)
                     activations are alive.  Unchunked, autograd keeps (E, 80) + (E, 160) + (E, 80) tensors and masks.
  weighted two-layer base model (128 features, nhid 64), forward + backward w.r.t. the edge values and the weights
    (a) hip          ``weighted_propagate`` twice (DecisiveEdge.weighted_base)
    (b) torch_f32    the same propagation as a gather and an ``index_add_`` per edge chunk:
                     ``out[rows] += (w / deg[rows])[:, None] * x[cols]``; autograd keeps the (E, F) gathered rows of
                     both layers.  (The reference's dense (N, N) matrix would need 4 N^2 bytes, 115 GB, and so does
                     the gradient w.r.t. the values of a ``torch.sparse`` product, which is therefore not the baseline.)

Times are device-event times of ``reps`` back-to-back calls after a warm-up, the paths alternating over ``rounds``
rounds in one process (median and range reported); peak memory is torch's allocator peak over one call of each path.
The model figure is the float32 matrix peak of the guide (157.3 TFLOP/s): 2 * E * (2C * 4C + 4C * 2C) flops forward,
three times that backward without g_emb's product (which adds 2 * E * 4C * 2C).  Writes one JSON line (also to
``--out``).

    python tools/dcgc_probe.py [--rounds 5] [--reps 2] [--out profiles/r14/dcgc_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "efficient-gnn_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import dcgc_ref as R  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip.graphgen import named_graph  # noqa: E402

PEAK_F32_MATRIX = 157.3e12


def event_time(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / reps


def alternate(paths, rounds, reps):
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(event_time(fn, reps))
    return {k: dict(ms=statistics.median(v) * 1e3, ms_range=[min(v) * 1e3, max(v) * 1e3],
                    ms_rounds=[t * 1e3 for t in v]) for k, v in times.items()}


def beats_every_round(res, a, b):
    spread = max(res[a]["ms_range"][1] - res[a]["ms_range"][0], res[b]["ms_range"][1] - res[b]["ms_range"][0])
    return bool(all(tb - ta > spread for ta, tb in zip(res[a]["ms_rounds"], res[b]["ms_rounds"])))


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--chunk", type=int, default=1 << 18, help="entries per chunk of the torch edge MLP")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dcgc_probe: needs a ROCm GPU (there is no CPU path to time)")
    dev = torch.device("cuda")
    g = named_graph(args.graph)
    A = g.to_scipy().tocsr()
    import scipy.sparse as sp
    A = ((A + A.T + sp.identity(g.n, format="csr")) > 0).astype(np.float32).tocsr()
    A.sort_indices()
    n, C = g.n, args.classes
    graph = wats_hip.EdgeWeightGraph(type("G", (), dict(n=n, indptr=A.indptr.astype(np.int64),
                                                       indices=A.indices.astype(np.int32)))(), device=dev)
    nnz = graph.nnz
    torch.manual_seed(0)
    ext = nn.Sequential(nn.Linear(2 * C, 4 * C), nn.ReLU(), nn.Dropout(0.5), nn.Linear(4 * C, 2 * C), nn.ReLU(),
                        nn.Dropout(0.5), nn.Linear(2 * C, 1)).to(dev)
    params = [ext[i].weight for i in (0, 3, 6)] + [ext[i].bias for i in (0, 3, 6)]
    ordered = [ext[0].weight, ext[0].bias, ext[3].weight, ext[3].bias, ext[6].weight, ext[6].bias]
    emb0 = torch.randn(n, C, device=dev)
    g_w = torch.randn(nnz, device=dev)
    rows, cols = graph.rows.long(), graph.cols.long()

    def hip_mlp(want_emb):
        def run():
            for p in params:
                p.grad = None
            emb = emb0.detach().requires_grad_(want_emb)
            w = wats_hip.edge_mlp_weights(graph, emb, ext, 0.0, 0)
            w.backward(g_w)
            return w.detach(), [p.grad for p in ordered], emb.grad
        return run

    def hip_mlp_forward():
        with torch.no_grad():
            return wats_hip.edge_mlp_weights(graph, emb0, ext, 0.0, 0)

    def torch_mlp(want_emb):
        def run():
            for p in params:
                p.grad = None
            emb = emb0.detach().requires_grad_(want_emb)
            ws = []
            for lo in range(0, nnz, args.chunk):
                hi = min(nnz, lo + args.chunk)
                w = R.edge_mlp(emb, ordered, rows[lo:hi], cols[lo:hi], None, torch.float32)[0]
                w.backward(g_w[lo:hi])
                ws.append(w.detach())
            return torch.cat(ws), [p.grad for p in ordered], emb.grad
        return run

    # the weighted base model
    gc1, gc2 = nn.Linear(128, 64).to(dev), nn.Linear(64, C).to(dev)
    x = torch.randn(n, 128, device=dev)
    w0 = torch.rand(nnz, device=dev) + 0.1
    gy = torch.randn(n, C, device=dev)

    def hip_base():
        w = w0.detach().requires_grad_(True)
        h = F.relu(gc1(wats_hip.weighted_propagate(graph, w, x)))
        out = gc2(wats_hip.weighted_propagate(graph, w, h))
        out.backward(gy)
        return out.detach(), w.grad

    def torch_base():
        w = w0.detach().requires_grad_(True)
        deg = torch.zeros(n, device=dev).index_add_(0, rows, w)
        deg = torch.where(deg == 0, torch.ones_like(deg), deg)
        a = w / deg[rows]

        def prop(v):
            y = torch.zeros(n, v.shape[1], device=dev)
            for lo in range(0, nnz, args.chunk):
                hi = min(nnz, lo + args.chunk)
                y = y.index_add(0, rows[lo:hi], a[lo:hi].unsqueeze(1) * v[cols[lo:hi]])
            return y

        h = F.relu(gc1(prop(x)))
        out = gc2(prop(h))
        out.backward(gy)
        return out.detach(), w.grad

    paths = {"hip_mlp": hip_mlp(True), "hip_mlp_no_gemb": hip_mlp(False), "hip_mlp_forward_only": hip_mlp_forward,
             "torch_mlp": torch_mlp(True), "torch_mlp_no_gemb": torch_mlp(False), "hip_base": hip_base,
             "torch_base": torch_base}
    a, b = hip_mlp(True)(), torch_mlp(True)()
    rel = lambda u, v: float((u.double() - v.double()).abs().max() / v.double().abs().max().clamp_min(1e-30))
    agree = dict(w=rel(a[0], b[0]), params=[rel(u, v) for u, v in zip(a[1], b[1])], g_emb=rel(a[2], b[2]))
    hb, tb = hip_base(), torch_base()
    agree["base_out"], agree["base_gw"] = rel(hb[0], tb[0]), rel(hb[1], tb[1])
    del a, b, hb, tb
    peaks = {k: peak_bytes(fn) for k, fn in paths.items()}
    res = alternate(paths, args.rounds, args.reps)
    fwd = 2.0 * nnz * (2 * C * 4 * C + 4 * C * 2 * C)
    model = dict(forward_ms=fwd / PEAK_F32_MATRIX * 1e3, forward_backward_ms=3 * fwd / PEAK_F32_MATRIX * 1e3,
                 forward_backward_gemb_ms=(3 * fwd + 2.0 * nnz * 4 * C * 2 * C) / PEAK_F32_MATRIX * 1e3)
    out = dict(tool="dcgc_probe", graph=args.graph, n=n, nnz=nnz, classes=C, chunk=args.chunk,
               device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, times=res, peak_bytes=peaks,
               workspace_bytes=wats_hip.dcgc.edge_mlp_workspace(n, nnz, C),
               unchunked_activation_bytes=4 * nnz * (2 * C + 4 * C + 4 * C + 2 * C + 2 * C),
               model_f32_matrix_peak=model,
               fraction_of_peak=dict(forward=model["forward_ms"] / res["hip_mlp_forward_only"]["ms"],
                                     forward_backward=model["forward_backward_ms"] / res["hip_mlp_no_gemb"]["ms"],
                                     forward_backward_gemb=model["forward_backward_gemb_ms"] / res["hip_mlp"]["ms"]),
               hip_vs_torch_rel_diff=agree,
               hip_beats_torch_every_round=dict(
                   mlp=beats_every_round(res, "hip_mlp", "torch_mlp"),
                   mlp_no_gemb=beats_every_round(res, "hip_mlp_no_gemb", "torch_mlp_no_gemb"),
                   base=beats_every_round(res, "hip_base", "torch_base")))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
