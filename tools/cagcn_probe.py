"""CaGCN aggregation measurement: forward + backward of the symmetric-normalised GCN aggregation on the HIP kernel
(csrc/symnorm.hip) against two torch paths on the same device, on the arxiv-size R-MAT graph of
``graphgen.named_graph`` at C = 40 with random float32 inputs.

  aggregate  one ``A_hat x`` forward + the gradient w.r.t. x:
             (a) ``sym_norm_aggregate``
             (b) the edge-list restatement (A) of tests/cagcn_ref.py in float32 (index_select / index_add_: one (E, C)
                 tensor, as PyG's message passing builds)
             (c) ``torch.sparse.mm`` on a valued CSR of ``A_hat`` and, for the backward, of its transpose, if this
                 torch build has it on the device (else the JSON says why not)
  scaling    the two-layer scaling model of CaGCN (CaGCN.py:105-108 without dropout): two GCNConv with their torch
             linears, ReLU between, forward + backward to the input and the four parameters, on the same three paths
  construct  ``SymNormGraph`` from the graph (CSR by destination, transpose map, dinv, hub lists): wall time around
             a device sync, median of ``rounds``; the valued CSR pair of (c) likewise

Times are device-event times of ``reps`` back-to-back calls after a warm-up, the paths alternating over ``rounds``
rounds (median and range reported).  ``--paths hip`` runs (a) alone (for a kernel trace).  Writes one JSON line (also
to ``--out``).

    python tools/cagcn_probe.py [--graph ogbn-arxiv] [--rounds 5] [--reps 20] [--out profiles/r12/cagcn_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "efficient-gnn_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cagcn_ref as R  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip import cagcn  # noqa: E402
from wats_hip.graphgen import named_graph  # noqa: E402


def event_time(fn, reps):
    """Seconds per call over `reps` calls between two device events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / reps


def alternate(paths, rounds, reps):
    """{name: {us, us_range, us_rounds}} of the callables in `paths`, alternating over `rounds` rounds."""
    for fn in paths.values():                   # warm-up: code objects, allocator blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(event_time(fn, reps))
    return {k: dict(us=statistics.median(v) * 1e6, us_range=[min(v) * 1e6, max(v) * 1e6],
                    us_rounds=[t * 1e6 for t in v]) for k, v in times.items()}


def beats_every_round(res, a, b):
    """(a) is faster than (b) in every round by more than the larger of the two paths' own run-to-run ranges."""
    spread = max(res[a]["us_range"][1] - res[a]["us_range"][0], res[b]["us_range"][1] - res[b]["us_range"][0])
    return bool(all(tb - ta > spread for ta, tb in zip(res[a]["us_rounds"], res[b]["us_rounds"])))


def wall(fn, rounds):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return dict(ms=statistics.median(out) * 1e3, ms_range=[min(out) * 1e3, max(out) * 1e3])


class _SpMM(torch.autograd.Function):
    """y = A x with the backward A^T g: two valued CSR matrices, no autograd through the sparse tensor."""

    @staticmethod
    def forward(ctx, x, A, At):
        ctx.At = At
        return torch.sparse.mm(A, x)

    @staticmethod
    def backward(ctx, g):
        return torch.sparse.mm(ctx.At, g.contiguous()), None, None


def valued_csr_pair(sg):
    """(A_hat, A_hat^T) as torch sparse CSR tensors with float32 values dinv_i dinv_j."""
    def one(indptr, indices):
        rows = torch.repeat_interleave(torch.arange(sg.n, device=sg.device), indptr[1:] - indptr[:-1])
        vals = sg.dinv[rows] * sg.dinv[indices.long()]
        return torch.sparse_csr_tensor(indptr, indices.long(), vals, size=(sg.n, sg.n))
    return one(sg.indptr, sg.indices), one(sg.t_indptr, sg.t_indices)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--C", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--paths", default="all", choices=["all", "hip"])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cagcn_probe: needs a ROCm GPU (there is no CPU path to time)")
    dev = torch.device("cuda")
    g = named_graph(args.graph)
    n, C = g.n, args.C
    sg = wats_hip.SymNormGraph(g, device=dev)
    construct = dict(sym_norm_graph=wall(lambda: wats_hip.SymNormGraph(g, device=dev), args.rounds))
    gen = torch.Generator("cuda").manual_seed(0)
    x0 = torch.randn(n, C, device=dev, generator=gen)
    Gs = torch.randn(n, C, device=dev, generator=gen)
    e_src, e_dst = sg.edge_list()
    torch.manual_seed(0)
    convs = [wats_hip.GCNConv(C, C, sg), wats_hip.GCNConv(C, C, sg)]
    with torch.no_grad():
        for conv in convs:
            conv.bias.normal_(0.0, 0.1)
    params = [p for conv in convs for p in (conv.lin.weight, conv.bias)]

    def fresh():
        for p in params:
            p.grad = None
        return x0.detach().requires_grad_(True)

    def agg_hip():
        x = fresh()
        y = wats_hip.sym_norm_aggregate(sg, x)
        y.backward(Gs)
        return y.detach(), x.grad

    def agg_torch():
        x = fresh()
        y = R.sym_norm_edges(e_src, e_dst, x, sg.dinv, None, False, torch.float32)
        y.backward(Gs)
        return y.detach(), x.grad

    def scaling(conv_fn):
        def run():
            x = fresh()
            t = conv_fn(convs[1], conv_fn(convs[0], x, True), False)
            t.backward(Gs)
            return t.detach(), x.grad, params[0].grad
        return run

    scale_hip = scaling(lambda conv, x, relu: conv(x, relu=relu))
    scale_torch = scaling(lambda conv, x, relu: R.gcn_conv(conv.lin.weight, conv.bias, e_src, e_dst, x, sg.dinv, relu,
                                                         torch.float32))
    paths_agg, paths_scale = {"aggregate_hip": agg_hip}, {"scaling_hip": scale_hip}
    sparse_note = "not run (--paths hip)"
    if args.paths == "all":
        paths_agg["aggregate_torch_f32"] = agg_torch
        paths_scale["scaling_torch_f32"] = scale_torch
        try:
            A, At = valued_csr_pair(sg)
            construct["valued_csr_pair"] = wall(lambda: valued_csr_pair(sg), args.rounds)

            def agg_sparse():
                x = fresh()
                y = _SpMM.apply(x, A, At)
                y.backward(Gs)
                return y.detach(), x.grad

            def conv_sparse(conv, x, relu):
                y = _SpMM.apply(conv.lin(x), A, At) + conv.bias
                return torch.relu(y) if relu else y

            agg_sparse()
            torch.cuda.synchronize()
            paths_agg["aggregate_sparse_mm"] = agg_sparse
            paths_scale["scaling_sparse_mm"] = scaling(conv_sparse)
            sparse_note = "torch.sparse.mm on CSR ran on the device"
        except Exception as e:  # noqa: BLE001 -- whatever this torch build raises for sparse CSR on the device
            sparse_note = f"torch.sparse.mm on a device CSR is not supported by this torch build: {type(e).__name__}: {e}"[:300]

    rel = lambda u, v: float((u.double() - v.double()).abs().max() / v.double().abs().max())
    agree = {}
    hip_agg, hip_scale = agg_hip(), scale_hip()
    for k, fn in list(paths_agg.items())[1:]:
        agree[k] = [rel(u, v) for u, v in zip(hip_agg, fn())]
    for k, fn in list(paths_scale.items())[1:]:
        agree[k] = [rel(u, v) for u, v in zip(hip_scale, fn())]
    res = alternate({**paths_agg, **paths_scale}, args.rounds, args.reps)
    verdict = {}
    for a, others in (("aggregate_hip", list(paths_agg)[1:]), ("scaling_hip", list(paths_scale)[1:])):
        for b in others:
            verdict[f"{a}_beats_{b}_every_round"] = beats_every_round(res, a, b)
    nnz = sg.nnz
    line = json.dumps(dict(
        tool="cagcn_probe", graph=args.graph, n=n, nnz_input=int(g.nnz), nnz_with_self_loops=nnz, C=C,
        device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, describe=sg.describe(),
        longest_row=int((sg.indptr[1:] - sg.indptr[:-1]).max()),
        longest_transposed_row=int((sg.t_indptr[1:] - sg.t_indptr[:-1]).max()),
        long_row_threshold=cagcn.symnorm_long_row_threshold(),
        bytes_per_aggregate=dict(ids=4 * nnz, gathered_rows=4 * nnz * C, own_rows=8 * n * C, dinv=4 * nnz + 4 * n,
                                 indptr=8 * (n + 1)),
        construct=construct, forward_backward=res, sparse_mm=sparse_note, hip_vs_other_rel_diff=agree, **verdict))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
