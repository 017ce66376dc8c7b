"""GATS attention measurement: the layer's forward + backward on the HIP kernels against the plain-torch edge-list
restatement (A) of tests/gats_ref.py in float32 on the same device (index_select / scatter_reduce / index_add_:
one (E, C) tensor per operand, as PyG's message passing builds), on the arxiv-size R-MAT graph of
``graphgen.named_graph`` at C = 40 classes and H = 8 heads with random float32 logits.

  layer      (a) ``CalibAttentionLayer.forward`` + ``backward`` (csrc/gats.hip between the layer's torch steps)
             (b) ``gats_ref.layer_reference`` (the same torch steps around (A)) + ``backward``
  attention  the same without the torch steps: ``edge_softmax_attention`` against ``gats_ref.attention_edges``,
             forward + backward w.r.t. a and t
  construct  the CSR by destination (``edge_index_to_csr`` of the swapped pairs, self loops replaced), its
             transpose map (``wg_csr_transpose_map``) and the BFS at depth 2 from 10 % of the nodes
             (``wg_bfs_levels``), wall time around a device sync, median of ``rounds``.  The reference's BFS (a
             Python loop over the masked nodes, each masking all E edges, GATS.py:37-40) is not timed at this size.

Times are device-event times of ``reps`` back-to-back calls after a warm-up, the paths alternating over ``rounds``
rounds (median and range reported).  Writes one JSON line (also to ``--out``).

    python tools/gats_probe.py [--graph ogbn-arxiv] [--rounds 5] [--reps 20] [--out profiles/r11/gats_probe.json]
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

import gats_ref as R  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip import gats  # noqa: E402
from wats_hip.graphgen import named_graph  # noqa: E402

PARAMS = ("temp_lin.weight", "conf_coef", "bias", "train_a", "dist1_a")


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
    """(a) is faster than (b) in every round by more than (b)'s own run-to-run range."""
    lo, hi = res[b]["us_range"]
    return bool(all(tb - ta > hi - lo for ta, tb in zip(res[a]["us_rounds"], res[b]["us_rounds"])))


def wall(fn, rounds):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return dict(ms=statistics.median(out) * 1e3, ms_range=[min(out) * 1e3, max(out) * 1e3])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--C", type=int, default=40)
    ap.add_argument("--H", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gats_probe: needs a ROCm GPU (there is no CPU path to time)")
    dev = torch.device("cuda")
    g = named_graph(args.graph)
    n, C, H = g.n, args.C, args.H
    indptr = torch.from_numpy(np.asarray(g.indptr)).to(dev)
    indices = torch.from_numpy(np.asarray(g.indices)).to(dev)
    src = torch.repeat_interleave(torch.arange(n, device=dev), (indptr[1:] - indptr[:-1]).long())
    dst = indices.long()
    gen = torch.Generator("cuda").manual_seed(0)
    mask = torch.rand(n, device=dev, generator=gen) < 0.1
    x = torch.randn(n, C, device=dev, generator=gen)

    # construction, step by step, then as the layer does it
    by_dst = lambda: wats_hip.edge_index_to_csr(torch.stack([dst, src]), n, self_loops="one", device=dev)
    csr = by_dst()
    ag = wats_hip.AttentionGraph(g, device=dev)
    assert torch.equal(ag.indices, csr.indices)
    construct = dict(
        csr_by_destination=wall(by_dst, args.rounds),
        transpose_map=wall(lambda: wats_hip.csr_transpose_map(csr.indptr, csr.indices), args.rounds),
        bfs_depth2_mask10pct=wall(lambda: ag.bfs(mask, 2), args.rounds),
        attention_graph_total=wall(lambda: wats_hip.AttentionGraph(g, device=dev), args.rounds),
        reference_host_loop_bfs="not timed at this size")

    torch.manual_seed(0)
    layer = wats_hip.CalibAttentionLayer(C, 1, ag, n, mask, heads=H, device=dev)
    with torch.no_grad():
        layer.conf_coef.fill_(0.3)
        layer.train_a.fill_(1.25)
        layer.dist1_a.fill_(0.8)
    params = {k: p for k, p in layer.named_parameters()}
    ref_params = {k: params[k].detach().clone().requires_grad_(True) for k in PARAMS}
    e_src, e_dst = ag.edge_list()
    dist = layer.dist_to_train

    def layer_hip():
        layer.zero_grad(set_to_none=True)
        layer(x).sum().backward()

    def layer_torch():
        for p in ref_params.values():
            p.grad = None
        R.layer_reference(ref_params, e_src, e_dst, x, dist, 0.2, torch.float32).sum().backward()

    with torch.no_grad():
        a0, t0, conf = layer.attention_inputs(x)
    Gs = torch.randn(n, H, device=dev, generator=gen)

    def attention_hip():
        a, t = a0.detach().requires_grad_(True), t0.detach().requires_grad_(True)
        sim, _ = wats_hip.edge_softmax_attention(ag, a, t, conf)
        sim.backward(Gs)
        return sim, a.grad, t.grad

    def attention_torch():
        a, t = a0.detach().requires_grad_(True), t0.detach().requires_grad_(True)
        sim, _ = R.attention_edges(e_src, e_dst, a, t, conf, 0.2, torch.float32)
        sim.backward(Gs)
        return sim, a.grad, t.grad

    rel = lambda u, v: float((u.double() - v.double()).abs().max() / v.double().abs().max())
    agree = dict(zip(("sim", "grad_a", "grad_t"), (rel(u, v) for u, v in zip(attention_hip(), attention_torch()))))
    res = alternate({"layer_hip": layer_hip, "layer_torch_f32": layer_torch, "attention_hip": attention_hip,
                     "attention_torch_f32": attention_torch}, args.rounds, args.reps)
    line = json.dumps(dict(
        tool="gats_probe", graph=args.graph, n=n, nnz_input=int(g.nnz), nnz_with_self_loops=ag.nnz, C=C, H=H,
        device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, describe=ag.describe(),
        longest_row=int((ag.indptr[1:] - ag.indptr[:-1]).max()), long_row_threshold=gats.long_row_threshold(),
        construct=construct, forward_backward=res, hip_vs_torch_rel_diff=agree,
        layer_hip_beats_torch_every_round=beats_every_round(res, "layer_hip", "layer_torch_f32"),
        attention_hip_beats_torch_every_round=beats_every_round(res, "attention_hip", "attention_torch_f32")))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
