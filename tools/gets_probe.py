"""GETS head measurement: the fused gated expert aggregation (csrc/gatedagg.hip through ``gated_sym_norm_head``)
against the composition that existed before it, on the same device in the same process: E ``sym_norm_aggregate``
calls of width C over the same CSR, ``torch.stack`` of their outputs, the product with the dense (n, E) gates, the sum
over the experts, ``softplus``, the product with the logits and ``log_softmax`` (GETS.py:402-417 on ``GCNConv``).

Workload: the arxiv-size R-MAT graph of ``graphgen.named_graph`` with self loops, C = 40, E = 3, k = 2, random
float32 inputs, a random distinct selection per row with softmax gates.  Both paths start from the experts' last
linear maps (the fused head from the stacked (n, E, C) tensor, the composition from E separate (n, C) tensors, so
neither pays for a slice) and end at ``out``; the backward goes to z, the gates, the biases and the logits.

Times are device-event times of ``reps`` back-to-back calls after a warm-up, the two paths alternating over
``rounds`` rounds (median and range reported).  Peak memory is ``torch.cuda.max_memory_allocated`` over one forward +
backward above what is allocated before it.  ``bytes`` is the byte model of the gathers alone (computed from the
shapes, not measured).  Writes one JSON line (also to ``--out``).

    python tools/gets_probe.py [--graph ogbn-arxiv] [--rounds 5] [--reps 20] [--out profiles/r18/gets_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "efficient-gnn_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import wats_hip  # noqa: E402
from wats_hip import gets  # noqa: E402
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


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--C", type=int, default=40)
    ap.add_argument("--E", type=int, default=3)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gets_probe: needs a ROCm GPU (there is no CPU path to time)")
    dev = torch.device("cuda")
    g = named_graph(args.graph)
    n, C, E, k = g.n, args.C, args.E, args.k
    sg = wats_hip.SymNormGraph(g, device=dev)
    gen = torch.Generator("cuda").manual_seed(0)
    z0 = torch.randn(n, E, C, device=dev, generator=gen)
    ze0 = [z0[:, e, :].contiguous() for e in range(E)]
    bias0 = 0.1 * torch.randn(E, C, device=dev, generator=gen)
    logits0 = 2 * torch.randn(n, C, device=dev, generator=gen)
    Gs = torch.randn(n, C, device=dev, generator=gen)
    sel = torch.argsort(torch.rand(n, E, device=dev, generator=gen), dim=1)[:, :k].to(torch.int32).contiguous()
    gate0 = torch.softmax(torch.randn(n, k, device=dev, generator=gen), dim=1)

    def leaves(*ts):
        return [t.detach().requires_grad_(True) for t in ts]

    def fused(z, gate, bias, logits):
        return wats_hip.gated_sym_norm_head(sg, z, sel, gate, bias, logits, check_selection=False)

    def composed(ze, gate, bias, logits):
        outs = torch.stack([wats_hip.sym_norm_aggregate(sg, ze[e], bias[e]) for e in range(E)], dim=1)
        dense = torch.zeros(n, E, device=dev).scatter(1, sel.long(), gate)
        t = (outs * dense.unsqueeze(-1)).sum(dim=1)
        return F.log_softmax(logits * F.softplus(t), dim=1)

    def fused_fwd():
        with torch.no_grad():
            return fused(z0, gate0, bias0, logits0)

    def composed_fwd():
        with torch.no_grad():
            return composed(ze0, gate0, bias0, logits0)

    def fused_fb():
        z, gate, bias, logits = leaves(z0, gate0, bias0, logits0)
        out = fused(z, gate, bias, logits)
        out.backward(Gs)
        return out.detach(), z.grad, gate.grad, bias.grad, logits.grad

    def composed_fb():
        *ze, gate, bias, logits = leaves(*ze0, gate0, bias0, logits0)
        out = composed(ze, gate, bias, logits)
        out.backward(Gs)
        return out.detach(), torch.stack([t.grad for t in ze], dim=1), gate.grad, bias.grad, logits.grad

    rel = lambda u, v: float((u.double() - v.double()).abs().max() / v.double().abs().max().clamp_min(1e-300))
    agree = dict(zip(("out", "g_z", "g_gate", "g_bias", "g_logits"),
                     (rel(u, v) for u, v in zip(fused_fb(), composed_fb()))))
    paths = dict(fused_forward=fused_fwd, composed_forward=composed_fwd, fused_forward_backward=fused_fb,
                 composed_forward_backward=composed_fb)
    res = alternate(paths, args.rounds, args.reps)
    peak = {name: peak_bytes(fn) for name, fn in paths.items()}
    nnz = sg.nnz
    row = 4 * C
    model = dict(
        forward=dict(composed=E * nnz * (4 + 4 + row), fused=nnz * (4 + 4 + k * row)),
        gradient_z=dict(composed=E * nnz * (4 + 4 + row), fused=nnz * (4 + 4 + 8 * k + row)))
    line = json.dumps(dict(
        tool="gets_probe", graph=args.graph, n=n, nnz_input=int(g.nnz), nnz_with_self_loops=nnz, C=C, E=E, k=k,
        device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps,
        long_row_threshold=gets.gated_long_row_threshold(),
        long_rows=[int(t.numel()) for t in gets._long_rows(sg)],
        longest_row=int((sg.indptr[1:] - sg.indptr[:-1]).max()),
        longest_transposed_row=int((sg.t_indptr[1:] - sg.t_indptr[:-1]).max()),
        gather_bytes_model=model, times=res, peak_bytes=peak, fused_vs_composed_rel_diff=agree,
        ratio=dict(forward=res["fused_forward"]["us"] / res["composed_forward"]["us"],
                   forward_backward=res["fused_forward_backward"]["us"] / res["composed_forward_backward"]["us"],
                   peak_forward_backward=peak["fused_forward_backward"] / peak["composed_forward_backward"]),
        fused_forward_beats_composed_every_round=beats_every_round(res, "fused_forward", "composed_forward"),
        fused_forward_backward_beats_composed_every_round=beats_every_round(res, "fused_forward_backward",
                                                                            "composed_forward_backward")))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
