"""Batched attack-step measurement: ``wg_fga_scores`` and ``Calib_FGA.attack_many`` against the single-target path
they batch, in the configuration of ``tools/attack_probe.py``: the arxiv-size R-MAT graph of ``graphgen.named_graph``,
``nhid = 64``, ``C = 40``, a ``TemperatureScaling`` surrogate, budget 5, 20 targets.

  scores   ``wg_fga_scores`` (``fga_scores``, buffers allocated ahead) at ``B = 1 / 8 / 32`` for ``G = 1`` and ``G = 3``
           against ``B x`` the single-target scored step it replaces (the probe forward, one or three ``autograd.grad``
           and ``wg_flip_select``); the kernel's byte model: one read of ``z`` and ``h`` per pass of 32 targets
  attack   ``attack_many`` over the targets against one ``flip_beam_hybridloss_attack`` call per target (the path
           before ``attack_many``); the flips must be the same on every target

Host-clock times around work that ends in a device synchronisation, the two sides alternating over ``rounds`` rounds
after a warm-up call each; medians.  Writes one JSON line (also to ``--out``).

    python tools/fga_many_probe.py [--targets 20] [--rounds 5] [--out profiles/r23/s1_fga_many_probe.json]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "efficient-gnn_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import wats_hip  # noqa: E402
from wats_hip import Calib_FGA, RowNormalizedAdjacency, SparseCompatibleGCN, fga_scores  # noqa: E402
from wats_hip.attack import _pack_toggles, fga_scores_workspace  # noqa: E402
from wats_hip.graphgen import named_graph  # noqa: E402

HBM_BYTES_PER_S = 8.0e12      # MI355X peak HBM bandwidth (the byte model's yardstick)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(paths, rounds):
    for fn in paths.values():
        fn()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(timed(fn))
    return {k: dict(us=statistics.median(v) * 1e6, us_range=[min(v) * 1e6, max(v) * 1e6]) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--nfeat", type=int, default=128)
    ap.add_argument("--nhid", type=int, default=64)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--targets", type=int, default=20)
    ap.add_argument("--budget", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fga_many_probe: needs a ROCm GPU (there is no CPU path to time)")
    g = named_graph(args.graph)
    op = RowNormalizedAdjacency.from_graph(g)
    n = g.n
    torch.manual_seed(0)
    base = SparseCompatibleGCN(args.nfeat, nclass=args.classes, nhid=args.nhid).cuda().eval()
    x = torch.randn(n, args.nfeat, device="cuda")
    with torch.no_grad():
        y = base(x, op).argmax(1)
    model = wats_hip.TemperatureScaling(base, x, y, op, torch.arange(0, n, 97, device="cuda"), verbose=False, epochs=1,
                                        frozen_logits=True)
    with torch.no_grad():
        model.temperature.fill_(1.5)
    model = model.eval()
    lengths = np.diff(g.indptr)
    rng = np.random.default_rng(0)
    pool = [int(t) for t in rng.choice(np.flatnonzero(lengths > 0), 2 * args.targets, replace=False)]
    atk = Calib_FGA(model)
    quiet = contextlib.redirect_stdout(io.StringIO())

    def one(t):
        kw = dict(n_perturb=[], best_conf=[])
        with quiet:
            atk.flip_beam_hybridloss_attack(x, op, t, args.budget, "under", res_gt=y, **kw)
        return list(atk.flips)

    # the targets: the first `targets` of the pool whose final label holds (the reference raises on the others)
    targets, flips_single, raised = [], [], 0
    for t in pool:
        if len(targets) == args.targets:
            break
        try:
            flips_single.append(one(t))
            targets.append(t)
        except ValueError:
            raised += 1

    def loop():
        return [one(t) for t in targets]

    def many():
        with quiet:
            return [r["flips"] for r in atk.attack_many(x, op, targets, args.budget, "under", res_gt=y)]

    attack = alternate({"attack_many": many, "single_target_loop": loop}, args.rounds)
    same = sum(int(a == b) for a, b in zip(many(), flips_single))

    # the scored step alone
    with torch.no_grad():
        z = (x @ base.gc1.weight.t()).contiguous()
        b1, W2 = base.gc1.bias.detach(), base.gc2.weight.detach().contiguous()
        h = torch.relu(op @ z + b1).contiguous()
    scores = {}
    for G in (1, 3):
        for B in (1, 8, 32):
            ts = (targets * (B // len(targets) + 1))[:B]
            tg, tog_ptr, tog_ids = _pack_toggles(n, ts, [[] for _ in ts], "cuda")
            gl = torch.randn(B, G, args.classes, device="cuda")
            rr = torch.ones(B, dtype=torch.int32, device="cuda") if G == 3 else None
            p2 = torch.tensor([[0.6, 0.3]] * B, device="cuda") if G == 3 else None
            cap = int(sum(lengths[t] for t in ts))
            ws = fga_scores_workspace(n, args.nhid, B, G, cap, "cuda")

            def kernel():
                fga_scores(n, op.indptr, op.indices, z, h, b1, W2, tg, (tog_ptr, tog_ids), gl, rr, p2, topk=1,
                           workspace=ws, local_cap=cap)

            def single_steps():
                for t in ts:
                    atk._begin(x, op, t)
                    out = atk._forward_probe(set())
                    loss = wats_hip.kl_divergence_with_uniform(out, out.argmax(1))
                    grad = atk._grad(loss, retain_graph=True)
                    atk._select(set(), grad, atk._rerank_terms(out) if G == 3 else None)

            r = alternate({"fga_scores": kernel, "single_target_steps": single_steps}, args.rounds)
            passes = (B + 31) // 32
            model_bytes = passes * 2 * n * args.nhid * 4
            r["byte_model"] = dict(bytes=model_bytes, us_at_peak=model_bytes / HBM_BYTES_PER_S * 1e6,
                                   fraction=model_bytes / HBM_BYTES_PER_S * 1e6 / r["fga_scores"]["us"])
            scores[f"G{G}_B{B}"] = r
    line = json.dumps(dict(tool="fga_many_probe", graph=args.graph, n=n, nnz=int(g.nnz), nfeat=args.nfeat,
                           nhid=args.nhid, classes=args.classes, budget=args.budget, surrogate="TemperatureScaling",
                           device=torch.cuda.get_device_name(0), rounds=args.rounds, targets=targets,
                           targets_raised_and_left_out=raised, attack=attack,
                           attack_speedup=attack["single_target_loop"]["us"] / attack["attack_many"]["us"],
                           targets_with_the_same_flips=same, scores=scores))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
