"""Attack-step measurement: ``wats_hip.Calib_FGA`` with its two kernels (``wg_flip_select``, ``wg_target_logits``)
against the same loop built only from the API that existed before them (``target_scores_from_grad`` + torch
elementwise ops + ``argmax`` for the selection, ``with_flips`` + a full forward for the candidate), on the
arxiv-size R-MAT graph of ``graphgen.named_graph`` with ``nhid = 64``, ``C = 40``, 20 targets, budget 5.

  step        one scored step of ``flip_beam_hybridloss_attack`` from the unflipped graph: the forward with the
              probe, three ``autograd.grad``, the selection, the candidate's logits
  selection   the selection alone, from gradients already taken
  candidate   the candidate's logits alone: ``wg_target_logits`` against a forward through the ``with_flips`` view
  attack      a whole ``flip_beam_hybridloss_attack``: with both kernels, with ``local_eval=False`` (the selection
              kernel only) and the earlier-API loop

Host-clock times around work that ends in a device synchronisation (every step ends in a host read of the chosen
partner), the variants alternating per target over ``rounds`` rounds; per measurement the median over targets of the
per-target median, and the range of the per-target medians.  Writes one JSON line (also to ``--out``).

    python tools/attack_probe.py [--graph ogbn-arxiv] [--targets 20] [--rounds 3] [--out profiles/r19/attack_probe.json]
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

from wats_hip import Calib_FGA, RowNormalizedAdjacency, SparseCompatibleGCN, target_scores_from_grad  # noqa: E402
from wats_hip.graphgen import named_graph  # noqa: E402


class EarlierApiFGA(Calib_FGA):
    """The same loop from ``INTEGRATION.md`` 3c's recipe: the score from ``target_scores_from_grad`` (a dense row of
    the adjacency), the rerank as torch elementwise operations, ``argmax`` read on the host, the candidate through the
    view."""

    def __init__(self, model, **kw):
        super().__init__(model, local_eval=False, **kw)

    def _select(self, toggles, grad_loss, rerank=None):
        n, t = self._n, self._t
        adj = self._view(toggles) if toggles else self._start
        scores = target_scores_from_grad(grad_loss, adj, t)
        if rerank is not None:
            top2, gp, gs = rerank
            delta = 1 - 2 * adj.dense_row(t)
            cond = top2[0] + gp[:n] * delta - top2[1] - gs[:n] * delta
            scores = scores * torch.where(cond > 0, torch.tensor(1, device=cond.device),
                                          torch.tensor(-1, device=cond.device))
        scores[t] = -10
        self._last_scores = None
        return int(torch.argmax(scores))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(paths, rounds):
    """{name: median seconds} of the callables, alternating over `rounds` rounds after one warm-up call each"""
    for fn in paths.values():
        fn()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in times.items()}


def summary(per_target):
    """{name: {us, us_range}} over the targets' medians"""
    names = per_target[0].keys()
    return {k: dict(us=statistics.median(r[k] for r in per_target) * 1e6,
                    us_range=[min(r[k] for r in per_target) * 1e6, max(r[k] for r in per_target) * 1e6])
            for k in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--nfeat", type=int, default=128)
    ap.add_argument("--nhid", type=int, default=64)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--targets", type=int, default=20)
    ap.add_argument("--budget", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attack_probe: needs a ROCm GPU (there is no CPU path to time)")
    g = named_graph(args.graph)
    op = RowNormalizedAdjacency.from_graph(g)
    torch.manual_seed(0)
    model = SparseCompatibleGCN(args.nfeat, nclass=args.classes, nhid=args.nhid).cuda().eval()
    x = torch.randn(g.n, args.nfeat, device="cuda")
    with torch.no_grad():
        y = model(x, op).argmax(1)
    lengths = np.diff(g.indptr)
    rng = np.random.default_rng(0)
    targets = [int(t) for t in rng.choice(np.flatnonzero(lengths > 0), args.targets, replace=False)]
    variants = {"kernels": Calib_FGA(model), "select_kernel_view_eval": Calib_FGA(model, local_eval=False),
                "earlier_api": EarlierApiFGA(model)}
    steps, selections, candidates, attacks, same, hops = [], [], [], [], 0, []
    quiet = contextlib.redirect_stdout(io.StringIO())
    for t in targets:
        state = {}
        for name, atk in variants.items():
            atk._begin(x, op, t)
            with torch.no_grad():
                label = atk._evaluate_start().argmax(1)
            out = atk._forward_probe(set())
            loss = -out[0, int(label)]
            grad = atk._grad(loss, retain_graph=True)
            rer = atk._rerank_terms(out)
            state[name] = (label, grad, rer, atk._select(set(), grad, rer))

        def step(name):
            atk = variants[name]
            j, _, _, _ = atk._hybrid_step(set(), state[name][0], True)
            return atk._evaluate({j})

        steps.append(alternate({k: (lambda k=k: step(k)) for k in variants}, args.rounds))
        selections.append(alternate({k: (lambda k=k: variants[k]._select(set(), state[k][1], state[k][2]))
                                     for k in ("kernels", "earlier_api")}, args.rounds))
        j = state["kernels"][3]
        a, b = variants["kernels"]._evaluate({j}), variants["earlier_api"]._evaluate({j})
        candidates.append(dict(alternate({"target_logits": lambda: variants["kernels"]._evaluate({j}),
                                          "view_forward": lambda: variants["earlier_api"]._evaluate({j})}, args.rounds),
                               diff=float((a - b).abs().max())))
        rows = [int(c) for c in g.indices[g.indptr[t]:g.indptr[t + 1]]]
        hops.append(dict(target=t, row_length=len(rows), two_hop_entries=int(sum(lengths[c] for c in rows))))

        def attack(name):
            kw = dict(n_perturb=[], best_conf=[])
            with quiet:
                try:
                    variants[name].flip_beam_hybridloss_attack(x, op, t, args.budget, "under", res_gt=y, **kw)
                except ValueError:      # the reference's final label check (calib_fga.py:957-958)
                    pass
            return list(variants[name].flips)
        attacks.append(alternate({k: (lambda k=k: attack(k)) for k in variants}, args.rounds))
        same += int(attack("kernels") == attack("earlier_api") == attack("select_kernel_view_eval"))
    diff = max(c.pop("diff") for c in candidates)
    line = json.dumps(dict(tool="attack_probe", graph=args.graph, n=g.n, nnz=int(g.nnz), nfeat=args.nfeat, nhid=args.nhid,
                           classes=args.classes, budget=args.budget, device=torch.cuda.get_device_name(0),
                           rounds=args.rounds, targets=hops, step=summary(steps), selection=summary(selections),
                           candidate=summary(candidates), attack=summary(attacks),
                           candidate_logits_max_diff=diff, targets_with_the_same_flips=same))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
