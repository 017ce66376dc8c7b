"""Random-attack measurement: one step's trials as one ``wg_trial_logits`` launch against the same trials as one
``wg_target_logits`` call each (the API before it) and against the view path (``with_flips`` + a full forward per
trial), and ``attack_many`` against single attacks, on the arxiv-size R-MAT graph of ``graphgen.named_graph`` with
``nhid = 64``, ``C = 40`` and a temperature-scaling calibrator over the base model.

  step_50 / step_100   the logits of 50 / 100 structure trials of one target: ``batched`` (one launch, the trials as
                       prebuilt device arrays), ``per_trial`` (one ``target_logits`` call per trial, prebuilt arrays;
                       a trial that removes the self loop is replaced by another partner there, which that entry
                       cannot express), ``view`` (the class's view path, trial by trial)
  step_50_features     the same with every second trial a feature flip: ``batched`` against ``view``
  attack_many          20 targets, budget 5, max_trials 50: ``attack_many`` (one launch per step for all targets)
                       against 20 single ``attack`` calls with the same seeds; structure only, and structure + features

Device events around each variant, the variants interleaved in one process over ``rounds`` rounds after a warm-up
call each; per measurement the median and the range over the rounds.  Writes one JSON line (also to ``--out``).

    python tools/random_probe.py [--graph ogbn-arxiv] [--targets 20] [--rounds 5] [--out profiles/r22/s1_random_probe.json]
"""
import argparse
import json
import os
import random
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "efficient-gnn_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from wats_hip import (Calib_Random, RowNormalizedAdjacency, SparseCompatibleGCN, TemperatureScaling,  # noqa: E402
                      target_logits, trial_logits)
from wats_hip.graphgen import named_graph  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3          # microseconds


def alternate(paths, rounds):
    for fn in paths.values():
        fn()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(timed(fn))
    return {k: dict(us=statistics.median(v), us_range=[min(v), max(v)]) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--nfeat", type=int, default=128)
    ap.add_argument("--nhid", type=int, default=64)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--targets", type=int, default=20)
    ap.add_argument("--budget", type=int, default=5)
    ap.add_argument("--max-trials", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("random_probe: needs a ROCm GPU (there is no CPU path to time)")
    g = named_graph(args.graph)
    op = RowNormalizedAdjacency.from_graph(g)
    torch.manual_seed(0)
    model = SparseCompatibleGCN(args.nfeat, nclass=args.classes, nhid=args.nhid).cuda().eval()
    x = (torch.rand(g.n, args.nfeat, device="cuda") < 0.3).float()
    with torch.no_grad():
        y = model(x, op).argmax(1)
    val_idx = torch.randperm(g.n, device="cuda")[:g.n // 10]
    cal = TemperatureScaling(model, x, y, op, val_idx, verbose=False, epochs=5, frozen_logits=True).eval()
    lengths = np.diff(g.indptr)
    rng = np.random.default_rng(0)
    targets = [int(t) for t in rng.choice(np.flatnonzero(lengths > 0), args.targets, replace=False)]
    t0 = targets[0]
    dev = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda")

    # ---- one step's trials of one target, drawn by the class itself
    result = {}
    for name, n_trials, features in (("step_50", 50, False), ("step_100", 100, False), ("step_50_features", 50, True)):
        atk = Calib_Random(cal, attack_structure=True, attack_features=features)
        view = Calib_Random(cal, attack_structure=True, attack_features=features, local_eval=False)
        for a in (atk, view):
            a._begin(x, op)
        T = atk._new_target(t0, random.Random(1))
        specs = []
        for d in atk._draw_step(T, n_trials)[0]:
            S, feats = atk._trial_spec(T, d)
            specs.append((t0, S, dict(feats)))
        model_args = (model.gc1.bias.detach(), model.gc2.weight.detach().contiguous(), model.gc2.bias.detach())
        z = (x @ model.gc1.weight.t()).contiguous()
        ptrs = np.concatenate([[0], np.cumsum([len(s[1]) for s in specs])])
        arrays = [dev([t0] * n_trials, torch.int32), dev(ptrs, torch.int32),
                  dev([j for s in specs for j in s[1]], torch.int32)]
        if features:
            fptr = np.concatenate([[0], np.cumsum([len(s[2]) for s in specs])])
            arrays += [dev(fptr, torch.int32), dev([f for s in specs for f in sorted(s[2])], torch.int32),
                       dev([s[2][f] for s in specs for f in sorted(s[2])], torch.float32)]
        w1 = model.gc1.weight.detach()
        paths = {"batched": lambda: cal.row_map(trial_logits(g.n, op.indptr, op.indices, z, *model_args, tuple(arrays),
                                                             W1=w1 if features else None))}
        if not features:
            other = next(j for j in range(g.n) if j != t0)
            singles = [(dev([0, len(S)], torch.int32), dev(S, torch.int32))
                       for S in (sorted({j if j != t0 else other for j in s[1]}) for s in specs)]
            paths["per_trial"] = lambda: [cal.row_map(target_logits(g.n, op.indptr, op.indices, z, *model_args, t0, c))
                                          for c in singles]
        Tv = view._new_target(t0, random.Random(1))
        paths["view"] = lambda: [view._forward_view(Tv, s[1], s[2]) for s in specs]
        result[name] = alternate(paths, args.rounds)
        result[name]["row_length"] = int(lengths[t0])

    # ---- attack_many against single attacks
    seeds = list(range(100, 100 + len(targets)))
    for name, features in (("attack_many_structure", False), ("attack_many_structure_features", True)):
        atk = Calib_Random(cal, attack_structure=True, attack_features=features)
        got = {}

        def many():
            got["many"] = atk.attack_many(x, op, targets, args.budget, "under", max_trials=args.max_trials, seed=seeds)

        def single():
            out = []
            for t, s in zip(targets, seeds):
                random.seed(s)
                atk.attack(x, op, t, args.budget, "under", max_trials=args.max_trials)
                out.append((list(atk.flips), dict(atk.feature_flips)))
            got["single"] = out
        result[name] = alternate({"attack_many": many, "single_attacks": single}, args.rounds)
        result[name]["same_results"] = [(r["flips"], r["feature_flips"]) for r in got["many"]] == got["single"]
        result[name]["accepted"] = int(sum(r["n_perturb"] for r in got["many"]))
    line = json.dumps(dict(tool="random_probe", graph=args.graph, n=g.n, nnz=int(g.nnz), nfeat=args.nfeat, nhid=args.nhid,
                           classes=args.classes, budget=args.budget, max_trials=args.max_trials, targets=len(targets),
                           device=torch.cuda.get_device_name(0), rounds=args.rounds, **result))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
