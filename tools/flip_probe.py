"""Edge-flip view measurement: one candidate of an attack iteration (calib_fga.py:901-913) as a rebuilt
operator against a view of its parent, on the arxiv-size R-MAT graph of ``graphgen.named_graph`` at F = 64.

  candidate  (a) ``op.flipped([t], [j])`` + one forward and one backward of ``propagate``
             (b) ``op.with_flips([t], [j])`` + the same forward and backward
             with the parent ``op`` the plain graph (P = 1) or the graph after 31 earlier flips of the same
             target (P = 32: (a) starts from the rebuilt operator of those 31, (b) from their view)
  commit     (a) ``toggle_edges`` of P pairs   (b) ``view.csr()`` of a view of those P pairs (``wg_csr_patch``
             alone; ``view+commit`` adds the ``with_flips`` that made the view)
  forward    the view's forward beside the parent's: the difference is what the overlay costs

for two targets, the hub (the longest row) and a row of median length among the rows that have entries.  Times
are device-event times of ``reps`` back-to-back calls after a warm-up, the paths alternating over ``rounds``
rounds (median and range reported).  Writes one JSON line (also to ``--out``).

    python tools/flip_probe.py [--graph ogbn-arxiv] [--rounds 5] [--reps 20] [--out profiles/r09/flip_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "efficient-gnn_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import wats_hip  # noqa: E402
from wats_hip import RowNormalizedAdjacency, propagate, toggle_edges  # noqa: E402
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
    """{name: {us, us_range}} of the callables in `paths`, alternating over `rounds` rounds."""
    for fn in paths.values():                   # warm-up: code objects, allocator blocks, step plans
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(event_time(fn, reps))
    return {k: dict(us=statistics.median(v) * 1e6, us_range=[min(v) * 1e6, max(v) * 1e6]) for k, v in times.items()}


def beats(res, a, b):
    """(b) is faster than (a) by more than (a)'s own run-to-run range."""
    lo, hi = res[a]["us_range"]
    return bool(res[a]["us"] - res[b]["us"] > hi - lo)


def flip_columns(g, t, count, rng):
    """`count` distinct columns != t, alternating absent and present entries of row t (absent first)."""
    row = set(int(c) for c in g.indices[g.indptr[t]:g.indptr[t + 1]])
    present = [c for c in sorted(row) if c != t]
    rng.shuffle(present)
    absent = []
    while len(absent) < count:
        c = int(rng.integers(0, g.n))
        if c != t and c not in row and c not in absent:
            absent.append(c)
    out = []
    for k in range(count):
        out.append(present.pop() if (k % 2 and present) else absent.pop())
    return out


def measure_target(name, g, op, t, x, gy, rounds, reps):
    rng = np.random.default_rng(t)
    cols = flip_columns(g, t, 32, rng)
    res = dict(target=name, row=int(t), row_length=int(g.indptr[t + 1] - g.indptr[t]), cases=[])

    def evaluate(adj):
        xi = x.detach().requires_grad_(True)
        y = propagate(adj, xi)
        y.backward(gy)
        return y, xi.grad

    for P in (1, 32):
        earlier = ([t] * (P - 1), cols[:P - 1])
        last = ([t], [cols[P - 1]])
        parent_real = op if P == 1 else op.flipped(*earlier)
        parent_view = op if P == 1 else op.with_flips(*earlier)
        ya, ga = evaluate(parent_real.flipped(*last))
        yb, gb = evaluate(parent_view.with_flips(*last))
        err = lambda u, v: float((u.double() - v.double()).abs().max() / v.double().abs().max())
        cand = alternate({"rebuild": lambda: evaluate(parent_real.flipped(*last)),
                          "view": lambda: evaluate(parent_view.with_flips(*last))}, rounds, reps)
        view = parent_view.with_flips(*last)
        fwd = alternate({"parent_forward": lambda: op.fwd.apply(x), "view_forward": lambda: view.fwd.apply(x),
                         "parent_backward": lambda: op.bwd.apply(gy), "view_backward": lambda: view.bwd.apply(gy)},
                        rounds, reps)
        rows_p, cols_p = [t] * P, cols[:P]

        def commit_only():
            view._csr = None
            return view.csr()

        com = alternate({"toggle_edges": lambda: toggle_edges(g.n, op.indptr, op.indices, op.values, rows_p, cols_p),
                         "view_csr": commit_only,
                         "view_and_commit": lambda: op.with_flips(rows_p, cols_p).csr()}, rounds, reps)
        ref = toggle_edges(g.n, op.indptr, op.indices, op.values, rows_p, cols_p)
        same = all(torch.equal(u, v) for u, v in zip(op.with_flips(rows_p, cols_p).csr(), ref))
        res["cases"].append(dict(
            P=P, overlay_positions=view.n_positions, candidate=cand, candidate_view_beats_rebuild=beats(cand, "rebuild", "view"),
            forward_rel_diff=err(yb, ya), backward_rel_diff=err(gb, ga), propagation=fwd,
            overlay_forward_cost_us=fwd["view_forward"]["us"] - fwd["parent_forward"]["us"],
            overlay_backward_cost_us=fwd["view_backward"]["us"] - fwd["parent_backward"]["us"],
            commit=com, commit_csr_beats_toggle=beats(com, "toggle_edges", "view_csr"),
            commit_view_and_csr_beats_toggle=beats(com, "toggle_edges", "view_and_commit"), commit_bitwise_equal=same))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--F", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flip_probe: needs a ROCm GPU (there is no CPU path to time)")
    g = named_graph(args.graph)
    lengths = np.diff(g.indptr)
    hub = int(np.argmax(lengths))
    with_entries = np.flatnonzero(lengths > 0)
    median = int(with_entries[np.argsort(lengths[with_entries], kind="stable")[len(with_entries) // 2]])
    op = RowNormalizedAdjacency.from_graph(g)
    gen = torch.Generator("cuda").manual_seed(0)
    x = torch.randn(g.n, args.F, device="cuda", generator=gen)
    gy = torch.randn(g.n, args.F, device="cuda", generator=gen)
    targets = [measure_target(name, g, op, t, x, gy, args.rounds, args.reps) for name, t in (("hub", hub), ("median", median))]
    line = json.dumps(dict(tool="flip_probe", graph=args.graph, n=g.n, nnz=int(g.nnz), F=args.F,
                           device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, targets=targets))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
