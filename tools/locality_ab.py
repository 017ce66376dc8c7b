"""Same-session A/B of the relabelling's tie order on one named config: rows of equal
length in caller order (WG_FLAG_CALLER_TIES) against the default, by hottest neighbour, the two
handles of the same graph alternating for --rounds rounds.  Per leg and round: the chain's time
(events around --reps chains, no per-launch events), the mean step-launch time of a profiled run,
and the max relative difference of S against the first leg.

    python tools/locality_ab.py --config ogbn-arxiv [--rounds 3] [--reps 20]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "efficient-gnn_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

import wats_hip  # noqa: E402
from sweep import time_chain  # noqa: E402
from wats_hip.graphgen import NAMED_CONFIGS, named_graph  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ogbn-arxiv")
    ap.add_argument("--F", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    n, nnz, K, F = NAMED_CONFIGS[a.config]
    F = a.F or F
    g = named_graph(a.config)
    handles = {"caller": wats_hip.NormalizedLaplacian.from_graph(g, neighbour_ties=False),
               "neighbour": wats_hip.NormalizedLaplacian.from_graph(g)}
    torch.manual_seed(1)
    X = torch.randn(g.n, F, device="cuda")
    ref = None
    for rnd in range(a.rounds):
        for ties, L in handles.items():
            H, S = wats_hip.graph_wavelet_features(L, X0=X, k=K, s=0.8, return_S=True)
            torch.cuda.synchronize()
            if ref is None:
                ref = S.clone()
            r = time_chain(L, X, K, a.reps)
            r.update(round=rnd, config=a.config, F=F, K=K, ties=ties,
                     S_rel_vs_first=((S - ref).abs().max() / ref.abs().max()).item())
            print(json.dumps(r), flush=True)
    for L in handles.values():
        L.close()


if __name__ == "__main__":
    main()
