"""Gather-line L2 misses of one arxiv-size F = 40 step under the plan's two locality choices (CPU
model; l2_lru_sim.py is the model of the parent plan alone).

Rows in internal order; rows longer than a share (G * tch * 4 ids: 576 at team_iter 96) are dealt
to part waves over contiguous ranges of their sorted columns, the rest to team waves of G = 6 rows;
waves dispatched alternately from the long and the short end (team_order 2), workgroups of 4 waves
dealt round-robin to the 8 XCDs; every gathered u row is 160 B at a 160-B stride; one LRU of
--cap lines (3.1 MB) per XCD for the gather lines.  Three plans:

  parent      ties of the degree sort in caller order, part waves where the dispatch order puts them
  ties        rows of equal length by hottest, then second-hottest neighbour (prologue.hip)
  ties+xcd    and the part waves re-dealt among their positions by column bucket, one bucket per XCD

Prints each plan's misses (total and per XCD) and each XCD's gathered-id total.

    python tools/locality_sim.py [--config ogbn-arxiv] [--team-iter 96] [--cap 24576]
"""
import argparse
import os
import sys
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "efficient-gnn_amd"))
from wats_hip.graphgen import named_graph  # noqa: E402

G, P, RB, WG = 6, 8, 160, 4   # rows per team wave, XCDs, bytes per gathered row, waves per workgroup


def rank_of(order, n):
    r = np.full(n, -1, np.int64)
    r[order] = np.arange(len(order))
    return r


def units_of(order, deg, ind, ip, share):
    """The waves' gathered internal columns, longest rows first; the first n_parts are part waves."""
    rank = rank_of(order, len(deg))
    units, i = [], 0
    while i < len(order) and deg[order[i]] > share:
        c = np.sort(rank[ind[ip[order[i]]:ip[order[i] + 1]]])
        units += [c[s:s + share] for s in range(0, len(c), share)]
        i += 1
    n_parts = len(units)
    while i < len(order):
        units.append(np.concatenate([rank[ind[ip[r]:ip[r + 1]]] for r in order[i:i + G]]))
        i += G
    return units, n_parts


def run(units, xcd, seq, cap):
    caches = [OrderedDict() for _ in range(P)]
    miss = np.zeros(P, np.int64)
    ids = np.zeros(P, np.int64)
    for k in seq:
        x = xcd[k]
        c = caches[x]
        b0 = units[k] * RB
        ids[x] += len(b0)
        for a, b in zip((b0 // 128).tolist(), ((b0 + RB - 1) // 128).tolist()):
            for line in range(a, b + 1):
                if line in c:
                    c.move_to_end(line)
                else:
                    miss[x] += 1
                    c[line] = 1
                    if len(c) > cap:
                        c.popitem(last=False)
    return miss, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ogbn-arxiv")
    ap.add_argument("--team-iter", type=int, default=96)
    ap.add_argument("--cap", type=int, default=24576, help="gather lines per XCD L2 (24576 = 3.1 MB)")
    a = ap.parse_args()
    A = named_graph(a.config).to_scipy().tocsr()
    deg, ind, ip = np.diff(A.indptr), A.indices, A.indptr
    n = A.shape[0]
    share = G * max(2, (a.team_iter // 4 + 1) // 2 * 2) * 4
    base = np.argsort(-deg, kind="stable")
    base = base[deg[base] > 0]
    r0 = rank_of(base, n)
    m = np.full((n, 2), n, np.int64)
    for r in base:
        nb = np.sort(r0[ind[ip[r]:ip[r + 1]]])[:2]
        m[r, :len(nb)] = nb
    ties = base[np.lexsort((base, m[base, 1], m[base, 0], -deg[base]))]
    for name, order, affine in (("parent", base, False), ("ties", ties, False), ("ties+xcd", ties, True)):
        units, n_parts = units_of(order, deg, ind, ip, share)
        N = len(units)
        seq, lo, hi = [], 0, N   # team_order 2: one wave from the long end, one from the short end
        while lo < hi:
            seq.append(lo)
            lo += 1
            if lo < hi:
                hi -= 1
                seq.append(hi)
        xcd = np.empty(N, np.int64)
        xcd[np.array(seq)] = (np.arange(N) // WG) % P
        if affine:   # the same part count per XCD, the parts chosen by middle column
            cnt = np.bincount(xcd[:n_parts], minlength=P)
            by_col = np.argsort([u[len(u) // 2] for u in units[:n_parts]], kind="stable")
            xcd[by_col] = np.repeat(np.arange(P), cnt)
        miss, ids = run(units, xcd, seq, a.cap)
        print(f"{name}: share {share} ids, {n_parts} part waves, gather line misses {miss.sum()} "
              f"(per XCD {miss.min()} .. {miss.max()}); ids per XCD {ids.tolist()}; "
              f"part ids per XCD {[int(sum(len(units[k]) for k in range(n_parts) if xcd[k] == x)) for x in range(P)]}",
              flush=True)


if __name__ == "__main__":
    main()
