"""Graph-ingestion measurement: ``edge_index`` -> symmetrised, clamped device
CSR without self loops (the ``"attack"`` convention minus its diagonal) on the
directed edge list of the arxiv-size R-MAT graph of ``graphgen.named_graph``
(one direction of every stored edge, about 1.17 M edges), three ways:

  (a) ``wats_hip.edge_index_to_csr`` (wg_coo_to_csr, csrc/ingest.hip);
  (b) torch on the device: keys ``row * n + col`` of both directions,
      ``torch.unique`` (sorted), ``bincount`` and ``cumsum`` for the row pointers;
  (c) the host path: scipy COO -> ``A + A.T`` -> clamp -> CSR, copied to the device.

(a) and (b) are timed between device events over ``reps`` back-to-back calls
after a warm-up, alternating over ``rounds`` rounds (median and range
reported).  (a) returns nnz to the host inside the call (one stream sync);
(b) is timed without a read-back (``unique`` synchronises internally for its
output size anyway) and with ``int(indptr[-1])`` added, so both pairs compare
like with like.  (c) is a host clock around the whole path, ending in a device
synchronise.  The three results are checked to be equal.  Prints one JSON line.

    python tools/ingest_probe.py [--graph ogbn-arxiv] [--rounds 5] [--reps 20]
"""
import argparse
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


def torch_baseline(ei, n):
    keys = torch.cat([ei[0] * n + ei[1], ei[1] * n + ei[0]])
    keys = torch.unique(keys[torch.cat([ei[0] != ei[1]] * 2)])
    rows = torch.div(keys, n, rounding_mode="floor")
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=ei.device)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return indptr, (keys - rows * n).to(torch.int32)


def host_path(src, dst, n):
    import scipy.sparse as sp
    A = sp.coo_matrix((np.ones(src.size, np.float32), (src, dst)), shape=(n, n)).tocsr()
    A = A + A.T
    A.setdiag(0)
    A.eliminate_zeros()
    A.data = np.minimum(A.data, 1.0)
    A.sort_indices()
    out = (torch.from_numpy(A.indptr.astype(np.int64)).cuda(), torch.from_numpy(A.indices.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    return out


def spread(ts):
    return dict(us=statistics.median(ts) * 1e6, us_range=[min(ts) * 1e6, max(ts) * 1e6])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_probe: needs a ROCm GPU (there is no CPU path to time)")
    g = named_graph(args.graph)
    n = g.n
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(g.indptr))
    cols = g.indices.astype(np.int64)
    one_way = rows < cols                           # one direction of every stored edge
    rng = np.random.default_rng(0)
    order = rng.permutation(int(one_way.sum()))     # an edge list arrives in no particular order
    src, dst = rows[one_way][order], cols[one_way][order]
    ei = torch.from_numpy(np.stack([src, dst])).cuda()

    def kernel():
        return wats_hip.edge_index_to_csr(ei, n, symmetric=True, self_loops="remove")

    def baseline():
        return torch_baseline(ei, n)

    def baseline_readback():
        out = torch_baseline(ei, n)
        return out, int(out[0][-1])

    a, b, c = kernel(), baseline(), host_path(src, dst, n)
    assert a.values is None
    for what, (indptr, indices) in (("torch", b), ("host", c)):
        assert torch.equal(a.indptr, indptr) and torch.equal(a.indices, indices), f"{what} path differs"
    assert a.nnz == g.nnz
    for fn in (kernel, baseline, baseline_readback):    # warm-up: code objects, allocator blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ta, tb, tbr, tc = [], [], [], []
    for _ in range(args.rounds):
        ta.append(event_time(kernel, args.reps))
        tb.append(event_time(baseline, args.reps))
        tbr.append(event_time(baseline_readback, args.reps))
        t0 = time.perf_counter()
        host_path(src, dst, n)
        tc.append(time.perf_counter() - t0)
    ka, kb, kbr, kc = (statistics.median(t) for t in (ta, tb, tbr, tc))
    emitted = 2 * int(src.size)
    print(json.dumps(dict(tool="ingest_probe", graph=args.graph, n=n, edges=int(src.size), emitted=emitted,
                          nnz=a.nnz, temp_bytes_model=emitted * 20, device=torch.cuda.get_device_name(0),
                          rounds=args.rounds, reps=args.reps,
                          edge_index_to_csr=spread(ta), torch_device=spread(tb), torch_device_with_nnz=spread(tbr),
                          host_scipy=spread(tc), speedup_vs_torch=kb / ka, speedup_vs_torch_with_nnz=kbr / ka,
                          speedup_vs_host=kc / ka)))


if __name__ == "__main__":
    main()
