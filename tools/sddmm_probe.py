"""Edge-gradient measurement: wg_sddmm (csrc/sddmm.hip) against the torch
baseline ``(A[rows] * B[cols]).sum(1)`` on the same device, on the arxiv-size
R-MAT graph of ``graphgen.named_graph``:

  (a) the ``EdgeProbe.for_target`` pairs (P = 2N: row t and column t) at F = 128 and F = 64,
  (b) the stored entries as pairs (P = nnz) at F = 64.

Times are device-event times of ``reps`` back-to-back calls after a warm-up,
kernel and baseline alternating over ``rounds`` rounds (median and range
reported).  ``model_bytes = P * 2 * F * 4 + P * 12`` (both rows of every pair,
the two ids and the result); ``fraction_of_hbm`` is model_bytes / time over the
measured 6.29 TB/s copy rate of the MI355X -- above 1 where rows repeat and
come from cache.  Prints one JSON line.

    python tools/sddmm_probe.py [--graph ogbn-arxiv] [--rounds 5] [--reps 50]
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
from wats_hip.graphgen import named_graph  # noqa: E402

HBM_COPY_BYTES_PER_S = 6.29e12


def event_time(fn, reps):
    """Seconds per call over `reps` calls between two device events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / reps


def measure(name, rows, cols, A, B, rounds, reps):
    P, F = int(rows.numel()), int(A.shape[1])
    lrows, lcols = rows.long(), cols.long()

    def kernel():
        return wats_hip.sddmm(rows, cols, A, B, validate=False)

    def baseline():
        return (A[lrows] * B[lcols]).sum(1)

    ref = (A.double()[lrows] * B.double()[lcols]).sum(1)
    scale = ref.abs().max()
    err_kernel = float((kernel().double() - ref).abs().max() / scale)
    err_base = float((baseline().double() - ref).abs().max() / scale)
    del ref
    for fn in (kernel, baseline):               # warm-up: code objects, allocator blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    tk, tb = [], []
    for _ in range(rounds):
        tk.append(event_time(kernel, reps))
        tb.append(event_time(baseline, reps))
    k, b = statistics.median(tk), statistics.median(tb)
    model_bytes = P * 2 * F * 4 + P * 12
    return dict(case=name, P=P, F=F, model_bytes=model_bytes,
                sddmm_us=k * 1e6, sddmm_us_range=[min(tk) * 1e6, max(tk) * 1e6],
                torch_us=b * 1e6, torch_us_range=[min(tb) * 1e6, max(tb) * 1e6],
                speedup_vs_torch=b / k, model_bytes_per_s=model_bytes / k,
                fraction_of_hbm=model_bytes / k / HBM_COPY_BYTES_PER_S,
                max_rel_err_sddmm=err_kernel, max_rel_err_torch=err_base)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sddmm_probe: needs a ROCm GPU (there is no CPU path to time)")
    g = named_graph(args.graph)
    n = g.n
    t = int(np.argmax(np.diff(g.indptr)))       # the hub: the target whose row has the most stored entries
    probe = wats_hip.EdgeProbe.for_target(n, t)
    row_of = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int32), np.diff(g.indptr))).cuda()
    col_of = torch.from_numpy(g.indices.astype(np.int32)).cuda()
    gen = torch.Generator("cuda").manual_seed(0)
    cases = []
    for F in (128, 64):
        A = torch.randn(n, F, device="cuda", generator=gen)
        B = torch.randn(n, F, device="cuda", generator=gen)
        cases.append(measure("for_target", probe.rows, probe.cols, A, B, args.rounds, args.reps))
        if F == 64:
            cases.append(measure("stored_entries", row_of, col_of, A, B, args.rounds, args.reps))
    print(json.dumps(dict(tool="sddmm_probe", graph=args.graph, n=n, nnz=int(g.nnz), target=t,
                          device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, cases=cases)))


if __name__ == "__main__":
    main()
