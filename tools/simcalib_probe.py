"""SimCalib similarity-temperature measurement: forward + backward of ``similarity_temperature`` on the HIP kernels
(csrc/simcalib.hip) against the torch restatement on the same device, at the ogbn-arxiv size (n = 169 343 latent
rows, m = 29 799 validation rows, d = 64) with random float32 inputs.

  (a) hip          ``wats_hip.similarity_temperature`` and its backward
  (b) torch_f32    the dense restatement of tests/simcalib_ref.py in float32 in row chunks, each chunk's forward and
                   backward before the next, so only (chunk, m) matrices are alive.  The unchunked reference needs
                   n * m * 4 bytes per copy (20 GB at this size) and several copies at once: it is not run.

Times are device-event times of ``reps`` back-to-back forward + backward calls after a warm-up, the paths alternating
over ``rounds`` rounds (median and range reported); peak memory is torch's allocator peak over one call of each path.
The model figure is the float32 matrix peak of the guide (157 TFLOP/s): one n x m x d product forward, two more backward.
Writes one JSON line (also to ``--out``).

    python tools/simcalib_probe.py [--rounds 5] [--reps 3] [--calibrator] [--out profiles/r13/simcalib_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "efficient-gnn_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import simcalib_ref as R  # noqa: E402
import wats_hip  # noqa: E402

PEAK_F32_MATRIX = 157.3e12


def event_time(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / reps


def alternate(paths, rounds, reps):
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(event_time(fn, reps))
    return {k: dict(ms=statistics.median(v) * 1e3, ms_range=[min(v) * 1e3, max(v) * 1e3],
                    ms_rounds=[t * 1e3 for t in v]) for k, v in times.items()}


def beats_every_round(res, a, b):
    spread = max(res[a]["ms_range"][1] - res[a]["ms_range"][0], res[b]["ms_range"][1] - res[b]["ms_range"][0])
    return bool(all(tb - ta > spread for ta, tb in zip(res[a]["ms_rounds"], res[b]["ms_rounds"])))


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def calibrator_run(dev, n_val):
    """The whole calibrator at the arxiv size: a SparseCompatibleGCN (128 features, nhid 64, 40 classes, random
    weights) on the arxiv-size R-MAT graph, ``n_val`` random validation nodes, one forward with the attack's probe
    (row and column of a target node) and one backward: wall times around device syncs and the allocator's peak."""
    import time

    from wats_hip.graphgen import named_graph
    g = named_graph("ogbn-arxiv")
    n = g.n
    torch.manual_seed(0)
    op = wats_hip.RowNormalizedAdjacency.from_graph(g, device=dev)
    base = wats_hip.SparseCompatibleGCN(nfeat=128, nclass=40, nhid=64).to(dev)
    x = torch.randn(n, 128, device=dev)
    y = torch.randint(0, 40, (n,), device=dev)
    val_mask = torch.zeros(n, dtype=torch.bool, device=dev)
    val_mask[torch.randperm(n, device=dev)[:n_val]] = True
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    cal = wats_hip.SimCalib(base, x, y, op, val_mask)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    probe = wats_hip.EdgeProbe.for_target(n, 12345, device=dev)
    out = cal(x, op, probe=probe)
    loss = torch.nn.functional.nll_loss(out[val_mask], y[val_mask])
    loss.backward()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    grad = probe.grad
    return dict(n=n, nnz=int(g.nnz), n_val=int(val_mask.sum()), construct_ms=(t1 - t0) * 1e3,
                forward_backward_ms=(t2 - t1) * 1e3, peak_bytes=int(torch.cuda.max_memory_allocated() - before),
                dense_matrix_bytes=4 * n * int(val_mask.sum()), probe_positions=len(probe),
                probe_grad_finite=bool(torch.isfinite(grad).all()), probe_grad_max=float(grad.abs().max()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=169343)
    ap.add_argument("--m", type=int, default=29799)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--tau", type=float, default=0.1)
    ap.add_argument("--chunk", type=int, default=8192, help="rows per chunk of the torch path")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--paths", default="all", choices=["all", "hip"])
    ap.add_argument("--calibrator", action="store_true",
                    help="also run wats_hip.SimCalib end to end on the arxiv-size graph with an EdgeProbe")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("simcalib_probe: needs a ROCm GPU (there is no CPU path to time)")
    dev = torch.device("cuda")
    n, m, d, tau = args.n, args.m, args.d, args.tau
    gen = torch.Generator("cuda").manual_seed(0)
    x0 = torch.randn(n, d, device=dev, generator=gen)
    bank = F.normalize(torch.randn(m, d, device=dev, generator=gen), p=2, dim=1)
    inv_conf = 1.0 / (0.1 + 0.9 * torch.rand(m, device=dev, generator=gen) + 1e-8)
    gt = torch.randn(n, device=dev, generator=gen)

    def hip():
        x = x0.detach().requires_grad_(True)
        t = wats_hip.similarity_temperature(x, bank, inv_conf, tau)
        t.backward(gt)
        return t.detach(), x.grad

    def hip_forward():
        with torch.no_grad():
            return wats_hip.similarity_temperature(x0, bank, inv_conf, tau)

    def torch_chunked():
        ts, gs = [], []
        for lo in range(0, n, args.chunk):
            x = x0[lo:lo + args.chunk].detach().requires_grad_(True)
            t = R.raw_temperature(x, bank, inv_conf, tau, torch.float32).clamp(min=R.T_MIN, max=R.T_MAX)
            t.backward(gt[lo:lo + args.chunk])
            ts.append(t.detach())
            gs.append(x.grad)
        return torch.cat(ts), torch.cat(gs)

    paths = {"hip": hip, "hip_forward_only": hip_forward}
    agree = None
    if args.paths == "all":
        paths["torch_f32_chunked"] = torch_chunked
        a, b = hip(), torch_chunked()
        agree = [float((u.double() - v.double()).abs().max() / v.double().abs().max()) for u, v in zip(a, b)]
    peaks = {k: peak_bytes(fn) for k, fn in paths.items()}
    res = alternate(paths, args.rounds, args.reps)
    flops = 2.0 * n * m * d
    model = dict(forward_ms=flops / PEAK_F32_MATRIX * 1e3, forward_backward_ms=3 * flops / PEAK_F32_MATRIX * 1e3)
    out = dict(tool="simcalib_probe", n=n, m=m, d=d, tau=tau, chunk=args.chunk,
               device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps,
               forward_backward=res, peak_bytes=peaks, dense_matrix_bytes=4 * n * m,
               model_f32_matrix_peak=model,
               fraction_of_peak=dict(forward=model["forward_ms"] / res["hip_forward_only"]["ms"],
                                     forward_backward=model["forward_backward_ms"] / res["hip"]["ms"]),
               hip_vs_torch_rel_diff=agree)
    if args.paths == "all":
        out["hip_beats_torch_every_round"] = beats_every_round(res, "hip", "torch_f32_chunked")
    if args.calibrator:
        out["calibrator"] = calibrator_run(dev, m)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
