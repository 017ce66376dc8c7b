"""Integrated-gradient scores measurement: ``wg_iga_path_logits``, ``wg_iga_scores`` and one whole
``Calib_IGA.attack`` on the arxiv-size R-MAT graph of ``graphgen.named_graph`` with ``nhid = 64``, ``C = 40``,
``steps = 10``, ``topk = 10`` and ``B`` in 1, 8, 32 targets.

Beside ``wg_iga_scores``: a torch composition of the same closed form from the kernel's own coefficients -- a float64
``[H Z] @ coeffs`` for both paths, the sign by a dense 0 / 1 row per target, ``-10`` at the target and ``torch.topk`` --
which is what the scoring pass would be without the kernel.  Also reported: the HBM copy rate measured here (a device
to device copy of 256 MiB, read plus write) and the fraction of it that the pass's byte model (``8 n Hd`` bytes per
launch: ``z`` and ``h`` read once) reaches.

Device times by events around ``iters`` back-to-back launches after a warm-up, the median of ``rounds`` rounds; the
whole attack by the host clock around a call that ends in host reads.  Writes one JSON line (also to ``--out``).

    python tools/iga_probe.py [--graph ogbn-arxiv] [--out profiles/r20/iga_probe.json]
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

from wats_hip import Calib_IGA, RowNormalizedAdjacency, SparseCompatibleGCN, iga_path_logits, iga_scores  # noqa: E402
from wats_hip.attack import iga_scores_workspace  # noqa: E402
from wats_hip.graphgen import named_graph  # noqa: E402


def device_us(fn, iters, rounds):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return dict(us=statistics.median(out), us_range=[min(out), max(out)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--nfeat", type=int, default=128)
    ap.add_argument("--nhid", type=int, default=64)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("iga_probe: needs a ROCm GPU (there is no CPU path to time)")
    g = named_graph(args.graph)
    op = RowNormalizedAdjacency.from_graph(g)
    n, Hd = g.n, args.nhid
    torch.manual_seed(0)
    model = SparseCompatibleGCN(args.nfeat, nclass=args.classes, nhid=Hd).cuda().eval()
    x = torch.randn(n, args.nfeat, device="cuda")
    with torch.no_grad():
        y = model(x, op).argmax(1)
    atk = Calib_IGA(model)
    atk._begin(x, op)
    z, h, zsum, hsum = atk._cache
    indptr, indices, _ = atk._csr
    b1, W2, b2 = model.gc1.bias.detach(), model.gc2.weight.detach().contiguous(), model.gc2.bias.detach()
    lengths = np.diff(g.indptr)
    rng = np.random.default_rng(0)
    pool = rng.choice(np.flatnonzero(lengths > 0), 32, replace=False)
    # the copy rate: read + write of a 256 MiB buffer
    src = torch.empty(64 << 20, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    copy = device_us(lambda: dst.copy_(src), args.iters, args.rounds)
    copy_rate = 2 * src.numel() * 4 / (copy["us"] * 1e-6)
    results = {}
    HZ = torch.cat([h, z], dim=1).double()
    for B in (1, 8, 32):
        tg = torch.tensor(pool[:B], dtype=torch.int32).cuda()
        logits, state = iga_path_logits(n, indptr, indices, z, h, zsum, hsum, b1, W2, b2, tg, args.steps)
        gl = torch.randn_like(logits)
        ws = iga_scores_workspace(B, Hd, "cuda")
        ids, best, co = iga_scores(n, indptr, indices, z, h, b1, W2, tg, args.steps, gl, state, topk=args.topk,
                                   return_coeffs=True, workspace=ws)
        present = torch.zeros((B, n), dtype=torch.bool, device="cuda")
        for b, t in enumerate(pool[:B]):
            present[b, torch.from_numpy(g.indices[g.indptr[t]:g.indptr[t + 1]].astype(np.int64)).cuda()] = True
        rows = torch.arange(B, device="cuda")

        def composition():
            both = HZ @ co[:, :, :2 * Hd].reshape(2 * B, 2 * Hd).t() + co[:, :, 2 * Hd].reshape(1, 2 * B)     # (n, 2 B)
            both = both.t().reshape(B, 2, n)
            s = torch.where(present, -both[:, 0], both[:, 1]).float()
            s[rows, tg.long()] = -10
            return torch.topk(s, args.topk, dim=1)

        ref = composition()
        same = bool((ref.indices == ids.long()).all())
        r = dict(path_logits=device_us(lambda: iga_path_logits(n, indptr, indices, z, h, zsum, hsum, b1, W2, b2, tg,
                                                               args.steps), args.iters, args.rounds),
                 scores=device_us(lambda: iga_scores(n, indptr, indices, z, h, b1, W2, tg, args.steps, gl, state,
                                                     topk=args.topk, workspace=ws), args.iters, args.rounds),
                 torch_composition=device_us(composition, args.iters, args.rounds), same_topk_as_composition=same)
        model_bytes = 8 * n * Hd
        r["byte_model_fraction_of_copy_rate"] = model_bytes / (r["scores"]["us"] * 1e-6) / copy_rate
        r["composition_over_kernel"] = r["torch_composition"]["us"] / r["scores"]["us"]
        results[f"B={B}"] = r
    # one whole attack (budget topk), host clock
    times = []
    for t in pool[:8]:
        kw = dict(n_perturb=[], best_conf=[])
        atk.attack(x, op, int(t), args.topk, "under", res_gt=y, steps=args.steps, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        atk.attack(x, op, int(t), args.topk, "under", res_gt=y, steps=args.steps, **kw)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    atk.attack_many(x, op, [int(t) for t in pool], args.topk, "under", y, steps=args.steps)
    torch.cuda.synchronize()
    many = time.perf_counter() - t0
    line = json.dumps(dict(tool="iga_probe", graph=args.graph, n=n, nnz=int(g.nnz), nfeat=args.nfeat, nhid=Hd,
                           classes=args.classes, steps=args.steps, topk=args.topk,
                           device=torch.cuda.get_device_name(0), iters=args.iters, rounds=args.rounds,
                           copy_256MiB=copy, copy_rate_GBps=copy_rate / 1e9, byte_model_bytes=8 * n * Hd,
                           kernels=results,
                           attack=dict(us=statistics.median(times) * 1e6, us_range=[min(times) * 1e6, max(times) * 1e6],
                                       targets=8),
                           attack_many_32=dict(us=many * 1e6, us_per_target=many * 1e6 / 32)))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
