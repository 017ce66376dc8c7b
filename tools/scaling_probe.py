"""Node-wise calibrator measurement at the ogbn-arxiv size: the R-MAT graph of ``graphgen.named_graph`` (N = 169 343),
``n_val = 29 799`` calibration rows, ``C = 40``, a ``SparseCompatibleGCN`` with ``nhid = 64``.

Timed, for TS, VS and MS:

* ``epoch``: one ``wg_scale_epoch`` launch (forward, loss, gradients, accuracy, Adam, early-stopping state), device
  events around ``iters`` back-to-back launches after a warm-up, the median of ``rounds`` rounds;
* ``run250``: a whole 250-epoch ``train_scaling`` run on frozen logits (250 launches enqueued back to back, the state
  read once), host clock around a call that ends in the host read.  Patience is set above 250 so that all 250
  epochs run, as in the two torch loops below;
* ``torch_cached250``: the reference's loop (TS.py:55-83) in torch ops on cached device logits: indexing, the map,
  ``nll_loss``, backward, ``Adam.step`` and the host sync of ``loss < best_loss``, 250 epochs;
* ``reference_style250``: the same loop with the frozen base model rerun over the whole graph every epoch in train
  mode, as the reference does (its dropout is live).

And ``ETS.fit``: ``wg_ets_label_probs`` plus SLSQP on two float64 vectors, against the reference's formulation
(ETS.py:39-76: the validation logits on the host, two full softmaxes per objective call), both by the host clock,
the median of ``fit_rounds``.  Writes one JSON line (also to ``--out``).

    python tools/scaling_probe.py [--out profiles/r21/s1_scaling_probe.json]
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
import scipy.optimize  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from wats_hip import RowNormalizedAdjacency, SparseCompatibleGCN  # noqa: E402
from wats_hip import scaling as S  # noqa: E402
from wats_hip.graphgen import named_graph  # noqa: E402

NEVER = 10 ** 6     # a patience that never runs out


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


def host_ms(fn, rounds):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=statistics.median(out), ms_range=[min(out), max(out)])


def torch_loop(mode, C, y, val, logits_of, epochs=250):
    """TS.py:55-83 / VS.py:61-89 / MS.py:60-89 in torch ops, early stopping switched off"""
    dev = y.device
    if mode == "ms":
        params = [torch.ones(C, C, device=dev, requires_grad=True), torch.ones(C, device=dev, requires_grad=True)]
        eye = torch.eye(C, device=dev)
    else:
        params = [torch.ones(1 if mode == "ts" else C, device=dev, requires_grad=True)]
    opt = torch.optim.Adam(params, lr=0.01, weight_decay=5e-4)
    best = float("inf")
    for _ in range(epochs):
        opt.zero_grad()
        z = logits_of()
        if mode == "ms":
            out = (z - z[:, -1:]) @ params[0] + params[1]
            loss = F.nll_loss(out[val], y[val]) + torch.sum(torch.abs(params[0] - eye))
        else:
            out = F.log_softmax(z * torch.log(torch.exp(params[0]) + 1.1), dim=1)
            loss = F.nll_loss(out[val], y[val])
        loss.backward()
        opt.step()
        with torch.no_grad():
            (out[val].argmax(1) == y[val]).sum() / val.numel()        # the accuracy of TS.py:68
        if loss < best:                                               # the host sync of TS.py:75
            best = loss
    return params


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--n-val", type=int, default=29799)
    ap.add_argument("--nfeat", type=int, default=128)
    ap.add_argument("--nhid", type=int, default=64)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--run-rounds", type=int, default=3)
    ap.add_argument("--fit-rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scaling_probe: needs a ROCm GPU (there is no CPU path to time)")
    g = named_graph(args.graph)
    op = RowNormalizedAdjacency.from_graph(g)
    n, C = g.n, args.classes
    torch.manual_seed(0)
    model = SparseCompatibleGCN(args.nfeat, nclass=C, nhid=args.nhid).cuda()
    for p in model.parameters():
        p.requires_grad = False
    x = torch.randn(n, args.nfeat, device="cuda")
    model.eval()
    with torch.no_grad():
        logits = (model(x, op) * 4).contiguous()             # overconfident, as a trained model's
        y = torch.where(torch.rand(n, device="cuda") < 0.6, logits.argmax(1), torch.randint(0, C, (n,), device="cuda"))
    val = torch.randperm(n, device="cuda")[:args.n_val].sort().values
    rows = val.to(torch.int32).contiguous()
    device = torch.device("cuda", torch.cuda.current_device())

    def train_mode_logits():
        model.train()
        with torch.no_grad():
            return model(x, op) * 4

    results = {}
    for mode in ("ts", "vs", "ms"):
        st = S._TrainingState(S._mode(mode), C, args.iters * (args.rounds + 2), rows.numel(), NEVER, False, device)
        r = dict(epoch=device_us(lambda: st.epoch(logits, rows, y), args.iters, args.rounds))
        assert not st.stopped()
        r["run250"] = host_ms(lambda: S.train_scaling(mode, logits, y, val, patience=NEVER), args.run_rounds)
        run = S.train_scaling(mode, logits, y, val, patience=NEVER)
        r["torch_cached250"] = host_ms(lambda: torch_loop(mode, C, y, val, lambda: logits), args.run_rounds)
        r["reference_style250"] = host_ms(lambda: torch_loop(mode, C, y, val, train_mode_logits), args.run_rounds)
        ref = torch_loop(mode, C, y, val, lambda: logits)
        r["max_parameter_distance_to_torch_cached"] = max(float((a - b.detach()).abs().max())
                                                          for a, b in zip(run.params, ref))
        r["epochs_run"] = run.epochs_run
        r["torch_cached_over_run250"] = r["torch_cached250"]["ms"] / r["run250"]["ms"]
        r["reference_style_over_run250"] = r["reference_style250"]["ms"] / r["run250"]["ms"]
        results[mode] = r
    model.eval()
    # ETS.fit: the label columns from the device, against the reference's host formulation
    tau = S.train_scaling("ts", logits, y, val).params[0]

    def fit_here():
        p0, p1 = S.ets_label_probs(logits, y, tau, rows=val)
        return S.ensemble_weights(p0.cpu().numpy(), p1.cpu().numpy(), C)

    def fit_reference_style():
        lg = logits[val]
        one_hot = torch.zeros_like(lg)
        one_hot.scatter_(1, y[val].unsqueeze(-1), 1)
        logit, label, t = lg.cpu().numpy(), one_hot.cpu().numpy(), tau.cpu().numpy()
        p1 = np.exp(logit) / np.sum(np.exp(logit), 1)[:, None]
        logit = logit / t
        p0 = np.exp(logit) / np.sum(np.exp(logit), 1)[:, None]
        p2 = np.ones_like(p0) / C

        def ll_w(w):
            return -np.sum(label * np.log(w[0] * p0 + w[1] * p1 + w[2] * p2)) / p0.shape[0]
        return scipy.optimize.minimize(ll_w, (1.0, 0.0, 0.0), method="SLSQP",
                                       constraints={"type": "eq", "fun": lambda v: np.sum(v) - 1},
                                       bounds=((0.0, 1.0),) * 3, tol=1e-12, options={"disp": False}).x

    with np.errstate(all="ignore"):
        w_here, w_ref = fit_here(), fit_reference_style()
        ets = dict(fit=host_ms(fit_here, args.fit_rounds), reference_style=host_ms(fit_reference_style, args.fit_rounds),
                   w=w_here.tolist(), w_reference_style=w_ref.tolist(), tau=float(tau))
    ets["reference_style_over_fit"] = ets["reference_style"]["ms"] / ets["fit"]["ms"]
    line = json.dumps(dict(tool="scaling_probe", graph=args.graph, n=n, nnz=int(g.nnz), n_val=int(rows.numel()),
                           classes=C, nfeat=args.nfeat, nhid=args.nhid, device=torch.cuda.get_device_name(0),
                           iters=args.iters, rounds=args.rounds, run_rounds=args.run_rounds, modes=results, ets=ets))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
