"""WATS training measurement at the ogbn-arxiv size: the R-MAT graph of ``graphgen.named_graph`` (N = 169 343),
``n_val = 29 799`` calibration rows, ``C = 40``, a ``SparseCompatibleGCN`` with ``nhid = 64``, the head
``Linear(F, 16) - ReLU - Linear(16, 1)`` at ``F = 1`` and ``F = 40`` on random features.

Timed, per F, 250 epochs each with the early stopping switched off so that every variant runs the same count:

* ``epoch``: one ``wg_wats_train_epoch`` launch (the head on the calibration rows, loss, gradients, accuracy, Adam,
  early-stopping state), device events around ``iters`` back-to-back launches after a warm-up, the median of
  ``rounds`` rounds;
* ``run250``: a whole ``train_wats_head`` run on frozen logits (250 launches enqueued back to back, the state read
  once), host clock around a call that ends in the host read;
* ``torch_cached250``: the loop of ``WATS.calib_train`` (WATS.py:132-170) in torch ops on cached device logits: the
  head on all n rows, ``log_softmax``, the indexing, ``nll_loss``, backward, ``Adam.step``, the accuracy and the host
  syncs of ``loss.item()`` and ``loss < best_loss``;
* ``torch_cached_fused_head250``: the same loop with ``wats_head`` (``fused_head=True``) for the head's forward and
  backward;
* ``reference_style250``: the torch loop with the frozen base model rerun over the whole graph every epoch in train
  mode, as the reference does (its dropout is live).

Warm-up first, then the median (and range) of ``run_rounds`` runs by the host clock.  Writes one JSON line (also to
``--out``).

    python tools/wats_train_probe.py [--out profiles/r33/s1_wats_train_probe.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "efficient-gnn_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scaling_probe import NEVER, device_us, host_ms  # noqa: E402
from wats_hip import RowNormalizedAdjacency, SparseCompatibleGCN, train_wats_head, wats_head  # noqa: E402
from wats_hip import head as HD  # noqa: E402
from wats_hip.graphgen import named_graph  # noqa: E402


def torch_loop(net0, H, y, val, logits_of, fused_head, epochs=250):
    """WATS.py:132-170 in torch ops, early stopping switched off; a copy of net0 is trained"""
    net = nn.Sequential(nn.Linear(H.shape[1], net0[0].out_features), nn.ReLU(), nn.Linear(net0[0].out_features, 1))
    net = net.to(H.device)
    net.load_state_dict(net0.state_dict())
    opt = torch.optim.Adam(net.parameters(), lr=0.01, weight_decay=5e-4)
    best = float("inf")
    for _ in range(epochs):
        opt.zero_grad()
        z = logits_of()
        if fused_head:
            out = wats_head(H, z, net)
        else:
            t = net(H).squeeze()
            T = torch.log(torch.exp(t) + torch.tensor(1.1, device=H.device))
            out = F.log_softmax(z / T.unsqueeze(1), dim=1)
        loss = F.nll_loss(out[val], y[val])
        loss.backward()
        opt.step()
        with torch.no_grad():
            ((out[val].argmax(1) == y[val]).sum() / val.numel()).item()     # accuracy(), WATS.py:155
            loss.item()                                                     # the printed line, WATS.py:157
        if loss < best:                                                     # the host sync of WATS.py:162
            best = loss
    return net


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="ogbn-arxiv")
    ap.add_argument("--n-val", type=int, default=29799)
    ap.add_argument("--nfeat", type=int, default=128)
    ap.add_argument("--nhid", type=int, default=64)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--widths", type=int, nargs="+", default=[1, 40])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--run-rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wats_train_probe: needs a ROCm GPU (there is no CPU path to time)")
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
    for width in args.widths:
        H = torch.randn(n, width, device="cuda")
        if width == 1:
            H = H.sign()                                     # the reference's one-column feature is +-1
        torch.manual_seed(1)
        net = nn.Sequential(nn.Linear(width, 16), nn.ReLU(), nn.Linear(16, 1)).cuda()
        st = HD._HeadTrainingState(width, 16, C, args.iters * (args.rounds + 2), rows.numel(), NEVER, device,
                                   [net[0].weight, net[0].bias, net[2].weight, net[2].bias], 0.01, 5e-4)
        r = dict(epoch=device_us(lambda: st.epoch(H, logits, rows, y), args.iters, args.rounds))
        assert not st.stopped()
        fused = lambda: train_wats_head(H, logits, y, val, net, patience=NEVER)   # noqa: E731
        r["run250"] = host_ms(fused, args.run_rounds)
        run = fused()
        r["torch_cached250"] = host_ms(lambda: torch_loop(net, H, y, val, lambda: logits, False), args.run_rounds)
        r["torch_cached_fused_head250"] = host_ms(lambda: torch_loop(net, H, y, val, lambda: logits, True),
                                                  args.run_rounds)
        r["reference_style250"] = host_ms(lambda: torch_loop(net, H, y, val, train_mode_logits, False),
                                          args.run_rounds)
        model.eval()
        ref = torch_loop(net, H, y, val, lambda: logits, False)
        r["max_parameter_distance_to_torch_cached"] = max(float((a.reshape(b.shape) - b.detach()).abs().max())
                                                          for a, b in zip(run.params, ref.parameters()))
        r["epochs_run"] = run.epochs_run
        r["final_loss"] = float(run.loss[-1])
        for k in ("torch_cached250", "torch_cached_fused_head250", "reference_style250"):
            r[k.replace("250", "") + "_over_run250"] = r[k]["ms"] / r["run250"]["ms"]
        results[f"F{width}"] = r
    line = json.dumps(dict(tool="wats_train_probe", graph=args.graph, n=n, nnz=int(g.nnz), n_val=int(rows.numel()),
                           classes=C, hid=16, nfeat=args.nfeat, nhid=args.nhid,
                           device=torch.cuda.get_device_name(0), iters=args.iters, rounds=args.rounds,
                           run_rounds=args.run_rounds, widths=results))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
