"""Evaluation-step measurement at the ogbn-arxiv size: ``n`` = 169 343 rows, ``C`` = 40, a test mask of about 30 % of
the rows, ``G`` = 1 and 2 sets of probabilities.

Timed per ``G``:

* ``kernels``: ``wg_calib_bins`` + ``wg_calib_ece`` on prepared buffers (the row list already an index tensor), device
  events around ``iters`` back-to-back calls after a warm-up, the median of ``rounds`` rounds;
* ``report``: one ``calibration_report`` call with an index tensor, and ``report_mask`` with the boolean mask (the
  mask costs a second host read, of its count), by the host clock: allocation, both launches and the host read;
* ``torch``: ``metrics.calculate_average_ece`` on the same device tensors (``probs[mask]``, ``labels[mask]``), once per
  set, host clock (it ends in a host read), and its device time by events;
* ``host``: the reference's path, ``probs[mask].cpu().numpy()`` then ``oracle/ece_oracle.py``, host clock.

The byte model is one read of the listed rows (``G * n_rows * C * 4`` bytes) plus their labels and ids.  Writes one
JSON line (also to ``--out``).

    python tools/calib_eval_probe.py [--out profiles/r24/s1_calib_eval_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "efficient-gnn_amd"))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import ece_oracle as O  # noqa: E402
from wats_hip import metrics as M  # noqa: E402


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


def host_us(fn, rounds):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return dict(us=statistics.median(out), us_range=[min(out), max(out)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=169343)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--share", type=float, default=0.3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    n, C = a.n, a.classes
    labels = torch.from_numpy(rng.integers(0, C, n)).to(dev)
    mask = torch.from_numpy(rng.random(n) < a.share).to(dev)
    idx = torch.nonzero(mask).flatten()
    n_rows = int(idx.numel())
    probs = [torch.softmax(torch.from_numpy((rng.standard_normal((n, C)) * s).astype(np.float32)).to(dev), dim=1)
             for s in (2.0, 3.0)]
    res = dict(probe="calib_eval", device=torch.cuda.get_device_name(0), n=n, C=C, n_rows=n_rows, iters=a.iters,
               rounds=a.rounds, sets={})
    for G in (1, 2):
        out = torch.stack(probs[:G]).contiguous()
        bytes_model = G * n_rows * C * 4 + n_rows * 16
        k = device_us(lambda: M._calib_launch(out, labels, idx, 0, 10, 4), a.iters, a.rounds)
        k["GBps_of_byte_model"] = bytes_model / (k["us"] * 1e-6) / 1e9
        r = dict(bytes_model=bytes_model, kernels=k,
                 report=host_us(lambda: M.calibration_report(out, labels, rows=idx), a.rounds),
                 report_mask=host_us(lambda: M.calibration_report(out, labels, rows=mask), a.rounds),
                 torch=host_us(lambda: [M.calculate_average_ece(p[mask], labels[mask], C, logits=False)
                                        for p in probs[:G]], a.rounds),
                 torch_device=device_us(lambda: [M._ece_all(p[mask], labels[mask], False, 10, list(range(C)))
                                                 for p in probs[:G]], 5, a.rounds),
                 host=host_us(lambda: [O.calculate_average_ece(p[mask].cpu().numpy(), labels[mask].cpu().numpy(), C,
                                                               logits=False) for p in probs[:G]], 3))
        new = [x.ece for x in M.calibration_report(out, labels, rows=idx)]
        old = [M.calculate_average_ece(p[mask], labels[mask], C, logits=False) for p in probs[:G]]
        r["max_abs_difference_to_torch"] = max(abs(x - y) for x, y in zip(new, old))
        res["sets"][str(G)] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
