"""Generate the fixtures of the evaluation step FROM THE REFERENCE (data only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_evaluation.py <reference checkout>

Imports the reference's own ``utils/ece.py`` (``calculate_ece``) and ``benchmark_calibration_methods.py``
(``evaluate_calibration`` :87-127, ``evaluate_calibration_probs`` :130-158) with stub modules for what they import
but these functions never use: seaborn, ``torch_geometric``, the calibrator packages and the plotting calls.  sklearn
supplies ``calibration_curve`` (what ``ece_chart`` plots, ``utils/ece.py:111-115``).  Written to
``tests/golden/evaluation/``: per case the inputs (outputs, labels, the row mask or index list), the reference's
triple (accuracy, average confidence, ECE), its per-class ECE and sklearn's curves, plus ``manifest.json`` with, per
quantity, ``f32_vs_f64``: the distance of the reference's float32 arithmetic to ``oracle/ece_oracle.py`` (and float64
means / curves) on float64 copies of the same float32 ``p``.  For the ``exp`` cases the reference's float32
arithmetic begins at the model's output ``x``: its ``p`` is torch's float32 ``exp``, which is not correctly rounded,
while the documented ``p`` of ``WG_CALIB_EXP`` is ``(float)exp((double)x)``.  The float64 side of those cases takes
float64 copies of the documented ``p`` (computed here with numpy), so ``f32_vs_f64`` includes what the float32 ``exp``
costs; the manifest records on how many entries the two differ.  Nothing of the reference's source travels.
"""
from __future__ import annotations

import contextlib
import hashlib
import importlib
import io
import json
import os
import sys
import types

os.environ.setdefault("MPLBACKEND", "Agg")
os.environ["MKL_ENABLE_INSTRUCTIONS"] = "AVX2"
os.environ["ATEN_CPU_CAPABILITY"] = "avx2"

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "evaluation")
sys.path.insert(0, REPO)
from oracle import ece_oracle as O  # noqa: E402


class _Stub(types.ModuleType):
    """A module whose every attribute is a placeholder class (``from calibration.TS import TemperatureScaling``)."""
    __path__: list = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def import_reference(ref: str):
    for name in ("seaborn", "torch_geometric", "torch_geometric.datasets", "torch_geometric.transforms", "src",
                 "src.gnn", "src.gnn.model", "calibration", "calibration.TS", "calibration.VS", "calibration.MS",
                 "calibration.SimCalib", "calibration.WATS", "calibration.GATS", "calibration.GETS", "calibration.ETS",
                 "calibration.DCGC", "calibration.CaGCN", "calibration.utils"):
        sys.modules[name] = _Stub(name)
    sys.path.insert(0, ref)
    E = importlib.import_module("utils.ece")
    B = importlib.import_module("benchmark_calibration_methods")
    return E, B


class Fixed(torch.nn.Module):
    """A model that returns a recorded output, whatever it is given."""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x, adj):
        return self.out


def softmax32(z):
    return torch.softmax(torch.from_numpy(z.astype(np.float32)), dim=1).numpy()


def cases():
    """name -> dict(outputs float32 (n, C), labels int64, rows (bool mask or int64 list), kind, n_bins, how)."""
    rng = np.random.default_rng(2407)
    out = {}

    def add(name, outputs, labels, rows, kind, n_bins=10):
        out[name] = dict(outputs=np.ascontiguousarray(outputs, np.float32), labels=np.asarray(labels, np.int64),
                         rows=np.asarray(rows), kind=kind, n_bins=n_bins)

    # probabilities under a mask (evaluate_calibration_probs)
    n, C = 1500, 7
    add("probs_mask_n1500_c7", softmax32(rng.standard_normal((n, C)) * 2.0), rng.integers(0, C, n),
        rng.random(n) < 0.3, "probs")
    # log-probabilities, what every calibrator returns (evaluate_calibration: exp)
    n, C = 2000, 10
    z = rng.standard_normal((n, C)) * 2.5
    add("logprobs_mask_n2000_c10", torch.log_softmax(torch.from_numpy(z.astype(np.float32)), 1).numpy(),
        rng.integers(0, C, n), rng.random(n) < 0.4, "exp")
    # raw logits through the same exp (a base model, MS's raw scores): p exceeds 1
    n, C = 800, 5
    add("rawlogits_mask_n800_c5", rng.standard_normal((n, C)) * 1.5, rng.integers(0, C, n), rng.random(n) < 0.5, "exp")
    # an unsorted index list with repeats
    n, C = 600, 4
    idx = rng.permutation(n)[:250]
    idx[7] = idx[3]
    idx[100] = idx[3]
    add("probs_index_n600_c4", softmax32(rng.standard_normal((n, C)) * 3.0), rng.integers(0, C, n), idx, "probs")
    # a class no row has, and labels outside [0, C)
    n, C = 400, 6
    y = rng.integers(0, C, n)
    y[y == 4] = 2
    y[:5] = -1
    y[5:9] = C
    p = softmax32(rng.standard_normal((n, C)) * 2.0)
    add("absent_class_bad_labels_n400_c6", p, y, np.ones(n, bool), "probs")
    # bins of 3 and of 4 rows (the reference skips below 4), the rest in one far bin
    C = 3
    col = np.array([0.25, 0.26, 0.27] + [0.55, 0.56, 0.57, 0.58] + [0.91] * 9 + [0.05] * 4, np.float32)
    p = np.stack([col, (1 - col) * np.float32(0.75), (1 - col) * np.float32(0.25)], axis=1)
    y = np.array([0, 1, 0, 0, 0, 1, 2] + [0] * 7 + [1, 2] + [0, 1, 2, 2])
    add("bins_of_3_and_4_c3", p, y, np.ones(len(col), bool), "probs")
    # every edge and one float32 ulp either side, each value four times (so its bin counts)
    e32 = np.linspace(0, 1, 11).astype(np.float32)
    vals = np.unique(np.concatenate([e32, np.nextafter(e32, np.float32(2))[:-1], np.nextafter(e32, np.float32(-1))[1:]]))
    col = np.repeat(vals, 4).astype(np.float32)
    p = np.stack([col, (np.float32(1) - col)], axis=1)
    add("edge_neighbours_c2", p, rng.integers(0, 2, len(col)), np.ones(len(col), bool), "probs")
    # exact zeros and ones
    n, C = 60, 4
    p = np.zeros((n, C), np.float32)
    p[np.arange(n), rng.integers(0, C, n)] = 1.0
    p[40:] = softmax32(rng.standard_normal((20, C)))
    add("exact_zero_one_c4", p, rng.integers(0, C, n), rng.random(n) < 0.8, "probs")
    # 15 bins (per-class ECE and curves; the harness's triple uses 10)
    n, C = 900, 5
    add("probs_15bins_n900_c5", softmax32(rng.standard_normal((n, C)) * 2.0), rng.integers(0, C, n),
        rng.random(n) < 0.5, "probs", n_bins=15)
    # few rows: every bin below 4
    add("tiny_n5_c3", softmax32(rng.standard_normal((5, 3))), rng.integers(0, 3, 5), np.ones(5, bool), "probs")
    return out


def flat_curves(curves):
    lens = np.array([len(t) for t, _ in curves], np.int64)
    return (lens, np.concatenate([np.asarray(t, np.float64) for t, _ in curves]),
            np.concatenate([np.asarray(q, np.float64) for _, q in curves]))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    E, B = import_reference(os.path.abspath(sys.argv[1]))
    from sklearn.calibration import calibration_curve
    import sklearn
    os.makedirs(OUT, exist_ok=True)
    manifest = {"source": "reference benchmark_calibration_methods.py:87-158 (evaluate_calibration, "
                          "evaluate_calibration_probs), utils/ece.py:8-62 (calculate_ece), sklearn calibration_curve; "
                          "imported with stub modules for seaborn, torch_geometric and the calibrator packages",
                "numpy": np.__version__, "torch": torch.__version__, "sklearn": sklearn.__version__, "seed": 2407,
                "cases": {}}
    arrays = {}
    for name, c in cases().items():
        outs, y, rows = torch.from_numpy(c["outputs"]), torch.from_numpy(c["labels"]), torch.from_numpy(c["rows"])
        n_bins, C = c["n_bins"], c["outputs"].shape[1]
        with contextlib.redirect_stdout(io.StringIO()) as printed:
            if c["kind"] == "exp":
                acc, conf, ece = B.evaluate_calibration(Fixed(outs), torch.zeros(1), y, torch.zeros(1), rows, name)
                p32 = outs.exp()[rows].numpy()
            else:
                acc, conf, ece = B.evaluate_calibration_probs(outs, y, rows, name)
                p32 = outs[rows].numpy()
        yy = c["labels"][c["rows"]]
        per = np.array([E.calculate_ece(p32, yy, k, logits=False, n_bins=n_bins) for k in range(C)], np.float64)
        if c["kind"] == "exp":
            # the float64 side starts where the documented arithmetic starts: p = (float)exp((double)x), which torch's
            # float32 exp (part of the reference's float32 arithmetic here) misses by an ulp on some elements
            spec = np.exp(c["outputs"].astype(np.float64)).astype(np.float32)[c["rows"]]
            exp_ulp = int(np.sum(spec != p32))
            p64 = spec.astype(np.float64)
        else:
            exp_ulp = 0
            p64 = p32.astype(np.float64)
        per64 = np.array([O.calculate_ece(p64, yy, k, logits=False, n_bins=n_bins) for k in range(C)])
        ece64 = float(np.mean([O.calculate_ece(p64, yy, k, logits=False, n_bins=10) for k in range(C)]))
        acc64 = float(np.mean(np.argmax(p64, axis=1) == yy))
        conf64 = float(np.mean(np.max(p64, axis=1)))
        info = {"kind": c["kind"], "n_bins": n_bins, "n": int(p32.shape[0]), "C": C,
                "rows": "mask" if c["rows"].dtype == bool else "index",
                "printed": printed.getvalue().splitlines(), "float32_exp_differs_on": exp_ulp,
                "f32_vs_f64": {"acc": abs(float(acc) - acc64), "conf": abs(float(conf) - conf64),
                               "ece": abs(float(ece) - ece64), "per_class": float(np.max(np.abs(per - per64)))}}
        arrays.update({f"{name}__outputs": c["outputs"], f"{name}__labels": c["labels"], f"{name}__rows": c["rows"],
                       f"{name}__triple": np.array([float(acc), float(conf), float(ece)], np.float64),
                       f"{name}__per_class": per})
        inside = bool(np.all((p32 >= 0) & (p32 <= 1)))
        info["curves"] = inside
        if inside:
            cur = [calibration_curve((yy == k).astype(int), p32[:, k], n_bins=n_bins) for k in range(C)]
            cur64 = [calibration_curve((yy == k).astype(int), p64[:, k], n_bins=n_bins) for k in range(C)]
            lens, t, q = flat_curves(cur)
            lens64, t64, q64 = flat_curves(cur64)
            assert np.array_equal(lens, lens64)
            info["f32_vs_f64"]["curves"] = float(max(np.max(np.abs(t - t64)), np.max(np.abs(q - q64))))
            arrays.update({f"{name}__curve_lens": lens, f"{name}__curve_true": t, f"{name}__curve_pred": q})
        manifest["cases"][name] = info
        print(f"{name}: acc {float(acc):.4f} conf {float(conf):.4f} ece {float(ece):.6f}  f32_vs_f64 "
              + " ".join(f"{k}={v:.2e}" for k, v in info["f32_vs_f64"].items()))
    path = os.path.join(OUT, "evaluation_cases.npz")
    np.savez_compressed(path, **arrays)
    with open(path, "rb") as f:
        manifest["sha256"] = hashlib.sha256(f.read()).hexdigest()
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print(f"wrote {path} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
