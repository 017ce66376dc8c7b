"""Generate the fixtures of the four node-wise calibrators FROM THE REFERENCE (``calibration/TS.py``, ``VS.py``,
``MS.py``, ``ETS.py``), on the CPU.

Run only in the build container, where the reference is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_scaling.py

The reference modules are imported through a stub package, as ``tools/gen_golden_gets.py`` does, with the same pinned
CPU code path.  ``TS.py`` imports ``utils.ece`` (which needs seaborn, not installed) for a plotting helper that is
never called here: a stub module with a placeholder of that name is registered.  The base model is the tests'
``CompatibleGCN`` (``tests/models.py``) with dropout ``p = 0``, trained for a few steps so that it is overconfident:
the reference's ``self.train()`` then changes nothing and every run is deterministic.  The reference's own classes
train with the harness's keywords (``benchmark_calibration_methods.py:198-257``).  Outputs are DATA only (arrays,
``allow_pickle=False``): ``tests/golden/scaling/*.npz`` plus ``manifest.json`` (versions, seeds, sha256,
``f32_vs_f64``).

Each case holds the inputs (``x``, ``y``, dense ``adj``, ``val``: a boolean mask or an index tensor), per calibrator
``c`` in ts / vs / ms / ets every array of its ``state_dict()`` under ``p__<c>__<name>``, the float32 loss of every
epoch (``loss_<c>``, read off the tensor that ``backward`` is called on), the stopping epoch (``stop_<c>``, -1: none)
and the epochs run, the eval-mode ``forward`` output (``out_<c>``), ETS's weights (``w_ets``, float64) and
``d sum(loss_weight * out) / d adj`` at the recorded positions through a dense leaf (``grad_<c>``).  ``f32_vs_f64``
in the manifest is, per quantity, the distance of the reference's float32 result to ``tests/scaling_ref.py``'s float64
restatement (trained on float64 logits of the same weights).  Seeds are searched until EVERY early-stopping comparison
of every run (``loss_e`` against ``best_loss``, in the reference's trace and in the restatement's) differs by more
than 100 times the loss's ``f32_vs_f64``, so that rounding cannot move a stopping epoch; this is asserted.
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

os.environ["MKL_ENABLE_INSTRUCTIONS"] = "AVX2"
os.environ["ATEN_CPU_CAPABILITY"] = "avx2"

import numpy as np  # noqa: E402
import scipy  # noqa: E402
import torch  # noqa: E402

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "scaling")
for p in (os.path.join(REPO, "efficient-gnn_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import scaling_ref as R  # noqa: E402
from models import CompatibleGCN  # noqa: E402
from wats_hip.graphgen import rmat_graph  # noqa: E402

NAMES = ("ts", "vs", "ms", "ets")
GAP_FACTOR = 100.0


def import_reference():
    ue = types.ModuleType("utils.ece")
    ue.calculate_average_ece = lambda *a, **k: (_ for _ in ()).throw(NotImplementedError("a placeholder"))
    u = types.ModuleType("utils")
    u.__path__ = []
    u.ece = ue
    sys.modules.update({"utils": u, "utils.ece": ue})
    pkg = types.ModuleType("calibration")
    pkg.__path__ = [os.path.join(REF, "calibration")]
    sys.modules["calibration"] = pkg
    return {n: importlib.import_module("calibration." + n.upper()) for n in NAMES}


@contextlib.contextmanager
def recorded_losses(store):
    """every tensor that ``backward`` is called on is a loss of the training loop: its float32 value, exactly"""
    real = torch.Tensor.backward

    def backward(self, *a, **k):
        store.append(float(self.detach()))
        return real(self, *a, **k)
    torch.Tensor.backward = backward
    try:
        yield
    finally:
        torch.Tensor.backward = real


def dist(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def stop_gaps(losses, patience=10):
    """|loss_e - best_loss| of every comparison TS.py:75 makes (the first, against inf, left out), and the stop"""
    best, left, gaps, stop = np.inf, patience, [], -1
    for e, v in enumerate(losses):
        if np.isfinite(best):
            gaps.append(abs(v - best))
        if v < best:
            best, left = v, patience
        else:
            left -= 1
        if left <= 0:
            stop = e
            break
    return (min(gaps) if gaps else np.inf), stop


def train_reference(cls, base, x, y, adj, val, fit_masks=None):
    losses = []
    with contextlib.redirect_stdout(io.StringIO()), recorded_losses(losses):
        ref = cls(base, x, y, adj, val) if fit_masks else cls(base_model=base, x=x, y=y, adj=adj, val_idx=val)
        if fit_masks:
            ref.fit(fit_masks)
    ref.eval()
    return ref, np.array(losses, dtype=np.float64)


def ref_params(name, ref):
    if name in ("ts", "vs"):
        return [ref.temperature.detach().numpy()]
    if name == "ms":
        return [ref.W.detach().numpy(), ref.b.detach().numpy()]
    return [ref.temp_model.temperature.detach().numpy()] + [np.asarray(float(w.detach()))
                                                           for w in (ref.w1, ref.w2, ref.w3)]


def try_case(mods, seed, n, n_edges, nfeat, ncls, nhid, n_val, index_val, rare_last, target):
    torch.manual_seed(seed)
    adj = torch.tensor(rmat_graph(n, n_edges, seed=seed).to_scipy().toarray(), dtype=torch.float32)
    adj = ((adj + adj.t()) > 0).float()
    adj.fill_diagonal_(1.0)                      # the attack convention: symmetric, self loops
    x = torch.randn(n, nfeat)
    teacher = torch.randn(nfeat, ncls)
    y = (x @ teacher + 1.5 * torch.randn(n, ncls)).argmax(dim=1)
    if rare_last:                                # the last class on a few nodes only (it still sets n_classes)
        y[y == ncls - 1] = torch.randint(0, ncls - 1, (int((y == ncls - 1).sum()),))
        y[torch.randperm(n)[:3]] = ncls - 1
    perm = torch.randperm(n)
    val_ids, train_ids = perm[:n_val], perm[n_val:n_val + n // 3]
    if rare_last:
        val_ids[0] = int(torch.nonzero(y == ncls - 1)[0])
        val_ids = torch.unique(val_ids)[torch.randperm(torch.unique(val_ids).numel())]   # unsorted, no repeats
    val_mask = torch.zeros(n, dtype=torch.bool)
    val_mask[val_ids] = True
    val = val_ids.clone() if index_val else val_mask
    base = CompatibleGCN(nfeat, ncls, nhid=nhid, dropout=0.0)
    opt = torch.optim.Adam(base.parameters(), lr=0.02)
    for _ in range(40):                          # a short fit on the training nodes: overconfident logits
        opt.zero_grad()
        torch.nn.functional.cross_entropy(base(x, adj)[train_ids], y[train_ids]).backward()
        opt.step()
    base.eval()
    P = {k: v.detach().numpy().copy() for k, v in base.state_dict().items()}
    z64 = R.base_logits(P, x.numpy(), adj.numpy())
    idx = val.numpy() if index_val else np.nonzero(val_mask.numpy())[0]
    loss_weight = torch.randn(n, ncls)
    g = torch.Generator().manual_seed(seed + 1)
    rows, cols = torch.nonzero(adj, as_tuple=True)
    ar, ac = torch.nonzero(adj == 0, as_tuple=True)
    pick = torch.randperm(ar.numel(), generator=g)[:rows.numel()]
    ids, tt = torch.arange(n), torch.full((n,), target)
    grows = torch.cat([rows, ar[pick], tt, ids]).to(torch.int32)
    gcols = torch.cat([cols, ac[pick], ids, tt]).to(torch.int32)

    arrays = dict(x=x.numpy(), adj=adj.numpy().astype(np.float32), y=y.numpy(), val=val.numpy(),
                  val_mask=val_mask.numpy(), loss_weight=loss_weight.numpy(), grad_rows=grows.numpy(),
                  grad_cols=gcols.numpy(), target=np.int64(target))
    f32_vs_f64, meta = {}, dict(seed=seed, entries=int(rows.numel()), n_val=int(len(idx)))
    for name in NAMES:
        cls = getattr(mods[name], {"ts": "TemperatureScaling", "vs": "VectorScaling", "ms": "MatrixScaling",
                                   "ets": "ETS"}[name])
        masks = [~val_mask, val, ~val_mask] if name == "ets" else None
        ref, losses = train_reference(cls, base, x, y, adj, val, masks)
        params = ref_params(name, ref)
        with torch.no_grad():
            out = ref(x, adj).numpy()
        a = adj.clone().requires_grad_(True)
        (ref(x, a) * loss_weight).sum().backward()
        grad = a.grad[grows.long(), gcols.long()].numpy()
        # the float64 restatement
        mode = "ts" if name == "ets" else name
        r = R.train(mode, z64, y.numpy(), idx)
        r_params = r["params"]
        if name == "ets":
            p0y, p1y = R.ets_label_probs(z64[idx], y.numpy()[idx], r_params[0])
            r_w = R.ets_fit(p0y, p1y, ncls)
            r_params = [r_params[0]] + [np.asarray(v) for v in r_w]
            w_ref = np.array([float(w.detach()) for w in (ref.w1, ref.w2, ref.w3)])
            f32_vs_f64["w_ets"] = dist(w_ref, r_w)
            arrays["w_ets"] = w_ref
        if len(losses) != r["epochs_run"]:
            return None, f"{name}: the reference ran {len(losses)} epochs, the restatement {r['epochs_run']}"
        f32_vs_f64["loss_" + name] = dist(losses, r["loss"])
        f32_vs_f64["params_" + name] = max(dist(a_, b_) for a_, b_ in zip(params, r_params))
        f32_vs_f64["out_" + name] = dist(out, R.forward(name, z64, r_params))
        f32_vs_f64["grad_" + name] = dist(grad, R.adjacency_gradient(name, P, r_params, x.numpy(), adj.numpy(),
                                                                     loss_weight.numpy(), grows.numpy(),
                                                                     gcols.numpy()))
        gap_ref, stop_ref = stop_gaps(losses)
        gap_r, stop_r = stop_gaps(r["loss"])
        need = GAP_FACTOR * f32_vs_f64["loss_" + name]
        if stop_ref != stop_r or min(gap_ref, gap_r) <= need:
            return None, f"{name}: stop {stop_ref} / {stop_r}, gap {min(gap_ref, gap_r):.3e} vs {need:.3e}"
        assert stop_ref == (r["stop_epoch"] if r["stop_epoch"] is not None else -1)
        if not (np.isfinite(grad).all() and np.isfinite(out).all() and float(np.abs(grad).max()) > 0):
            return None, f"{name}: a non-finite output or gradient (max |z| {np.abs(z64).max():.1f})"
        meta[name] = dict(epochs=int(len(losses)), stop_epoch=int(stop_ref), min_gap=float(min(gap_ref, gap_r)))
        arrays.update({"loss_" + name: losses, "stop_" + name: np.int64(stop_ref),
                       "epochs_" + name: np.int64(len(losses)), "out_" + name: out, "grad_" + name: grad})
        arrays.update({f"p__{name}__{k}": v.detach().numpy() for k, v in ref.state_dict().items()})
    meta["f32_vs_f64"] = f32_vs_f64
    return (arrays, meta), None


def make_case(mods, name, seeds, **kw):
    for seed in seeds:
        got, why = try_case(mods, seed, **kw)
        if got is not None:
            arrays, meta = got
            print(f"{name}: seed {seed}: " + ", ".join(f"{c} {meta[c]['epochs']} epochs (stop {meta[c]['stop_epoch']}, "
                                                       f"gap {meta[c]['min_gap']:.2e})" for c in NAMES))
            print(f"  f32_vs_f64 {meta['f32_vs_f64']}")
            return arrays, meta
        print(f"{name}: seed {seed} rejected: {why}")
    raise AssertionError(f"{name}: no seed of {list(seeds)} keeps every early-stopping comparison {GAP_FACTOR:.0f} x "
                         "f32_vs_f64 apart")


def save(name, manifest, arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 200 * 1024, f"{path}: {size} B"
    with open(path, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    manifest["files"][name + ".npz"] = dict(sha256=digest, keys=sorted(arrays.keys()))
    print(f"wrote {path} ({size} B)")


def main():
    os.makedirs(OUT, exist_ok=True)
    mods = import_reference()
    manifest = dict(generator="tools/gen_golden_scaling.py",
                    reference="calibration/TS.py, VS.py, MS.py, ETS.py (2026-02-06); the base model is tests/models.py",
                    numpy=np.__version__, torch=torch.__version__, scipy=scipy.__version__,
                    cpu_code_path=dict(MKL_ENABLE_INSTRUCTIONS="AVX2", ATEN_CPU_CAPABILITY="avx2"),
                    gap_factor=GAP_FACTOR, cases={}, files={})
    # 1. 5 classes, a boolean mask of 40
    arrays, meta = make_case(mods, "plain120", range(41, 81), n=120, n_edges=600, nfeat=16, ncls=5, nhid=32, n_val=40,
                             index_val=False, rare_last=False, target=5)
    manifest["cases"]["plain120"] = meta
    save("plain120", manifest, arrays)
    # 2. 7 classes, an index val_idx (unsorted), the last class rare
    arrays, meta = make_case(mods, "wide96", range(57, 97), n=96, n_edges=400, nfeat=12, ncls=7, nhid=24, n_val=30,
                             index_val=True, rare_last=True, target=40)
    manifest["cases"]["wide96"] = meta
    save("wide96", manifest, arrays)
    # "measured": the device run's distance of ETS's w to the fixture, per case, as tests/test_scaling.py
    # (test_ets_weights) printed it on the GPU; it cannot be generated here, so a regeneration keeps it
    old = os.path.join(OUT, "manifest.json")
    if os.path.exists(old):
        with open(old) as f:
            manifest["measured"] = json.load(f).get("measured", {})
    with open(old, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("manifest written")


if __name__ == "__main__":
    main()
