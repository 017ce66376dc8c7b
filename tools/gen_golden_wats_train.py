"""Generate the fixtures of WATS's training FROM THE REFERENCE (``calibration/WATS.py``), on the CPU.

Run only in the build container, where the reference is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_wats_train.py

The reference module is imported through a stub package, as ``tools/gen_golden_scaling.py`` does, with the same pinned
CPU code path.  The base model is the tests' ``CompatibleGCN`` (``tests/models.py``) with dropout ``p = 0``, fitted for
a few steps so that it is overconfident: the reference's ``self.train()`` then changes nothing and every run is
deterministic.  Outputs are DATA only (arrays, ``allow_pickle=False``): ``tests/golden/wats_train/*.npz`` plus
``manifest.json`` (versions, seeds, sha256, ``f32_vs_f64``).

Each case holds the inputs (``x``, ``y``, dense ``adj``, ``val``: a boolean mask or an unsorted index tensor, the base
model's arrays ``base__*``), the head's initial parameters as they are when the reference creates its optimizer
(``init__net.*``), the float32 loss of every epoch (``loss``, read off the tensor that ``backward`` is called on), the
stopping epoch (``stop``, -1: none) and the epochs run, the trained ``p__net.*``, ``wavelet_feats`` and the eval-mode
``forward`` output (``out``).  ``f32_vs_f64`` in the manifest is, per quantity, the distance of the reference's float32
result to ``tests/wats_train_ref.py``'s float64 restatement (trained on float64 logits of the same weights, from the
same initial parameters and the recorded features).

Seed condition, asserted: the reference and the restatement run the same number of epochs with the same stop, and every
``loss_e`` / ``best_loss`` comparison of both traces differs by more than GAP_FACTOR = 10 times ``f32_vs_f64["loss"]``.
A moved loss changes a comparison only when the gap is below twice that distance, so 10 leaves a factor of five; the
scaling fixtures' 100 is out of reach here because WATS stops exactly where its loss plateaus (scratch runs over both
recipes: loss distances 3e-7 .. 9e-7, the closest comparison of most early-stopped runs below 20 times that, none at
100).  ``stop120`` must stop early; ``full96`` must run all 250 epochs and takes an unsorted index ``val_mask``.
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
OUT = os.path.join(REPO, "tests", "golden", "wats_train")
for p in (os.path.join(REPO, "efficient-gnn_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import scaling_ref as SR  # noqa: E402
import wats_train_ref as R  # noqa: E402
from models import CompatibleGCN  # noqa: E402
from wats_hip.graphgen import rmat_graph  # noqa: E402

GAP_FACTOR = 10.0


def import_reference():
    pkg = types.ModuleType("calibration")
    pkg.__path__ = [os.path.join(REF, "calibration")]
    sys.modules["calibration"] = pkg
    return importlib.import_module("calibration.WATS")


@contextlib.contextmanager
def recorded(losses, inits):
    """every tensor that ``backward`` is called on is a loss of the training loop: its float32 value, exactly; the
    parameters handed to ``torch.optim.Adam`` are the head's initial ones"""
    real_backward, real_adam = torch.Tensor.backward, torch.optim.Adam

    def backward(self, *a, **k):
        losses.append(float(self.detach()))
        return real_backward(self, *a, **k)

    def adam(params, *a, **k):
        params = list(params)
        inits.append([p.detach().numpy().copy() for p in params])
        return real_adam(params, *a, **k)
    torch.Tensor.backward, torch.optim.Adam = backward, adam
    try:
        yield
    finally:
        torch.Tensor.backward, torch.optim.Adam = real_backward, real_adam


def try_case(mod, seed, n, n_edges, nfeat, ncls, nhid, n_val, index_val, want_stop):
    torch.manual_seed(seed)
    adj = torch.tensor(rmat_graph(n, n_edges, seed=seed).to_scipy().toarray(), dtype=torch.float32)
    adj = ((adj + adj.t()) > 0).float()
    adj.fill_diagonal_(1.0)                      # the attack convention: symmetric, self loops
    x = torch.randn(n, nfeat)
    teacher = torch.randn(nfeat, ncls)
    y = (x @ teacher + 1.5 * torch.randn(n, ncls)).argmax(dim=1)
    perm = torch.randperm(n)
    val_ids, train_ids = perm[:n_val], perm[n_val:n_val + n // 3]
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
    z64 = SR.base_logits(P, x.numpy(), adj.numpy())
    idx = val.numpy() if index_val else np.nonzero(val_mask.numpy())[0]

    losses, inits = [], []
    with contextlib.redirect_stdout(io.StringIO()), recorded(losses, inits):
        ref = mod.WATS(base, x, y, adj, val)
    ref.eval()
    losses = np.array(losses, dtype=np.float64)
    assert len(inits) == 1 and len(inits[0]) == 4
    feats = ref.wavelet_feats.detach().numpy()
    with torch.no_grad():
        out = ref(x, adj).numpy()
    state = {k: v.detach().numpy() for k, v in ref.state_dict().items() if k.startswith("net.")}
    assert tuple(state) == R.NET_KEYS, tuple(state)

    r = R.train(feats, z64, y.numpy(), idx, inits[0])
    if len(losses) != r["epochs_run"]:
        return None, f"the reference ran {len(losses)} epochs, the restatement {r['epochs_run']}"
    f = dict(loss=R.dist(losses, r["loss"]),
             params=max(R.dist(a, b) for a, b in zip(R.as_params([state[k] for k in R.NET_KEYS]), r["params"])),
             out=R.dist(out, R.forward(feats, z64, r["params"])))
    gap_ref, stop_ref = R.stop_gaps(losses)
    gap_r, stop_r = R.stop_gaps(r["loss"])
    need = GAP_FACTOR * f["loss"]
    if stop_ref != stop_r or min(gap_ref, gap_r) <= need:
        return None, f"stop {stop_ref} / {stop_r}, gap {min(gap_ref, gap_r):.3e} vs {need:.3e}"
    assert stop_ref == (r["stop_epoch"] if r["stop_epoch"] is not None else -1)
    if want_stop != (stop_ref >= 0):
        return None, f"stop {stop_ref} after {len(losses)} epochs, wanted {'a stop' if want_stop else 'all 250 epochs'}"
    if not want_stop:
        assert len(losses) == 250
    if not np.isfinite(out).all():
        return None, "a non-finite output"
    arrays = dict(x=x.numpy(), adj=adj.numpy().astype(np.float32), y=y.numpy(), val=val.numpy(),
                  val_mask=val_mask.numpy(), loss=losses, stop=np.int64(stop_ref), epochs=np.int64(len(losses)),
                  wavelet_feats=feats, out=out)
    arrays.update({"base__" + k: v for k, v in P.items()})
    arrays.update({"init__" + k: v for k, v in zip(R.NET_KEYS, inits[0])})
    arrays.update({"p__" + k: v for k, v in state.items()})
    meta = dict(seed=seed, n_val=int(len(idx)), epochs=int(len(losses)), stop_epoch=int(stop_ref),
                min_gap=float(min(gap_ref, gap_r)), f32_vs_f64=f,
                feats_constant=bool(np.all(feats == feats[0])))
    return (arrays, meta), None


def make_case(mod, name, seeds, **kw):
    for seed in seeds:
        got, why = try_case(mod, seed, **kw)
        if got is not None:
            arrays, meta = got
            print(f"{name}: seed {seed}: {meta['epochs']} epochs (stop {meta['stop_epoch']}, gap {meta['min_gap']:.2e})")
            print(f"  f32_vs_f64 {meta['f32_vs_f64']}")
            return arrays, meta
        print(f"{name}: seed {seed} rejected: {why}")
    raise AssertionError(f"{name}: no seed of {list(seeds)} meets the conditions")


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
    mod = import_reference()
    manifest = dict(generator="tools/gen_golden_wats_train.py",
                    reference="calibration/WATS.py (2026-02-06); the base model is tests/models.py",
                    numpy=np.__version__, torch=torch.__version__, scipy=scipy.__version__,
                    cpu_code_path=dict(MKL_ENABLE_INSTRUCTIONS="AVX2", ATEN_CPU_CAPABILITY="avx2"),
                    gap_factor=GAP_FACTOR, cases={}, files={})
    # 1. 5 classes, a boolean mask of 40: early stopping fires
    arrays, meta = make_case(mod, "stop120", range(41, 90), n=120, n_edges=600, nfeat=16, ncls=5, nhid=32, n_val=40,
                             index_val=False, want_stop=True)
    manifest["cases"]["stop120"] = meta
    save("stop120", manifest, arrays)
    # 2. 7 classes, an unsorted index val_mask: all 250 epochs
    arrays, meta = make_case(mod, "full96", range(57, 130), n=96, n_edges=400, nfeat=12, ncls=7, nhid=24, n_val=30,
                             index_val=True, want_stop=False)
    manifest["cases"]["full96"] = meta
    save("full96", manifest, arrays)
    # "measured": the device run's distance of the eval-mode output to the fixture, per case, as
    # tests/test_wats_train.py printed it on the GPU; it cannot be generated here, so a regeneration keeps it
    old = os.path.join(OUT, "manifest.json")
    if os.path.exists(old):
        with open(old) as f:
            manifest["measured"] = json.load(f).get("measured", {})
    with open(old, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("manifest written")


if __name__ == "__main__":
    main()
