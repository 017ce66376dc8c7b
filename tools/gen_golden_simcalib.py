"""Generate the SimCalib fixtures FROM THE REFERENCE (``calibration/SimCalib.py`` on ``src/gnn/model.py``'s
``CompatibleGCN``), on the CPU.

Run only in the build container, where the reference is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_simcalib.py

The reference modules are imported through a stub package, as ``tools/gen_golden.py`` does.  Outputs are DATA only
(arrays, ``allow_pickle=False``): ``tests/golden/simcalib/*.npz`` plus ``tests/golden/simcalib/manifest.json``
(versions, seeds, sha256).  The directory is its own on purpose: ``tests/golden/*.npz`` feeds existing parametrised
tests.

Each case holds the inputs (``x``, dense ``adj``, ``val_mask``, the base model's four parameter arrays), the
reference's ``features_val``, ``val_confidence`` and forward log-probs ``out``, the unclamped temperatures
``raw_t`` (the reference's own similarity matrix, then SimCalib.py:98-105), and the dense gradient
``d sum(loss_weight * out) / d adj`` at the recorded positions ``(grad_rows, grad_cols)``: every present edge, as
many absent ones, and the whole row and column of ``target``.
"""
from __future__ import annotations

import hashlib
import importlib
import importlib.util
import json
import os
import sys
import types

# The float32 results of torch's CPU kernels depend on the instruction set MKL and ATen dispatch to (measured: the
# AVX-512 and the AVX2 paths differ in the last bit of a matrix product, which softmax(. / 0.1) amplifies to about
# 4 * 2^-24 of the temperatures).  The fixtures are generated on the AVX2 paths, which every x86-64 machine this
# project runs on can take, and tests/test_simcalib_host.py runs the float32 restatement under the same two settings
# (simcalib_ref.PINNED_CPU_PATH), in a process of its own: they are read when torch starts.
os.environ["MKL_ENABLE_INSTRUCTIONS"] = "AVX2"
os.environ["ATEN_CPU_CAPABILITY"] = "avx2"

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "simcalib")
sys.path.insert(0, os.path.join(REPO, "efficient-gnn_amd"))

from wats_hip.graphgen import rmat_graph  # noqa: E402


def import_reference():
    pkg = types.ModuleType("calibration")
    pkg.__path__ = [os.path.join(REF, "calibration")]
    sys.modules["calibration"] = pkg
    S = importlib.import_module("calibration.SimCalib")
    spec = importlib.util.spec_from_file_location("ref_gnn_model", os.path.join(REF, "src", "gnn", "model.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    return S, M


def make_case(S, M, seed, n, n_edges, nfeat, ncls, nhid, weight_scale, n_val, isolated, target):
    torch.manual_seed(seed)
    adj = torch.tensor(rmat_graph(n, n_edges, seed=seed).to_scipy().toarray(), dtype=torch.float32)
    adj = ((adj + adj.t()) > 0).float()
    adj.fill_diagonal_(1.0)                      # the attack convention: symmetric, self loops
    for i in isolated:                           # no entry at all in its row and column
        adj[i, :] = 0
        adj[:, i] = 0
    x = torch.randn(n, nfeat)
    y = torch.randint(0, ncls, (n,))
    val_mask = torch.zeros(n, dtype=torch.bool)
    val_mask[torch.randperm(n)[:n_val]] = True
    base = M.CompatibleGCN(nfeat=nfeat, nclass=ncls, nhid=nhid, dropout=0.5)
    with torch.no_grad():
        base.gc2.weight.mul_(weight_scale)
        base.gc2.bias.mul_(weight_scale)
    base.eval()
    for p in base.parameters():
        p.requires_grad = False
    ref = S.SimCalib(base, x, y, adj, val_mask)
    with torch.no_grad():
        out = ref(x, adj)
        sim = ref.compute_similarity_matrix(ref.latent_feature_1(x, adj), ref.features_val)
        w = F.softmax(sim / 0.1, dim=1)                                            # SimCalib.py:95-98
        raw_t = torch.mm(w, (1.0 / (ref.val_confidence + ref.epsilon)).unsqueeze(1)).squeeze(1)   # :102-105
    loss_weight = torch.randn(n, ncls)
    a = adj.clone().requires_grad_(True)
    (ref(x, a) * loss_weight).sum().backward()
    g = torch.Generator().manual_seed(seed + 1)
    pr, pc = torch.nonzero(adj, as_tuple=True)
    ar, ac = torch.nonzero(adj == 0, as_tuple=True)
    pick = torch.randperm(ar.numel(), generator=g)[:pr.numel()]
    ids = torch.arange(n)
    tt = torch.full((n,), target)
    rows = torch.cat([pr, ar[pick], tt, ids]).to(torch.int32)
    cols = torch.cat([pc, ac[pick], ids, tt]).to(torch.int32)
    arrays = dict(x=x.numpy(), adj=adj.numpy().astype(np.float32), val_mask=val_mask.numpy(), y=y.numpy(),
                  gc1_weight=base.gc1.weight.numpy(), gc1_bias=base.gc1.bias.numpy(),
                  gc2_weight=base.gc2.weight.numpy(), gc2_bias=base.gc2.bias.numpy(),
                  features_val=ref.features_val.numpy(), val_confidence=ref.val_confidence.numpy(),
                  out=out.numpy(), raw_t=raw_t.numpy(), loss_weight=loss_weight.numpy(),
                  grad_rows=rows.numpy(), grad_cols=cols.numpy(), grad=a.grad[rows.long(), cols.long()].numpy(),
                  target=np.int64(target), isolated=np.asarray(isolated, np.int64), epsilon=np.float64(ref.epsilon))
    return arrays, raw_t


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
    S, M = import_reference()
    manifest = dict(generator="tools/gen_golden_simcalib.py",
                    reference="calibration/SimCalib.py + src/gnn/model.py (2026-02-06)",
                    numpy=np.__version__, torch=torch.__version__,
                    cpu_code_path=dict(MKL_ENABLE_INSTRUCTIONS="AVX2", ATEN_CPU_CAPABILITY="avx2"), cases={}, files={})

    # 1. the plain case: 5 classes, 37 validation nodes, one isolated node; no temperature reaches the clamp
    arrays, raw = make_case(S, M, seed=21, n=120, n_edges=600, nfeat=16, ncls=5, nhid=32, weight_scale=1.0,
                            n_val=37, isolated=[17], target=5)
    n_val = int(arrays["val_mask"].sum())
    print(f"plain: {n_val} validation nodes, raw t in [{float(raw.min()):.4f}, {float(raw.max()):.4f}]")
    manifest["cases"]["plain120"] = dict(seed=21, n_val=n_val, clamped=int((raw > 5.0).sum()), unclamped=int((raw <= 5.0).sum()))
    save("plain120", manifest, arrays)

    # 2. 8 classes and a low-confidence base model (the default initialisation's output layer doubled: validation
    #    confidences 0.14 to 0.39, so 1 / confidence straddles 5): rows on both sides of the clamp, none within 0.1 of it
    arrays, raw = make_case(S, M, seed=33, n=96, n_edges=400, nfeat=12, ncls=8, nhid=24, weight_scale=2.0,
                            n_val=24, isolated=[], target=40)
    assert float((raw - 5.0).abs().min()) > 0.1
    clamped, unclamped = int((raw > 5.0).sum()), int((raw <= 5.0).sum())
    print(f"clamp: raw t in [{float(raw.min()):.4f}, {float(raw.max()):.4f}], {clamped} clamped, "
          f"{unclamped} unclamped")
    assert clamped > 0 and unclamped > 0, "case two needs rows on both sides of the clamp"
    manifest["cases"]["clamp96"] = dict(seed=33, n_val=int(arrays["val_mask"].sum()), clamped=clamped, unclamped=unclamped)
    save("clamp96", manifest, arrays)

    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("manifest written")


if __name__ == "__main__":
    main()
