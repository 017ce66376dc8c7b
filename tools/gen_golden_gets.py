"""Generate the GETS fixtures FROM THE REFERENCE (``calibration/GETS.py`` on ``src/gnn/model.py``'s
``CompatibleGCN``), on the CPU.

Run only in the build container, where the reference is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_gets.py

The reference modules are imported through a stub package, as ``tools/gen_golden_dcgc.py`` does, with the same pinned
CPU code path.  ``torch_geometric`` is not installed: a stub is registered whose ``GCNConv`` is the few-line dense
restatement of ``gcn_norm`` + ``propagate`` below (PyG's parameter names ``lin.weight`` / ``bias``), whose ``degree``
is a ``bincount``, and whose ``GATConv`` / ``GINConv`` are placeholders.  The reference's own ``GETSCalibrator``
(gating, mixture, loss, training loop) then trains with the harness's keywords
(``exp/ablation/ugca_full_multi_dataset.py:543-558``).  Outputs are DATA only (arrays, ``allow_pickle=False``):
``tests/golden/gets/*.npz`` plus ``tests/golden/gets/manifest.json`` (versions, seeds, sha256, ``f32_vs_f64``).

Each case holds the inputs (``x``, ``y``, dense ``adj``, ``val_mask``), every array of the trained calibrator's
``state_dict()`` under ``p__<name>`` (the base model's and the degree embeddings, which no optimiser step touched,
among them), the eval-mode ``forward`` output (``out``) with its dense gates, selection and clean gating logits, the
gradient ``d sum(loss_weight * out) / d adj`` at the recorded positions through a dense leaf, and one train-mode
forward with ``dropout_rate = 0`` (the base model in eval mode) whose ``randn_like`` sample is stored (``noise``) with
its output, gates, selection and ``aux_loss``.  ``f32_vs_f64`` in the manifest is, per quantity, the largest distance
of the reference's float32 result to ``tests/gets_ref.py``'s float64 restatement on the same arrays; every row's gap
between its k-th and (k+1)-th gating logit exceeds 100 times that of the gating logits, so that no rounding can change
a selection.
"""
from __future__ import annotations

import contextlib
import hashlib
import importlib
import importlib.util
import io
import json
import os
import sys
import types

# the same pinned CPU code paths as the DCGC fixtures; read when torch starts
os.environ["MKL_ENABLE_INSTRUCTIONS"] = "AVX2"
os.environ["ATEN_CPU_CAPABILITY"] = "avx2"

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "gets")
for p in (os.path.join(REPO, "efficient-gnn_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import gets_ref as R  # noqa: E402
from wats_hip.graphgen import rmat_graph  # noqa: E402

HARNESS = dict(num_experts=3, expert_select=2, hidden_dim=32, dropout_rate=0.1, num_layers=2, feature_hidden_dim=16,
               degree_hidden_dim=8, noisy_gating=True, loss_coef=1e-2, backbone="gcn")
CONF = {"lr": 0.01, "max_epoch": 100, "patience": 10, "weight_decay": 5e-4}


class GCNConv(nn.Module):
    """PyG's GCNConv with its defaults, dense: M[target, source] = 1 for every edge that is no loop, one loop per
    node, deg = the row sums, out = D^-1/2 M D^-1/2 (x W^T) + b."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        nn.init.xavier_uniform_(self.lin.weight)

    def forward(self, x, edge_index):
        n = x.size(0)
        m = torch.zeros(n, n, dtype=x.dtype)
        m[edge_index[1], edge_index[0]] = 1.0
        m.fill_diagonal_(1.0)
        dinv = m.sum(1).pow(-0.5)
        return (dinv.unsqueeze(1) * m * dinv.unsqueeze(0)) @ self.lin(x) + self.bias


class _Placeholder(nn.Module):
    def __init__(self, *a, **k):
        raise NotImplementedError("a placeholder: only the 'gcn' backbone is generated")


def degree(index, num_nodes):
    return torch.bincount(index, minlength=num_nodes).to(torch.float32)


def import_reference():
    tg, tgn, tgu = (types.ModuleType(m) for m in ("torch_geometric", "torch_geometric.nn", "torch_geometric.utils"))
    tgn.GCNConv, tgn.GATConv, tgn.GINConv = GCNConv, _Placeholder, _Placeholder
    tgu.degree = degree
    tg.nn, tg.utils = tgn, tgu
    sys.modules.update({"torch_geometric": tg, "torch_geometric.nn": tgn, "torch_geometric.utils": tgu})
    pkg = types.ModuleType("calibration")
    pkg.__path__ = [os.path.join(REF, "calibration")]
    sys.modules["calibration"] = pkg
    Gm = importlib.import_module("calibration.GETS")
    spec = importlib.util.spec_from_file_location("ref_gnn_model", os.path.join(REF, "src", "gnn", "model.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    return Gm, M


@contextlib.contextmanager
def recorded_randn_like(store):
    real = torch.randn_like

    def randn_like(t, *a, **k):
        v = real(t, *a, **k)
        store.append(v.clone())
        return v
    torch.randn_like = randn_like
    try:
        yield
    finally:
        torch.randn_like = real


def dist(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def make_case(Gm, M, seed, n, n_edges, nfeat, ncls, nhid, n_val, isolated, target):
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
    base.eval()
    ref = Gm.GETSCalibrator(base_model=base, num_classes=ncls, device=torch.device("cpu"), conf=CONF, **HARNESS)
    with contextlib.redirect_stdout(io.StringIO()) as log:     # one line per epoch
        ref.fit(adj, x, y, [None, val_mask, None])
    epochs = sum(1 for line in log.getvalue().splitlines() if line.startswith("epoch:"))
    E, k = HARNESS["num_experts"], HARNESS["expert_select"]
    # eval mode
    ref.eval()
    with torch.no_grad():
        out = ref(x, adj)
        gi = torch.cat([ref.proj_feature(x), base(x, adj)], dim=1)
        clean = gi @ ref.w_gate
        gates, _ = ref.noisy_top_k_gating(gi, False)
    sel = clean.topk(k, dim=1).indices
    loss_weight = torch.randn(n, ncls)
    a = adj.clone().requires_grad_(True)
    (ref(x, a) * loss_weight).sum().backward()
    g = torch.Generator().manual_seed(seed + 1)
    rows, cols = torch.nonzero(adj, as_tuple=True)
    ar, ac = torch.nonzero(adj == 0, as_tuple=True)
    pick = torch.randperm(ar.numel(), generator=g)[:rows.numel()]
    ids, tt = torch.arange(n), torch.full((n,), target)
    grows = torch.cat([rows, ar[pick], tt, ids]).to(torch.int32)
    gcols = torch.cat([cols, ac[pick], ids, tt]).to(torch.int32)
    grad = a.grad[grows.long(), gcols.long()]
    # one train-mode forward without dropout, its noise recorded (the base model stays in eval mode)
    ref.train()
    base.eval()
    for expert in ref.experts:
        expert.dropout_rate = 0.0
    noise = []
    with torch.no_grad(), recorded_randn_like(noise):
        train_out = ref(x, adj)
        train_aux = ref.aux_loss.clone()
    assert len(noise) == 1 and tuple(noise[0].shape) == (n, E)
    with torch.no_grad():
        noisy = clean + noise[0] * (ref.softplus(gi @ ref.w_noise) + 1e-2)
        top, idx = noisy.topk(k + 1, dim=1)
        train_sel = idx[:, :k]
        train_gates = torch.zeros_like(noisy).scatter(1, train_sel, torch.softmax(top[:, :k], dim=1))
    ref.eval()
    P = {name: v.detach().clone() for name, v in ref.state_dict().items()}
    # the float64 restatement on the same arrays
    kw = dict(num_experts=E, k=k, loss_coef=HARNESS["loss_coef"])
    with torch.no_grad():
        r_eval = R.calibrator_forward(P, x, adj, adj, **kw)
        r_train = R.calibrator_forward(P, x, adj, adj, train=True, noise=noise[0], **kw)
    r_grad = R.adjacency_gradient(P, x, adj, loss_weight, grows, gcols, **kw)
    f32_vs_f64 = dict(out=dist(out, r_eval["out"]), gates=dist(gates, r_eval["gates"]),
                      clean_logits=dist(clean, r_eval["clean_logits"]), grad=dist(grad, r_grad),
                      train_out=dist(train_out, r_train["out"]), train_gates=dist(train_gates, r_train["gates"]),
                      aux_loss=dist(train_aux, r_train["aux_loss"]))
    assert torch.equal(sel, r_eval["sel"]) and torch.equal(train_sel, r_train["sel"])
    # no rounding may change a selection: the k-th and (k+1)-th gating logit of every row are far apart
    gap = float(min((t[:, k - 1] - t[:, k]).min() for t in (clean.topk(k + 1, dim=1).values, top)))
    assert gap > 100 * f32_vs_f64["clean_logits"], f"seed {seed}: gap {gap:.3e} vs {f32_vs_f64['clean_logits']:.3e}"
    assert float(grad.abs().max()) > 0 and len(set(sel.flatten().tolist())) == E
    arrays = dict(x=x.numpy(), adj=adj.numpy().astype(np.float32), val_mask=val_mask.numpy(), y=y.numpy(),
                  out=out.numpy(), gates=gates.numpy(), sel=sel.numpy(), clean_logits=clean.numpy(),
                  loss_weight=loss_weight.numpy(), grad_rows=grows.numpy(), grad_cols=gcols.numpy(), grad=grad.numpy(),
                  noise=noise[0].numpy(), train_out=train_out.numpy(), train_gates=train_gates.numpy(),
                  train_sel=train_sel.numpy(), aux_loss=train_aux.numpy().reshape(-1),
                  target=np.int64(target), isolated=np.asarray(isolated, np.int64))
    arrays.update({"p__" + name: v.numpy() for name, v in P.items()})
    print(f"seed {seed}: {rows.numel()} entries, {epochs} epochs, gap {gap:.3e}, f32_vs_f64 {f32_vs_f64}")
    return arrays, dict(seed=seed, entries=int(rows.numel()), epochs=epochs, gate_gap=gap, f32_vs_f64=f32_vs_f64,
                        keywords=HARNESS)


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
    Gm, M = import_reference()
    manifest = dict(generator="tools/gen_golden_gets.py",
                    reference="calibration/GETS.py + src/gnn/model.py (2026-02-06)",
                    numpy=np.__version__, torch=torch.__version__,
                    cpu_code_path=dict(MKL_ENABLE_INSTRUCTIONS="AVX2", ATEN_CPU_CAPABILITY="avx2"), cases={}, files={})
    # 1. 5 classes, one isolated node
    arrays, meta = make_case(Gm, M, seed=21, n=120, n_edges=600, nfeat=16, ncls=5, nhid=32, n_val=37, isolated=[17],
                             target=5)
    manifest["cases"]["iso120"] = meta
    save("iso120", manifest, arrays)
    # 2. 8 classes
    arrays, meta = make_case(Gm, M, seed=33, n=96, n_edges=400, nfeat=12, ncls=8, nhid=24, n_val=24, isolated=[],
                             target=40)
    manifest["cases"]["wide96"] = meta
    save("wide96", manifest, arrays)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("manifest written")


if __name__ == "__main__":
    main()
