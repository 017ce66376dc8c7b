"""Test-only dense restatement of the reference's SimCalib (``calibration/SimCalib.py:49-58, 78-111``) and of the
base model it wraps (``src/gnn/model.py:37-53``) in plain torch, in a chosen dtype, on the CPU.  The product never
imports this file.  Every function takes float32 (or any) inputs and converts them to ``dtype`` first, so the
float64 run starts from the same float32 numbers as the float32 run and the kernels."""
import torch
import torch.nn.functional as F

TAU, T_MIN, T_MAX = 0.1, 0.1, 5.0     # SimCalib.py:95, :106
# the CPU code paths the fixtures were generated on (tools/gen_golden_simcalib.py); read when torch starts
PINNED_CPU_PATH = {"MKL_ENABLE_INSTRUCTIONS": "AVX2", "ATEN_CPU_CAPABILITY": "avx2"}


def compute_similarity_matrix(X1, X2):
    """SimCalib.py:49-58."""
    return torch.mm(F.normalize(X1, p=2, dim=1), F.normalize(X2, p=2, dim=1).t())


def raw_temperature(latent, bank, inv_conf, tau=TAU, dtype=torch.float64):
    """SimCalib.py:52, :56, :98, :105 against an ALREADY normalised bank: the unclamped temperatures (n,)."""
    a = F.normalize(latent.to(dtype), p=2, dim=1)
    sim = torch.mm(a, bank.to(dtype).t())
    w = F.softmax(sim / tau, dim=1)
    return torch.mm(w, inv_conf.to(dtype).unsqueeze(1)).squeeze(1)


def temperature_and_grad(latent, bank, inv_conf, g, tau=TAU, t_min=T_MIN, t_max=T_MAX, dtype=torch.float64):
    """(unclamped t, clamped t, d(sum(g * clamped t)) / d latent) in ``dtype`` from the given inputs."""
    x = latent.detach().clone().to(dtype).requires_grad_(True)
    raw = raw_temperature(x, bank, inv_conf, tau, dtype)
    t = raw.clamp(min=t_min, max=t_max)
    (t * g.to(dtype)).sum().backward()
    return raw.detach(), t.detach(), x.grad


def gcn_hidden(adj, x, w1, b1):
    """model.py:43-48 / SimCalib.py:67-73: (adj_norm, relu(gc1(adj_norm @ x)))."""
    deg = adj.sum(dim=1, keepdim=True)
    deg[deg == 0] = 1
    adj_norm = adj / deg
    return adj_norm, F.relu(F.linear(torch.mm(adj_norm, x), w1, b1))


def gcn_logits(adj, x, w1, b1, w2, b2):
    """model.py:37-53 in eval mode."""
    adj_norm, h = gcn_hidden(adj, x, w1, b1)
    return F.linear(torch.mm(adj_norm, h), w2, b2), h


def calibration_state(adj, x, params, val_mask, dtype=torch.float64):
    """SimCalib.py:38-47: (features_val, val_confidence)."""
    adj, x = adj.to(dtype), x.to(dtype)
    w1, b1, w2, b2 = (p.to(dtype) for p in params)
    logits, h = gcn_logits(adj, x, w1, b1, w2, b2)
    return h[val_mask], F.softmax(logits[val_mask], dim=1).max(dim=1).values


def forward(adj, x, params, features_val, val_confidence, epsilon=1e-8, tau=TAU, dtype=torch.float64):
    """SimCalib.py:78-111: (log-probs, unclamped temperatures).  ``adj`` may require grad."""
    adj, x = adj.to(dtype), x.to(dtype)
    w1, b1, w2, b2 = (p.to(dtype) for p in params)
    logits, latent = gcn_logits(adj, x, w1, b1, w2, b2)
    sim = compute_similarity_matrix(latent, features_val.to(dtype))
    w = F.softmax(sim / tau, dim=1)
    inv_conf = 1.0 / (val_confidence.to(dtype) + epsilon)
    raw = torch.mm(w, inv_conf.unsqueeze(1)).squeeze(1)
    t = raw.clamp(min=T_MIN, max=T_MAX)
    return F.log_softmax(logits / t.unsqueeze(1), dim=1), raw


def adjacency_gradient(adj, x, params, features_val, val_confidence, loss_weight, rows, cols, dtype=torch.float64):
    """d sum(loss_weight * log-probs) / d adj at (rows, cols), the dense way of the attack
    (calib_fga.py:864-881)."""
    a = adj.detach().clone().to(dtype).requires_grad_(True)
    out, _ = forward(a, x, params, features_val, val_confidence, dtype=dtype)
    (out * loss_weight.to(dtype)).sum().backward()
    return a.grad[rows.long(), cols.long()]


def fixture_differences(path):
    """{key: [max|float32 restatement - recorded array|, max|recorded array|]} for one fixture file."""
    import numpy as np
    with np.load(path, allow_pickle=False) as d:
        c = {k: torch.from_numpy(np.asarray(d[k])) for k in d.files}
    params = (c["gc1_weight"], c["gc1_bias"], c["gc2_weight"], c["gc2_bias"])
    fv, conf = calibration_state(c["adj"], c["x"], params, c["val_mask"].bool(), torch.float32)
    out, raw = forward(c["adj"], c["x"], params, c["features_val"], c["val_confidence"], float(c["epsilon"]),
                       dtype=torch.float32)
    grad = adjacency_gradient(c["adj"], c["x"], params, c["features_val"], c["val_confidence"], c["loss_weight"],
                              c["grad_rows"], c["grad_cols"], torch.float32)
    got = dict(features_val=fv, val_confidence=conf, out=out, raw_t=raw, grad=grad)
    return {k: [float((v.detach() - c[k]).abs().max()), float(c[k].abs().max())] for k, v in got.items()}


if __name__ == "__main__":
    # python tests/simcalib_ref.py <fixture.npz> ...: one JSON line {file: fixture_differences(file)}
    import json
    import sys
    print(json.dumps({p: fixture_differences(p) for p in sys.argv[1:]}))
