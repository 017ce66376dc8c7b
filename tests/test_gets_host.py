"""CPU tests of the GETS yardsticks (tests/gets_ref.py), of the fixtures the reference recorded (tests/golden/gets) and
of the host side of wats_hip.gets: truth and second evaluation agree, the documented model is inside every bound, the
float32-accumulator mutant (a) is outside the t_save bound on a hub row of positive values, the composition's mutant
(b) is outside it there too (found by the search of test_mutant_b_report, which prints every case), the float64
restatement reproduces what the reference recorded within the manifest's f32_vs_f64, the ABI's argument checks, the
refused backbones and the optimiser's parameter list."""
import hashlib
import inspect
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import agg_ref as A
import gets_ref as R
import wats_hip
from wats_hip import cagcn, gets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gets")
CASES = ("iso120", "wide96")
GRAPHS = ("path", "hole", "star127", "star128", "star129", "random300")
_refs = {}


def refs_of(name, kind, E=3, k=2, Cw=7):
    key = (name, kind, E, k, Cw)
    if key not in _refs:
        indptr, indices, n = R.graph_csr(name)
        dinv = R.dinv_of(indptr)
        I = R.head_inputs(n, E, k, Cw, kind, 3)
        fwd = R.forward(indptr, indices, dinv, **I)
        g_out = A.signal(n, Cw, kind, 9)
        t_in = np.clip(fwd["t_save"].model, -30, 60)      # the head's own inputs: softplus stays a normal float32
        bwd = R.head_backward(g_out, fwd["out"].model, I["logits"], t_in, fwd["o_save"].model)
        t_indptr, order = A.transpose_order(indptr, indices)
        g_z = R.transposed(t_indptr, A.row_ids(indptr)[order], dinv, I["sel"], I["gate"], bwd["g_t"].model, E)
        _refs[key] = dict(fwd, g_z=g_z, **bwd)
    return _refs[key]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", GRAPHS)
def test_truth_agrees_with_its_second_evaluation_and_the_model_is_inside(name, kind):
    for what, ref in refs_of(name, kind).items():
        agree, c = ref.agreement(), ref.c(ref.model, what)
        print(f"{name} {kind} {what}: truth vs second {agree:.2e}, model c = {c:.4f} (bound {ref.bound})")
        assert agree <= R.TRUTH_AGREE, (what, agree)
        assert c <= ref.bound, (what, c)


def test_mutant_a_is_outside_the_t_save_bound_on_a_hub_of_positive_values():
    """one float32 accumulator over the hub's 129 entries of one sign: several roundings, not one"""
    ref = refs_of("star129", "positive")["t_save"]
    hub = ref.rows(np.array([0]))
    c = hub.c(hub.mutant, "mutant (a)")
    print(f"mutant (a) on the hub row: c = {c:.3f}")
    assert c > ref.bound
    assert hub.c(hub.model, "model") <= ref.bound


def test_mutant_b_report():
    """Each O_s rounded to float32 before a float32 mixture, the composition's arithmetic: k + 1 roundings where the
    fused head has one.  Printed for every case; it is outside the bound wherever more than one of them lands on the
    same side, which a search over these cases finds on the star's positive values (asserted)."""
    found = {}
    for name in GRAPHS:
        for kind in R.KINDS:
            ref = refs_of(name, kind)["t_save"]
            found[name, kind] = ref.c(ref.mutant_b, "mutant (b)")
            print(f"mutant (b) {name} {kind}: c = {found[name, kind]:.3f}")
    assert found["star129", "positive"] > R.BOUND_ONE
    assert max(found.values()) <= 2 + 1 + R.SLACK      # k + 1 roundings at k = 2


def test_an_empty_range_gives_the_gated_bias():
    indptr, indices, n = R.graph_csr("hole")
    assert indptr[3] == indptr[2]
    I = R.head_inputs(n, 3, 2, 5, "normal", 1)
    t = R.forward(indptr, indices, R.dinv_of(indptr), **I)["t_save"]
    want = sum(I["gate"][2, s].astype(np.float64) * I["bias"][I["sel"][2, s]].astype(np.float64) for s in range(2))
    assert np.allclose(t.truth[2], want, rtol=1e-15, atol=0)


def test_head_restatement_is_the_truth_of_out():
    """the differentiable torch restatement (every expert aggregated, dense gates) and the numpy truth (selected
    slices only) are the same function"""
    indptr, indices, n = R.graph_csr("random300")
    dinv = R.dinv_of(indptr)
    I = R.head_inputs(n, 4, 2, 7, "normal", 5)
    ref = R.forward(indptr, indices, dinv, **I)["out"]
    t = {key: torch.from_numpy(v) for key, v in I.items()}
    src, dst = torch.from_numpy(indices), torch.from_numpy(A.row_ids(indptr))
    out = R.head_torch(src, dst, torch.from_numpy(dinv), t["z"], t["sel"], t["gate"], t["bias"], t["logits"])
    assert ref.c(out.numpy(), "head_torch") <= 1e-3


# ---------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------
def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def test_fixture_integrity():
    m = manifest()
    assert m["generator"] == "tools/gen_golden_gets.py" and sorted(m["cases"]) == sorted(CASES)
    for name, meta in m["files"].items():
        path = os.path.join(GOLDEN, name)
        assert os.path.getsize(path) < 200 * 1024
        with open(path, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == meta["sha256"], name
        with np.load(path, allow_pickle=False) as f:      # arrays only
            assert sorted(f.files) == meta["keys"]
    assert sorted(os.listdir(GOLDEN)) == sorted(list(m["files"]) + ["manifest.json"])


@pytest.mark.parametrize("name", CASES)
def test_the_float64_restatement_reproduces_the_recorded_outputs(name):
    meta = manifest()["cases"][name]
    rec = meta["f32_vs_f64"]
    c = R.load_case(os.path.join(GOLDEN, name + ".npz"))
    P = R.case_params(c)
    kw = dict(num_experts=meta["keywords"]["num_experts"], k=meta["keywords"]["expert_select"],
              loss_coef=meta["keywords"]["loss_coef"])
    with torch.no_grad():
        ev = R.calibrator_forward(P, c["x"], c["adj"], c["adj"], **kw)
        tr = R.calibrator_forward(P, c["x"], c["adj"], c["adj"], train=True, noise=c["noise"], **kw)
    grad = R.adjacency_gradient(P, c["x"], c["adj"], c["loss_weight"], c["grad_rows"], c["grad_cols"], **kw)
    assert torch.equal(ev["sel"], c["sel"]) and torch.equal(tr["sel"], c["train_sel"])
    got = dict(out=(ev["out"], c["out"]), gates=(ev["gates"], c["gates"]),
               clean_logits=(ev["clean_logits"], c["clean_logits"]), grad=(grad, c["grad"]),
               train_out=(tr["out"], c["train_out"]), train_gates=(tr["gates"], c["train_gates"]),
               aux_loss=(tr["aux_loss"].reshape(-1), c["aux_loss"]))
    assert sorted(got) == sorted(rec)
    for what, (mine, theirs) in got.items():
        d = float((mine.double() - theirs.double()).abs().max())
        print(f"{name} {what}: |float64 restatement - recorded float32| = {d:.3e} (manifest {rec[what]:.3e})")
        # the float64 side may differ from the generator's machine by its own last bits only
        assert d <= rec[what] * (1 + 1e-6) + 1e-13, what
    # no rounding can change a selection
    assert meta["gate_gap"] > 100 * rec["clean_logits"]
    top = ev["clean_logits"].topk(kw["k"] + 1, dim=1).values
    assert float((top[:, kw["k"] - 1] - top[:, kw["k"]]).min()) > 100 * rec["clean_logits"]
    # the frozen degree embeddings are in the fixture under the reference's names
    assert "experts.1.degree_embedder.weight" in P and "experts.0.convs.0.lin.weight" in P


# ---------------------------------------------------------------------------------------------------------
# the host side of wats_hip.gets
# ---------------------------------------------------------------------------------------------------------
def test_abi_checks_arguments_before_any_device_work():
    lib = wats_hip._lib.load()
    assert lib.wg_gated_symnorm_long_row() == R.LONG == gets.gated_long_row_threshold()
    one = 4096     # any non-NULL address: no call below reaches the device
    p = [one + 256 * q for q in range(12)]
    fwd, tr, hb = lib.wg_gated_symnorm_forward, lib.wg_gated_symnorm_transposed, lib.wg_gets_head_backward
    #         n  nnz indptr indices n_long long  dinv  C  E  k  z     sel   gate  bias  logits out   t     o     stream
    ok_f = [3, 3, p[0], p[1], 0, None, p[2], 4, 3, 2, p[3], p[4], p[5], None, p[6], p[7], None, None, None]
    ok_t = [3, 3, p[0], p[1], 0, None, p[2], 4, 3, 2, p[4], p[5], p[6], p[7], None]
    ok_h = [3, 4, 2] + p[:8] + [None]

    def bad(f, ok, status, word, **changes):
        args = list(ok)
        for pos, v in changes.items():
            args[int(pos[1:])] = v
        assert f(*args) == status, (f.__name__, changes)
        assert word in lib.wg_last_error(), (f.__name__, changes, lib.wg_last_error())

    for f, ok in ((fwd, ok_f), (tr, ok_t)):
        # n == 0: nothing to do, whatever the pointers
        assert f(*([0, 0, None, None, 0, None, None, 4, 3, 2] + [None] * (len(ok) - 10))) == 0
        for pos in ("a0", "a1", "a4"):
            bad(f, ok, -1, b"negative", **{pos: -1})
        for pos, v in (("a7", 0), ("a8", 0), ("a9", 0), ("a9", 4)):     # C < 1, E < 1, k < 1, k > E
            bad(f, ok, -1, b"needs 1 <= k <= E", **{pos: v})
        bad(f, ok, -4, b"above", a7=257)
        bad(f, ok, -4, b"above", a8=5, a9=5)
        bad(f, ok, -4, b"int32", a0=2 ** 31)
        bad(f, ok, -4, b"int32", a1=2 ** 31)
        bad(f, ok, -1, b"long rows", a4=4, a5=one)
        bad(f, ok, -1, b"long_rows", a4=1)
        for pos in ("a2", "a3", "a6"):
            bad(f, ok, -1, b"NULL", **{pos: None})
    for pos in ("a10", "a11", "a12", "a14", "a15"):
        bad(fwd, ok_f, -1, b"NULL", **{pos: None})
    bad(fwd, ok_f, -1, b"go together", a16=p[8])
    bad(fwd, ok_f, -1, b"go together", a17=p[8])
    bad(fwd, ok_f, -1, b"alias", a15=p[3])             # out == z
    bad(fwd, ok_f, -1, b"alias", a15=p[6])             # out == logits
    bad(fwd, ok_f, -1, b"alias", a16=p[7], a17=p[9])   # t_save == out
    bad(fwd, ok_f, -1, b"alias", a16=p[9], a17=p[9])   # o_save == t_save
    for pos in ("a10", "a11", "a12", "a13"):
        bad(tr, ok_t, -1, b"NULL", **{pos: None})
    bad(tr, ok_t, -1, b"alias", a13=p[6])              # g_z == g_t
    assert hb(0, 4, 2, *([None] * 9)) == 0
    bad(hb, ok_h, -1, b"negative", a0=-1)
    bad(hb, ok_h, -1, b"needs 1 <= k", a1=0)
    bad(hb, ok_h, -1, b"needs 1 <= k", a2=0)
    bad(hb, ok_h, -4, b"above", a1=257)
    bad(hb, ok_h, -4, b"above", a2=5)
    bad(hb, ok_h, -4, b"int32", a0=2 ** 31)
    for q in range(3, 11):
        bad(hb, ok_h, -1, b"NULL", **{f"a{q}": None})


def test_exported_surface_and_signatures():
    for name in ("GETSCalibrator", "GCNExpert", "gated_sym_norm_head", "calibrate_with_gets"):
        assert getattr(wats_hip, name) is getattr(gets, name)
    sig = inspect.signature(gets.GETSCalibrator.__init__)
    want = dict(num_experts=3, expert_select=2, hidden_dim=64, dropout_rate=0.1, num_layers=2, feature_hidden_dim=32,
                degree_hidden_dim=16, noisy_gating=True, loss_coef=1e-2, backbone="gcn")     # GETS.py:260-269
    assert {key: sig.parameters[key].default for key in want} == want
    assert list(sig.parameters)[:9] == ["self", "base_model", "num_classes", "device", "conf", "x", "y", "adj", "val_idx"]
    assert all(sig.parameters[key].kind is inspect.Parameter.KEYWORD_ONLY
               for key in ("graph", "verbose", "train_degree_embedding"))
    assert sig.parameters["train_degree_embedding"].default is False
    ct = inspect.signature(gets.GETSCalibrator.calib_train)
    assert {key: p.default for key, p in ct.parameters.items() if key != "self"} == \
        dict(patience=10, epochs=250, lr=0.01, weight_decay=5e-4)
    for name in ("fit", "forward", "noisy_top_k_gating", "cv_squared", "aux_loss"):
        assert name == "aux_loss" or callable(getattr(gets.GETSCalibrator, name))


@pytest.mark.parametrize("backbone, why", [("gat", "GATConv"), ("gin", "MLP after the neighbour sum")])
def test_other_backbones_are_refused_with_the_reason(backbone, why):
    with pytest.raises(NotImplementedError, match=why):
        gets.GETSCalibrator(nn.Linear(3, 3), 3, backbone=backbone)


def host_calibrator(train_degree_embedding=False):
    """the calibrator's networks on the CPU: parameters need no graph (as test_cagcn_host builds a GCNConv)"""
    graph = object.__new__(cagcn.SymNormGraph)
    graph.device = torch.device("cpu")
    cal = gets.GETSCalibrator.__new__(gets.GETSCalibrator)
    nn.Module.__init__(cal)
    cal.device, cal.graph, cal.num_classes, cal.num_experts = graph.device, graph, 5, 4
    cal.hidden_dim, cal.dropout_rate, cal.num_layers, cal.feature_dim = 32, 0.1, 3, 6
    cal.feature_hidden_dim, cal.degree_hidden_dim = 16, 8
    cal.expert_configs = [list(c) for c in gets.EXPERT_CONFIGS]
    cal.degrees = torch.tensor([0, 3, 7, 2])
    cal.train_degree_embedding = train_degree_embedding
    cal._build_networks()
    return cal


def test_the_optimiser_leaves_the_degree_embeddings_out():
    cal = host_calibrator()
    names = dict(cal.named_parameters())
    emb = [key for key in names if "degree_embedder" in key]
    assert sorted(emb) == [f"experts.{e}.degree_embedder.weight" for e in (1, 2, 3)]
    assert all(names[key].requires_grad and tuple(names[key].shape) == (8, 8) for key in emb)   # max degree 7
    chosen = {id(p) for p in cal.optimizer_parameters()}
    assert all(id(names[key]) not in chosen for key in emb)
    assert all(id(p) in chosen for key, p in names.items() if key not in emb)
    assert len(host_calibrator(True).optimizer_parameters()) == len(names)


def test_state_dict_has_the_reference_names():
    keys = set(host_calibrator().state_dict())
    for e, config in enumerate(gets.EXPERT_CONFIGS):
        want = {f"experts.{e}.convs.{layer}.{p}" for layer in (0, 1) for p in ("lin.weight", "bias")}
        if "features" in config:
            want |= {f"experts.{e}.proj_feature.weight", f"experts.{e}.proj_feature.bias"}
        if "degrees" in config:
            want.add(f"experts.{e}.degree_embedder.weight")
        assert {key for key in keys if key.startswith(f"experts.{e}.")} == want
    assert {key for key in keys if not key.startswith("experts.")} == \
        {"proj_feature.weight", "proj_feature.bias", "w_gate", "w_noise", "mean", "std"}


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU refusal")
def test_refuses_to_run_without_a_gpu():
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        gets.GETSCalibrator(nn.Linear(3, 3), 3)
    with pytest.raises(ValueError, match="SymNormGraph"):
        gets.gated_sym_norm_head(torch.eye(3), torch.zeros(3, 2, 3), torch.zeros(3, 1, dtype=torch.int32),
                                 torch.zeros(3, 1), None, torch.zeros(3, 3))
