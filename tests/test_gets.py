"""GPU tests of the gated expert aggregation (csrc/gatedagg.hip), its autograd wrapper and the GETS calibrator
(wats_hip/gets.py).

Kernel outputs are held to tests/gets_ref.py in row units: c = max |got - truth| / unit over EVERY element (output
buffers start as NaN, and c_of refuses a non-finite value, so an element the kernel left out fails), c <= BOUND_ONE
for t_save, o_save, g_z, g_logits, g_t and g_gate, and the bound of `out` from that module's docstring.  The
gradients of the autograd function are held to the float64 restatement's autograd inside
gets_ref.autograd_bounds, the sum of the documented bounds.  The fused head is held to the unfused mixture of
GCNExpert.forward inside the unfused path's own roundings: each O_s rounded (one unit of T in all, the unit being the
gated sum of theirs), each product gate * O_s rounded (one more), k - 1 float32 additions, and the fused T's own
rounding: k + 2.  The calibrator is held to the fixtures the reference recorded within 4 x the manifest's f32_vs_f64
of each quantity (another summation order and float32 GEMMs on another machine), the selection exactly.
"""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import agg_ref as A  # noqa: E402
import cagcn_ref  # noqa: E402
import gets_ref as R  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip import gets  # noqa: E402
from wats_hip._lib import ptr  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gets")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()
    assert gets.gated_long_row_threshold() == R.LONG


# ---------------------------------------------------------------------------------------------------------
# device graphs and raw calls
# ---------------------------------------------------------------------------------------------------------
_graphs = {}


def device_graph(name):
    """what the kernels read of a graph, as SymNormGraph holds it, from the numpy CSR of gets_ref.graph_csr (the
    "hole" graph has a row without its self loop, which SymNormGraph would not build)"""
    if name not in _graphs:
        indptr, indices, n = R.graph_csr(name)
        t_indptr, order = A.transpose_order(indptr, indices)
        t_indices = A.row_ids(indptr)[order]
        g = types.SimpleNamespace(n=n, nnz=len(indices), device=torch.device(DEV, torch.cuda.current_device()),
                                  np_indptr=indptr, np_indices=indices, np_t_indptr=t_indptr, np_t_indices=t_indices,
                                  np_dinv=R.dinv_of(indptr))
        g.indptr, g.t_indptr = (torch.from_numpy(v).to(DEV) for v in (indptr, t_indptr))
        g.indices, g.t_indices = (torch.from_numpy(v.astype(np.int32)).to(DEV) for v in (indices, t_indices))
        g.dinv = torch.from_numpy(g.np_dinv).to(DEV)
        _graphs[name] = g
    return _graphs[name]


def listed(lengths, listing):
    """the ascending list the caller passes: "exact" the rows of at least LONG entries, "none" nothing (a long row is
    then computed by a sub-group), "extra" the first row (the star's hub, long or not) and a short row"""
    if listing == "exact":
        rows = np.flatnonzero(lengths >= R.LONG)
    elif listing == "none":
        rows = np.zeros(0, np.int64)
    else:
        assert listing == "extra", listing
        rows = np.array([0, 5])
        assert lengths[5] < R.LONG
    return torch.from_numpy(rows.astype(np.int32)).to(DEV)


def dev(a, misalign=False):
    """a device copy; misalign: at an address that is 4 modulo 16"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misalign:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def nan_buffer(shape, misalign=False):
    return dev(np.full(shape, np.nan, np.float32), misalign)


def run_forward(g, I, listing="exact", save=True, misalign=False):
    n, E, Cw = I["z"].shape
    k = I["sel"].shape[1]
    d = {key: None if v is None else dev(v, misalign and key != "sel") for key, v in I.items()}
    out = nan_buffer((n, Cw), misalign)
    t = nan_buffer((n, Cw), misalign) if save else None
    o = nan_buffer((n, k, Cw), misalign) if save else None
    long_rows = listed(np.diff(g.np_indptr), listing)
    rc = wats_hip._lib.load().wg_gated_symnorm_forward(
        g.n, g.nnz, ptr(g.indptr), ptr(g.indices), int(long_rows.numel()), ptr(long_rows), ptr(g.dinv), Cw, E, k,
        ptr(d["z"]), ptr(d["sel"]), ptr(d["gate"]), ptr(d["bias"]), ptr(d["logits"]), ptr(out), ptr(t), ptr(o),
        gets.stream_handle(g.device))
    assert rc == 0, wats_hip._lib.load().wg_last_error()
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in (out, t, o))


def run_transposed(g, sel, gate, g_t, E, listing="exact", misalign=False):
    n, Cw = g_t.shape
    g_z = nan_buffer((n, E, Cw), misalign)
    long_rows = listed(np.diff(g.np_t_indptr), listing)
    d_sel, d_gate, d_gt = dev(sel), dev(gate), dev(g_t, misalign)
    rc = wats_hip._lib.load().wg_gated_symnorm_transposed(
        g.n, g.nnz, ptr(g.t_indptr), ptr(g.t_indices), int(long_rows.numel()), ptr(long_rows), ptr(g.dinv), Cw, E,
        sel.shape[1], ptr(d_sel), ptr(d_gate), ptr(d_gt), ptr(g_z), gets.stream_handle(g.device))
    assert rc == 0, wats_hip._lib.load().wg_last_error()
    torch.cuda.synchronize()
    return g_z.cpu().numpy()


def check_forward(g, I, got, what):
    refs = R.forward(g.np_indptr, g.np_indices, g.np_dinv, **I)
    for key, value in zip(("out", "t_save", "o_save"), got):
        ref = refs[key]
        c = ref.c(value, f"{what} {key}")
        print(f"{what} {key}: c = {c:.4f} (bound {ref.bound}; model {ref.c(ref.model):.4f}, "
              f"float32-sum mutant {ref.c(ref.mutant):.4f})")
        assert c <= ref.bound, (what, key, c)
    return refs


def forward_cases():
    cases = [("star129", Cw, 3, 2, "positive") for Cw in R.WIDTHS]
    cases += [("random300", Cw, E, k, "normal") for E, k in R.EXPERTS for Cw in (7, 40)]
    cases += [(name, Cw, E, k, kind) for name in ("path", "hole", "star128", "random300") for kind in R.KINDS
              for Cw in (5, 64) for E, k in ((3, 2), (4, 4))]
    return list(dict.fromkeys(cases))


# ---------------------------------------------------------------------------------------------------------
# the forward kernel
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, Cw, E, k, kind", forward_cases())
def test_forward_against_the_truth_in_row_units(name, Cw, E, k, kind):
    g = device_graph(name)
    I = R.head_inputs(g.n, E, k, Cw, kind, 3)
    got = run_forward(g, I)
    check_forward(g, I, got, f"{name} C={Cw} E={E} k={k} {kind}")
    inference = run_forward(g, I, save=False)[0]
    assert np.array_equal(inference.view(np.int32), got[0].view(np.int32))


@pytest.mark.parametrize("Cw", [7, 64])
@pytest.mark.parametrize("listing", ["exact", "none", "extra"])
@pytest.mark.parametrize("hub", [127, 128, 129])
def test_bins_on_the_star(hub, listing, Cw):
    """the hub has LONG - 1, LONG and LONG + 1 entries as a row and as a column; it is listed, not listed (a long row
    is then a sub-group's), and listed with a short row beside it: every row is written and right in each"""
    g = device_graph(f"star{hub}")
    assert np.diff(g.np_indptr)[0] == hub == np.diff(g.np_t_indptr)[0]
    I = R.head_inputs(g.n, 3, 2, Cw, "positive", 4)
    what = f"star{hub} {listing} C={Cw}"
    refs = check_forward(g, I, run_forward(g, I, listing), what)
    g_t = A.signal(g.n, Cw, "positive", 6)
    ref = R.transposed(g.np_t_indptr, g.np_t_indices, g.np_dinv, I["sel"], I["gate"], g_t, 3)
    c = ref.c(run_transposed(g, I["sel"], I["gate"], g_t, 3, listing), what + " g_z")
    print(f"{what} g_z: c = {c:.4f}")
    assert c <= ref.bound
    # the float32-accumulator mutant would have failed on the hub's row
    hub_row = refs["t_save"].rows(np.array([0]))
    assert hub_row.c(hub_row.mutant) > refs["t_save"].bound


@pytest.mark.parametrize("Cw", [8, 64, 5])
def test_misaligned_buffers_take_the_dword_path(Cw):
    g = device_graph("random300")
    I = R.head_inputs(g.n, 3, 2, Cw, "normal", 8)
    got = run_forward(g, I, misalign=True)
    check_forward(g, I, got, f"misaligned C={Cw}")
    aligned = run_forward(g, I)
    for a, b in zip(got, aligned):      # the same sums in the same order
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    g_t = A.signal(g.n, Cw, "normal", 2)
    ref = R.transposed(g.np_t_indptr, g.np_t_indices, g.np_dinv, I["sel"], I["gate"], g_t, 3)
    assert ref.c(run_transposed(g, I["sel"], I["gate"], g_t, 3, misalign=True), "misaligned g_z") <= ref.bound


def test_an_empty_range_gives_the_gated_bias():
    g = device_graph("hole")
    I = R.head_inputs(g.n, 3, 2, 5, "normal", 1)
    _, t, o = run_forward(g, I)
    want = sum(I["gate"][2, s].astype(np.float64) * I["bias"][I["sel"][2, s]].astype(np.float64) for s in range(2))
    assert np.array_equal(t[2], want.astype(np.float32))
    assert np.array_equal(o[2], I["bias"][I["sel"][2]])
    _, t, o = run_forward(g, dict(I, bias=None))
    assert not t[2].any() and not o[2].any()


# ---------------------------------------------------------------------------------------------------------
# the two backward kernels on their own inputs
# ---------------------------------------------------------------------------------------------------------
def head_backward_inputs(n, k, Cw, kind, seed):
    """T on both sides of the threshold 20, and at it; out a log_softmax; the rest of `kind`"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-30, 60, (n, Cw)).astype(np.float32)
    t[0, :] = 20.0
    t[1, :] = np.nextafter(np.float32(20), np.float32(30))
    t[2, :] = np.nextafter(np.float32(20), np.float32(10))
    v = 3 * rng.standard_normal((n, Cw))
    out = (v - np.log(np.exp(v).sum(1, keepdims=True))).astype(np.float32)
    return dict(g_out=A.signal(n, Cw, kind, seed + 1), out=out, logits=A.signal(n, Cw, "normal", seed + 2), t_save=t,
                o_save=A.signal(n, k * Cw, kind, seed + 3).reshape(n, k, Cw))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("Cw", R.WIDTHS)
def test_head_backward_on_its_own_inputs(Cw, k, kind):
    n = 300      # more than one workgroup at every width
    I = head_backward_inputs(n, k, Cw, kind, 5)
    d = {key: dev(v) for key, v in I.items()}
    assert float((d["t_save"] > 20).float().mean()) > 0.2 and float((d["t_save"] <= 20).float().mean()) > 0.2
    got = gets.gets_head_backward(d["g_out"], d["out"], d["logits"], d["t_save"], d["o_save"])
    refs = R.head_backward(**I)
    for key, value in zip(("g_logits", "g_t", "g_gate"), got):
        c = refs[key].c(value.cpu().numpy(), key)
        print(f"head backward C={Cw} k={k} {kind} {key}: c = {c:.4f} (float32-sum mutant "
              f"{refs[key].c(refs[key].mutant):.4f})")
        assert c <= refs[key].bound, (key, c)


@pytest.mark.parametrize("name, Cw, E, k, kind", [(n, c, e, k, kd) for n in ("random300", "path", "hole")
                                                  for c in (5, 40, 64, 256) for e, k in R.EXPERTS
                                                  for kd in ("normal", "spread") if (n == "random300" or c == 5)])
def test_transposed_on_its_own_inputs(name, Cw, E, k, kind):
    g = device_graph(name)
    I = R.head_inputs(g.n, E, k, Cw, "normal", 11)
    g_t = A.signal(g.n, Cw, kind, 12)
    ref = R.transposed(g.np_t_indptr, g.np_t_indices, g.np_dinv, I["sel"], I["gate"], g_t, E)
    got = run_transposed(g, I["sel"], I["gate"], g_t, E)
    c = ref.c(got, "g_z")
    print(f"transposed {name} C={Cw} E={E} k={k} {kind}: c = {c:.4f} (mutant {ref.c(ref.mutant):.4f})")
    assert c <= ref.bound
    nobody = (ref.unit == 0).all(2)     # slices that no gathering row selected: exact zeros
    assert not got[nobody].any()


def test_an_expert_that_nobody_selects_gets_a_zero_slice():
    g = device_graph("random300")
    I = R.head_inputs(g.n, 3, 2, 7, "normal", 13)
    sel = I["sel"]      # ids in {0, 1, 2}, of E = 4 below
    g_t = A.signal(g.n, 7, "normal", 14)
    got = run_transposed(g, sel, I["gate"], g_t, 4)
    assert not got[:, 3, :].any() and np.abs(got[:, :3, :]).max() > 0
    assert R.transposed(g.np_t_indptr, g.np_t_indices, g.np_dinv, sel, I["gate"], g_t, 4).c(got) <= R.BOUND_ONE


# ---------------------------------------------------------------------------------------------------------
# the autograd function
# ---------------------------------------------------------------------------------------------------------
_sym = {}


def sym_graph(name):
    if name not in _sym:
        if name == "cora":
            src, dst, n, _ = cagcn_ref.cora_like_edges(seed=1, n=500)
        else:
            g = device_graph(name)
            src, dst, n = g.np_indices, A.row_ids(g.np_indptr), g.n
        graph = wats_hip.SymNormGraph(torch.from_numpy(np.stack([src, dst])), n)
        indptr, indices = graph.indptr.cpu().numpy(), graph.indices.cpu().numpy().astype(np.int64)
        _sym[name] = (graph, indptr, indices, graph.dinv.cpu().numpy())
    return _sym[name]


@pytest.mark.parametrize("kind", ["normal", "positive"])
@pytest.mark.parametrize("name, Cw, E, k", [("random300", 7, 3, 2), ("random300", 40, 4, 2), ("star129", 5, 3, 3),
                                            ("cora", 7, 3, 2), ("random300", 64, 1, 1)])
def test_gradients_against_the_float64_autograd(name, Cw, E, k, kind):
    graph, indptr, indices, dinv = sym_graph(name)
    I = R.head_inputs(graph.n, E, k, Cw, kind, 21)
    g_out = A.signal(graph.n, Cw, kind, 22)
    leaves = {key: torch.from_numpy(I[key]).to(DEV).requires_grad_(True) for key in ("z", "gate", "bias", "logits")}
    out = wats_hip.gated_sym_norm_head(graph, leaves["z"], torch.from_numpy(I["sel"]).to(DEV), leaves["gate"],
                                       leaves["bias"], leaves["logits"])
    out.backward(torch.from_numpy(g_out).to(DEV))
    ref_leaves = {key: torch.from_numpy(I[key]).double().requires_grad_(True) for key in leaves}
    ref = R.head_torch(torch.from_numpy(indices), torch.from_numpy(A.row_ids(indptr)), torch.from_numpy(dinv),
                       ref_leaves["z"], torch.from_numpy(I["sel"]), ref_leaves["gate"], ref_leaves["bias"],
                       ref_leaves["logits"])
    ref.backward(torch.from_numpy(g_out).double())
    fwd = R.forward(indptr, indices, dinv, **I)["out"]
    assert fwd.c(out.detach().cpu().numpy(), "out") <= fwd.bound
    assert fwd.c(ref.detach().numpy(), "restatement") <= 1e-3
    bounds = R.autograd_bounds(indptr, indices, dinv, I, g_out)
    for key, b in (("z", "g_z"), ("gate", "g_gate"), ("bias", "g_bias"), ("logits", "g_logits")):
        got, want = leaves[key].grad.cpu().double().numpy(), ref_leaves[key].grad.numpy()
        assert np.isfinite(got).all()
        err, bound = np.abs(got - want), bounds[b].reshape(want.shape)
        worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        print(f"{name} C={Cw} E={E} k={k} {kind} grad {key}: worst err / bound = {worst:.4f}, "
              f"max |grad| = {np.abs(want).max():.3e}")
        assert not err[bound == 0].any() and worst <= 1.0, (key, worst)


def test_inference_saves_nothing_and_is_the_same_bits():
    graph, indptr, indices, dinv = sym_graph("random300")
    I = {key: torch.from_numpy(v).to(DEV) for key, v in R.head_inputs(graph.n, 3, 2, 40, "normal", 2).items()}
    with torch.no_grad():
        a = wats_hip.gated_sym_norm_head(graph, **I)
    b = wats_hip.gated_sym_norm_head(graph, I["z"].clone().requires_grad_(True), I["sel"], I["gate"], I["bias"],
                                     I["logits"])
    assert not a.requires_grad and b.requires_grad and torch.equal(a, b)
    c = wats_hip.gated_sym_norm_head(graph, I["z"], I["sel"].long(), I["gate"], I["bias"], I["logits"])
    assert torch.equal(a, c)


def test_python_argument_checks():
    graph, *_ = sym_graph("random300")
    I = {key: torch.from_numpy(v).to(DEV) for key, v in R.head_inputs(graph.n, 3, 2, 5, "normal", 2).items()}

    def call(**kw):
        return wats_hip.gated_sym_norm_head(graph, **dict(I, **kw))

    dup = I["sel"].clone()
    dup[7, 1] = dup[7, 0]
    with pytest.raises(ValueError, match="twice"):
        call(sel=dup)
    far = I["sel"].clone()
    far[3, 0] = 3
    with pytest.raises(ValueError, match="outside"):
        call(sel=far)
    for bad in (dict(z=I["z"][:-1]), dict(z=I["z"][:, 0]), dict(sel=I["sel"][:, :0]), dict(sel=I["sel"].float()),
                dict(gate=I["gate"][:, :1]), dict(logits=I["logits"][:, :-1]), dict(bias=I["bias"][:2]),
                dict(z=I["z"].long()), dict(z=torch.zeros(graph.n, 5, 5, device=DEV)),
                dict(z=torch.zeros(graph.n, 3, 257, device=DEV), logits=torch.zeros(graph.n, 257, device=DEV),
                     bias=None)):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError, match="SymNormGraph"):
        wats_hip.gated_sym_norm_head(graph.ag, **I)


# ---------------------------------------------------------------------------------------------------------
# bits and NaNs
# ---------------------------------------------------------------------------------------------------------
def three_calls(graph, I, g_out):
    out, t, o = gets.gated_forward(graph, I["z"], I["sel"], I["gate"], I["bias"], I["logits"], True)
    g_logits, g_t, g_gate = gets.gets_head_backward(g_out, out, I["logits"], t, o)
    g_z = gets.gated_transposed(graph, I["sel"], I["gate"], g_t, I["z"].shape[1])
    return out, t, o, g_logits, g_t, g_gate, g_z


@pytest.mark.parametrize("name, Cw", [("random300", 40), ("star129", 7)])
def test_same_bits_twice_and_from_a_replayed_graph(name, Cw):
    graph, *_ = sym_graph(name)
    I = {key: torch.from_numpy(v).to(DEV) for key, v in R.head_inputs(graph.n, 3, 2, Cw, "normal", 31).items()}
    g_out = torch.from_numpy(A.signal(graph.n, Cw, "normal", 32)).to(DEV)
    first = three_calls(graph, I, g_out)
    second = three_calls(graph, I, g_out)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, second))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        three_calls(graph, I, g_out)      # the capture allocates from a warm pool
        with torch.cuda.graph(cg, stream=side):
            captured = three_calls(graph, I, g_out)
    for t in captured:
        t.fill_(float("nan"))
    cg.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, captured))


def test_nan_containment():
    g = device_graph("random300")
    I = R.head_inputs(g.n, 3, 2, 7, "normal", 41)
    lens = np.diff(g.np_t_indptr)
    j = int(np.flatnonzero(lens >= 4)[0])
    gatherers = g.np_t_indices[g.np_t_indptr[j]:g.np_t_indptr[j + 1]]
    clean = run_forward(g, I)
    # (1) a NaN in a slice that no row gathering j selected reaches no output
    sel = I["sel"].copy()
    sel[gatherers] = np.array([[0, 1]], np.int32)
    z = I["z"].copy()
    z[j, 2, :] = np.nan
    got = run_forward(g, dict(I, sel=sel, z=z))
    assert all(np.isfinite(v).all() for v in got)
    # (2) a NaN in a selected slice reaches exactly the rows that have j in their range and select that expert
    sel[gatherers[::2]] = np.array([[1, 2]], np.int32)      # every other gatherer does not select expert 0
    z = I["z"].copy()
    z[j, 0, :] = np.nan
    base = run_forward(g, dict(I, sel=sel))
    got = run_forward(g, dict(I, sel=sel, z=z))
    hit = np.zeros(g.n, bool)
    hit[gatherers] = (sel[gatherers] == 0).any(1)
    assert 0 < hit.sum() < len(gatherers)
    for name, a, b in zip(("out", "t_save", "o_save"), got, base):
        bad = np.isnan(a).reshape(g.n, -1)
        if name == "o_save":      # only the slot that holds expert 0
            assert np.array_equal(np.isnan(a).all(2), (sel == 0) & hit[:, None]) and \
                np.array_equal(np.isnan(a).any(2), np.isnan(a).all(2))
        else:
            assert np.array_equal(bad.all(1), hit) and np.array_equal(bad.any(1), hit), name
        assert np.array_equal(a[~np.isnan(a)].view(np.int32), b[~np.isnan(a)].view(np.int32)), name
    assert clean[0].shape == got[0].shape
    # the transposed pass: a NaN row of g_t reaches only the experts its row selected, in the nodes of its range
    i = int(gatherers[0])
    g_t = A.signal(g.n, 7, "normal", 42)
    g_t[i, :] = np.nan
    got = run_transposed(g, sel, I["gate"], g_t, 3)
    want = np.zeros((g.n, 3), bool)
    want[np.ix_(g.np_indices[g.np_indptr[i]:g.np_indptr[i + 1]], sel[i])] = True
    assert np.array_equal(np.isnan(got).all(2), want) and np.array_equal(np.isnan(got).any(2), want)


# ---------------------------------------------------------------------------------------------------------
# fused against unfused, and the calibrator
# ---------------------------------------------------------------------------------------------------------
def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


_cases = {}


def case(name):
    if name not in _cases:
        c = R.load_case(os.path.join(GOLDEN, name + ".npz"))
        c["meta"] = manifest()["cases"][name]
        c["P"] = R.case_params(c)
        _cases[name] = c
    return _cases[name]


def calibrator(c, adj_kind, base_cls=None):
    """the fixture's trained calibrator: adj_kind "dense" builds the experts' graph from the dense adjacency,
    "graph" takes a prebuilt SymNormGraph and gives the base model its own sparse operator"""
    P, kw = c["P"], dict(c["meta"]["keywords"])
    nhid, nfeat = P["base_model.gc1.weight"].shape
    ncls = P["base_model.gc2.weight"].shape[0]
    base = (base_cls or wats_hip.SparseCompatibleGCN)(nfeat=nfeat, nclass=ncls, nhid=nhid)
    adj = c["adj"].to(DEV)
    graph = wats_hip.SymNormGraph(adj) if adj_kind == "graph" else None
    cal = wats_hip.GETSCalibrator(base, ncls, None, None, graph=graph, **kw)
    cal.fit(adj, c["x"], c["y"], [None, c["val_mask"].bool(), None], train=False)
    assert set(cal.state_dict()) == set(P)      # the reference's names, the base model's among them
    cal.load_state_dict(P)
    cal.eval()
    return cal, (wats_hip.RowNormalizedAdjacency.from_dense(adj) if adj_kind == "graph" else adj)


def close(got, want, tol, what):
    d = float((got.detach().double().cpu() - want.double()).abs().max())
    print(f"{what}: distance {d:.3e}, tolerance {tol:.3e}")
    assert d <= tol, (what, d, tol)


@pytest.mark.parametrize("adj_kind", ["dense", "graph"])
@pytest.mark.parametrize("name", ["iso120", "wide96"])
def test_calibrator_reproduces_the_reference(name, adj_kind):
    c = case(name)
    rec = c["meta"]["f32_vs_f64"]
    cal, adj = calibrator(c, adj_kind)
    x = c["x"].to(DEV)
    what = f"{name} {adj_kind}"
    probe = wats_hip.EdgeProbe(c["grad_rows"], c["grad_cols"])
    out = cal(x, adj, probe=probe)
    close(out, c["out"], 4 * rec["out"], what + " out")
    close(cal.last_gates, c["gates"], 4 * rec["gates"], what + " gates")
    assert torch.equal(cal.last_selection.cpu(), c["sel"])
    (out * c["loss_weight"].to(DEV)).sum().backward()
    close(probe.grad, c["grad"], 4 * rec["grad"], what + " adjacency gradient")
    # one train-mode forward with the recorded noise, no dropout, the base model in eval mode
    cal.train()
    cal.base_model.eval()
    for expert in cal.experts:
        expert.dropout_rate = 0.0
    cal.gating_noise = c["noise"].to(DEV)
    with torch.no_grad():
        train_out = cal(x, adj)
    close(train_out, c["train_out"], 4 * rec["train_out"], what + " train-mode out")
    close(cal.last_gates, c["train_gates"], 4 * rec["train_gates"], what + " train-mode gates")
    assert torch.equal(cal.last_selection.cpu(), c["train_sel"])
    close(cal.aux_loss.reshape(-1), c["aux_loss"], 4 * rec["aux_loss"], what + " aux_loss")


def test_calibrator_on_a_dense_base_model():
    from models import CompatibleGCN
    c = case("wide96")
    cal, adj = calibrator(c, "dense", CompatibleGCN)
    with torch.no_grad():
        out = cal(c["x"].to(DEV), adj)
    close(out, c["out"], 4 * c["meta"]["f32_vs_f64"]["out"], "dense base model out")


def test_fused_head_equals_the_unfused_mixture():
    """T of the fused head against sum_e gates_e * GCNExpert.forward_e in float32, in units of T: k + 2 roundings"""
    c = case("iso120")
    cal, adj = calibrator(c, "dense")
    x = c["x"].to(DEV)
    k = cal.k
    with torch.no_grad():
        logits = cal.base_model(x, adj)
        gates, _, sel, top = cal._gating(cal.gating_input(x, logits), False)
        gates, top = gates.float(), top.float()      # what the head and the float32 composition receive
        z = torch.stack([e.last_linear(logits, x) for e in cal.experts], dim=1).contiguous()
        bias = torch.stack([e.convs[-1].bias for e in cal.experts]).contiguous()
        _, t_fused, _ = gets.gated_forward(cal.graph, z, sel.to(torch.int32).contiguous(), top.contiguous(), bias,
                                           logits.contiguous(), True)
        unfused = torch.stack([e(logits, x) for e in cal.experts], dim=1)
        t_unfused = (unfused * gates.unsqueeze(-1)).sum(dim=1)
    I = dict(z=z.cpu().numpy(), sel=sel.cpu().numpy().astype(np.int32), gate=top.cpu().numpy(),
             bias=bias.cpu().numpy(), logits=logits.cpu().numpy())
    ref = R.forward(cal.graph.indptr.cpu().numpy(), cal.graph.indices.cpu().numpy().astype(np.int64),
                    cal.graph.dinv.cpu().numpy(), **I)["t_save"]
    assert ref.c(t_fused.cpu().numpy(), "fused T") <= ref.bound
    diff = np.abs(t_fused.cpu().double().numpy() - t_unfused.cpu().double().numpy())
    assert not diff[ref.unit == 0].any()
    c_rel = float((diff[ref.unit > 0] / ref.unit[ref.unit > 0]).max())
    print(f"fused T against the unfused mixture: c = {c_rel:.4f} (bound {k + 2}); the composition's model (mutant b): "
          f"{ref.c(ref.mutant_b):.4f}")
    assert c_rel <= k + 2 + R.SLACK


def test_fit_lowers_the_loss_and_leaves_the_degree_embeddings_alone():
    src, dst, n, y = cagcn_ref.cora_like_edges()
    torch.manual_seed(0)
    adj = torch.zeros(n, n)
    adj[torch.from_numpy(src), torch.from_numpy(dst)] = 1.0
    x = torch.randn(n, 24) + torch.nn.functional.one_hot(torch.from_numpy(y), 24).float()
    val = torch.zeros(n, dtype=torch.bool)
    val[torch.randperm(n)[:500]] = True
    base = wats_hip.SparseCompatibleGCN(nfeat=24, nclass=7, nhid=16)
    with torch.no_grad():
        base.gc2.weight.mul_(30.0)      # an overconfident base model: something to calibrate
    cal = wats_hip.GETSCalibrator(base, 7, hidden_dim=32, feature_hidden_dim=16, degree_hidden_dim=8)
    cal.fit(adj.to(DEV), x, torch.from_numpy(y), [None, val, None], train=False)
    before = {key: v.detach().clone() for key, v in cal.named_parameters() if "degree_embedder" in key}
    assert len(before) == 2 and all(p.requires_grad for key, p in cal.named_parameters() if key in before)
    cal.calib_train(epochs=40)
    h = cal.history
    print(f"GETS on a Cora-shaped graph: loss {h[0]:.4f} -> {h[-1]:.4f} in {len(h)} epochs")
    assert len(h) >= 10 and np.isfinite(h).all() and min(h[-3:]) < h[0]
    after = dict(cal.named_parameters())
    for key, v in before.items():
        assert torch.equal(v.view(torch.int32), after[key].detach().view(torch.int32)), key
    moved = [key for key, v in cal.named_parameters() if key.startswith("experts.0.convs") and v.grad is not None]
    assert moved
    out = cal(x, adj.to(DEV))
    assert out.shape == (n, 7) and float(out.detach().exp().sum(1).sub(1).abs().max()) < 1e-5


def test_calibrate_with_gets_builds_and_fits():
    c = case("wide96")
    P = c["P"]
    nhid, nfeat = P["base_model.gc1.weight"].shape
    base = wats_hip.SparseCompatibleGCN(nfeat=nfeat, nclass=8, nhid=nhid)
    torch.manual_seed(1)
    cal = wats_hip.calibrate_with_gets(base, c["x"], c["y"], c["adj"].to(DEV), c["val_mask"].bool(), hidden_dim=32)
    assert isinstance(cal, wats_hip.GETSCalibrator) and cal.num_classes == 8 and len(cal.history) >= 1
