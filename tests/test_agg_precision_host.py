"""The row-unit method of tests/test_agg_precision.py, pinned without a GPU (tests/agg_ref.py).

For every operation and every case of the GPU test (agg_ref.cases(), agg_ref.FLIP_CASES):
  * the truth agrees with its second evaluation (float64 np.add.reduceat against sequential np.longdouble) within
    agg_ref.TRUTH_AGREE units: the yardstick is not the source of an error;
  * the arithmetic the kernel headers document (float64 sums, the documented roundings) is within its bound;
  * on the positive signal (|N(0, 1)| + 0.5) the same expression with ONE sequential float32 accumulator is above the
    bound -- the GPU test rejects a kernel that sums a row in float32 -- and
  * that same mutant PASSES the yardstick of the kernel's existing test file: gats_ref.error_bound against a torch
    float32 restatement (test_cagcn.py, test_dcgc.py, test_gats.py) or 1e-5 * max|ref| (test_edge_grad.py,
    test_flip_view.py).  That last assertion is the record of the gap the row units close.
Where a case cannot show a float32 accumulator for certain (C = 1 on the star, where the hub's one sum is the only
long chain and may round well by chance; a pair of fewer than 5 columns; the flip case on the weighted graph, whose
rows hold about nine entries against a bound of 2 and 4) the mutant's figure is printed and not asserted.
"""
import numpy as np
import pytest
import torch

import agg_ref as A
import cagcn_ref
import cheb_ref as C
import gats_ref as G

CASES = A.cases()
IDS = [f"{g}-{w}-{k}" for g, w, k in CASES]
HOST_THRESHOLD = {"symnorm": 128, "edge": 128, "gat": 256}   # numpy has no paths: the GPU test reads the kernels' own
_CSR = {}


def csr(gname, family):
    """(indptr, indices, n) by destination; symnorm and gat with the calibrators' self-loop step"""
    loops = family != "edge"
    key = (gname, family if gname == "threshold" else loops)
    if key not in _CSR:
        src, dst, n = A.graph_edges(gname, HOST_THRESHOLD[family], loops)
        _CSR[key] = (*A.by_destination(src, dst, n, loops), n)
    return _CSR[key]


def seed_of(gname, w, kind):
    return 1000 * A.GRAPHS.index(gname) + 10 * w + A.KINDS.index(kind)


def check(what, ref, kind, mutant_shows=True, old=None, old_holds=True, w=None):
    """the three assertions of the module docstring for one Ref; old(mutant) -> (passes, text) is the old yardstick
    (old_holds False: printed, not asserted); w: the width of a graph aggregation"""
    agree = ref.agreement()
    assert agree <= A.TRUTH_AGREE, f"{what}: truth and second evaluation are {agree:.2e} units apart"
    cm = ref.c(ref.mutant, what + " mutant")
    C.report(f"{what} model", ref.c(ref.model, what + " model"), ref.bound, f"(float32-sum mutant {cm:.2f})")
    if kind == "positive" and mutant_shows and (w is None or w >= 3):
        assert cm > ref.bound, f"{what}: the float32-sum mutant is at {cm:.3f}, inside the bound {ref.bound:.3f}"
        if old is not None:
            ok, text = old(ref.mutant)
            print(f"{what} mutant against the old yardstick: {text}")
            assert ok or not old_holds, f"{what}: the float32-sum mutant no longer passes the old yardstick ({text})"


def old_error_bound(ref32, ref64):
    """gats_ref.assert_close's rule: max|got - ref64| <= max(2 max|ref32 - ref64|, 4 * 2^-24 max|ref64|)"""
    ref32, ref64 = torch.as_tensor(np.asarray(ref32)), torch.as_tensor(np.asarray(ref64))
    bound, err32 = G.error_bound(ref32, ref64)

    def old(mutant):
        err = float(np.abs(np.asarray(mutant, np.float64).reshape(ref64.shape) - ref64.numpy()).max())
        return err <= bound, f"err={err:.3e} bound={bound:.3e} (err32 {err32:.3e})"
    return old


def old_rel_tol(truth, tol=1e-5):
    """test_edge_grad.py / test_flip_view.py: max|got - ref| / max|ref| <= 1e-5"""
    def old(mutant):
        err = float(np.abs(np.asarray(mutant, np.float64).reshape(truth.shape) - truth).max() / np.abs(truth).max())
        return err <= tol, f"max err / max|ref| = {err:.3e} (bound {tol:g})"
    return old


def test_the_table_of_the_issue():
    """the figures this work started from: symnorm on star_graph(700, 50), C = 7, in row units and in the old scale"""
    ip, ix, n = csr("star", "symnorm")
    dinv = (np.diff(ip).astype(np.float32) ** np.float32(-0.5)).astype(np.float32)
    for kind, lo in (("normal", 1.2), ("positive", 5.0)):
        ref = A.symnorm(ip, ix, dinv, A.signal(n, 7, kind, 1))
        cm, c_old = ref.c(ref.mutant), float(np.abs(ref.mutant - ref.truth).max() / (A.EPS * np.abs(ref.truth).max()))
        print(f"star {kind}: model c={ref.c(ref.model):.3f} mutant c={cm:.2f}, in 2^-24 max|ref|: {c_old:.2f}")
        assert ref.c(ref.model) <= A.BOUND_ONE and cm > lo


def test_threshold_graph_has_the_three_row_lengths():
    for family, thr in HOST_THRESHOLD.items():
        ip, ix, n = csr("threshold", family)
        lens = np.diff(ip)
        assert list(lens[:3]) == [thr - 1, thr, thr + 1] and lens.min() == (0 if family == "edge" else 1)
        t_ip, _ = A.transpose_order(ip, ix)
        assert list(np.diff(t_ip)[:3]) == [thr - 1, thr, thr + 1]


@pytest.mark.parametrize("gname,w,kind", CASES, ids=IDS)
def test_symnorm(gname, w, kind):
    ip, ix, n = csr(gname, "symnorm")
    rows = A.row_ids(ip)
    dinv = (np.diff(ip).astype(np.float32) ** np.float32(-0.5)).astype(np.float32)
    s = seed_of(gname, w, kind)
    x, bias = A.signal(n, w, kind, s), A.signal(1, w, kind, s + 1)[0]
    xt, dt = torch.from_numpy(x), torch.from_numpy(dinv)

    def old(src, dst, b, relu):
        return old_error_bound(*(cagcn_ref.sym_norm_edges(src, dst, xt, dt, None if b is None else torch.from_numpy(b),
                                                          relu, d).numpy() for d in (torch.float32, torch.float64)))
    positive = kind == "positive"
    check(f"symnorm {gname} C={w} {kind}", A.symnorm(ip, ix, dinv, x), kind, old=old(ix, rows, None, False) if positive else None, w=w)
    check(f"symnorm bias relu {gname} C={w} {kind}", A.symnorm(ip, ix, dinv, x, bias, True), kind,
          old=old(ix, rows, bias, True) if positive else None, w=w)
    t_ip, order = A.transpose_order(ip, ix)
    check(f"symnorm transposed {gname} C={w} {kind}", A.symnorm(t_ip, rows[order], dinv, x), kind,
          old=old(rows, ix, None, False) if positive else None, w=w)


@pytest.mark.parametrize("gname,w,kind", CASES, ids=IDS)
def test_edge_aggregate(gname, w, kind):
    ip, ix, n = csr(gname, "edge")
    rows = A.row_ids(ip)
    s = seed_of(gname, w, kind)
    rng = np.random.default_rng(s)
    val = (rng.random(len(ix)) + 0.1).astype(np.float32)
    scale = (rng.random(n) + 0.5).astype(np.float32)
    x = A.signal(n, w, kind, s + 2)
    t_ip, order = A.transpose_order(ip, ix)

    def old(transposed, rs, cs):
        refs = []
        for d in (torch.float32, torch.float64):
            a = torch.zeros(n, n, dtype=d).index_put((torch.from_numpy(rows), torch.from_numpy(ix)),
                                                     torch.from_numpy(val).to(d))
            y = torch.from_numpy(x).to(d)
            y = (a.t() if transposed else a) @ (y * torch.from_numpy(scale).to(d).unsqueeze(1) if cs else y)
            refs.append((y * torch.from_numpy(scale).to(d).unsqueeze(1) if rs else y).numpy())
        return old_error_bound(*refs)
    positive = kind == "positive"
    # test_dcgc.py's float32 restatement is a dense torch product, whose blocked sums are closer to float64 than one
    # sequential chain: on the star it catches the mutant's hub row of 700 terms in some cases (never a leaf, which
    # the hub's scale hides), so the old yardstick's verdict is printed there and asserted on the other graphs
    holds = gname != "star"
    for rs, cs in ((True, False), (False, False), (True, True)):
        check(f"edge_aggregate {gname} C={w} {kind} row_scale={rs} col_scale={cs}",
              A.edge_aggregate(ip, ix, val, None, scale if rs else None, scale if cs else None, x), kind,
              old=old(False, rs, cs) if positive else None, old_holds=holds, w=w)
    for rs, cs in ((False, True), (False, False)):
        check(f"edge_aggregate transposed {gname} C={w} {kind} row_scale={rs} col_scale={cs}",
              A.edge_aggregate(t_ip, rows[order], val, order, None, scale if cs else None, x), kind,
              old=old(True, rs, cs) if positive else None, old_holds=holds, w=w)


@pytest.mark.parametrize("gname,w,kind", CASES, ids=IDS)
def test_attention(gname, w, kind):
    ip, ix, n = csr(gname, "gat")
    rows = A.row_ids(ip)
    Hh = A.HEADS[CASES.index((gname, w, kind)) % len(A.HEADS)]
    a, t, conf, g = A.attention_inputs(n, w, Hh, kind, seed_of(gname, w, kind))
    sim, dconf = A.gat_forward(ip, ix, a, t, conf)
    grad_a, grad_t = A.gat_backward(ip, ix, a, t, g)
    olds = [None] * 4
    if kind == "positive":
        res = []
        for d in (torch.float32, torch.float64):
            al, tl = (torch.from_numpy(v).to(d).requires_grad_(True) for v in (a, t))
            s_, dc_ = G.attention_edges(ix, rows, al, tl, torch.from_numpy(conf), 0.2, d)
            (s_ * torch.from_numpy(g).to(d)).sum().backward()
            res.append([v.detach().numpy() for v in (s_, dc_, al.grad, tl.grad)])
        olds = [old_error_bound(r32, r64) for r32, r64 in zip(*res)]
    what = f"{gname} C={w} Hh={Hh} {kind}"
    check(f"gat sim {what}", sim, kind, old=olds[0], w=w)
    check(f"gat dconf {what}", dconf, kind, old=olds[1], w=w)
    check(f"gat grad_a {what}", grad_a, kind, old=olds[2], w=w)
    check(f"gat grad_t {what}", grad_t, kind, old=olds[3], w=w)


@pytest.mark.parametrize("gname,w,kind", CASES, ids=IDS)
def test_pairs(gname, w, kind):
    """wg_sddmm, wg_rowdot and wg_edge_pair_inv_distance at the stored entries of the graph without the self-loop step
    plus one self loop per node, a pair of identical rows and a pair that differs in the last bit of one column"""
    ip, ix, n = csr(gname, "edge")
    rows, cols = np.concatenate([A.row_ids(ip), np.arange(n)]), np.concatenate([ix, np.arange(n)])
    s = seed_of(gname, w, kind)
    Am, Bm, term = A.signal(n, w, kind, s + 3), A.signal(n, w, kind, s + 4), A.signal(n, 1, kind, s + 5)[:, 0]
    scale = (np.random.default_rng(s).random(n) + 0.5).astype(np.float32)
    shows = w >= 5
    ref = A.sddmm(rows, cols, Am, Bm, term, scale)
    check(f"sddmm {gname} F={w} {kind}", ref, kind, shows, old_rel_tol(ref.truth))
    ref = A.sddmm(rows, cols, Am, Bm)
    check(f"sddmm no term {gname} F={w} {kind}", ref, kind, shows, old_rel_tol(ref.truth))
    ref = A.rowdot(Am, Bm)
    check(f"rowdot {gname} F={w} {kind}", ref, kind, shows, old_rel_tol(ref.truth))
    Q, prow, pcol = A.pair_inputs(n, w, kind, s + 6, rows, cols)
    ref = A.pair_inv_distance(prow, pcol, Q, 0.5)
    loops = prow == pcol
    assert np.all(ref.model[loops] == np.float32(2.0)) and ref.model[-2] == np.float32(2.0)   # exactly 1 / alpha
    assert ref.truth[-1] < 2.0
    # 1 / (|d| + alpha) hardly moves with the sum's last bits (the square root halves them, alpha dilutes them): the
    # mutant is above the bound from 64 columns on, by less than 1.5 x, and is asserted there only
    check(f"pair_inv_distance {gname} C={w} {kind}", ref, kind, mutant_shows=w >= 64)


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("F", [5, 64])
@pytest.mark.parametrize("name", A.FLIP_CASES)
def test_flip_views(name, F, kind):
    gname, rows, cols, symmetric = A.flip_case(name)
    M = A.flip_graph(gname)
    ov = A.flip_overlay(M, rows, cols, symmetric)
    x = A.signal(M.shape[0], F, kind, 7 * F + A.KINDS.index(kind))
    shows = gname == "hub"   # the weighted graph's rows hold about nine entries
    ref = A.flip_rows(M, ov, x)
    check(f"flip rows {name} F={F} {kind}", ref, kind, shows, old_rel_tol(ref.truth))
    ref = A.flip_backward(M, ov, x)
    check(f"flip backward {name} F={F} {kind}", ref, kind, shows, old_rel_tol(ref.truth))
