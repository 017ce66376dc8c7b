"""The float64-sum aggregation kernels against a float64 truth in ROW units (tests/agg_ref.py).

csrc/symnorm.hip, edgeagg.hip, gats.hip, sddmm.hip and flips.hip promise float64 products and sums rounded once to
float32.  Their own tests allow twice the error of a torch float32 restatement, or 1e-5 of the tensor's maximum: a
kernel that summed every row in float32 passes those (tests/test_agg_precision_host.py shows it), and a hub's row or
a large-norm row hides every other.  Here every output element is measured against its own absolute sum,
  c = max |got - truth| / unit,   unit = 2^-24 * (the expression with every added term replaced by its absolute value)
and the bounds count the roundings the headers document, never a kernel's output (agg_ref's docstring):
  wg_symnorm_aggregate, wg_edge_aggregate, wg_gat_forward, wg_gat_backward, wg_sddmm, wg_rowdot     c <= 1
  wg_edge_pair_inv_distance        |got - truth| <= 2^-24 |truth|
  wg_flip_rows (touched rows)      c <= 2   + the float32 quotient a' / deg'
  the view's backward              c <= 4   scaled g, the parent's stored a / deg, its float32 gx, wg_flip_cols
each plus 1e-3 for the float64 accumulation.  The truth is computed on exactly the float32 inputs the kernel receives:
dinv, the long-row lists, 1 / deg, deg' and the overlay are read from the wrappers' objects, never recomputed.
Graphs: gats_ref.star_graph(700, 50) (a hub row longer than a workgroup pass beside leaves), random graphs, rows of
thr - 1, thr, thr + 1 entries around each kernel's own threshold, empty rows; widths 1 .. 260; a normal, a positive
and a "spread" signal (rows over six orders of magnitude).  wg_gat_* compute a long row only from the caller's list
(csrc/gats.hip pick_row), so the unlisted-long-row case exists for symnorm and edge_aggregate alone.
"""
import numpy as np
import pytest
import torch

import agg_ref as A
import cheb_ref as C

pytestmark = pytest.mark.gpu

import wats_hip  # noqa: E402
from wats_hip import cagcn, dcgc, gats  # noqa: E402
from wats_hip._lib import ptr  # noqa: E402
from wats_hip.gcn import RowNormalizedAdjacency, propagate, rowdot, sddmm  # noqa: E402

DEV = "cuda"
CASES = A.cases()
IDS = [f"{g}-{w}-{k}" for g, w, k in CASES]
MISALIGNED_AT = (4, 64, 256)   # the widths that take 16-byte loads from an aligned base


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def _lib():
    return wats_hip._lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _np(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _misaligned(t):
    """the same values 4 bytes past a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def seed_of(gname, w, kind):
    return 1000 * A.GRAPHS.index(gname) + 10 * w + A.KINDS.index(kind)


class Record:
    """every measurement printed beside its bound; the assertion after the last one, so a failing case shows all"""

    def __init__(self):
        self.bad = []

    def add(self, what, got, ref):
        c = ref.c(_np(got) if torch.is_tensor(got) else got, what)
        try:
            C.report(what, c, ref.bound)
        except AssertionError as e:
            self.bad.append(str(e))

    def check(self):
        assert not self.bad, "\n".join(self.bad)


# ------------------------------------------------------------------------------- graphs, once per module
_GRAPHS = {}


def threshold(family):
    return {"symnorm": cagcn.symnorm_long_row_threshold, "gat": gats.long_row_threshold,
            "edge": lambda: int(_lib().wg_edge_aggregate_long_row())}[family]()


def graph(gname, family):
    """(device object, indptr, indices, n): the object's own CSR, checked against numpy's"""
    if (gname, family) not in _GRAPHS:
        loops = family != "edge"
        src, dst, n = A.graph_edges(gname, threshold(family), loops)
        if family == "edge":   # row = destination, column = source; the self loops of the input stay
            g = wats_hip.EdgeWeightGraph(torch.from_numpy(np.stack([dst, src])), n, DEV)
        else:
            ei = torch.from_numpy(np.stack([src, dst]))
            g = cagcn.SymNormGraph(ei, n, DEV) if family == "symnorm" else gats.AttentionGraph(ei, n, True, DEV)
        ip, ix = _np(g.indptr).astype(np.int64), _np(g.indices).astype(np.int64)
        want_ip, want_ix = A.by_destination(src, dst, n, loops)
        assert np.array_equal(ip, want_ip) and np.array_equal(ix, want_ix)
        lens, thr = np.diff(ip), threshold(family)
        assert np.array_equal(_np(g.long_rows), np.flatnonzero(lens >= thr))
        if gname == "threshold":
            assert list(lens[:3]) == [thr - 1, thr, thr + 1] and lens.min() == (0 if family == "edge" else 1)
        if gname == "star":
            assert lens[0] > 2 * thr
        _GRAPHS[(gname, family)] = (g, ip, ix, n)
    return _GRAPHS[(gname, family)]


def other_list(g, ip, thr):
    """the caller's list without its first long row and with a short row instead (ascending, as the header asks)"""
    lens = np.diff(ip)
    longs = np.flatnonzero(lens >= thr)
    short = np.flatnonzero((lens > 0) & (lens < thr))[-1]
    rows = np.sort(np.concatenate([longs[1:], [short]])).astype(np.int32)
    assert longs.size and longs[0] not in rows
    return _dev(rows)


# ------------------------------------------------------------------------------- wg_symnorm_aggregate
def symnorm_raw(g, indptr, indices, long_rows, x, bias, relu):
    out = torch.full_like(x, float("nan"))
    rc = _lib().wg_symnorm_aggregate(g.n, g.nnz, ptr(indptr), ptr(indices), int(long_rows.numel()), ptr(long_rows),
                                     ptr(g.dinv), x.shape[1], ptr(x), ptr(bias), int(relu), ptr(out), _stream())
    assert rc == 0, _lib().wg_last_error()
    return out


@pytest.mark.parametrize("gname,w,kind", CASES, ids=IDS)
def test_symnorm(gname, w, kind):
    g, ip, ix, n = graph(gname, "symnorm")
    s = seed_of(gname, w, kind)
    x, bias = A.signal(n, w, kind, s), A.signal(1, w, kind, s + 1)[0]
    dinv = _np(g.dinv)
    xd, bd = _dev(x), _dev(bias)
    rec, what = Record(), f"symnorm {gname} C={w} {kind}"
    plain, full = A.symnorm(ip, ix, dinv, x), A.symnorm(ip, ix, dinv, x, bias, True)
    rec.add(what, cagcn.sym_norm_aggregate(g, xd), plain)
    rec.add(what + " bias relu", cagcn.sym_norm_aggregate(g, xd, bd, True), full)
    t_ip, order = A.transpose_order(ip, ix)
    assert np.array_equal(_np(g.t_indptr), t_ip)
    grad = A.symnorm(t_ip, A.row_ids(ip)[order], dinv, x)
    leaf = xd.clone().requires_grad_(True)
    cagcn.sym_norm_aggregate(g, leaf).backward(xd)    # the gradient: the transposed call on the upstream gradient
    rec.add(what + " transposed (the gradient)", leaf.grad, grad)
    if w in MISALIGNED_AT:
        rec.add(what + " misaligned x", g.aggregate(_misaligned(xd), bd, True), full)
    if gname in ("star", "threshold"):
        rows = other_list(g, ip, threshold("symnorm"))
        rec.add(what + " a long row unlisted, a short row listed",
                symnorm_raw(g, g.indptr, g.indices, rows, xd, bd, True), full)
    rec.check()


# ------------------------------------------------------------------------------- wg_edge_aggregate
def edge_raw(g, transposed, long_rows, val, rs, cs, x):
    indptr, indices, pos = (g.t_indptr, g.t_indices, g.t_pos) if transposed else (g.indptr, g.indices, None)
    out = torch.full_like(x, float("nan"))
    rc = _lib().wg_edge_aggregate(g.n, g.nnz, ptr(indptr), ptr(indices), int(long_rows.numel()), ptr(long_rows),
                                  ptr(val), ptr(pos), ptr(rs), ptr(cs), x.shape[1], ptr(x), ptr(out), _stream())
    assert rc == 0, _lib().wg_last_error()
    return out


@pytest.mark.parametrize("gname,w,kind", CASES, ids=IDS)
def test_edge_aggregate(gname, w, kind):
    g, ip, ix, n = graph(gname, "edge")
    s = seed_of(gname, w, kind)
    rng = np.random.default_rng(s)
    val = (rng.random(len(ix)) + 0.1).astype(np.float32)
    scale = (rng.random(n) + 0.5).astype(np.float32)
    x = A.signal(n, w, kind, s + 2)
    vd, sd, xd = _dev(val), _dev(scale), _dev(x)
    rows = A.row_ids(ip)
    t_ip, order = A.transpose_order(ip, ix)
    assert np.array_equal(_np(g.t_indptr), t_ip) and np.array_equal(_np(g.t_pos), order)
    rec, what = Record(), f"edge_aggregate {gname} C={w} {kind}"
    for rs, cs in ((True, False), (False, False), (True, True)):
        ref = A.edge_aggregate(ip, ix, val, None, scale if rs else None, scale if cs else None, x)
        rec.add(f"{what} row_scale={rs} col_scale={cs}", g._aggregate(False, vd, sd if rs else None, sd if cs else None, xd), ref)
    for cs in (True, False):
        ref = A.edge_aggregate(t_ip, rows[order], val, order, None, scale if cs else None, x)
        rec.add(f"{what} transposed (map) col_scale={cs}", g._aggregate(True, vd, None, sd if cs else None, xd), ref)
    both = A.edge_aggregate(ip, ix, val, None, scale, scale, x)
    if w in MISALIGNED_AT:
        rec.add(what + " misaligned x", g._aggregate(False, vd, sd, sd, _misaligned(xd)), both)
    if gname in ("star", "threshold"):
        lst = other_list(g, ip, threshold("edge"))
        rec.add(what + " a long row unlisted, a short row listed", edge_raw(g, False, lst, vd, sd, sd, xd), both)
        t_lst = other_list(g, t_ip, threshold("edge"))
        rec.add(what + " transposed, a long row unlisted, a short row listed", edge_raw(g, True, t_lst, vd, None, sd, xd),
                A.edge_aggregate(t_ip, rows[order], val, order, None, scale, x))
    rec.check()


@pytest.mark.parametrize("gname,w,kind", [c for c in CASES if c[1] in (5, 64, 260) or c[0] != "star"],
                         ids=[i for c, i in zip(CASES, IDS) if c[1] in (5, 64, 260) or c[0] != "star"])
def test_weighted_propagate(gname, w, kind):
    """the wrapper: y = (sum_c w_rc x_c) / deg_r, its gradient w.r.t. x (transposed, col_scale = 1 / deg) and w.r.t.
    w (wg_sddmm on wg_rowdot's float32 result).  The truth divides by the float32 1 / deg the wrapper passes."""
    g, ip, ix, n = graph(gname, "edge")
    s = seed_of(gname, w, kind)
    val = (np.random.default_rng(s).random(len(ix)) + 0.1).astype(np.float32)
    val[ip[5]:ip[6]] = 0       # a row whose weights are all zero: deg -> 1, y = 0
    x, gy = A.signal(n, w, kind, s + 2), A.signal(n, w, kind, s + 3)
    vd, xd, gd = _dev(val).requires_grad_(True), _dev(x).requires_grad_(True), _dev(gy)
    inv_d = 1.0 / g.degree(vd.detach())      # _WeightedPropagate.forward's own expression
    inv = _np(inv_d)
    y = wats_hip.weighted_propagate(g, vd, xd)
    y.backward(gd)
    rows = A.row_ids(ip)
    t_ip, order = A.transpose_order(ip, ix)
    rec, what = Record(), f"weighted_propagate {gname} C={w} {kind}"
    rec.add(what + " y", y, A.edge_aggregate(ip, ix, val, None, inv, None, x))
    rec.add(what + " grad x", xd.grad, A.edge_aggregate(t_ip, rows[order], val, order, None, inv, gy))
    term = rowdot(gd, y.detach())             # float32: an input of wg_sddmm
    rec.add(what + " rowdot(g, y)", term, A.rowdot(gy, _np(y)))
    rec.add(what + " grad w", vd.grad, A.sddmm(rows, ix, gy, x, _np(term), inv))
    rec.check()


# ------------------------------------------------------------------------------- wg_gat_forward / wg_gat_backward
@pytest.mark.parametrize("gname,w,kind", CASES, ids=IDS)
def test_attention(gname, w, kind):
    g, ip, ix, n = graph(gname, "gat")
    Hh = A.HEADS[CASES.index((gname, w, kind)) % len(A.HEADS)]
    a, t, conf, gs = A.attention_inputs(n, w, Hh, kind, seed_of(gname, w, kind))
    ad, td, cd, gd = _dev(a).requires_grad_(True), _dev(t).requires_grad_(True), _dev(conf), _dev(gs)
    sim, dconf = wats_hip.edge_softmax_attention(g, ad, td, cd, 0.2)
    sim.backward(gd)
    r_sim, r_dconf = A.gat_forward(ip, ix, a, t, conf)
    r_a, r_t = A.gat_backward(ip, ix, a, t, gs)
    rec, what = Record(), f"gat {gname} C={w} Hh={Hh} {kind}"
    rec.add(what + " sim", sim, r_sim)
    rec.add(what + " dconf", dconf, r_dconf)
    rec.add(what + " grad_a", ad.grad, r_a)
    rec.add(what + " grad_t", td.grad, r_t)
    if w in MISALIGNED_AT:
        am, gm = _misaligned(ad.detach()), _misaligned(gd)
        sim2, dconf2, saved = g.forward(am, td.detach(), cd, 0.2, save=True)
        ga2, gt2 = g.backward(am, td.detach(), saved, gm, 0.2)
        rec.add(what + " misaligned a: sim", sim2, r_sim)
        rec.add(what + " misaligned a: dconf", dconf2, r_dconf)
        rec.add(what + " misaligned a, g_sim: grad_a", ga2, r_a)
        rec.add(what + " misaligned a, g_sim: grad_t", gt2, r_t)
    rec.check()


# ------------------------------------------------------------------------------- wg_sddmm, wg_rowdot, pair distance
@pytest.mark.parametrize("gname,w,kind", CASES, ids=IDS)
def test_pairs(gname, w, kind):
    _, ip, ix, n = graph(gname, "edge")
    rows, cols = np.concatenate([A.row_ids(ip), np.arange(n)]), np.concatenate([ix, np.arange(n)])
    s = seed_of(gname, w, kind)
    Am, Bm, term = A.signal(n, w, kind, s + 3), A.signal(n, w, kind, s + 4), A.signal(n, 1, kind, s + 5)[:, 0]
    scale = (np.random.default_rng(s).random(n) + 0.5).astype(np.float32)
    rd, cd = _dev(rows.astype(np.int32)), _dev(cols.astype(np.int32))
    Ad, Bd = _dev(Am), _dev(Bm)
    rec, what = Record(), f"{gname} F={w} {kind}"
    rec.add("sddmm " + what, sddmm(rd, cd, Ad, Bd, _dev(term), _dev(scale)), A.sddmm(rows, cols, Am, Bm, term, scale))
    plain = A.sddmm(rows, cols, Am, Bm)
    rec.add("sddmm no term, no scale " + what, sddmm(rd, cd, Ad, Bd), plain)
    rec.add("rowdot " + what, rowdot(Ad, Bd), A.rowdot(Am, Bm))
    if w in MISALIGNED_AT:
        rec.add("sddmm misaligned A " + what, sddmm(rd, cd, _misaligned(Ad), Bd), plain)
        rec.add("rowdot misaligned B " + what, rowdot(Ad, _misaligned(Bd)), A.rowdot(Am, Bm))
    # the pair distance on the same pairs (an EdgeWeightGraph merges and sorts them: read them back), with the self
    # loops, a pair of identical rows and a pair that differs in the last bit of one column
    Q, prow, pcol = A.pair_inputs(n, w, kind, s + 6, rows, cols)
    pg = wats_hip.EdgeWeightGraph(torch.from_numpy(np.stack([prow, pcol])), n, DEV)
    prow, pcol = _np(pg.rows).astype(np.int64), _np(pg.cols).astype(np.int64)
    got = _np(dcgc.pair_inv_distance(pg, _dev(Q), 0.5))
    assert np.all(got[prow == pcol] == np.float32(2.0)) and got[(prow == 10) & (pcol == 11)] == np.float32(2.0)
    rec.add("pair_inv_distance " + what, got, A.pair_inv_distance(prow, pcol, Q, 0.5))
    if w in MISALIGNED_AT:
        rec.add("pair_inv_distance misaligned Q " + what, dcgc.pair_inv_distance(pg, _misaligned(_dev(Q)), 0.5),
                A.pair_inv_distance(prow, pcol, Q, 0.5))
    rec.check()


# ------------------------------------------------------------------------------- wg_flip_rows, wg_flip_cols
_OPS = {}


def flip_parent(gname):
    if gname not in _OPS:
        M = A.flip_graph(gname)
        unit = bool(np.all(M.data == 1))
        _OPS[gname] = RowNormalizedAdjacency(M.shape[0], torch.from_numpy(M.indptr.astype(np.int64)),
                                             torch.from_numpy(M.indices.astype(np.int32)),
                                             None if unit else torch.from_numpy(M.data.astype(np.float32)))
        assert np.array_equal(_np(_OPS[gname].deg), A.parent_degree(M))
    return _OPS[gname]


FLIPS = [("hub_64_symmetric", F, "positive") for F in A.WIDTHS]
FLIPS += [(name, F, kind) for name in A.FLIP_CASES for kind in A.KINDS for F in (5, 64) if (name, F, kind) not in FLIPS]


@pytest.mark.parametrize("name,F,kind", FLIPS, ids=[f"{n_}-{F}-{k}" for n_, F, k in FLIPS])
def test_flip_views(name, F, kind):
    """through RowNormalizedAdjacency.with_flips and propagate: the touched rows of the forward against the flipped
    row, every other row bitwise the parent's wg_spmm (held in test_step_precision.py), and the backward against
    the three steps of wats_hip/flips.py.  The overlay and deg' are the view's own."""
    gname, rows, cols, symmetric = A.flip_case(name)
    M, op = A.flip_graph(gname), flip_parent(gname)
    view = op.with_flips(rows, cols, symmetric)
    ov = dict(rows=view._rows.numpy(), cols=view._cols.numpy(), a_old=view._a_old.numpy(), a_new=view._a_new.numpy(),
              t_rows=_np(view._dev["t_rows64"]), deg_new=_np(view._dev["deg_new"]))
    want = A.flip_overlay(M, rows, cols, symmetric)
    for k in ("rows", "cols", "a_old", "a_new", "t_rows"):
        assert np.array_equal(ov[k], want[k]), k
    x, gy = A.signal(M.shape[0], F, kind, 7 * F + A.KINDS.index(kind)), A.signal(M.shape[0], F, kind, 7 * F + 5)
    rec, what = Record(), f"flip {name} F={F} {kind}"
    r_rows, r_back = A.flip_rows(M, ov, x), A.flip_backward(M, ov, gy)
    untouched = np.setdiff1d(np.arange(M.shape[0]), ov["t_rows"])

    def forward(y, parent, tag):
        assert np.array_equal(_np(y)[untouched].view(np.int32), _np(parent)[untouched].view(np.int32))
        rec.add(f"{what} touched rows{tag}", _np(y)[ov["t_rows"]], r_rows)

    xd, gd = _dev(x).requires_grad_(True), _dev(gy)
    y = propagate(view, xd)
    forward(y, propagate(op, xd.detach()), "")
    y.backward(gd)
    rec.add(f"{what} backward", xd.grad, r_back)
    if F in MISALIGNED_AT:   # the operators themselves: autograd would hand an aligned copy on
        xm, gm = _misaligned(xd.detach()), _misaligned(gd)
        forward(view.fwd.apply(xm), op.fwd.apply(xm), " misaligned x")
        rec.add(f"{what} backward misaligned g", view.bwd.apply(gm), r_back)
    rec.check()
