"""Float64 truth, row-wise error units, models and float32-sum mutants of the aggregation kernels that promise
"every product and sum is float64, rounded once" (csrc/symnorm.hip, edgeagg.hip, gats.hip, sddmm.hip, flips.hip), numpy
only.  Helpers of tests/test_agg_precision_host.py and tests/test_agg_precision.py; not a test.

Every operation returns a Ref:
  truth    the value on exactly the float32 inputs the kernel receives (dinv, row_scale, val, a_new, deg_new, ... are
           inputs, never recomputed), summed sequentially in np.longdouble and stored as float64
  second   the same in float64 by np.add.reduceat (another order, another format): Ref.agreement() is their distance
           in units, which the host test holds below TRUTH_AGREE so that the yardstick is not the source of an error
  unit     2^-24 times the same expression with every added term replaced by its absolute value, per output element
  model    the arithmetic the kernel's header documents: float64 accumulation, the documented roundings, nothing else
  mutant   WRONG on purpose: the same with one sequential float32 accumulator in entry order
  bound    on c = max |got - truth| / unit (cheb_ref.c_of; an element whose unit is 0 must be exact)

Bounds count the roundings in the headers, never a kernel's output.  One rounding of a float64 v to float32 errs by
at most 2^-24 |v| and |v| <= unit / 2^-24, so one rounding is c <= 1; the 1e-3 on top pays for the float64
accumulation (rows of up to 2^16 terms: 2^16 * 2^-53 = 2^-37 of the absolute sum, 2^-13 of a unit).

  BOUND_ONE        1   symnorm, edge_aggregate, gat forward / backward, sddmm, rowdot, pair_inv_distance (relative)
  BOUND_FLIP_ROWS  2   + the float32 quotient a' / deg' (flips.hip flip_rows_kernel), as cheb_ref.BOUND_VALUED
  BOUND_FLIP_COLS  4   the view's backward (wats_hip/flips.py): g_r deg_r / deg'_r rounded to float32 on the touched
                       rows (1), the parent's stored float32 a / deg (2), the parent's wg_spmm result gx rounded to
                       float32 (3), flip_cols' final rounding (4); a column that is in no overlay stops at 3

The attention's logits stay within |d_ij| <= MAX_LOGIT = 1e3: the float64 error of a C-term dot product is then at
most C * 2^-53 * 1e3, which for C = 260 is 2.9e-11 in the exponent, below half of 1e-3 * 2^-24 = 6e-11.
"""
import numpy as np

import cheb_ref as C
import gats_ref as G

EPS = C.EPS
LD = np.longdouble
SLACK = 1e-3
BOUND_ONE = 1.0 + SLACK                      # one rounding of the float64 result
BOUND_FLIP_ROWS = C.BOUND_VALUED + SLACK     # 2: the float32 quotient a' / deg', the result
BOUND_FLIP_COLS = 4.0 + SLACK                # 4: scaled g, stored a / deg, the parent's gx, the result
TRUTH_AGREE = 1e-3
MAX_LOGIT = 1e3
WIDTHS = (1, 3, 4, 5, 7, 64, 65, 256, 260)
HEADS = (1, 8, 9)
KINDS = ("normal", "positive", "spread")

f32, f64 = C.f32, C.f64


class Ref:
    def __init__(self, truth, second, unit, model, mutant, bound):
        self.truth, self.second, self.unit, self.bound = f64(truth), f64(second), f64(unit), bound
        self.model, self.mutant = np.asarray(model, np.float32), np.asarray(mutant, np.float32)

    def c(self, got, what=""):
        return C.c_of(got, self.truth, self.unit, what)

    def agreement(self):
        return C.c_of(self.second, self.truth, self.unit, "second evaluation")

    def rows(self, idx):
        """the same restricted to some output rows"""
        return Ref(*(v[idx] for v in (self.truth, self.second, self.unit, self.model, self.mutant)), self.bound)


# --------------------------------------------------------------------------------------------------- segment sums
def seg_sum(indptr, terms, dtype):
    """per segment [indptr[i], indptr[i + 1]) the sum of terms (nnz, C) in entry order with ONE accumulator of
    `dtype`: acc = dtype(acc + term) per entry (float32: each addition rounded to float32)"""
    indptr = np.asarray(indptr, np.int64)
    n, lens = len(indptr) - 1, np.diff(indptr)
    acc = np.zeros((n, terms.shape[1]), dtype)
    order = np.argsort(-lens, kind="stable")      # the rows longer than k are a prefix
    for k in range(int(lens.max()) if n else 0):
        rows = order[:int(np.count_nonzero(lens > k))]
        acc[rows] = (acc[rows] + terms[indptr[rows] + k]).astype(dtype)
    return acc


def seg_reduce(indptr, terms):
    """the same sums by np.add.reduceat in the dtype of terms (another order)"""
    indptr = np.asarray(indptr, np.int64)
    assert indptr[-1] == len(terms)
    out = np.zeros((len(indptr) - 1, terms.shape[1]), terms.dtype)
    ne = np.flatnonzero(np.diff(indptr) > 0)
    if ne.size:
        out[ne] = np.add.reduceat(terms, indptr[ne], axis=0)
    return out


def seg_max(indptr, v):
    out = np.full(len(indptr) - 1, -np.inf, v.dtype)
    ne = np.flatnonzero(np.diff(indptr) > 0)
    if ne.size:
        out[ne] = np.maximum.reduceat(v, np.asarray(indptr, np.int64)[ne])
    return out


def row_ids(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def transpose_order(indptr, indices):
    """(t_indptr, order): the entries by column, ascending row within a column (wg_csr_transpose_map's t_pos)"""
    indices = np.asarray(indices, np.int64)
    order = np.argsort(indices, kind="stable")
    n = len(indptr) - 1
    return np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=n))]).astype(np.int64), order


def aggregate(indptr, weight, xg, row_scale=None, add=None, relu=False, bound=BOUND_ONE, model_weight=None):
    """out_i = act(row_scale_i * sum over the entries e of segment i of weight_e * xg_e + add_i).
    weight(dtype) -> (nnz,): the exact weight in that format; model_weight(dtype): what the kernel multiplies by where
    that is a rounded number (default: the same); xg (nnz, C) float32; add broadcasts against (n, C)."""
    indptr = np.asarray(indptr, np.int64)
    n = len(indptr) - 1
    xg = np.asarray(xg).reshape(len(xg), -1)
    rs = np.ones((n, 1)) if row_scale is None else f64(row_scale).reshape(n, 1)
    ad = np.zeros((1, 1)) if add is None else f64(add)
    model_weight = model_weight or weight

    def terms(w, dt):
        return np.asarray(w(dt), dt).reshape(-1, 1) * xg.astype(dt)

    def fin(acc, dt):
        return rs.astype(dt) * acc + ad.astype(dt)

    act = (lambda v: np.maximum(v, 0)) if relu else (lambda v: v)
    t64, m64 = terms(weight, np.float64), terms(model_weight, np.float64)
    truth = f64(fin(seg_sum(indptr, terms(weight, LD), LD), LD))
    second = fin(seg_reduce(indptr, t64), np.float64)
    unit = EPS * (np.abs(rs) * seg_reduce(indptr, np.abs(t64)) + np.abs(ad))
    model = f32(fin(seg_sum(indptr, m64, np.float64), np.float64))
    mutant = f32(fin(f64(seg_sum(indptr, m64, np.float32)), np.float64))
    return Ref(act(truth), act(second), unit, act(model), act(mutant), bound)   # a ReLU does not enlarge an error


def _const(v):
    return lambda dt: np.asarray(v, dt)


# --------------------------------------------------------------------------------------------------- the operations
def symnorm(indptr, indices, dinv, x, bias=None, relu=False):
    """wg_symnorm_aggregate: act(dinv_i sum_p dinv_j x_j + bias); the gradient is the same call on the transpose"""
    indices = np.asarray(indices, np.int64)
    return aggregate(indptr, _const(np.asarray(dinv)[indices]), np.asarray(x)[indices], row_scale=dinv,
                     add=None if bias is None else np.asarray(bias).reshape(1, -1), relu=relu)


def edge_aggregate(indptr, indices, val, emap, row_scale, col_scale, x):
    """wg_edge_aggregate: row_scale_i sum_p val[map ? map[p] : p] col_scale[j_p] x[j_p] (either scale None = 1)"""
    indices = np.asarray(indices, np.int64)
    v = np.asarray(val)[np.asarray(emap, np.int64)] if emap is not None else np.asarray(val)
    cs = None if col_scale is None else np.asarray(col_scale)[indices]
    weight = (lambda dt: v.astype(dt)) if cs is None else (lambda dt: v.astype(dt) * cs.astype(dt))
    return aggregate(indptr, weight, np.asarray(x)[indices], row_scale=row_scale)


def sddmm(rows, cols, A, B, term=None, scale=None):
    """wg_sddmm: scale_r (A_r . B_c - term_r); a pair is a segment of F products and, last, the term times -1"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    P, F = len(rows), A.shape[1]
    a, b = np.asarray(A, np.float32)[rows], np.asarray(B, np.float32)[cols]
    if term is not None:
        a = np.concatenate([a, np.asarray(term, np.float32)[rows].reshape(-1, 1)], axis=1)
        b = np.concatenate([b, np.full((P, 1), -1, np.float32)], axis=1)
    ref = aggregate(np.arange(P + 1) * a.shape[1], _const(a.reshape(-1)), b.reshape(-1, 1),
                    row_scale=None if scale is None else np.asarray(scale)[rows])
    for k in ("truth", "second", "unit", "model", "mutant"):
        setattr(ref, k, getattr(ref, k).reshape(-1))
    return ref


def rowdot(A, B):
    """wg_rowdot: A_i . B_i"""
    i = np.arange(A.shape[0])
    return sddmm(i, i, A, B)


def pair_inv_distance(rows, cols, Q, alpha):
    """wg_edge_pair_inv_distance: 1 / (|Q_r - Q_c|_2 + alpha); the unit is 2^-24 |truth| (a relative bound)"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    P, Cw = len(rows), Q.shape[1]
    indptr = np.arange(P + 1) * Cw

    def sq(dt):
        d = np.asarray(Q, dt)[rows] - np.asarray(Q, dt)[cols]    # exact in float64
        return (d * d).reshape(-1, 1)

    def fin(s, dt):
        return (1 / (np.sqrt(s) + dt(alpha))).reshape(-1)

    truth = f64(fin(seg_sum(indptr, sq(LD), LD), LD))
    second = fin(seg_reduce(indptr, sq(np.float64)), np.float64)
    model = f32(fin(seg_sum(indptr, sq(np.float64), np.float64), np.float64))
    mutant = f32(fin(f64(seg_sum(indptr, sq(np.float64), np.float32)), np.float64))
    return Ref(truth, second, EPS * np.abs(truth), model, mutant, BOUND_ONE)


class Attention:
    """the float64 edge quantities of csrc/gats.hip in one format: d, e = leaky_relu(d), p = softmax over the row"""

    def __init__(self, indptr, indices, a, slope, dt):
        self.indptr, self.indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
        self.rows = row_ids(self.indptr)
        a = np.asarray(a).astype(dt)
        self.d = (a[self.rows] * a[self.indices]).sum(1)
        assert not self.d.size or float(np.abs(self.d).max()) <= MAX_LOGIT, "a logit beyond MAX_LOGIT (module docstring)"
        self.e = np.where(self.d > 0, self.d, dt(slope) * self.d)
        ex = np.exp(self.e - seg_max(self.indptr, self.e)[self.rows])
        self.den = seg_sum(self.indptr, ex.reshape(-1, 1), dt)[:, 0]
        self.p = ex / self.den[self.rows]
        self.dt, self.slope = dt, slope

    def s(self, t, g):
        """s_ij = p_ij (q_ij - m_i) leaky_relu'(d_ij), q_ij = g_i . t_j, m_i = sum_j p_ij q_ij (d == 0: the slope)"""
        t, g = np.asarray(t).astype(self.dt), np.asarray(g).astype(self.dt)
        q = (g[self.rows] * t[self.indices]).sum(1)
        m = seg_sum(self.indptr, (self.p * q).reshape(-1, 1), self.dt)[:, 0]
        return self.p * (q - m[self.rows]) * np.where(self.e > 0, self.dt(1), self.dt(self.slope))


def _by_format(make):
    """weight(dtype) of `aggregate` from make(Attention-like of that dtype), each format computed once"""
    cache = {}

    def weight(dt):
        if dt not in cache:
            cache[dt] = make(dt)
        return cache[dt]
    return weight


def gat_forward(indptr, indices, a, t, conf, slope=0.2):
    """wg_gat_forward: (sim, dconf); sim_i = sum_j p_ij t_j, dconf_i = sum_j (conf_i - conf_j)"""
    att = _by_format(lambda dt: Attention(indptr, indices, a, slope, dt))
    indices = np.asarray(indices, np.int64)
    sim = aggregate(indptr, lambda dt: att(dt).p, np.asarray(t)[indices])
    rows = row_ids(np.asarray(indptr, np.int64))
    conf = np.asarray(conf)
    diff = f64(conf)[rows] - f64(conf)[indices]     # exact: a difference of two float32
    dconf = aggregate(indptr, lambda dt: diff.astype(dt), np.ones((len(indices), 1), np.float32))
    for k in ("truth", "second", "unit", "model", "mutant"):
        setattr(dconf, k, getattr(dconf, k).reshape(-1))
    return sim, dconf


def gat_backward(indptr, indices, a, t, g_sim, slope=0.2):
    """wg_gat_backward: (grad_a, grad_t); grad_t_j = sum over the rows i that list j of p_ij g_i (ascending i),
    grad_a_i = sum over row i of s_ij a_j, then over the transposed row of s_ki a_k (ascending k)"""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    rows = row_ids(indptr)
    t_indptr, order = transpose_order(indptr, indices)
    att = _by_format(lambda dt: Attention(indptr, indices, a, slope, dt))
    s = _by_format(lambda dt: att(dt).s(t, g_sim))
    grad_t = aggregate(t_indptr, lambda dt: att(dt).p[order], np.asarray(g_sim)[rows[order]])
    # node i: its own entries, then its transposed entries
    node = np.concatenate([rows, indices[order]])
    both = np.argsort(node, kind="stable")
    b_indptr = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=len(indptr) - 1))])
    src = np.concatenate([indices, rows[order]])[both]
    grad_a = aggregate(b_indptr, lambda dt: np.concatenate([s(dt), s(dt)[order]])[both], np.asarray(a)[src])
    return grad_a, grad_t


# --------------------------------------------------------------------------------------------------- flips
def flip_overlay(A, rows, cols, symmetric):
    """The overlay of RowNormalizedAdjacency.with_flips (wats_hip/flips.py) in numpy from the dense update
    (calib_attack/calib_fga.py:901-904): positions where A' != A bitwise by (row, column), a_old, a_new, the touched
    rows and deg' = float32(s + sum(double(a_new) - double(a_old))), 0 -> 1."""
    dense = np.asarray(A.toarray(), np.float32)
    new = dense.copy()
    for r, c in zip(rows, cols):
        v = np.float32(-2) * new[r, c] + np.float32(1)
        new[r, c] += v
        if symmetric:
            new[c, r] += v
    pos = np.argwhere(new.view(np.int32) != dense.view(np.int32))
    a_old, a_new = dense[pos[:, 0], pos[:, 1]], new[pos[:, 0], pos[:, 1]]
    t_rows, seg_of = np.unique(pos[:, 0], return_inverse=True)
    diff = np.zeros(len(t_rows))
    np.add.at(diff, seg_of, a_new.astype(np.float64) - a_old.astype(np.float64))
    s = np.asarray(A.astype(np.float64).sum(axis=1)).ravel()
    deg_new = (s[t_rows] + diff).astype(np.float32)
    deg_new[deg_new == 0] = 1
    return dict(rows=pos[:, 0], cols=pos[:, 1], a_old=a_old, a_new=a_new, t_rows=t_rows, deg_new=deg_new)


def parent_degree(A):
    """RowNormalizedAdjacency.deg: the float64 row sum rounded to float32, 0 -> 1"""
    deg = np.asarray(A.astype(np.float64).sum(axis=1)).ravel().astype(np.float32)
    deg[deg == 0] = 1
    return deg


def _flipped_entries(A, ov):
    """(rows, cols, values float32) of A' by (row, column): the parent's entries the overlay leaves, and a_new != 0"""
    A = A.tocsr()
    n = A.shape[0]
    pr, pc = row_ids(A.indptr), A.indices.astype(np.int64)
    keep = ~np.isin(pr * n + pc, ov["rows"] * n + ov["cols"])
    on = ov["a_new"] != 0
    r = np.concatenate([pr[keep], ov["rows"][on]])
    c = np.concatenate([pc[keep], ov["cols"][on]])
    v = np.concatenate([A.data.astype(np.float32)[keep], ov["a_new"][on]])
    order = np.argsort(r * n + c, kind="stable")
    return r[order], c[order], v[order]


def flip_rows(A, ov, x):
    """the touched rows of the view's forward, in the order of ov["t_rows"]: y'_r = sum_c (a'_rc / deg'_r) x_c, the
    kernel multiplying by the float32 quotient (wg_flip_rows)"""
    r, c, v = _flipped_entries(A, ov)
    t_rows = np.asarray(ov["t_rows"], np.int64)
    sel = np.isin(r, t_rows)
    r, c, v = r[sel], c[sel], v[sel]
    seg = np.searchsorted(t_rows, r)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(seg, minlength=len(t_rows)))])
    deg = np.asarray(ov["deg_new"], np.float32)[seg]
    return aggregate(indptr, lambda dt: v.astype(dt) / deg.astype(dt), np.asarray(x)[c], bound=BOUND_FLIP_ROWS,
                     model_weight=lambda dt: (v / deg).astype(np.float32).astype(dt))


def flip_backward(A, ov, g):
    """adj_norm(A')^T g through the view, all n columns, as the three steps of wats_hip/flips.py: (1) g' = g with the
    touched rows scaled by deg / deg' (a float64 quotient) and rounded to float32, (2) the parent's transposed wg_spmm
    gx = fl32(sum_r fl32(a_rc / deg_r) g'_r), (3) wg_flip_cols: fl32(gx_c + sum_p ((a_new - a_old) / deg'_r) g_r) on
    the overlay's columns.  truth and unit are of that expression with exact weights (a removed entry cancels there
    too, and counts twice in the unit); `second` is sum_r (a'_rc / deg'_r) g_r over the entries of A' itself."""
    A = A.tocsr()
    n = A.shape[0]
    g = np.asarray(g, np.float32)
    deg = parent_degree(A)
    t_rows = np.asarray(ov["t_rows"], np.int64)
    deg_new = np.asarray(ov["deg_new"], np.float32)
    seg = np.searchsorted(t_rows, ov["rows"])
    scale = np.ones(n)
    scale[t_rows] = deg[t_rows].astype(np.float64) / deg_new.astype(np.float64)
    g1 = (g.astype(np.float64) * scale[:, None]).astype(np.float32)     # untouched rows: unchanged
    pr, pc, pv = row_ids(A.indptr), A.indices.astype(np.int64), A.data.astype(np.float32)
    # the terms of column c: the parent's entries by ascending row, then the overlay's
    ow = lambda dt: (ov["a_new"].astype(dt) - ov["a_old"].astype(dt)) / deg_new[seg].astype(dt)
    col = np.concatenate([pc, ov["cols"]])
    order = np.argsort(col, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))])
    exact = lambda dt: np.concatenate([pv.astype(dt) / deg[pr].astype(dt) * scale[pr].astype(dt), ow(dt)])[order]
    xg = np.concatenate([g[pr], g[ov["rows"]]])[order]
    ref = aggregate(indptr, exact, xg, bound=BOUND_FLIP_COLS)
    # second: the entries of A' with their own degree
    degp = deg.copy()
    degp[t_rows] = deg_new
    r2, c2, v2 = _flipped_entries(A, ov)
    o2 = np.argsort(c2, kind="stable")
    ip2 = np.concatenate([[0], np.cumsum(np.bincount(c2, minlength=n))])
    ref.second = seg_reduce(ip2, (v2.astype(np.float64) / degp[r2].astype(np.float64))[o2].reshape(-1, 1)
                            * g[r2[o2]].astype(np.float64))
    # the three steps
    t_ip, t_order = transpose_order(A.indptr, A.indices)
    w32 = (pv / deg[pr]).astype(np.float32).astype(np.float64)[t_order].reshape(-1, 1)
    ocol = np.asarray(ov["cols"], np.int64)
    oo = np.argsort(ocol, kind="stable")
    o_ip = np.concatenate([[0], np.cumsum(np.bincount(ocol, minlength=n))])
    ot = ow(np.float64)[oo].reshape(-1, 1) * g[ov["rows"][oo]].astype(np.float64)
    in_overlay = np.diff(o_ip) > 0
    for name, dt in (("model", np.float64), ("mutant", np.float32)):
        gx = f64(f32(seg_sum(t_ip, w32 * g1[pr[t_order]].astype(np.float64), dt)))
        if dt is np.float32:   # the accumulator starts at gx, as the kernel's does
            acc = gx.astype(np.float32)
            lens = np.diff(o_ip)
            for k in range(int(lens.max()) if lens.size else 0):
                rr = np.flatnonzero(lens > k)
                acc[rr] = (acc[rr] + ot[o_ip[rr] + k]).astype(np.float32)
            out = acc
        else:
            out = f32(gx + seg_sum(o_ip, ot, np.float64))
        setattr(ref, name, np.where(in_overlay[:, None], out, f32(gx)).astype(np.float32))
    return ref


# --------------------------------------------------------------------------------------------------- graphs, signals
def by_destination(src, dst, n, self_loops):
    """(indptr, indices) of the canonical CSR whose row i lists the sources of the edges into i (duplicates merged;
    self_loops: gats_ref.with_self_loops, the calibrators' self-loop step)"""
    if self_loops:
        src, dst = G.with_self_loops(src, dst, n)
    else:
        key = np.unique(np.asarray(dst, np.int64) * n + np.asarray(src, np.int64))
        src, dst = key % n, key // n
    return np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]).astype(np.int64), src.astype(np.int64)


def threshold_graph(thr, self_loops, extra=40, seed=5):
    """(src, dst, n): rows 0, 1, 2 have exactly thr - 1, thr and thr + 1 entries (the self loop counted where the
    caller adds one), and so have columns 0, 1, 2 (every edge goes both ways); `extra` further nodes hold a few random
    edges, and the last five nothing at all (empty rows, or rows of the self loop alone)"""
    n = thr + 2 + extra
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for k in range(3):   # row k lists the first `want` nodes from 3 on, and is listed by them
        want = thr - 1 + k - (1 if self_loops else 0)
        src += list(range(3, 3 + want))
        dst += [k] * want
    m = rng.integers(thr + 5, n - 5, (2, 2 * extra))
    src, dst = np.concatenate([src, m[0]]), np.concatenate([dst, m[1]])
    keep = src != dst
    src, dst = src[keep], dst[keep]
    return np.concatenate([src, dst]), np.concatenate([dst, src]), n


def graph_edges(name, thr=128, self_loops=True):
    if name == "star":
        return G.star_graph(700, 50)
    if name == "directed":
        return G.random_graph(600, 12, True, 3, loops=5)
    if name == "undirected":
        return G.random_graph(600, 12, False, 4)
    assert name == "threshold", name
    return threshold_graph(thr, self_loops)


GRAPHS = ("star", "directed", "undirected", "threshold")


def signal(n, F, kind, seed, spread=3.0):
    """"normal": N(0, 1); "positive": |N(0, 1)| + 0.5 (no cancellation: every rounding of a sum shows); "spread":
    N(0, 1) with every row scaled by 10^U(-spread, spread), the case a tensor-wide maximum hides"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, F))
    if kind == "positive":
        x = np.abs(x) + 0.5
    elif kind == "spread":
        x = x * 10.0 ** rng.uniform(-spread, spread, (n, 1))
    else:
        assert kind == "normal", kind
    return x.astype(np.float32)


def cases():
    """(graph, width, signal) of every operation: every width on the star with the positive signal (the hub row and
    its leaves), every graph with every signal at the widths 7 (dwords, two lanes) and 64 (16 bytes)"""
    out = [("star", w, "positive") for w in WIDTHS]
    out += [(g, w, k) for g in GRAPHS for k in KINDS for w in (7, 64) if (g, w, k) not in out]
    return out


def attention_inputs(n, Cw, Hh, kind, seed):
    """(a, t, conf, g_sim).  a is scaled so that |d_ij| stays far below MAX_LOGIT and no softmax saturates (spread:
    10^U(-0.25, 0.25) per row of a, the full six orders on t, conf and g_sim): with one p_ij within 2^-30 of 1 the
    float64 difference q_ij - m_i of the backward cancels and s_ij itself, which the header hands on in float64, is
    no longer good to a unit.  That is the documented arithmetic's own limit and no rounding to float32; the host
    test's agreement of truth and second evaluation is what notices it.  "positive": conf_0 is the largest, so that
    node 0 (the star's hub, the threshold graph's first row) adds differences of one sign."""
    a = signal(n, Cw, kind, seed, spread=0.25) * np.float32(1.0 / np.sqrt(Cw))
    conf = signal(n, 1, kind, seed + 2).reshape(-1)
    if kind == "positive":
        conf[0] = conf.max() + np.float32(1)
    return a.astype(np.float32), signal(n, Hh, kind, seed + 1), conf, signal(n, Hh, kind, seed + 3)


# --------------------------------------------------------------------------------------------------- flip cases
HUB_N = 2100     # row 0 of the hub graph has HUB_N - 1 entries: more than one pass of flip_rows' sub-groups at F <= 4
FLIP_CASES = ("hub_64_symmetric", "hub_65_one_row", "weighted_mixed")
_FLIP = {}


def flip_graph(name):
    """the `hub` (a star on node 0 plus a ring, unit values) and `weighted` (directed, weighted, self loops, empty
    rows) graphs of tests/test_flip_view.py by the same recipe, the hub with HUB_N nodes; scipy CSR, float32"""
    import scipy.sparse as sp
    if name not in _FLIP:
        if name == "hub":
            ring = np.arange(1, HUB_N)
            src = np.concatenate([np.zeros(HUB_N - 1, np.int64), ring, ring, np.roll(ring, -1)])
            dst = np.concatenate([ring, np.zeros(HUB_N - 1, np.int64), np.roll(ring, -1), ring])
            A = sp.csr_matrix((np.ones(src.size, np.float32), (src, dst)), shape=(HUB_N, HUB_N))
        else:
            from wats_hip.graphgen import random_graph
            assert name == "weighted", name
            A = sp.csr_matrix(random_graph(300, 0.03, directed=True, weighted=True, self_loop_frac=0.1,
                                           isolated_frac=0.05).to_scipy(), dtype=np.float32)
        A.sum_duplicates()
        A.sort_indices()
        _FLIP[name] = A
    return _FLIP[name]


def flip_case(name):
    """(graph name, rows, cols, symmetric) of the named flip calls of tests/test_flip_view.py"""
    rng = np.random.default_rng(11)
    if name == "hub_64_symmetric":      # 65 touched rows, the hub among them; column 0 has 64 overlay positions
        return "hub", [0] * 64, [int(c) for c in rng.choice(np.arange(1, HUB_N), 64, replace=False)], True
    if name == "hub_65_one_row":        # one touched row: the hub loses 65 of its entries
        return "hub", [0] * 65, [int(c) for c in rng.choice(np.arange(1, HUB_N), 65, replace=False)], False
    assert name == "weighted_mixed", name   # weights change without leaving; an empty row gains an entry
    A = flip_graph("weighted")
    dense = A.toarray()
    counts = np.diff(A.indptr)
    present = np.argwhere(np.triu(dense != 0, 1))
    absent = np.argwhere(np.triu((dense + dense.T) == 0, 1))
    sel = np.concatenate([present[rng.choice(len(present), 5, replace=False)],
                          absent[rng.choice(len(absent), 5, replace=False)]])
    r, c = [int(v) for v in sel[:, 0]], [int(v) for v in sel[:, 1]]
    empty = [int(i) for i in np.flatnonzero((counts == 0) & (dense.sum(0) == 0))[:2]]
    taken = set(r) | set(c)
    partner = [int(i) for i in np.flatnonzero(counts > 0) if int(i) not in taken][:2]
    return "weighted", r + empty, c + partner, True


def pair_inputs(n, Cw, kind, seed, rows, cols):
    """(Q, rows, cols) of wg_edge_pair_inv_distance: rows of a distribution (DCGC's softmax), "spread": scaled per row
    so that |Q_r - Q_c| runs from far below alpha to far above it; two pairs are appended: rows 10 / 11 identical
    (exactly 1 / alpha) and rows 20 / 21 differing in the last bit of one column"""
    q = np.abs(signal(n, Cw, "normal", seed)).astype(np.float64) + 1e-3
    q = q / q.sum(1, keepdims=True)
    if kind == "spread":
        q = q * 10.0 ** np.random.default_rng(seed).uniform(-3, 3, (n, 1))
    q = q.astype(np.float32)
    q[11], q[21] = q[10], q[20]
    q[21, Cw // 2] = np.nextafter(q[20, Cw // 2], np.float32(4e3))
    return q, np.concatenate([rows, [10, 20]]), np.concatenate([cols, [11, 21]])
