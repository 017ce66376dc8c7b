"""Float64 truth, row-wise error units and float32 models of the Chebyshev step (reference calibration/WATS.py:29-37,
:65-68), numpy / scipy only.  Helpers of tests/test_step_precision_host.py and tests/test_step_precision.py; not a test.

The operator is the reference's: oracle.wats_oracle.rescaled_laplacian, the float32 values -((a_ij / sqrt(w_i)) /
sqrt(w_j)) upcast to float64 with the -1 diagonal of isolated rows.  Everything here is in the CALLER's row order.

  truth_step / truth_chain   the float64 yardstick with its row units
  c_of                       max over rows and columns of |got - truth| / unit (exactly 0 where the unit is 0)
  model_forward (i), model_clenshaw (ii), model_clenshaw_u (iii), model_step_f32 (iv)
                             the arithmetic DESIGN.md documents, float32 storage and float64 sums; the bounds of the
                             GPU tests come from these, never from a kernel
  model_step_valued, model_step_u, model_step_hybrid
                             one step of the valued, the value-free and (crudely) the hybrid form
  mutant_*                   two wrong kernels the tests must reject: u split into two bf16 pieces instead of three,
                             and float32 sequential row sums

A unit is what one float32 rounding of a row's absolute sum costs:
  step   unit_i = 2^-24 (|ck x0_i| + |cacc| sum_j |L_ij| |b1_j| + |b2_i|)
  chain  unit_i = 2^-24 max_k (2 |L| |T_k| + |T_k|)_i   over the float64 T_k
so a hub does not hide its leaves: every row is measured against its own sum.
"""
import numpy as np
import scipy.sparse as sp

from oracle import wats_oracle as O

EPS = 2.0 ** -24

# bounds on c (the issue this module was written for derives them; restated in DESIGN.md section 5)
BOUND_VALUED = 2.0       # float64 sums rounded once + the rounding of the stored operator value
BOUND_VALUE_FREE = 6.0   # final rounding, u, dinv_j, dinv_i, two roundings inside the reference's float32 L_hat value
CHAIN_FACTOR = 2.0       # another, equally valid order of roundings (gats_ref.error_bound's factor)
H_BOUND = 1.5 * EPS      # H against the float64 normalisation of the returned S: one rounding of a float64 quotient


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def f64(x):
    return np.asarray(x, dtype=np.float64)


# --------------------------------------------------------------------------------------------------- operators
class Operator:
    """L_hat of an adjacency with what the models need: the float64 CSR (float32 values), its absolute value, the
    float32 CSR, and for the value-free form the 0/1 off-diagonal pattern, the isolated rows and dinv = 1 / fl32(sqrt(w))
    (float64 reciprocal of scipy's float32 square root, 1 where w = 0)."""

    def __init__(self, A):
        A = sp.csr_matrix(A)
        self.n = A.shape[0]
        self.L = O.rescaled_laplacian(A).tocsr()
        self.L.sort_indices()
        self.absL = abs(self.L).tocsr()
        self.L32 = self.L.astype(np.float32)
        indptr, indices, _, iso, sw = O.laplacian_explicit(A)
        self.iso = iso.astype(np.float64).reshape(-1, 1)
        self.dinv = (1.0 / sw.astype(np.float64)).reshape(-1, 1)
        self.unit = bool(np.all(A.data == 1.0))
        self.P = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=A.shape)   # off-diagonal pattern
        self.P32 = self.P.astype(np.float32)

    def apply_u(self, u, sums=None):
        """L_hat b from u = b * dinv on an unweighted graph: -dinv_i sum_j u_j, and -b_i on an isolated row"""
        acc = self.P @ f64(u) if sums is None else sums
        return -self.dinv * acc - self.iso * (f64(u) / self.dinv)


class Literal:
    """any float64 CSR as an operator of truth_step (the row-normalised adjacency of wg_spmm)"""

    def __init__(self, M):
        self.L = sp.csr_matrix(M, dtype=np.float64)
        self.absL = abs(self.L).tocsr()
        self.n = self.L.shape[0]


_OPS = {}


def operator(A):
    """Operator(A), built once per adjacency object"""
    if id(A) not in _OPS:
        _OPS[id(A)] = (A, Operator(A))
    return _OPS[id(A)][1]


def rownorm(A, transpose=False, float32_degree=True):
    """adj_norm = a_ij / deg_i as a float64 quotient (0 -> 1 in deg), or its transpose.  deg_i is the reference's: a
    float32 tensor (src/gnn/model.py:43 `deg = adj.sum(dim=1)`), here the correctly rounded float32 of the exact row
    sum, so the stored float32 value is ONE rounding from this truth, the one BOUND_VALUED's second unit pays for.
    float32_degree = False divides by the float64 row sum instead: a third rounding away (model_spmm)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    deg = np.asarray(A.sum(axis=1)).ravel()
    if float32_degree:
        deg = deg.astype(np.float32).astype(np.float64)
    deg[deg == 0] = 1.0
    M = sp.diags(1.0 / deg) @ A
    return Literal(M.T.tocsr() if transpose else M.tocsr())


def model_spmm(A, x, transpose=False):
    """wg_spmm's documented arithmetic (include/wats_hip.h, csrc/gcn.hip; the reference's float32 `adj / deg`): the
    degree is the float64 row sum rounded to float32, each stored value the float32 quotient a_ij / deg_i, the
    product float64 sums rounded once.  Against rownorm's float64 a_ij / deg_i that is three roundings, not two."""
    A = sp.csr_matrix(A, dtype=np.float32)
    deg = np.asarray(sp.csr_matrix(A, dtype=np.float64).sum(axis=1)).ravel().astype(np.float32)
    deg[deg == 0] = np.float32(1)
    V = A.copy()
    V.data = (A.data / np.repeat(deg, np.diff(A.indptr))).astype(np.float32)
    V = V.astype(np.float64)
    return f32((V.T.tocsr() if transpose else V) @ f64(f32(x)))


def _op(A):
    return A if isinstance(A, (Operator, Literal)) else operator(A)


# --------------------------------------------------------------------------------------------------- truth and units
def truth_step(A, b1, b2, x0, ck, cacc):
    """(y, unit) of y = ck x0 + cacc (L b1) - b2 in float64; b2 / x0 None = 0"""
    op = _op(A)
    b1 = f64(b1)
    z = np.zeros_like(b1)
    b2 = z if b2 is None else f64(b2)
    x0 = z if x0 is None else f64(x0)
    y = ck * x0 + cacc * (op.L @ b1) - b2
    unit = EPS * (np.abs(ck * x0) + abs(cacc) * (op.absL @ np.abs(b1)) + np.abs(b2))
    return y, unit


def truth_chain(A, X, K, s):
    """dict(S, H, T = [T_0 .. T_K], unit) of the oracle's chain in float64"""
    op = _op(A)
    T = [f64(t) for t in O.chebyshev_polynomials(op.L, K, f64(X))]
    S = np.asarray(O.heat_kernel_combine(T, s), dtype=np.float64)
    unit = np.zeros_like(S)
    for t in T:
        unit = np.maximum(unit, 2.0 * (op.absL @ np.abs(t)) + np.abs(t))
    return dict(S=S, H=O.row_l1_normalize(S), T=T, unit=EPS * unit)


def c_of(got, truth, unit, what=""):
    """max |got - truth| / unit over every row and column; an entry whose unit is 0 must be exact"""
    got = f64(got).reshape(truth.shape)
    assert np.all(np.isfinite(got)), f"{what}: non-finite output"
    err = np.abs(got - truth)
    zero = unit == 0
    assert not np.any(err[zero]), f"{what}: {int(np.count_nonzero(err[zero]))} entries with unit 0 are not exact"
    return float((err[~zero] / unit[~zero]).max()) if np.any(~zero) else 0.0


def h_error(H, S):
    """max |H - S / (sum|S| + 1e-8)| / |H| over the entries of the returned H, in units of 2^-24 (an entry of H
    that is 0 must be exact)"""
    H, S = f64(H), f64(S)
    ref = S / (np.abs(S).sum(axis=1, keepdims=True) + 1e-8)
    err = np.abs(H - ref)
    zero = H == 0
    assert not np.any(err[zero]), "an entry of H is 0 where S / (|S|_1 + 1e-8) is not"
    return float((err[~zero] / np.abs(H[~zero])).max() / EPS) if np.any(~zero) else 0.0


# --------------------------------------------------------------------------------------------------- bf16 pieces
def bf16_pieces(u, pieces=3):
    """u as a sum of `pieces` bf16 numbers, each the high half of a float32 (truncated), as csrc/tiles.hip split3:
    three pieces hold a float32 exactly, two drop up to 2^-16 of it"""
    r = np.ascontiguousarray(u, dtype=np.float32)
    total = np.zeros(r.shape, np.float64)
    for _ in range(pieces):
        p = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        total += p
        r = (r - p).astype(np.float32)   # exact: the difference of a float32 and its own leading bits
    return total


# --------------------------------------------------------------------------------------------------- one step
def _epilogue(acc, b2, x0, ck, cacc):
    z = np.zeros_like(acc)
    return ck * (z if x0 is None else f64(x0)) + cacc * acc - (z if b2 is None else f64(b2))


def model_step_valued(A, b1, b2, x0, ck, cacc):
    """the valued path: float32 operator values, float64 sums, one rounding"""
    op = _op(A)
    return f32(_epilogue(op.L @ f64(f32(b1)), b2, x0, ck, cacc))


def model_step_u(A, b1, b2, x0, ck, cacc, pieces=3, u_out=False):
    """the value-free path: gathers u = fl32(b1 dinv), float64 sums, scales by dinv_i; b2 arrives as fl32(b2 dinv)
    and, with u_out, the result leaves as fl32(y dinv) and is returned divided by dinv again"""
    op = _op(A)
    u1 = f32(f64(b1) * op.dinv)
    if pieces != 3:
        u1 = bf16_pieces(u1, pieces)
    prev = None if b2 is None else f64(f32(f64(b2) * op.dinv)) / op.dinv
    y = _epilogue(op.apply_u(u1), prev, x0, ck, cacc)
    return f64(f32(y * op.dinv)) / op.dinv if u_out else f32(y)


def _chunk_sums32(op, u32, chunk):
    """row sums of u over the pattern: float32 sequential sums over runs of `chunk` entries, the runs in float64"""
    lens = np.diff(op.P.indptr)
    runs = (lens + chunk - 1) // chunk
    starts = np.concatenate([[0], np.cumsum(runs)])
    ptr = np.concatenate([np.minimum(op.P.indptr[i] + chunk * np.arange(runs[i] + 1), op.P.indptr[i + 1])[:-1]
                          for i in range(op.n)] + [[op.P.indptr[-1]]]).astype(np.int64)
    Pc = sp.csr_matrix((np.ones(op.P.nnz, np.float32), op.P.indices, ptr), shape=(len(ptr) - 1, op.n))
    part = Pc @ np.ascontiguousarray(u32, dtype=np.float32)          # float32 sequential (sparsetools csr_matvecs)
    join = sp.csr_matrix((np.ones(len(ptr) - 1), np.arange(len(ptr) - 1), starts), shape=(op.n, len(ptr) - 1))
    return join @ f64(part)


def model_step_hybrid(A, b1, b2, x0, ck, cacc, chunk=128):
    """a crude model of the hybrid step: float32 sums over at most `chunk` entries of a row (three exact bf16
    pieces: the products are exact), the partial sums joined in float64"""
    op = _op(A)
    u1 = f32(f64(b1) * op.dinv)
    prev = None if b2 is None else f64(f32(f64(b2) * op.dinv)) / op.dinv
    return f32(_epilogue(op.apply_u(u1, sums=_chunk_sums32(op, u1, chunk)), prev, x0, ck, cacc))


def model_step_f32(A, b1, b2, x0, ck, cacc):
    """(iv) the plain float32 CSR product: scipy float32 matrix times float32 array (one sequential float32 sum per
    row), the recurrence in float32"""
    op = _op(A)
    acc = op.L32 @ np.ascontiguousarray(b1, dtype=np.float32)
    z = np.zeros_like(acc)
    y = np.float32(ck) * (z if x0 is None else np.asarray(x0, np.float32)) + np.float32(cacc) * acc
    return (y - (z if b2 is None else np.asarray(b2, np.float32))).astype(np.float32)


def mutant_step_two_pieces(A, b1, b2, x0, ck, cacc):
    """WRONG on purpose: the hybrid step with u split into two bf16 pieces (the third dropped)"""
    return model_step_u(A, b1, b2, x0, ck, cacc, pieces=2)


def mutant_step_f32_sums(A, b1, b2, x0, ck, cacc):
    """WRONG on purpose: the value-free step with one sequential float32 sum per row where float64 is documented"""
    op = _op(A)
    u1 = f32(f64(b1) * op.dinv)
    prev = None if b2 is None else f64(f32(f64(b2) * op.dinv)) / op.dinv
    return f32(_epilogue(op.apply_u(u1, sums=f64(op.P32 @ u1)), prev, x0, ck, cacc))


# --------------------------------------------------------------------------------------------------- chains
def model_forward(A, X, K, s):
    """(i) the forward recurrence, every T_k and the running S rounded to float32, sums in float64"""
    op = _op(A)
    a = [float(v) for v in O.heat_coefficients(K, s)]
    T0 = f64(f32(X))
    if K == 0:
        return f32(a[0] * T0)
    t = op.L @ T0
    S = f64(f32(a[0] * T0 + a[1] * t))
    Tm2, Tm1 = T0, f64(f32(t))
    for k in range(2, K + 1):
        t = 2.0 * (op.L @ Tm1) - Tm2
        S = f64(f32(S + a[k] * t))
        Tm2, Tm1 = Tm1, f64(f32(t))
    return f32(S)


def model_clenshaw(A, X, K, s):
    """(ii) Clenshaw's recurrence b_k = a_k X + 2 L b_{k+1} - b_{k+2}, S = a_0 X + L b_1 - b_2, every b_k rounded to
    float32, sums in float64"""
    op = _op(A)
    a = [float(v) for v in O.heat_coefficients(K, s)]
    X = f64(f32(X))
    b1, b2 = np.zeros_like(X), np.zeros_like(X)
    for k in range(K, 0, -1):
        b1, b2 = f64(f32(a[k] * X + 2.0 * (op.L @ b1) - b2)), b1
    return f32(a[0] * X + (op.L @ b1) - b2)


def model_clenshaw_u(A, X, K, s, pieces=3):
    """(iii) Clenshaw value-free: the chain carries u_k = fl32(b_k dinv), gathers it without values and scales the row
    sum by dinv_i (unweighted graphs).  pieces = 2 is the two-piece mutant through the whole chain."""
    op = _op(A)
    assert op.unit, "the value-free form exists on unweighted graphs only"
    a = [float(v) for v in O.heat_coefficients(K, s)]
    X = f64(f32(X))
    u1, u2 = np.zeros_like(X), np.zeros_like(X)
    gathered = (lambda u: u) if pieces == 3 else (lambda u: bf16_pieces(u, pieces))
    for k in range(K, 0, -1):
        b = a[k] * X + 2.0 * op.apply_u(gathered(u1)) - u2 / op.dinv
        u1, u2 = f64(f32(b * op.dinv)), u1
    return f32(a[0] * X + op.apply_u(gathered(u1)) - u2 / op.dinv)


def chain_models(A, X, K, s):
    """{name: S} of the documented chain arithmetic that applies to this graph"""
    out = {"forward": model_forward(A, X, K, s), "clenshaw": model_clenshaw(A, X, K, s)}
    if _op(A).unit:
        out["clenshaw_u"] = model_clenshaw_u(A, X, K, s)
    return out


def chain_bound(A, X, K, s, truth=None):
    """(bound, {name: c}): CHAIN_FACTOR times the largest c of the models (i), (ii), (iii) on these inputs"""
    truth = truth or truth_chain(A, X, K, s)
    cs = {k: c_of(v, truth["S"], truth["unit"], k) for k, v in chain_models(A, X, K, s).items()}
    return CHAIN_FACTOR * max(cs.values()), cs


def hybrid_step_bound(A, b1, b2, x0, ck, cacc, truth=None):
    """(bound, c of model (iv)): the hybrid step's float32 chains cover at most 128 terms and must not do worse than
    one float32 chain over the whole row"""
    y, unit = truth or truth_step(A, b1, b2, x0, ck, cacc)
    c4 = c_of(model_step_f32(A, b1, b2, x0, ck, cacc), y, unit, "model (iv)")
    return max(BOUND_VALUE_FREE, c4), c4


# --------------------------------------------------------------------------------------------------- signals
def signal(n, F, kind, seed):
    """kind "normal": N(0, 1); "positive": |N(0, 1)| + 0.5 (no cancellation: every rounding of a sum shows)"""
    x = np.random.default_rng(seed).standard_normal((n, F))
    if kind == "positive":
        x = np.abs(x) + 0.5
    else:
        assert kind == "normal", kind
    return x.astype(np.float32)


def report(what, c, bound, extra=""):
    """one line per measurement, as gats_ref.assert_close prints, then the assertion"""
    print(f"{what}: c={c:.3f} bound={bound:.3f}{' ' + extra if extra else ''}")
    assert c <= bound, f"{what}: c {c:.3f} > bound {bound:.3f}{' ' + extra if extra else ''}"
