"""Bit-level models, long-double truths, per-element error units, documented-arithmetic models and one-property
mutants of the two kernel files that run on the matrix cores: csrc/edgemlp.hip (the DCGC edge MLP) and
csrc/simcalib.hip (the SimCalib similarity temperature).  numpy only (torch is used to draw inputs the way
tests/test_dcgc.py and tests/test_simcalib.py draw theirs).  Helpers of tests/test_mfma_precision_host.py and
tests/test_mfma_precision.py; not a test.

v_mfma_f32_32x32x2_f32 is a k-ordered chain of float32 fused multiply-adds, one rounding per product and no wider
accumulator: D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), k0 on lanes 0-31 and k1 on lanes 32-63.  fma32 below is that
operation exactly, so everything the kernels build from MFMA chains, float64 additions and single roundings can be
restated to the bit:

  model_edge_mlp_forward   w, h1, h2 and the three ReLU patterns of mlp_forward (edgemlp.hip), bit for bit
  model_sim_scores         x_ij = fl32(s_ij * fl32(1 / tau)) of sim_tile (simcalib.hip), bit for bit

What passes through expf (a device function with an error of its own) or through a sum whose order the model does not
restate (a float64 butterfly, the float64 partials of several workgroups) is measured in units instead:

  truth    sequential np.longdouble on exactly the float32 inputs the kernel receives (`truth`), and the same in
           float64 through BLAS (`second`); the host test holds them within TRUTH_AGREE units of each other
  unit     2^-24 times the same expression with every added term replaced by its absolute value
  c        max |got - truth| / unit (cheb_ref.c_of); an element whose unit is 0 must be exact
  model    the arithmetic the kernel headers document, in numpy (exp correctly rounded)
  mutant   the model with ONE documented property replaced by the cheaper, wrong one

The edge MLP's backward truth takes the ReLU pattern from the FORWARD MODEL (z > 0 of the float32 pre-activations the
kernel itself computes), not from float64 pre-activations: the gradient is then a polynomial in the inputs, the
recomputing backward has to take the same side of every kink as the forward did, and no entry is left out.

Bounds (tests/test_mfma_precision_host.py derives and pins them, DESIGN.md section 5 tabulates them):
  * a count of roundings + SLACK where the arithmetic is float64 sums of float32 numbers rounded once;
  * where float32 chains enter: CHAIN_FACTOR (2, the project's margin for another equally valid order of roundings)
    times the documented model's c ON THE SAME INPUTS, with the count of roundings as a floor;
  * for what passes through expf: the model's exp is correctly rounded, and the device's expf is allowed EXPF_ULP per
    call on top (1 ulp = 2 units of 2^-24), times the number of exps between a term and the result.
EXPF_ULP = 1 is ASSUMED: neither the ROCm headers nor the documents installed with them state a figure for expf.
"""
import fractions

import numpy as np

import agg_ref as A
import cheb_ref as C
import dcgc_ref as D

EPS = C.EPS
LD = np.longdouble
F32, F64 = np.float32, np.float64
f32, f64 = C.f32, C.f64
SLACK = 1e-3
TRUTH_AGREE = 1e-3
CHAIN_FACTOR = C.CHAIN_FACTOR
EXPF_ULP = 1.0          # assumed, see the module docstring
TURN, TILE = 128, 1024  # entries of a turn / of a workgroup tile of the edge MLP's backward (edgemlp.hip)
MLP_CS = (1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48)     # both edges of every (NB0, NB1) instantiation
NAMES = ("W1", "b1", "W2", "b2", "w3", "b3")


# ----------------------------------------------------------------------------------------------------- float32 fma
def fma32(a, b, acc):
    """fl32(a * b + acc) with ONE rounding, elementwise on float32 arrays.  The product of two float32 numbers is
    exact in float64; TwoSum gives the float64 sum s and its exact error; where the error is not zero s is rounded to
    odd (of the two float64 neighbours of the exact sum, the one with the odd last bit), and a round-to-odd value of
    53 >= 2 * 24 + 2 bits rounds to float32 as the exact sum would."""
    a, b, acc = (np.asarray(v, F32) for v in (a, b, acc))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a.astype(F64) * b.astype(F64)
        c = acc.astype(F64)
        s = np.asarray(p + c)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64)
        # The odd rounding changes the float32 result only where s is a tie of the float32 grid (the 29 bits below a
        # normal float32's last place are 1 0...0; below 2^-125 the grid is coarser: taken as a candidate) and the
        # exact sum is not s: everywhere else s and the exact sum round alike, and the step is skipped.
        fix = (err != 0) & (((bits & 0x1FFFFFFF) == 0x10000000) | (np.abs(s) < 2.0 ** -125)) & np.isfinite(s)
        if fix.any():
            fix &= (bits & 1) == 0
            away = (err > 0) == (s > 0)        # the exact sum lies beyond s, away from zero
            s = (bits + np.where(fix, np.where(away, 1, -1), 0)).view(F64)
        return s.astype(F32)


def fma_exact(a, b, c):
    """the same for three Python floats that hold float32 values, by exact rational arithmetic (no overflow)"""
    exact = fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c)
    if exact == 0:
        return np.float32(0.0)
    # round the rational to float32, ties to even: scale to an integer significand of 24 bits (or the subnormal step)
    sign, mag = (-1 if exact < 0 else 1), abs(exact)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()
    if fractions.Fraction(2) ** e > mag:
        e -= 1
    step = fractions.Fraction(2) ** (max(e, -126) - 23)
    q = mag / step
    n = q.numerator // q.denominator
    rem = q - n
    if rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and n & 1):
        n += 1
    return np.float32(sign * float(n * step))


def acc_row(r, h):
    """the unit (bank row) of accumulator register r in lane half h: the C/D map of the 32 x 32 MFMA shapes"""
    return (r & 3) + 8 * (r >> 2) + 4 * h


ACC_ORDER = [acc_row(r, h) for r in range(16) for h in (0, 1)]       # the k order of a product fed by an accumulator
HALF_ORDER = [[acc_row(r, h) for r in range(16)] for h in (0, 1)]   # the units a lane half holds, register order


def blocked_product(W, X, blocks, whole=False):
    """(E, U) float64: sum_k W[u, k] X[e, k] as the kernels do it.  `blocks`: lists of k; inside a block one float32
    fma chain from zero in the listed order, the blocks added in float64 in the listed order.  whole=True (a mutant):
    ONE float32 chain over every k in the same order."""
    W, X = np.asarray(W, F32), np.asarray(X, F32)
    acc = np.zeros((X.shape[0], W.shape[0]), F64)
    part = np.zeros(acc.shape, F32)
    for blk in blocks:
        if not whole:
            part = np.zeros(acc.shape, F32)
        for k in blk:
            if k < W.shape[1]:       # a padded k adds a zero product: the chain's value does not move
                part = fma32(W[None, :, k], X[:, k, None], part)
        if not whole:
            acc += part.astype(F64)
    return part.astype(F64) if whole else acc


def mlp_shape(Cw):
    return -(-2 * Cw // 32), -(-4 * Cw // 32)       # (NB0, NB1)


def asc_blocks(nb):
    return [list(range(32 * b, 32 * b + 32)) for b in range(nb)]


def acc_blocks(nb):
    return [[32 * b + u for u in ACC_ORDER] for b in range(nb)]


def np_params(params):
    """the six arrays as float32 numpy: W1 (4C, 2C), b1, W2 (2C, 4C), b2, w3 (2C,), b3 ()"""
    W1, b1, W2, b2, w3, b3 = (np.asarray(p.detach().cpu().numpy() if hasattr(p, "detach") else p, F32) for p in params)
    return W1, b1, W2, b2, w3.reshape(-1), b3.reshape(())


def drop_scale(p):
    return F32(1.0 / (1.0 - p)) if p else F32(1.0)


def drop_masks(nnz, Cw, p, seed):
    """(D1 (nnz, 4C), D2 (nnz, 2C)) float32: scale where the hashed bit keeps the unit, else 0"""
    sc = drop_scale(p)
    return tuple(np.where(D.keep_mask(seed, layer, nnz, units, p), sc, F32(0)).astype(F32)
                 for layer, units in ((1, 4 * Cw), (2, 2 * Cw)))


# ------------------------------------------------------------------------------------------------ edge MLP, forward
def model_edge_mlp_forward(emb, params, rows, cols, p, seed, whole=False, last32=False):
    """mlp_forward of csrc/edgemlp.hip, bit for bit: dict(w, h1, h2, h2lo, s1, s2, s3) with float32 w (nnz,),
    h1 (nnz, 4C), h2 (nnz, 2C), h2lo (what rounding h2 dropped, used by g_w3 when 2C <= 32) and the patterns
    s = (pre-activation > 0).
      layer 1: k ascending over [emb_r ; emb_c] padded to 32 NB0, float32 chains of 32 from zero, the blocks added in
               float64 ascending, + b1 in float64, ONE rounding, z < 0 -> 0, the dropout product in float32
      layer 2: the same with k in accumulator order inside a block (acc_row(r, 0), acc_row(r, 1) for r = 0..15)
      last:    float64 sums over the units of lane half 0, then of half 1, lower + upper, + b3 in float64, one rounding
    Mutants: whole = one float32 chain over all k of a layer; last32 = the last layer summed in float32."""
    emb = np.asarray(emb, F32)
    W1, b1, W2, b2, w3, b3 = np_params(params)
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    Cw, nnz = emb.shape[1], len(rows)
    NB0, NB1 = mlp_shape(Cw)
    D1, D2 = drop_masks(nnz, Cw, p, seed)
    f = np.concatenate([emb[rows], emb[cols]], axis=1).reshape(nnz, 2 * Cw)
    z1 = (blocked_product(W1, f, asc_blocks(NB0), whole) + b1.astype(F64)).astype(F32)
    h1 = np.where(z1 < 0, F32(0), z1)
    if p:
        h1 = (h1 * D1).astype(F32)
    z2d = blocked_product(W2, h1, acc_blocks(NB1), whole) + b2.astype(F64)
    z2 = z2d.astype(F32)
    h2 = np.where(z2 < 0, F32(0), z2)
    if p:
        h2 = (h2 * D2).astype(F32)
    h2lo = np.where(z2 > 0, ((z2d - z2.astype(F64)) * D2.astype(F64)).astype(F32), F32(0))
    w3p = np.zeros(32 * NB0, F32)
    w3p[:2 * Cw] = w3
    h2p = np.zeros((nnz, 32 * NB0), F32)
    h2p[:, :2 * Cw] = h2
    halves = []
    for h in (0, 1):
        s = np.zeros(nnz, F32 if last32 else F64)
        for b in range(NB0):
            for u in HALF_ORDER[h]:
                k = 32 * b + u
                if last32:
                    s = fma32(w3p[k], h2p[:, k], s)
                else:
                    s = s + w3p[k].astype(F64) * h2p[:, k].astype(F64)      # the product is exact in float64
        halves.append(s)
    if last32:
        z3 = ((halves[0] + halves[1]).astype(F32) + b3).astype(F32)
    else:
        z3 = ((halves[0] + halves[1]) + b3.astype(F64)).astype(F32)
    w = np.where(z3 < 0, F32(0), z3)
    return dict(w=w, h1=h1, h2=h2, h2lo=h2lo, z3=z3, s1=z1 > 0, s2=z2 > 0, s3=z3 > 0, f=f, D1=D1, D2=D2)


def scatter_nodes(n, rows, cols, per_entry, Cw):
    """g_emb from the (nnz, 2C) per-entry gradient of [emb_r ; emb_c]"""
    out = np.zeros((n, Cw), per_entry.dtype)
    np.add.at(out, rows, per_entry[:, :Cw])
    np.add.at(out, cols, per_entry[:, Cw:])
    return out


def edge_mlp_truth(n, emb, params, rows, cols, fwd, g_w, dt=LD):
    """Forward and backward on the float32 inputs in `dt`, the ReLU patterns and dropout masks of the forward model:
    (values, units), dicts over w, W1, b1, W2, b2, w3, b3, g_emb.  The units are 2^-24 times the same expressions with
    every added term replaced by its absolute value (the forward's through the three layers, the gradients' as sums
    over the entries of |d| |h|)."""
    W1, b1, W2, b2, w3, b3 = (v.astype(dt) for v in np_params(params))
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    Cw = W1.shape[1] // 2
    f = fwd["f"].astype(dt)
    D1, D2 = fwd["D1"].astype(dt), fwd["D2"].astype(dt)
    M1, M2, s3 = D1 * fwd["s1"], D2 * fwd["s2"], fwd["s3"].astype(dt)
    h1 = M1 * (f @ W1.T + b1)
    h2 = M2 * (h1 @ W2.T + b2)
    w = s3 * (h2 @ w3 + b3)
    # the units are sums of non-negative terms: float64 through BLAS is good to 1e-13 of them, and a long-double
    # product of this size costs seconds
    ab = lambda v: np.abs(v).astype(F64)
    h1a = ab(D1) * (ab(f) @ ab(W1).T + ab(b1))
    h2a = ab(D2) * (h1a @ ab(W2).T + ab(b2))
    val, unit = dict(w=w), dict(w=EPS * (h2a @ ab(w3) + ab(b3)))
    if g_w is not None:
        d3 = np.asarray(g_w, F32).astype(dt) * s3
        d2 = d3[:, None] * w3[None, :] * M2
        d1 = (d2 @ W2) * M1
        val.update(W1=d1.T @ f, b1=d1.sum(0), W2=d2.T @ h1, b2=d2.sum(0), w3=d3 @ h2, b3=d3.sum().reshape(1),
                   g_emb=scatter_nodes(n, rows, cols, d1 @ W1, Cw))
        a1, a2, a3 = ab(d1), ab(d2), ab(d3)
        unit.update(W1=a1.T @ ab(f), b1=a1.sum(0), W2=a2.T @ ab(h1), b2=a2.sum(0), w3=a3 @ ab(h2),
                    b3=a3.sum().reshape(1), g_emb=scatter_nodes(n, rows, cols, a1 @ ab(W1), Cw))
        for k in NAMES + ("g_emb",):
            unit[k] = EPS * unit[k]
    return {k: f64(v) for k, v in val.items()}, {k: f64(v) for k, v in unit.items()}


def entry_chains(Aop, Bop, length, across32=False):
    """(U, V) float64 (float32 if across32): sum_e A[e, u] B[e, v], float32 fma chains over `length` consecutive
    entries from zero in ascending order, the chains added in float64 in ascending order (across32, a mutant: in
    float32).  All chains advance together: step j takes entry j of every chain."""
    Aop, Bop = np.asarray(Aop, F32), np.asarray(Bop, F32)
    E = Aop.shape[0]
    nch = -(-E // length)
    pad = nch * length - E
    Ap = np.concatenate([Aop, np.zeros((pad, Aop.shape[1]), F32)]).reshape(nch, length, -1)
    Bp = np.concatenate([Bop, np.zeros((pad, Bop.shape[1]), F32)]).reshape(nch, length, -1)
    acc = np.zeros((nch, Aop.shape[1], Bop.shape[1]), F32)
    for j in range(length):
        acc = fma32(Ap[:, j, :, None], Bp[:, j, None, :], acc)
    if across32:
        tot = np.zeros(acc.shape[1:], F32)
        for t in range(nch):
            tot = (tot + acc[t]).astype(F32)
        return tot
    tot = np.zeros(acc.shape[1:], F64)
    for t in range(nch):
        tot += acc[t].astype(F64)
    return tot


def model_edge_mlp_backward(n, emb, params, rows, cols, p, fwd, g_w, chain=TURN, across32=False, node32=False,
                            want=NAMES + ("g_emb",)):
    """The arithmetic edge_mlp_bwd_kernel documents, from the forward model's activations: float32 dict.
      d3 = g (z3 > 0); d2 = fl(fl(d3 w3) scale) where h2 > 0; d1 = fl((W2^T d2 in chains of 32 met in float64) scale)
      where h1 > 0; g_W2, g_W1: float32 chains over the 128 entries of a turn, ascending from zero, float64 across
      turns, tiles and workgroups; g_b1, g_b2, g_w3, g_b3: float64 sums (g_w3 with h2's rounding residue when
      2C <= 32); g_emb: per entry fl(W1^T d1 in chains of 32 met in float64), a float64 sum per node, one rounding.
    Mutants: chain = TILE (chains over a whole tile), across32 (float32 across turns and tiles), node32 (a float32
    sum per node: the row's entries in CSR order, then the column's in transposed order)."""
    W1, b1, W2, b2, w3, b3 = np_params(params)
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    Cw = W1.shape[1] // 2
    NB0, NB1 = mlp_shape(Cw)
    sc = drop_scale(p)
    h1, h2, f = fwd["h1"], fwd["h2"], fwd["f"]
    d3 = np.where(fwd["z3"] > 0, np.asarray(g_w, F32), F32(0))
    d2 = np.where(h2 > 0, ((d3[:, None] * w3[None, :]).astype(F32) * sc).astype(F32), F32(0))
    d1 = np.where(h1 > 0, (blocked_product(W2.T, d2, acc_blocks(NB0)) * F64(sc)).astype(F32), F32(0))
    out = {}
    if "W2" in want:
        out["W2"] = entry_chains(d2, h1, chain, across32)
    if "W1" in want:
        out["W1"] = entry_chains(d1, f, chain, across32)
    out["b1"], out["b2"] = d1.astype(F64).sum(0), d2.astype(F64).sum(0)
    hv = h2.astype(F64) + (fwd["h2lo"].astype(F64) if NB0 == 1 else 0.0)
    out["w3"] = (d3.astype(F64)[:, None] * hv).sum(0)
    out["b3"] = d3.astype(F64).sum().reshape(1)
    if "g_emb" in want:
        ge = np.concatenate([blocked_product(W1[:, :Cw].T, d1, acc_blocks(NB1)),
                             blocked_product(W1[:, Cw:].T, d1, acc_blocks(NB1))], axis=1).astype(F32)
        if node32:
            indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
            t_indptr, order = A.transpose_order(indptr, cols)
            out["g_emb"] = (A.seg_sum(indptr, ge[:, :Cw], F32) + A.seg_sum(t_indptr, ge[order, Cw:], F32))
        else:
            out["g_emb"] = scatter_nodes(n, rows, cols, ge.astype(F64), Cw)
    return {k: np.asarray(v, F64).astype(F32) for k, v in out.items()}


# ------------------------------------------------------------------------------------------- edge MLP, inputs
def canonical(n, rows, cols):
    key = np.unique(np.asarray(rows, np.int64) * n + np.asarray(cols, np.int64))
    return n, key // n, key % n


def hub_graph(leaves):
    """node 0 with `leaves` entries as a row and as a column, and the self loops (tests/test_dcgc.py)"""
    l, ids = np.arange(1, leaves + 1), np.arange(leaves + 1)
    z = np.zeros(leaves, np.int64)
    return canonical(leaves + 1, np.r_[z, l, ids], np.r_[l, z, ids])


def random_pattern(n, nnz, seed):
    key = np.sort(np.random.default_rng(seed).choice(n * n, nnz, replace=False))
    return n, key // n, key % n


def median_split(z3):
    """tests/test_dcgc.py's recipe for -b3: a point BETWEEN two adjacent values of z3 near the median (numpy)"""
    v, counts = np.unique(z3, return_counts=True)
    if len(v) < 2:
        return v[0] - 1.0
    mids, gaps = (v[:-1] + v[1:]) / 2, v[1:] - v[:-1]
    above = 1.0 - np.cumsum(counts)[:-1] / len(z3)
    ok = (above >= 0.35) & (above <= 0.65)
    if ok.any():
        return mids[np.where(ok, gaps, 0.0).argmax()]
    return mids[np.abs(above - 0.5).argmin()]


def mlp_inputs(n, rows, cols, Cw, p, seed, kind="normal"):
    """(emb, params, g_w) float32 numpy.  normal: tests/test_dcgc.py's make_mlp (emb N(0, 1), nn.Linear's default
    initialisation from torch.manual_seed(seed)); positive: emb = |N(0, 1)| + 0.5 and every weight and bias of the
    two hidden layers and w3 replaced by its absolute value (no cancellation: a sum's error is visible against its
    absolute sum); spread: the rows of emb scaled by 10^U(-3, 3).  b3 = -median_split(z3) in float64 with the masks of
    (p, seed), so that about half of the weights are positive."""
    import torch
    import torch.nn as nn
    torch.manual_seed(seed)
    lin = [nn.Linear(2 * Cw, 4 * Cw), nn.Linear(4 * Cw, 2 * Cw), nn.Linear(2 * Cw, 1)]
    params = [t.detach().clone().numpy() for l in lin for t in (l.weight, l.bias)]
    emb = torch.randn(n, Cw).numpy()
    g_w = torch.randn(len(rows)).numpy()
    rng = np.random.default_rng(seed)
    if kind == "positive":
        emb = (np.abs(emb) + 0.5).astype(F32)
        params = [np.abs(t) for t in params]
    elif kind == "spread":
        emb = (emb * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(F32)
    else:
        assert kind == "normal", kind
    W1, b1, W2, b2, w3, b3 = np_params(params)
    if len(rows):
        D1, D2 = (m.astype(F64) for m in drop_masks(len(rows), Cw, p, seed))
        f = np.concatenate([emb[rows], emb[cols]], axis=1).astype(F64)
        h1 = np.maximum(f @ W1.astype(F64).T + b1, 0) * D1
        h2 = np.maximum(h1 @ W2.astype(F64).T + b2, 0) * D2
        b3 = F32(-median_split(h2 @ w3.astype(F64)))
    return emb, [W1, b1, W2, b2, w3.reshape(1, -1), np.asarray(b3, F32).reshape(1)], g_w.astype(F32)


# ----------------------------------------------------------------------------------------------------- SimCalib
NORM_EPS = F32(1e-12)


def padded_d(d):
    return 32 if d <= 32 else 64 if d <= 64 else 128 if d <= 128 else 256


def exp32(x):
    """the correctly rounded float32 exp of float32 arguments"""
    with np.errstate(under="ignore"):
        return np.exp(np.asarray(x, F32).astype(LD)).astype(F32)


def model_sim_scores(x, bank, tau):
    """sim_tile of csrc/simcalib.hip, bit for bit: dict(xs (n, m) float32 = fl(s_ij * fl(1 / tau)), a (n, d) the
    normalised rows, nrm (n,)).  nrm = fl32(sqrt(ss)), ss the float64 sum of squares over the even columns, then the
    odd ones, lower + upper; a = x / max(nrm, 1e-12) in float32; s_ij = the chain fma32(b_jk, a_ik, acc), k ascending
    (the zero columns up to the padded width do not move it)."""
    x, bank = np.asarray(x, F32), np.asarray(bank, F32)
    n, d = x.shape
    sq = x.astype(F64) ** 2
    halves = []
    for h in (0, 1):
        s = np.zeros(n, F64)
        for k in range(h, d, 2):
            s = s + sq[:, k]
        halves.append(s)
    nrm = np.sqrt(halves[0] + halves[1]).astype(F32)
    a = (x / np.maximum(nrm, NORM_EPS)[:, None]).astype(F32)
    acc = np.zeros((n, bank.shape[0]), F32)
    for k in range(d):
        acc = fma32(bank[None, :, k], a[:, k, None], acc)
    inv_tau = F32(1.0 / tau)
    return dict(xs=(acc * inv_tau).astype(F32), a=a, nrm=nrm, inv_tau=inv_tau)


def _softmax(xs, v):
    """(M, w, t, v - t): softmax over the rows of xs and its mean of v.  v is taken relative to the value at the row's
    largest weight, so that v_j - t_i under a weight near 1 is a sum of small terms and not the difference of two
    large ones: with inv_conf up to 1e8 and weights down to e^-100 even the long double's 64 bits lose that term when
    t_i is formed first (found on the host case `on a bank row`)."""
    M = xs.max(1, keepdims=True)
    e = np.exp(xs - M)
    w = e / e.sum(1, keepdims=True)
    ref = v[xs.argmax(1)]
    vs = v[None, :] - ref[:, None]
    ts = (w * vs).sum(1)
    return M, w, ref + ts, vs - ts[:, None]


def sim_truth(x, bank, v, g, tau, sc, dt=LD):
    """dict of (value, unit) pairs in `dt` (np.longdouble: the truth; np.float64: the second evaluation, through BLAS):
      tA   softmax and t on the model's float32 x_ij (isolates exp, the float64 sums, the rescaling, the half merge):
           unit 2^-24 (|t_i| + sum_j w_ij |v_j - t_i| (1 + |x_ij - M_i|))
      tB   end to end from x, bank, inv_conf: the same + 2^-24 (1 / tau) sum_j w_ij |v_j - t_i| sum_k |a_ik b_jk|
      gx   the weights and t of (A), a_i and |x_i| in `dt`, 1 / tau as the kernel's float32: g_i / (tau |x_i|) times
           (ga_i - a_i (a_i . ga_i)); unit 2^-24 (|g_i| / (tau |x_i|)) (G_ic + |a_ic| sum_c' |a_ic'| G_ic') with
           G_ic = sum_j w_ij |v_j - t_i| |b_jc|
    and the sensitivities to a relative error delta_j of the weights' exps, per unit of 2^-24 of max |delta|:
      tA_exp   2^-24 sum_j w_ij |v_j - t_i|                       (d t = sum_j w_j (v_j - t) delta_j)
      gx_w     the gx unit itself (G_ic): the backward's weight exp(x_ij - M_i) / den moves by w_j (delta_j - mean delta),
               delta_j of its own exp (one call) and mean delta of the forward's den (a weighted mean of its terms')
      gx_t     the gx unit with G_ic replaced by (sum_k w_ik |v_k - t_i|) (sum_j w_ij |b_jc|): the forward's t moves by
               d t above, and ga by -d t sum_j w_ij b_j, to first order"""
    x, bank, v, g = (np.asarray(t, F32).astype(dt) for t in (x, bank, v, g))
    xs = sc["xs"].astype(dt)
    M, w, t, vt = _softmax(xs, v)
    dev = w * np.abs(vt)
    out = dict(tA=(t, EPS * (np.abs(t) + (dev * (1 + np.abs(xs - M))).sum(1))), tA_exp=(t, EPS * dev.sum(1)))
    nx = np.sqrt((x * x).sum(1))
    a = x / np.maximum(nx, dt(1e-12))[:, None]
    xb = (a @ bank.T) / dt(tau)
    Mb, wb, tb, vtb = _softmax(xb, v)
    devb = wb * np.abs(vtb)
    out["tB"] = (tb, EPS * (np.abs(tb) + (devb * (1 + np.abs(xb - Mb))).sum(1)
                            + (devb * (np.abs(a) @ np.abs(bank).T)).sum(1) / dt(tau)))
    it = dt(sc["inv_tau"])
    scale = (np.abs(g) * it / nx)[:, None]
    ga = (g * it)[:, None] * ((w * vt) @ bank)
    gx = (ga - a * (a * ga).sum(1, keepdims=True)) / nx[:, None]
    jac = lambda G: EPS * scale * (G + np.abs(a) * (np.abs(a) * G).sum(1, keepdims=True))
    G = dev @ np.abs(bank)
    out["gx"] = (gx, jac(G))
    out["gx_w"] = (gx, jac(G))
    out["gx_t"] = (gx, jac(dev.sum(1, keepdims=True) * (w @ np.abs(bank))))
    return {k: (f64(a_), f64(b_)) for k, (a_, b_) in out.items()}


def _tiles(m):
    return -(-m // 32)


def model_sim_forward(xs, v, sums=F64):
    """The forward's softmax as simcalib_fwd_kernel documents it: per lane half a running maximum, den and num in
    `sums` (float64; float32 is the mutant) rescaled by exp(old max - new max) per 32-row tile, float32 exp
    (correctly rounded here), the two halves merged lower first.  Returns (t float32, stats (n, 3) float64, exps (n,):
    the largest number of exps a term of the row passes through: its own, one per rescaling by a factor other than
    exp(0) or exp(-inf), one for the merge of the halves)."""
    xs, v = np.asarray(xs, F32), np.asarray(v, F32)
    n, m = xs.shape
    nt = _tiles(m)
    xp = np.full((n, 32 * nt), -np.inf, F32)
    xp[:, :m] = xs
    vp = np.zeros(32 * nt, F32)
    vp[:m] = v
    run, moves = [], np.zeros(n, np.int64)
    with np.errstate(invalid="ignore"):
        for h in (0, 1):
            mrun = np.full(n, -np.inf, F32)
            den, num = np.zeros(n, sums), np.zeros(n, sums)
            mv = np.zeros(n, np.int64)
            for tix in range(nt):
                idx = [32 * tix + u for u in HALF_ORDER[h]]
                xr = xp[:, idx]
                mnew = np.maximum(mrun, xr.max(1))
                ms = np.where(mnew == -np.inf, F32(0), mnew)
                scale = exp32(mrun - ms)
                mv += (mnew > mrun) & (mrun > -np.inf)
                dt_, nt_ = np.zeros(n, sums), np.zeros(n, sums)
                for r in range(16):
                    e = exp32(xr[:, r] - ms)
                    if sums is F64:
                        dt_ = dt_ + e.astype(F64)
                        nt_ = nt_ + e.astype(F64) * F64(vp[idx[r]])
                    else:
                        dt_ = (dt_ + e).astype(F32)
                        nt_ = fma32(e, vp[idx[r]], nt_)
                if sums is F64:
                    den, num = den * scale.astype(F64) + dt_, num * scale.astype(F64) + nt_
                else:
                    den, num = fma32(den, scale, dt_), fma32(num, scale, nt_)
                mrun = mnew
            run.append((mrun, den, num))
            moves = np.maximum(moves, mv)
        (m0, d0, n0), (m1, d1, n1) = run
        mx = np.maximum(m0, m1)
        ms = np.where(mx == -np.inf, F32(0), mx)
        e0, e1 = exp32(m0 - ms).astype(sums), exp32(m1 - ms).astype(sums)
        dd = (d1 * e1 + d0 * e0).astype(sums)
        nn = (n1 * e1 + n0 * e0).astype(sums)
        td = (nn / dd).astype(sums)
    return td.astype(F32), np.stack([mx.astype(F64), dd.astype(F64), td.astype(F64)], axis=1), moves + 2


def model_sim_backward(x, bank, v, g, sc, stats, use_tlo=True, dot32=False):
    """simcalib_bwd_kernel as documented: the weights from the saved maximum and float64 denominator, t_i as a float32
    pair (thi, tlo), coef = fl(g / tau / den), p = fl(fl(exp * fl(fl(v - thi) - tlo)) * coef), ga += P . B_tile as ONE
    float32 chain over the whole bank in tile / accumulator order, the normalise Jacobian with a float64 row dot.
    Mutants: use_tlo=False (t_i as one float32), dot32 (the row dot in float32)."""
    x, bank, v, g = (np.asarray(t, F32) for t in (x, bank, v, g))
    n, d = x.shape
    m = bank.shape[0]
    xs, a, nrm = sc["xs"], sc["a"], sc["nrm"]
    mi = stats[:, 0].astype(F32)
    thi = stats[:, 2].astype(F32)
    tlo = (stats[:, 2] - thi.astype(F64)).astype(F32) if use_tlo else np.zeros(n, F32)
    coef = (g.astype(F64) * F64(sc["inv_tau"]) / stats[:, 1]).astype(F32)
    ga = np.zeros((n, d), F32)
    for tix in range(_tiles(m)):
        for u in ACC_ORDER:
            j = 32 * tix + u
            if j >= m:
                continue        # exp(-inf) = 0 times a zero row
            pj = ((exp32(xs[:, j] - mi) * ((v[j] - thi).astype(F32) - tlo).astype(F32)).astype(F32) * coef).astype(F32)
            ga = fma32(pj[:, None], bank[None, j, :], ga)
    if dot32:
        dot = np.zeros(n, F32)
        for k in range(d):
            dot = (dot + (a[:, k] * ga[:, k]).astype(F32)).astype(F32)
    else:
        dot = (a.astype(F64) * ga.astype(F64)).sum(1)
    fd = dot.astype(F32)
    return ((ga - (a * fd[:, None]).astype(F32)).astype(F32) / nrm[:, None]).astype(F32)


def expf_allowance(exps, sens):
    """the error the device's expf may add on top of the model's correctly rounded one: EXPF_ULP per call, 1 ulp =
    2^-23 relative = 2 units of 2^-24, `exps` calls on a term's way, times the sensitivity `sens` (sim_truth's
    tA_exp / gx_w / gx_t, which carry the 2^-24)"""
    exps = np.asarray(exps, F64)
    return 2.0 * EXPF_ULP * (exps if np.ndim(sens) == 1 else exps[:, None]) * sens


def gx_allowance(exps, tr):
    """the same for gx: its own exp and the mean of the forward's `exps` on the weights, the forward's on t"""
    exps = np.asarray(exps, F64)
    return expf_allowance(exps + 1, tr["gx_w"][1]) + expf_allowance(exps, tr["gx_t"][1])


def c_after(got, truth, unit, allow, what=""):
    """c_of with an absolute allowance taken off every element's error first"""
    got = f64(got).reshape(truth.shape)
    assert np.all(np.isfinite(got)), f"{what}: non-finite output"
    err = np.maximum(np.abs(got - truth) - allow, 0.0)
    zero = unit == 0
    assert not np.any(err[zero]), f"{what}: {int(np.count_nonzero(err[zero]))} entries with unit 0 are not exact"
    return float((err[~zero] / unit[~zero]).max()) if np.any(~zero) else 0.0


def sim_inputs(n, m, d, seed, kind="normal"):
    """tests/test_simcalib.py's make_inputs; spread: the latent rows scaled by 10^U(-3, 3); dominant: row i sits on
    bank row i mod m (similarity 1 up to rounding); flat: inv_conf = 3 + 1e-4 U, nearly constant."""
    import torch
    import torch.nn.functional as Fn
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=gen).float()
    bank = Fn.normalize(torch.randn(m, d, generator=gen).float(), p=2, dim=1)
    v = 1.0 / (0.1 + 0.9 * torch.rand(m, generator=gen).float() + 1e-8)
    gt = torch.randn(n, generator=gen).float()
    x, bank, v, gt = (t.numpy() for t in (x, bank, v, gt))
    rng = np.random.default_rng(seed)
    if kind == "spread":
        x = (x * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(F32)
    elif kind == "dominant":
        x = (bank[np.arange(n) % m] * rng.uniform(0.5, 3.0, (n, 1))).astype(F32)
    elif kind == "flat":
        v = (3.0 + 1e-4 * rng.uniform(0, 1, m)).astype(F32)
    else:
        assert kind == "normal", kind
    return x, bank, v, gt
