"""Bit-level model, long-double truths, per-element error units, a float32 model and one-property mutants of the fused
temperature head, csrc/head.hip (wg_wats_head_forward, wg_wats_head_backward).  numpy only.  Helpers of
tests/test_head_precision_host.py and tests/test_head_precision.py; not a test.

Everything works on exactly the float32 inputs the kernel receives.  EPS = 2^-24 is half a float32 ulp, relative.

t, bit for bit (model_t, head_mlp of head.hip).  pre_l = b1_l, then pre_l = fma32(W1[l, f], H[i, f], pre_l) for
f = 0..F-1 in that order; contrib_l = fl32(W2_l * max(pre_l, 0)) on the lanes l < hid and 0 on the others; the xor
butterfly over 64 lanes at the offsets 32, 16, 8, 4, 2, 1, each level fl32(v + v[lane ^ off]); t = fl32(v + b2).  The
gfx950 assembly of head.hip has the fma chain in this order (one v_fmac_f32 per f) and an unfused butterfly (six
v_add_f32), so the kernel's t_save has to EQUAL this model.  max(pre, 0) hands a NaN on (head_relu), as torch's ReLU.

Forward truth (forward_truth): np.longdouble on the kernel's own float32 t_save.  T = log(exp(t) + 1.1f) (the float32
constant, as in the kernel and in torch's float32 expression), cal = logits / T, out = cal - logsumexp(cal).  With
E = EXPF_ULP and L = LOGF_ULP the device's allowed extra error of expf and logf in ulps (1 ulp = 2 EPS; a correctly
rounded function costs 1 EPS), y = exp(t) + 1.1f, d = cal - max(cal), p = exp(out), ls = log(sum exp(d)) and
ks = ceil(C / 64) + 6:

  dT   = EPS ((1 + 2E) exp(t) / y     expf(t): its relative error reaches log(y) scaled by exp(t) / y
              + 1                     the rounding of the float32 sum y
              + (1 + 2L) T)           logf(y)
  rT   = dT / T + EPS                 the relative error of T, and the rounding of the quotient logits / T
  unit_c = rT (|cal_c| + max|cal|)    the error of cal_c and of the maximum that is taken off it
         + EPS ((1 + 2E)              expf(d_c'): a relative error of every term of the sum is at most that of the sum
                + sum_c' p_c' |d_c'|  the rounding of each d_c' = fl32(cal_c' - m) inside its exponential
                + ks                  the float32 sum: ceil(C / 64) additions per lane and six butterfly levels
                + (1 + 2L) |ls|       logf(s)
                + |d_c|               the rounding of d_c = fl32(cal_c - m)
                + |out_c|)            the rounding of out_c = fl32(d_c - ls)
  c = max |got - truth| / unit <= 1.

Backward truth (backward_truth): on the kernel's own float32 out (as lp), t_save, grad_out g and logits.
p = exp(lp), gs = sum g, dcal = g - p gs, g_logits = dcal / T, dt = -(sum_c dcal_c logits_c) exp(t) / (y T^2).

  ddcal_c = EPS (|dcal_c|                       the rounding of dcal_c (one fma in the kernel)
                 + p_c ((1 + 2E) |gs|           expf(lp_c)
                        + ks sum|g|))           the float32 sum gs
  unit_glogits_c = (ddcal_c + |dcal_c| rT) / T
  unit_dt = (sum_c |logits_c| ddcal_c + EPS (ks + 1) sum_c |dcal_c logits_c|) exp(t) / (y T^2)
                                                the error of every dcal_c, and the float32 fma chain and butterfly
          + |dt| (2 dT / T + (1 + 2E) EPS)      T twice, expf(t)
          + |sum_c dcal_c logits_c| / (y T^2) 2^-126
                                                an ABSOLUTE allowance on expf(t) where it is subnormal or flushed

The backward adds the same float32 constant 1.1f as the forward (head.hip was changed to do so; with the double 1.1 it
held before, exp(t) / (exp(t) + 1.1) differed from the forward's y by up to 0.37 EPS at small t and the unit needed
another EPS / 2 |dt|).  The parameter gradients are float64 sums over the rows, rounded once:
  g_b2 = sum_i dt_i, g_W2[l] = sum_i dt_i z_il, g_b1[l] = sum_i [pre_il > 0] dt_i W2_l,
  g_W1[l, f] = sum_i [pre_il > 0] dt_i W2_l H_if
with the ReLU pattern and z from the BIT-LEVEL model of pre; no entry is zeroed and no row is left out.  Their units
are the same sums with unit_dt_i in place of dt_i and absolute values elsewhere, plus EPS |truth| for the final
rounding.  Every bound is c <= 1 (BOUND); an element whose unit is 0 (a dead unit, a row without a gradient) must be
exactly 0.

EXPF_ULP = 1 (mfma_ref) and LOGF_ULP = 1 are ASSUMED: neither the ROCm headers nor the documents installed with them
state a figure for expf or logf.

model_forward / model_backward restate the kernels in float32 numpy with correctly rounded exp and log (the lane sums,
the butterflies, the two contracted fmas of the backward, the float64 tail); their keyword arguments turn ONE property
into the cheaper, wrong one (the mutants tests/test_head_precision_host.py rejects).
"""
import functools

import numpy as np

import agg_ref as A
import cheb_ref as C
import mfma_ref as M

EPS = A.EPS
LD = np.longdouble
F32, F64 = np.float32, np.float64
f64 = C.f64
fma32 = M.fma32
EXPF_ULP = M.EXPF_ULP   # assumed, see the module docstring
LOGF_ULP = 1.0          # assumed, see the module docstring
BOUND = 1.0
C11 = F32(1.1)
TINY = 2.0 ** -126
GRADS = ("g_logits", "W1", "b1", "W2", "b2")
PARAMS = GRADS[1:]

NS = (1, 2, 3, 4, 5, 4095, 4096, 4097)          # 4096 rows fill the grid of 1024 blocks of 4 waves once
CS = (1, 2, 7, 63, 64, 65, 129, 260)
SHAPES = ((1, 1), (15, 2), (16, 1), (16, 7), (16, 40), (17, 3), (63, 5), (64, 29))      # (hid, F)
SCALES = (1, 30)
T_LO, T_HI = -100.0, 80.0


def cases():
    """(n, C, hid, F, scale, gkind) of the GPU test: n x C at (16, 1), (hid, F) x C in {7, 65} at n in {5, 4097},
    both logit scales each, and two rows-of-one-sign gradients (inputs: "nll") at n = 4097"""
    out = [(n, Cw, 16, 1, s, "randn") for n in NS for Cw in CS for s in SCALES]
    out += [(n, Cw, hid, F, s, "randn") for hid, F in SHAPES for Cw in (7, 65) for n in (5, 4097) for s in SCALES]
    out += [(4097, 7, 16, 1, 1, "nll"), (4097, 65, 16, 7, 1, "nll")]
    return list(dict.fromkeys(out))


def case_id(case):
    return "n{}-C{}-hid{}-F{}-s{}-{}".format(*case)


# ------------------------------------------------------------------------------------------------------- inputs
def make_logits(n, Cw, scale, seed):
    """the recipe of tests/test_scaling.py's make_logits: float32 logits at the given scale; row 0 constant, row 1
    holding +-1e4 (where the shape has them)"""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((n, Cw)) * scale).astype(F32)
    if n >= 3:
        z[0] = F32(0.75 * scale)
        z[1, 0], z[1, -1] = 1e4, -1e4
    return z


def inputs(n, Cw, hid, F, scale, gkind="randn", hot_row=None):
    """dict of float32 arrays H (n, F), logits (n, C), W1 (hid, F), b1, W2 (hid,), b2 (1,), g (n, C) and the roles.

    Row i sits at h_i d + noise along one direction d, h spread evenly over [-1, 1] in a shuffled order.  The units
    alternate between +d (active for h > 0, W2 > 0, together 80 at h = 1) and -d (active for h < 0, W2 < 0, together
    -100 at h = -1), so t covers about [-100, 80] over the rows.  For hid >= 4 the last unit is DEAD on every row
    (b1 = -50, W2 = 7) and the one before it NEARLY DEAD (active for h > 0.97 only, where T is about 80 and dt small, W2 = 0.05).
    Row `zero` has H = 0; units 0 and 1 have b1 = 0, so pre == 0 there exactly.  hid = 1: one unit along +d,
    t = 180 relu(h) - 100 with h over [-0.2, 1].
    g: "randn", or "nll": -1 at argmax logits and -2^-20 elsewhere, which gives the dt_i one sign, with row 3 scaled
    by 2^24 and placed at t near 0: a float32 running sum over the rows then loses every later row.
    hot_row: that row is moved to h = 1.25, t near 100, where expf(t) is inf."""
    rng = np.random.default_rng([n, Cw, hid, F, int(scale), 0 if gkind == "randn" else 1])
    d = rng.uniform(0.5, 1.0, F) * rng.choice([-1.0, 1.0], F)
    d /= np.sqrt((d * d).sum())
    lo = -0.2 if hid == 1 else -1.0
    h = np.array([0.4]) if n == 1 else np.linspace(lo, 1.0, n)[rng.permutation(n)]
    if gkind == "nll" and n > 3:
        h[3] = 0.02
    if hot_row is not None:
        h[hot_row] = 1.25
    H = h[:, None] * d[None, :] + 0.01 * rng.standard_normal((n, F))
    zero = 2 if n >= 3 else (1 if n == 2 else None)
    if zero is not None:
        H[zero] = 0.0
    dead = hid - 1 if hid >= 4 else None
    near = hid - 2 if hid >= 4 else None
    live = [l for l in range(hid) if l not in (dead, near)]
    gain = rng.uniform(0.5, 1.5, hid)
    sgn = np.where(np.arange(hid) % 2 == 0, 1.0, -1.0)
    W1 = (sgn * gain)[:, None] * d[None, :] + 0.01 * rng.standard_normal((hid, F))
    b1 = 0.05 * rng.standard_normal(hid)
    b1[:2] = 0.0
    u = rng.uniform(0.7, 1.3, hid)
    W2 = np.zeros(hid)
    for s, top in ((1.0, T_HI), (-1.0, T_LO)):
        idx = [l for l in live if sgn[l] == s]
        if idx:
            W2[idx] = s * abs(top) * u[idx] / (gain[idx] * u[idx].sum())
    b2 = 0.3
    if hid == 1:
        W1, b1, W2, b2 = d[None, :].copy(), np.zeros(1), np.array([T_HI - T_LO]), T_LO
    if near is not None:
        W1[near], b1[near], W2[near] = gain[near] * d, -0.97 * gain[near], 0.05
    if dead is not None:
        W1[dead], b1[dead], W2[dead] = 0.1 * rng.standard_normal(F), -50.0, 7.0
    logits = make_logits(n, Cw, scale, n * 1000 + Cw)
    if gkind == "nll":
        g = np.full((n, Cw), -2.0 ** -20)     # no exact zero: dcal_c stays far above float32's underflow
        g[np.arange(n), logits.argmax(1)] = -1.0
        if n > 3:
            g[3] *= 2.0 ** 24
    else:
        assert gkind == "randn", gkind
        g = rng.standard_normal((n, Cw))
    f = lambda a: np.ascontiguousarray(a, F32)   # noqa: E731
    return dict(H=f(H), logits=logits, W1=f(W1), b1=f(b1), W2=f(W2), b2=f([b2]), g=f(g), n=n, C=Cw, hid=hid, F=F,
                zero=zero, dead=dead, near=near, hot_row=hot_row)


@functools.lru_cache(maxsize=4)
def case_inputs(case):
    """inputs(*case) with the bit-level model's t and pre (treat as read-only)"""
    I = inputs(*case)
    I["t"], I["pre"] = model_t(I)
    assert I["t"].max() < 87.0 and (I["dead"] is None or (I["pre"][:, I["dead"]] < 0).all())
    return I


# ------------------------------------------------------------------------------------------------------- float32
def exp32(x):
    """the correctly rounded float32 exp of float32 arguments"""
    with np.errstate(under="ignore", over="ignore"):
        return np.exp(np.asarray(x, F32).astype(LD)).astype(F32)


def log32(x):
    """the correctly rounded float32 log of float32 arguments"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.asarray(x, F32).astype(LD)).astype(F32)


_XOR = [np.arange(64) ^ off for off in (32, 16, 8, 4, 2, 1)]


def butterfly(v):
    """wave_sum of head.hip on (n, 64) float32 lane values: (n,) what every lane holds afterwards"""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for idx in _XOR:
            v = (v + v[:, idx]).astype(F32)
    return v[:, 0]


def by_lane(a):
    """(n, C) -> (n, ceil(C / 64), 64): column c on lane c % 64, turn c // 64; the missing columns hold 0"""
    n, Cw = a.shape
    K = -(-Cw // 64)
    p = np.zeros((n, K * 64), a.dtype)
    p[:, :Cw] = a
    return p.reshape(n, K, 64)


def lane_sum(a, drop_tail=False):
    """sum over the columns as the kernels do it: per lane in ascending turns, then the butterfly.  drop_tail (a
    mutant): a last turn that does not fill the wave is left out."""
    ch = by_lane(np.asarray(a, F32))
    turns = ch.shape[1] - (1 if drop_tail and a.shape[1] % 64 else 0)
    acc = np.zeros((a.shape[0], 64), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(turns):
            acc = (acc + ch[:, k]).astype(F32)
    return butterfly(acc)


def relu(pre):
    """head_relu of head.hip: +0 for pre <= 0, a NaN stays"""
    return np.where(pre > 0, pre, np.where(np.isnan(pre), pre, F32(0))).astype(pre.dtype)


def model_t(I, extra_lanes=False):
    """(t (n,), pre (n, hid)) float32 of head_mlp, bit for bit.  extra_lanes (a mutant): the lanes >= hid contribute
    as well, lane l with the values of unit l % hid."""
    H, W1, b1, W2, b2 = I["H"], I["W1"], I["b1"], I["W2"], I["b2"]
    n, hid = H.shape[0], W1.shape[0]
    pre = np.broadcast_to(b1[None, :], (n, hid)).astype(F32)
    for f in range(H.shape[1]):
        pre = fma32(W1[None, :, f], H[:, f, None], pre)
    with np.errstate(invalid="ignore", over="ignore"):
        contrib = (W2[None, :] * relu(pre)).astype(F32)
        lanes = np.zeros((n, 64), F32)
        lanes[:, :hid] = contrib
        if extra_lanes:
            lanes = contrib[:, np.arange(64) % hid]
        t = (butterfly(lanes) + b2[0]).astype(F32)
    return t, pre


def model_temperature(t):
    et = exp32(t)
    with np.errstate(over="ignore"):
        return et, log32((et + C11).astype(F32))


def model_forward(logits, t, first64=False, drop_tail=False, neighbour_T=False, skip_rows=()):
    """head_forward_kernel in float32 numpy, exp and log correctly rounded.  Mutants: first64 (the running maximum
    over the first 64 columns only), drop_tail (lane_sum), neighbour_T (row i divides by the T of row i - 1),
    skip_rows (those rows are never written: NaN, as the tests pre-fill)."""
    logits = np.asarray(logits, F32)
    _, T = model_temperature(t)
    if neighbour_T:
        T = np.roll(T, 1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        cal = (logits / T[:, None]).astype(F32)
        m = (cal[:, :64] if first64 else cal).max(1, keepdims=True)
        d = (cal - m).astype(F32)
        ls = log32(lane_sum(exp32(d), drop_tail))
        out = (d - ls[:, None]).astype(F32)
    out[list(skip_rows)] = np.nan
    return out


def model_backward(I, t, pre, lp, g=None, acc32=False, ge=False, no_inv_T=False, skip_rows=(), double_11=False):
    """head_backward_kernel and head_reduce_kernel in numpy: dict over GRADS, float32.  gs by lane_sum,
    dcal = fma32(-gs, exp(lp), g), g_logits = fl32(dcal / T), sum_c dcal_c logits_c as one fma chain per lane and the
    butterfly, dt and the parameter sums in float64, one rounding.  Mutants: acc32 (the parameter gradients as
    sequential float32 sums over the rows of float32 terms), ge ([pre >= 0] for [pre > 0]), no_inv_T (g_logits = dcal),
    skip_rows (rows the grid never reaches: no g_logits, no contribution), double_11 (the double 1.1 in dt that
    head.hip held before)."""
    lg, H, W2 = I["logits"], I["H"], I["W2"]
    g = np.asarray(I["g"] if g is None else g, F32)
    n, Cw = lg.shape
    et, T = model_temperature(t)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        gs = lane_sum(g)
        dcal = fma32(-gs[:, None], exp32(lp), g)
        glog = dcal if no_inv_T else (dcal / T[:, None]).astype(F32)
        dl, ll = by_lane(dcal), by_lane(lg)
        acc = np.zeros((n, 64), F32)
        for k in range(dl.shape[1]):
            acc = fma32(dl[:, k], ll[:, k], acc)
        dTs = butterfly(acc)
        dT = -dTs.astype(F64) / (T.astype(F64) * T.astype(F64))
        dt = dT * et.astype(F64) / (et.astype(F64) + (1.1 if double_11 else F64(C11)))
    keep = np.ones(n, bool)
    keep[list(skip_rows)] = False
    glog = np.where(keep[:, None], glog, F32(0))
    dt = np.where(keep, dt, 0.0)
    act = (pre >= 0) if ge else (pre > 0)
    z = relu(pre).astype(F64)
    dz = np.where(act, dt[:, None] * W2.astype(F64)[None, :], 0.0)
    if acc32:
        seq = lambda terms: np.cumsum(terms.astype(F32), axis=0, dtype=F32)[-1]   # noqa: E731
        out = dict(W1=seq(dz[:, :, None] * H.astype(F64)[:, None, :]), b1=seq(dz), W2=seq(dt[:, None] * z),
                   b2=seq(dt[:, None]))
    else:
        out = dict(W1=dz.T @ H.astype(F64), b1=dz.sum(0), W2=dt @ z, b2=dt.sum().reshape(1))
    out = {k: np.asarray(v, F64).astype(F32) for k, v in out.items()}
    out["g_logits"] = glog
    return out


# ------------------------------------------------------------------------------------------------------- truths
def _temperature(t):
    """long-double et, y, T and the absolute and relative error allowances dT, rT of the kernel's float32 T"""
    t = np.asarray(t, F32).astype(LD)
    et = np.exp(t)
    y = et + LD(C11)
    T = np.log(y)
    dT = EPS * ((1 + 2 * EXPF_ULP) * et / y + 1 + (1 + 2 * LOGF_ULP) * T)
    return et, y, T, dT, dT / T + EPS


def _ks(Cw):
    return -(-Cw // 64) + 6


def forward_truth(logits, t):
    """(truth, unit) float64 (n, C) of out on the float32 logits and the kernel's own float32 t"""
    lg = np.asarray(logits, F32).astype(LD)
    _, _, T, _, rT = _temperature(t)
    cal = lg / T[:, None]
    d = cal - cal.max(1, keepdims=True)
    ed = np.exp(d)
    s = ed.sum(1, keepdims=True)
    ls = np.log(s)
    out = d - ls
    p = ed / s
    ac = np.abs(cal)
    unit = rT[:, None] * (ac + ac.max(1, keepdims=True)) + EPS * (
        (1 + 2 * EXPF_ULP) + (p * np.abs(d)).sum(1, keepdims=True) + _ks(lg.shape[1]) + (1 + 2 * LOGF_ULP) * np.abs(ls)
        + np.abs(d) + np.abs(out))
    return f64(out), f64(unit)


def backward_truth(I, t, pre, lp, g=None):
    """{name: (truth, unit)} float64 over GRADS, on the float32 inputs, the kernel's own t and lp = out, and the
    bit-level model's pre"""
    lg, H, W2 = (I[k].astype(LD) for k in ("logits", "H", "W2"))
    g = np.asarray(I["g"] if g is None else g, F32).astype(LD)
    Cw = lg.shape[1]
    ks, E = _ks(Cw), EXPF_ULP
    et, y, T, dT, rT = _temperature(t)
    p = np.exp(np.asarray(lp, F32).astype(LD))
    gs = g.sum(1, keepdims=True)
    dcal = g - p * gs
    ddcal = EPS * (np.abs(dcal) + p * ((1 + 2 * E) * np.abs(gs) + ks * np.abs(g).sum(1, keepdims=True)))
    out = dict(g_logits=(dcal / T[:, None], (ddcal + np.abs(dcal) * rT[:, None]) / T[:, None]))
    s = (dcal * lg).sum(1)
    fac = et / (y * T * T)
    dt = -s * fac
    udt = (((np.abs(lg) * ddcal).sum(1) + EPS * (ks + 1) * np.abs(dcal * lg).sum(1)) * fac
           + np.abs(dt) * (2 * dT / T + (1 + 2 * E) * EPS) + np.abs(s) / (y * T * T) * TINY)
    pre = np.asarray(pre, F32)
    act = (pre > 0).astype(LD)
    z = relu(pre).astype(LD)
    aW2, aH = np.abs(W2), np.abs(H)
    dz, udz = act * dt[:, None] * W2[None, :], act * udt[:, None] * aW2[None, :]
    out["W1"] = (dz.T @ H, udz.T @ aH)
    out["b1"] = (dz.sum(0), udz.sum(0))
    out["W2"] = (dt @ z, udt @ z)
    out["b2"] = (dt.sum().reshape(1), udt.sum().reshape(1))
    for k in PARAMS:
        out[k] = (out[k][0], out[k][1] + EPS * np.abs(out[k][0]))
    out["dt"] = (dt, udt)
    return {k: (f64(a), f64(b)) for k, (a, b) in out.items()}


# ------------------------------------------------------------------------------------------------------- measuring
def forward_c(logits, t, out, what="out"):
    truth, unit = forward_truth(logits, t)
    return C.c_of(out, truth, unit, what)


def backward_c(I, t, pre, lp, grads, g=None, names=GRADS, truth=None):
    """{name: c} of the gradients in `grads` (a dict over `names`)"""
    truth = truth or backward_truth(I, t, pre, lp, g)
    return {k: C.c_of(grads[k], truth[k][0], truth[k][1], k) for k in names}


def rejected(fn):
    """True where the measurement fn() leaves BOUND or trips c_of's own assertions (a non-finite value, an error
    where the unit is 0); the largest c otherwise found, for the report"""
    try:
        c = fn()
    except AssertionError as e:
        return True, str(e)
    c = max(c.values()) if isinstance(c, dict) else c
    return c > BOUND, f"c={c:.3f}"
