"""Caller-owned buffers: alignment, optional outputs, and the small ABI kernels on their own.

include/wats_hip.h asks for 4-byte aligned float buffers only; 16-byte aligned ones take the vector
paths.  pick_vec (csrc/step.hip) chooses VEC 4 / 2 / 1 from the alignment of every pointer of a launch,
and a misaligned S or H also switches the chain (no folded first launch, the generic kernel for the
final step), so the same call runs other kernels on a torch allocation (256-byte aligned, the only
kind the rest of the suite passes) than on a view into one.  Views at element offsets 1 and 2 of a
larger allocation have 4- and 8-byte aligned bases; offset 4 is 16-byte aligned again and must give
the bits of offset 0.
"""
import math

import numpy as np
import pytest
import torch

import test_handle_reuse as R
from conftest import assert_parity
from oracle import wats_oracle as O

pytestmark = pytest.mark.gpu

import wats_hip  # noqa: E402
from wats_hip import NormalizedLaplacian  # noqa: E402
from wats_hip.graphgen import random_graph  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def _np(t):
    return t.detach().cpu().numpy()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def view_at(o, n, F, src=None, dtype=torch.float32):
    """a contiguous (n, F) view at element offset o of a larger allocation, NaN (or src) inside"""
    flat = torch.full((n * F + 16,), float("nan") if dtype.is_floating_point else -1, dtype=dtype, device="cuda")
    v = flat[o:o + n * F].view(n, F)
    if src is not None:
        v.copy_(src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src)))
    assert v.is_contiguous() and v.data_ptr() == flat.data_ptr() + o * flat.element_size()
    return v


# ----------------------------------------------------------------- wg_wavelet_features
FAMILIES = {
    "g0": (R.graph_g0, {}, ["team:"]),
    "hybrid": (R.graph_hybrid, dict(tiles=1, tile_th=8, tile_max=3), ["tiles:"]),
    "valued": (R.graph_valued, {}, []),
    "lds": (lambda: R.graph_named("dense-rmat", 3000, 240000, 0), dict(lds=2, lds_cb=2048, chain=0), ["lds1:", "windows"]),
}
OFFSETS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (2, 0, 0), (0, 2, 0), (0, 0, 2), (2, 2, 2), (4, 4, 4)]


@pytest.mark.parametrize("fam,F", [("g0", F) for F in (4, 8, 40, 64, 2, 6)] + [("hybrid", F) for F in (4, 8, 40, 64)] +
                         [("valued", F) for F in (4, 8, 40, 64)] + [("lds", 1)])
def test_wavelet_features_misaligned_buffers(fam, F):
    """X0 only, S only, H only, then all three at element offsets 1 and 2 (4- and 8-byte aligned
    bases), K = 1, 3, 16: oracle parity; all three at offset 4 (16-byte aligned): the bits of offset 0."""
    get, knobs, names = FAMILIES[fam]
    A = get()
    n = A.shape[0]
    L = R.make_handle(A, knobs)
    for K in (1, 3, 16):
        Xh, ref = R.signal(fam, A, F, K), R.oracle(fam, A, F, K)
        S0, H0 = R.checked_call(L, Xh, K)
        R.check_oracle(S0, H0, ref, F, f"{fam} F={F} K={K} aligned")
        desc = L.describe(R.padded_width(F))
        if R.padded_width(F) % (16 if fam == "hybrid" else 4) == 0:   # else the family's other kernels run
            for nm in names:
                assert nm in desc, desc
        for ox, os_, oh in OFFSETS:
            X, S, H = view_at(ox, n, F, Xh), view_at(os_, n, F), view_at(oh, n, F)
            R.wf_call(L, X, S, H, K)
            torch.cuda.synchronize()
            what = f"{fam} F={F} K={K} offsets X0/S/H = {ox}/{os_}/{oh}"
            R.check_oracle(S, H, ref, F, what)
            if ox % 4 == 0 and os_ % 4 == 0 and oh % 4 == 0:
                assert torch.equal(S, S0) and torch.equal(H, H0), f"{what}: 16-byte aligned views changed the bits"
    L.close()


# which of the two judgements applies follows wavelet_chain (csrc/capi.hip): the finalize fused into the
# chain (fuse_fin: F % 4 == 0 ... and S && H), with it the folded first launch, and the one-launch F = 1
# chain all need both outputs, so a call with one of them NULL takes the multi-launch / separate-finalize
# path there ("oracle").  Where the call with both outputs already runs a separate finalize (Fp != F,
# fuse_finalize = 0, the F = 1 LDS kernels) the same kernels run and the bits are the same ("bitwise").
OPTIONAL = [
    ("g0", R.graph_g0, {}, 40, 3, "oracle"),
    ("g0", R.graph_g0, dict(fuse_finalize=0), 40, 3, "bitwise"),
    ("g0", R.graph_g0, {}, 6, 5, "bitwise"),
    ("hybrid", R.graph_hybrid, dict(tiles=1, tile_th=8, tile_max=3), 48, 3, "oracle"),
    ("valued", R.graph_valued, {}, 16, 6, "oracle"),
    ("valued", R.graph_valued, {}, 12, 6, "bitwise"),   # Fp = 16
    ("valued", R.graph_valued, {}, 3, 6, "bitwise"),
    ("lds", FAMILIES["lds"][0], FAMILIES["lds"][1], 1, 16, "bitwise"),
    ("cora-rmat", lambda: R.graph_named("cora-rmat", 2708, 10556, 0), {}, 1, 16, "oracle"),
]


@pytest.mark.parametrize("fam,get,knobs,F,K,judge", OPTIONAL,
                         ids=[f"{c[0]}-F{c[3]}-{'-'.join(c[2]) or 'default'}-{c[5]}" for c in OPTIONAL])
def test_wavelet_features_optional_outputs(fam, get, knobs, F, K, judge):
    """S = NULL or H = NULL (the other given, prefilled with NaN)"""
    A = get()
    L = R.make_handle(A, knobs)
    Xh, ref = R.signal(fam, A, F, K), R.oracle(fam, A, F, K)
    S0, H0 = R.checked_call(L, Xh, K)
    X = torch.from_numpy(Xh).cuda()
    S1, H1 = R.nan_like(*Xh.shape), R.nan_like(*Xh.shape)
    R.wf_call(L, X, S1, None, K)
    R.wf_call(L, X, None, H1, K)
    torch.cuda.synchronize()
    assert not L.chain_status()
    if judge == "bitwise":
        assert torch.equal(S1, S0), "S alone differs from S of the call with both outputs"
        assert torch.equal(H1, H0), "H alone differs from H of the call with both outputs"
    R.check_oracle(S1, H1, ref, F, f"{fam} F={F} one output")
    # both again on the same handle: the one-output calls left nothing behind
    S2, H2 = R.checked_call(L, Xh, K)
    assert torch.equal(S2, S0) and torch.equal(H2, H0)
    L.close()


# ----------------------------------------------------------------- other entry points
@pytest.mark.parametrize("o", [1, 2])
@pytest.mark.parametrize("F,K", [(40, 3), (8, 16), (6, 5)])
def test_python_entry_misaligned_signal(F, K, o):
    """graph_wavelet_features(L, X0=view): _signal's .contiguous() does not copy a contiguous view"""
    A = R.graph_g0()
    L = R.make_handle(A)
    Xh, ref = R.signal("g0", A, F, K), R.oracle("g0", A, F, K)
    X = view_at(o, A.shape[0], F, Xh)
    H, S = wats_hip.graph_wavelet_features(L, k=K, s=0.8, X0=X, return_S=True)
    torch.cuda.synchronize()
    R.check_oracle(S, H, ref, F, f"python X0 view offset {o} F={F}")
    L.close()


@pytest.mark.parametrize("o", [1, 2])
@pytest.mark.parametrize("F", [7, 64, 500])
def test_propagate_misaligned(F, o):
    """adj_norm @ x and adj_norm^T @ grad with x and grad views at 4- / 8-byte aligned bases, against the
    dense float64 product"""
    g = random_graph(900, 0.01, seed=7, directed=True, weighted=True, self_loop_frac=0.1, isolated_frac=0.05)
    adj = torch.tensor(g.to_scipy().toarray(), dtype=torch.float32, device="cuda")
    deg = adj.sum(dim=1, keepdim=True)
    deg[deg == 0] = 1
    norm = adj / deg
    op = wats_hip.RowNormalizedAdjacency.from_dense(adj)
    gen = torch.Generator("cuda").manual_seed(F)
    x = view_at(o, g.n, F, torch.randn(g.n, F, device="cuda", generator=gen)).requires_grad_(True)
    gy = view_at(o, g.n, F, torch.randn(g.n, F, device="cuda", generator=gen))
    y = wats_hip.propagate(op, x)
    y.backward(gy)
    torch.cuda.synchronize()
    assert_parity(_np(y), _np(norm.double() @ x.detach().double()), what=f"propagate view F={F}")
    assert_parity(_np(x.grad), _np(norm.double().t() @ gy.double()), what=f"propagate view grad F={F}")


@pytest.mark.parametrize("o", [1, 2])
@pytest.mark.parametrize("F,C,n", [(1, 7, 2708), (40, 41, 3000), (3, 1, 17)])
def test_fused_head_misaligned(F, C, n, o):
    """wats_head forward and backward with H, logits and the upstream gradient as misaligned views,
    against torch (test_fused_head_forward_backward_vs_torch)"""
    from torch import nn
    torch.manual_seed(F * 100 + C)
    net = nn.Sequential(nn.Linear(F, 16), nn.ReLU(), nn.Linear(16, 1)).cuda()
    H = view_at(o, n, F, torch.randn(n, F, device="cuda"))
    logits = view_at(o, n, C, 3 * torch.randn(n, C, device="cuda")).requires_grad_(True)
    out = wats_hip.wats_head(H, logits, net)
    t = net(H).squeeze(-1)
    T = torch.log(torch.exp(t) + 1.1)
    ref = torch.log_softmax(logits / T.unsqueeze(1), dim=1)
    assert_parity(_np(out), _np(ref).astype(np.float64), what="head forward")
    g = view_at(o, n, C, torch.randn(n, C, device="cuda"))
    grads = torch.autograd.grad(out, [logits] + list(net.parameters()), grad_outputs=g)
    refg = torch.autograd.grad(ref, [logits] + list(net.parameters()), grad_outputs=g)
    for a, b, name in zip(grads, refg, ["logits", "W1", "b1", "W2", "b2"]):
        assert_parity(_np(a).reshape(-1, 1), _np(b).reshape(-1, 1).astype(np.float64), tol=2e-5, what=f"d{name}")


# ----------------------------------------------------------------- the small ABI kernels, against numpy
def _lib():
    return wats_hip._lib.load()


def _map_rows(L, direction, rows):
    rows = torch.as_tensor(rows, dtype=torch.int32, device="cuda")
    out = torch.full((max(rows.numel(), 1),), -7, dtype=torch.int32, device="cuda")
    wats_hip._lib.check(_lib().wg_laplacian_map_rows(L.handle, direction, rows.data_ptr() if rows.numel() else None,
                                                     rows.numel(), out.data_ptr() if rows.numel() else None, _stream()),
                        "map_rows")
    torch.cuda.synchronize()
    return _np(out)[:rows.numel()]


@pytest.fixture(scope="module")
def g0_handle():
    L = R.make_handle(R.graph_g0())
    yield L
    L.close()


def test_map_rows(g0_handle):
    """both directions are inverse permutations of range(n); n = 0 launches nothing; a subset with
    repeats maps id by id"""
    L, n = g0_handle, g0_handle.n
    to_int = _map_rows(L, 0, np.arange(n))
    to_caller = _map_rows(L, 1, np.arange(n))
    assert np.array_equal(np.sort(to_int), np.arange(n)) and np.array_equal(np.sort(to_caller), np.arange(n))
    assert np.array_equal(to_caller[to_int], np.arange(n)) and np.array_equal(to_int[to_caller], np.arange(n))
    assert L.info["reordered"] == 1 and not np.array_equal(to_int, np.arange(n))
    assert _map_rows(L, 0, np.zeros(0)).size == 0
    sub = np.array([5, 2000, 5, n - 1, 0, 5, 2063, 7, 17, 17])
    assert np.array_equal(_map_rows(L, 0, sub), to_int[sub])
    assert np.array_equal(_map_rows(L, 1, sub), to_caller[sub])


@pytest.mark.parametrize("o", [0, 1])
@pytest.mark.parametrize("F", [1, 2, 3, 4, 40, 41, 64, 130, 256, 257, 300])
def test_permute_rows(g0_handle, F, o):
    """wg_permute_rows, exact: direction 0 puts caller row r at internal row iperm[r] (ids from
    wg_laplacian_map_rows), direction 1 undoes it (the round trip is the identity); every lane layout
    (VEC 4 / 2 / 1, F <= 64 VEC) and the wide kernel (F = 130 at VEC 2, 257, 300), aligned and
    offset-1 buffers."""
    L, n = g0_handle, g0_handle.n
    iperm = _map_rows(L, 0, np.arange(n))
    xh = np.random.default_rng(F).standard_normal((n, F)).astype(np.float32)
    x, mid, back = view_at(o, n, F, xh), view_at(o, n, F), view_at(o, n, F)
    for d, src, dst in ((0, x, mid), (1, mid, back)):
        wats_hip._lib.check(_lib().wg_permute_rows(L.handle, d, F, src.data_ptr(), dst.data_ptr(), _stream()), "permute")
    torch.cuda.synchronize()
    assert np.array_equal(_np(mid)[iperm], xh), "out[iperm] != in"
    assert np.array_equal(_np(back), xh), "the round trip is not the identity"


@pytest.mark.parametrize("F", [1, 3, 4, 48])
def test_gather_rows(F):
    """dst[i] = src[rows[i]], exact: repeats, an empty list"""
    n_src = 1000
    src = np.random.default_rng(F).standard_normal((n_src, F)).astype(np.float32)
    rows = np.r_[np.random.default_rng(1).integers(0, n_src, 700), [0, 0, n_src - 1, n_src - 1, 5, 5, 5]].astype(np.int32)
    s, r = torch.from_numpy(src).cuda(), torch.from_numpy(rows).cuda()
    dst = R.nan_like(rows.size, F)
    wats_hip._lib.check(_lib().wg_gather_rows(s.data_ptr(), r.data_ptr(), rows.size, F, dst.data_ptr(), _stream()), "gather")
    torch.cuda.synchronize()
    assert np.array_equal(_np(dst), src[rows])
    wats_hip._lib.check(_lib().wg_gather_rows(s.data_ptr(), None, 0, F, None, _stream()), "gather (empty)")
    keep = R.nan_like(4, F)
    wats_hip._lib.check(_lib().wg_gather_rows(s.data_ptr(), r.data_ptr(), 0, F, keep.data_ptr(), _stream()), "gather (n = 0)")
    torch.cuda.synchronize()
    assert bool(torch.isnan(keep).all())


def test_scale_dinv():
    """u[i] = x[i] * dinv[i] on internal rows, dinv = 1 / sqrt(w) with the oracle's degree (column sums
    minus the diagonal, w == 0 -> 1): a float32 product of a float64 dinv, so assert_parity"""
    g = random_graph(3000, 0.004, seed=1, directed=True, weighted=False, self_loop_frac=0.05, isolated_frac=0.05)
    A = g.to_scipy()
    L = NormalizedLaplacian.from_graph(g)
    assert L.info["n_isolated"] > 0
    w = np.asarray(A.sum(axis=0)).ravel().astype(np.float64) - A.diagonal().astype(np.float64)
    dinv = 1.0 / np.sqrt(np.where(w == 0, 1.0, w))
    to_caller = _map_rows(L, 1, np.arange(g.n))
    xh = np.random.default_rng(0).standard_normal(g.n).astype(np.float32)
    for o in (0, 1):
        x, u = view_at(o, g.n, 1, xh.reshape(-1, 1)), view_at(o, g.n, 1)
        wats_hip._lib.check(_lib().wg_scale_dinv(L.handle, x.data_ptr(), u.data_ptr(), _stream()), "scale_dinv")
        torch.cuda.synchronize()
        assert_parity(_np(u), (xh.astype(np.float64) * dinv[to_caller]).reshape(-1, 1), what=f"scale_dinv offset {o}")
    L.close()


def _ulps(a, b):
    """distance in float32 units in the last place (finite inputs)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("n", [1, 5, 4097])
@pytest.mark.parametrize("F", [1, 2, 3, 4, 41, 64, 65, 256, 257, 1000])
def test_row_l1_normalize(F, n):
    """wg_row_l1_normalize and the Python row_l1_normalize against O.row_l1_normalize in float64 rounded
    to float32, to 1 ulp (the kernel divides in float64 by a float64 row sum in another order than
    numpy's: the quotient differs by a few float64 ulps, which moves the float32 rounding of a near-tie
    by at most one).  An all-zero row gives H = 0 exactly; a row whose |S|_1 is 1e-9 (the 1e-8 term
    dominates); a row of 1e30 entries."""
    S = np.random.default_rng(100 * F + n).standard_normal((n, F)).astype(np.float32)
    zero_row, tiny_row, huge_row = 0, min(1, n - 1), min(2, n - 1)
    if n >= 5:
        S[zero_row] = 0.0
        S[tiny_row] = 0.0
        S[tiny_row, F // 2] = 1e-9
        S[huge_row] = 1e30
    ref = O.row_l1_normalize(S.astype(np.float64)).astype(np.float32)
    for o in (0, 1):
        s, h = view_at(o, n, F, S), view_at(o, n, F)
        wats_hip._lib.check(_lib().wg_row_l1_normalize(s.data_ptr(), h.data_ptr(), n, F, _stream()), "l1")
        torch.cuda.synchronize()
        got = _np(h)
        assert np.all(np.isfinite(got))
        assert _ulps(got, ref).max() <= 1, f"F={F} n={n} offset {o}: {_ulps(got, ref).max()} ulps"
        if n >= 5:
            assert np.all(got[zero_row] == 0.0)
            assert abs(float(got[tiny_row, F // 2]) - 1e-9 / 1.1e-8) <= 1e-7
            np.testing.assert_allclose(got[huge_row], 1.0 / F, rtol=1e-6)
    hp = wats_hip.row_l1_normalize(torch.from_numpy(S).cuda())
    assert _ulps(_np(hp), ref).max() <= 1
    assert wats_hip._lib.load().wg_row_l1_normalize(None, None, 0, F, _stream()) == 0


def _cheb_step(L, k, F, t_km1, t_km2, t_k, S=None, H=None, a0=1.0, ak=0.0):
    p = lambda t: None if t is None else t.data_ptr()
    wats_hip._lib.check(_lib().wg_cheb_step(L.handle, k, F, p(t_km1), p(t_km2), p(t_k), p(S), p(H), a0, ak, _stream()),
                        "cheb_step")


@pytest.mark.parametrize("fam,F", [("g0", 40), ("valued", 12)])
def test_cheb_step_in_place_and_fused(fam, F):
    """wg_cheb_step: t_k aliasing t_km2 (the header allows it) gives the bits of separate buffers; the
    fused S / H accumulation over K = 4 steps through the ABI equals graph_wavelet_features with the
    forward recurrence (clenshaw = 0) to assert_parity, and the oracle."""
    A = FAMILIES[fam][0]()
    n = A.shape[0]
    L = R.make_handle(A)
    rng = np.random.default_rng(F)
    t1 = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)).cuda()
    t0 = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)).cuda()
    out = R.nan_like(n, F)
    _cheb_step(L, 2, F, t1, t0, out)
    alias = t0.clone()
    _cheb_step(L, 2, F, t1, alias, alias)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out, alias), "t_k aliasing t_km2 changed the step's result"
    # the fused heat sum and normalisation, K = 4
    K, s = 4, 0.8
    Xh, ref = R.signal(fam, A, F, K), R.oracle(fam, A, F, K)
    bufs = [L.permute(torch.from_numpy(Xh).cuda(), to_internal=True), R.nan_like(n, F)]
    S, H = R.nan_like(n, F), R.nan_like(n, F)
    for k in range(1, K + 1):
        cur, nxt = bufs[(k - 1) % 2], bufs[k % 2]
        _cheb_step(L, k, F, cur, nxt if k >= 2 else None, nxt, S, H if k == K else None, 1.0, math.exp(-s * k))
    S, H = L.permute(S, to_internal=False), L.permute(H, to_internal=False)
    L.tune(clenshaw=0)
    H1, S1 = wats_hip.graph_wavelet_features(L, k=K, s=s, X0=torch.from_numpy(Xh), return_S=True)
    torch.cuda.synchronize()
    assert_parity(_np(S), _np(S1).astype(np.float64), what=f"{fam} fused steps vs clenshaw=0 S")
    assert_parity(_np(H), _np(H1).astype(np.float64), what=f"{fam} fused steps vs clenshaw=0 H")
    R.check_oracle(S, H, ref, F, f"{fam} fused steps")
    L.close()
