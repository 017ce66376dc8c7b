"""A call does not depend on the handle's history (DESIGN.md "State a handle carries between calls").

Every operator handle owns state that outlives a call: one workspace carved into T / u / S buffers at a
stride that depends on the padded width, plans cached per lane layout, float64 partial slots and
arrival counters of long rows, the hybrid step's tail-sum buffer, the one-launch chain's tagged
granules.  The rest of the suite runs one (X0, F, K) per fresh handle, where a read of a workspace row
or pad column the call did not write finds the right bytes.  Here one handle runs a scripted sequence
of widths and orders.  Before each checked call a POISON call (the same entry point, X0 all NaN, at
least as wide and as long) leaves NaN in every buffer the checked call may touch, and the outputs are
prefilled with NaN through the C ABI, so a stale read or an unwritten output row shows.  Each checked
call is compared bitwise with a fresh handle of the same tuning (plans are deterministic functions of
graph, width and knobs) and with the oracle at the suite's tolerances; describe() names the kernel.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import assert_parity
from oracle import wats_oracle as O
from test_team_spec import spec_graph

pytestmark = pytest.mark.gpu

import wats_hip  # noqa: E402
from wats_hip import NormalizedLaplacian  # noqa: E402
from wats_hip.graphgen import random_graph, rmat_graph  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wats_hip._lib.load()


def _np(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------- graphs (built once per process)
_GRAPHS = {}


def graph_g0():
    """spec_graph(2000) plus a 64-node path (caller ids 2000 .. 2063), block-diagonal: unweighted and
    symmetric, n = 2064, 12 948 stored entries.  The path's degree-1 and degree-2 rows interleave with
    the first component's leaves under the degree relabelling."""
    if "g0" not in _GRAPHS:
        m = 64
        i = np.arange(m - 1)
        P = sp.coo_matrix((np.ones(2 * (m - 1), np.float32), (np.r_[i, i + 1], np.r_[i + 1, i])), shape=(m, m))
        A = sp.block_diag([spec_graph(2000), P], format="csr").astype(np.float32)
        A.sort_indices()
        assert A.shape == (2064, 2064) and A.nnz == 12948 and (A != A.T).nnz == 0
        _GRAPHS["g0"] = A
    return _GRAPHS["g0"]


def graph_valued():
    if "valued" not in _GRAPHS:
        _GRAPHS["valued"] = random_graph(600, 0.02, seed=11, directed=True, weighted=True, self_loop_frac=0.05,
                                         isolated_frac=0.05).to_scipy()
    return _GRAPHS["valued"]


def graph_named(name, n, nnz, seed):
    if name not in _GRAPHS:
        _GRAPHS[name] = rmat_graph(n, nnz, seed=seed).to_scipy()
    return _GRAPHS[name]


def graph_hybrid():
    return graph_named("hybrid", 4000, 120000, 0)


def make_handle(A, knobs=None, **kw):
    unit = bool(np.all(A.data == 1.0))
    L = NormalizedLaplacian.from_csr(A.indptr.astype(np.int64), A.indices.astype(np.int32),
                                     None if unit else A.data.astype(np.float32), n=A.shape[0], **kw)
    if knobs:
        L.tune(**knobs)
    return L


def padded_width(F, fpad=0):
    """csrc/step.hip padded_features: the internal width of an F-column signal"""
    if F < 3:
        return F
    if fpad:
        return (F + fpad - 1) // fpad * fpad

    def lines(W):
        return sum(((4 * W * i) % 128 + 4 * W + 127) // 128 for i in range(32)) / 32.0
    f4, f8 = (F + 3) // 4 * 4, (F + 7) // 8 * 8
    return f8 if lines(f8) < lines(f4) - 1e-9 else f4


# ----------------------------------------------------------------- calls through the C ABI
def wf_call(L, X, S, H, K, s=0.8):
    """wg_wavelet_features on raw pointers (S or H may be None = NULL)"""
    lib = wats_hip._lib.load()
    wats_hip._lib.check(lib.wg_wavelet_features(L.handle, X.data_ptr(), X.shape[1], K, s,
                                                None if S is None else S.data_ptr(),
                                                None if H is None else H.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "wavelet_features")


def nan_like(n, F):
    return torch.full((n, F), float("nan"), dtype=torch.float32, device="cuda")


def checked_call(L, Xh, K):
    """one call with S and H prefilled with NaN: an output row the chain does not write shows"""
    X = torch.from_numpy(Xh).cuda()
    S, H = nan_like(*Xh.shape), nan_like(*Xh.shape)
    wf_call(L, X, S, H, K)
    torch.cuda.synchronize()
    return S, H


def poison_call(L, n, F, K):
    """X0 all NaN at (F, K): NaN in the workspace buffers, u buffers, partial slots, tail sums and
    granules a call at most this wide and this long uses"""
    S, H = torch.empty(n, F, device="cuda"), torch.empty(n, F, device="cuda")
    wf_call(L, nan_like(n, F), S, H, K)
    torch.cuda.synchronize()
    assert bool(torch.isnan(S).all()), "the poison call left finite rows"


def poison_shape(F, K):
    """at least as wide as the checked call's padded width (its pad columns hold NaN, not the zeros an
    equal-width call would leave) and at least as many steps; F = 1 stays on the F = 1 kernels"""
    return (1 if F == 1 else max(F, padded_width(F), (F + 7) // 8 * 8 if F % 4 else F)), max(K, 1)


# ----------------------------------------------------------------- references, once per module
_SIG, _ORACLE, _FRESH = {}, {}, {}


def signal(gkey, A, F, K, kind="rand"):
    """kind "rand": a seeded normal signal; "deg": the reference's log1p(row sums) (F = 1).  The C ABI takes no
    NULL X0 (the Python X0 = None builds this very vector with wg_log1p_degree and passes it), so the reference
    signal is computed once on a handle of its own and passed explicitly like any other."""
    key = (gkey, F, K, kind)
    if key not in _SIG:
        if kind == "deg":   # what X0 = None gives: wg_log1p_degree
            L = make_handle(A)
            _SIG[key] = _np(L.log1p_degree())
            L.close()
        else:
            _SIG[key] = np.random.default_rng(1000 * F + K).standard_normal((A.shape[0], F)).astype(np.float32)
    return _SIG[key]


def oracle(gkey, A, F, K, kind="rand"):
    key = (gkey, F, K, kind)
    if key not in _ORACLE:
        _ORACLE[key] = O.graph_wavelet_features(A, k=K, s=0.8, X0=signal(gkey, A, F, K, kind), return_all=True)
    return _ORACLE[key]


def fresh(gkey, A, knobs, F, K, kind="rand", **kw):
    """S and H of a handle that has run nothing else, per (graph, knobs, F, K, signal)"""
    key = (gkey, tuple(sorted((knobs or {}).items())), tuple(sorted(kw.items())), F, K, kind)
    if key not in _FRESH:
        L = make_handle(A, knobs, **kw)
        _FRESH[key] = checked_call(L, signal(gkey, A, F, K, kind), K)
        assert not L.chain_status()
        L.close()
    return _FRESH[key]


def check_oracle(S, H, ref, F, what):
    """assert_parity defaults on S and H; at F = 1 H = S / (|S| + 1e-8) is ill-conditioned where |S| is
    tiny, so H is compared where |S| is not and checked to be the normalisation of the S returned
    (test_lds1_directed_isolated_selfloops)"""
    Sg, Hg = _np(S), _np(H)
    assert_parity(Sg, ref["S"], what=f"{what} S")
    if F > 1:
        assert_parity(Hg, ref["H"], what=f"{what} H")
        return
    assert np.all(np.isfinite(Hg)), f"{what} H: non-finite output"
    ok = np.abs(ref["S"]) > 1e-3 * np.abs(ref["S"]).max()
    assert np.abs(Hg.astype(np.float64)[ok] - ref["H"][ok]).max() <= 1e-5, f"{what} H"
    S64 = Sg.astype(np.float64)
    np.testing.assert_allclose(Hg, (S64 / (np.abs(S64) + 1e-8)).astype(np.float32), rtol=1e-6, atol=1e-7)


def pending_zero(desc):
    for ln in desc.splitlines():
        if "pending_arrivals=" in ln:
            assert "pending_arrivals=0" in ln, ln


def is_debug_build():
    """the bounds-checked variant always runs the generic team kernel (csrc/team_dev.h team_mode_of)"""
    return "debug" in wats_hip._lib.LIB_PATH.rsplit("/", 1)[-1]


def run_sequence(gkey, A, knobs, seq, names, absent=(), repeat_at=None, kind="rand", L=None, **kw):
    """One handle through `seq` = [(F, K), ...]: a poison call before every checked call except the
    back-to-back repeat at index `repeat_at`; each checked call against the kernel named in
    describe() (`names` present -- a list, or a dict of lists per width with None for the rest --,
    `absent` missing, at the padded width), a fresh handle (bitwise) and the oracle."""
    own = L is None
    if own:
        L = make_handle(A, knobs, **kw)
    n = A.shape[0]
    for i, (F, K) in enumerate(seq):
        tag = f"{gkey} {knobs} call {i} (F={F}, K={K}, {kind})"
        if i != repeat_at:
            poison_call(L, n, *poison_shape(F, K))
            assert not L.chain_status(), f"{tag}: the poison call's chain gave up a wait"
        S, H = checked_call(L, signal(gkey, A, F, K, kind), K)
        assert not L.chain_status(), f"{tag}: a chain wait gave up"
        desc = L.describe(padded_width(F, (knobs or {}).get("fpad", 0)))
        for nm in (names.get(F, names[None]) if isinstance(names, dict) else names):
            assert nm in desc, f"{tag}: '{nm}' not in\n{desc}"
        for nm in absent:
            assert nm not in desc, f"{tag}: '{nm}' in\n{desc}"
        pending_zero(desc)
        S0, H0 = fresh(gkey, A, knobs, F, K, kind, **kw)
        bad = (~((S == S0) | (torch.isnan(S) & torch.isnan(S0)))).any(dim=1).nonzero().flatten()
        assert torch.equal(S, S0), f"{tag}: S differs from a fresh handle's in {bad.numel()} rows, first {bad[:8].tolist()}"
        assert torch.equal(H, H0), f"{tag}: H differs from a fresh handle's"
        check_oracle(S, H, oracle(gkey, A, F, K, kind), F, tag)
    if own:
        L.close()
    return L


# ----------------------------------------------------------------- the team kernel, value-free VEC 4
TEAM_SEQ = [(40, 16), (8, 3), (64, 2), (40, 16), (40, 16), (4, 1), (6, 5), (41, 4), (40, 0)]
TEAM_SHORT = [(40, 16), (8, 3), (40, 16)]


def test_team_sequence():
    """(40,16) baseline, (8,3) narrower, (64,2) wide and short, (40,16) again and once more back to back
    without a poison call, (4,1) the first launch is the final one, (6,5) Fp = 8 and (41,4) Fp = 48
    (permute_pad and a separate finalize), (40,0) no step at all."""
    A = graph_g0()
    run_sequence("g0", A, {}, TEAM_SEQ, ["team:", "spec=1"], repeat_at=4)
    if is_debug_build():
        pytest.skip("the bounds-checked build runs the generic team kernel: spec=1 names the knob only")


@pytest.mark.parametrize("F,K", [(6, 5), (41, 4)])
def test_team_padded_width_after_wider_call(F, K):
    """Fp = 8 / 48 as the first call at that width, right after a NaN call at the padded width: the
    permute_pad pass, the separate u_0 = X0 * dinv pass and the separate finalize.  What this catches is a
    stale ROW of T, u_0 or S (a scratch build that kept u_0 from the previous call at the same inner width
    fails both cases).  It does not observe the pad COLUMNS: a step is column-wise and the finalize reads F
    columns at leading dimension Fp, so a permute_pad that leaves its pad columns unwritten changes no output
    and passes (tried on a scratch build); zeroing them is hygiene, not a result the suite can pin."""
    A = graph_g0()
    run_sequence("g0", A, {}, [(F, K)], ["team:"])


@pytest.mark.parametrize("knobs,names", [
    (dict(team_spec=0), ["team:", "spec=0"]),
    (dict(fold=0), ["team:", "spec=1"]),
    (dict(team_iter=32), ["team:", "spec=1", "npot_rows="]),
    (dict(team=0, block_iter=16, chunk_iter=8, inkernel_combine=0), {40: ["split rows"], None: ["block rows"]}),
    (dict(team=0, block_iter=16, chunk_iter=8, inkernel_combine=1), {40: ["split rows"], None: ["block rows"]}),
    (dict(fuse_finalize=0), ["team:", "spec=1"]),
    (dict(clenshaw=0), ["block rows"]),
], ids=["spec0", "fold0", "team_iter32", "wg-split-combine0", "wg-split-combine1", "fuse_finalize0", "clenshaw0"])
def test_team_short_sequence_knobs(knobs, names):
    """(40,16) -> (8,3) -> (40,16) under the knobs that move state: the generic team kernel, a
    permute-in pass instead of the folded first launch, hubs as 7 part waves (a last arriver's loop),
    the workgroup kernel with split rows and arrival counters (combine kernel and in-kernel combine),
    a separate finalize, the forward recurrence (S accumulated in the workspace)."""
    A = graph_g0()
    absent = ["team:"] if knobs.get("team") == 0 or knobs.get("clenshaw") == 0 else []   # the workgroup kernel
    run_sequence("g0", A, knobs, TEAM_SHORT, names, absent=absent)
    if "spec=1" in names and is_debug_build():
        pytest.skip("the bounds-checked build runs the generic team kernel: spec=1 names the knob only")


# ----------------------------------------------------------------- the valued path
VALUED_SEQ = [(12, 6), (3, 1), (130, 0), (1, 6), (300, 6), (12, 6), (12, 6)]


@pytest.mark.parametrize("knobs,seq,rep", [({}, VALUED_SEQ, 6), (dict(tile_f=8), [(12, 6), (3, 1), (12, 6)], None)],
                         ids=["widths", "tile_f8"])
def test_valued_sequence(knobs, seq, rep):
    """A weighted directed graph (self loops, isolated nodes; the workgroup kernel with CSR values):
    widths 12 -> 3 -> 130 -> 1 -> 300 (several F tiles) -> 12 at orders 6, 1, 0, 6; tile_f = 8 splits
    F = 12 into two tiles."""
    A = graph_valued()
    # the workgroup kernel with CSR values: its row segments, and at F = 300 the widest lane layout (several F tiles)
    names = {300: ["team rows", "VEC=4 LF=64"], None: ["team rows"]}
    run_sequence("valued", A, knobs, seq, names, absent=["team:", "tiles:", "lds1:", "chain1:"], repeat_at=rep)


# ----------------------------------------------------------------- the hybrid step
HYBRID_SEQ = [(48, 6), (16, 1), (41, 3), (64, 6), (48, 6)]


@pytest.mark.parametrize("extra", [dict(hyb_conc=0), dict(hyb_conc=1), dict(hyb_conc=2), dict(team=0)],
                         ids=["conc0", "conc1", "conc2", "team0"])
def test_hybrid_sequence(extra):
    """Dense blocks on the matrix cores plus the gathered tail (its tail-sum buffer is handle state):
    widths 48 -> 16 -> 41 (Fp = 48) -> 64 -> 48 at orders 6, 1, 3, 6, sequential / auto / fused forms
    and the workgroup kernel for the tail."""
    A = graph_hybrid()
    knobs = dict(tiles=1, tile_th=8, tile_max=3, **extra)
    run_sequence("hybrid", A, knobs, HYBRID_SEQ, ["tiles:"])


# ----------------------------------------------------------------- F = 1
F1_ORDERS = [16, 1, 32, 2, 16]


@pytest.mark.parametrize("gname,gargs,knobs,names,absent", [
    ("dense-rmat", (3000, 240000, 0), dict(lds=1, lds_cb=2048, chain=0), ["lds1:", "(+combine)"], ["chain1:"]),
    ("dense-rmat", (3000, 240000, 0), dict(lds=2, lds_cb=2048, chain=0), ["lds1:", "windows"], ["chain1:"]),
    ("dense-rmat", (3000, 240000, 0), dict(lds=4, lds_cb=1024, chain=0), ["lds1:", "hub teams"], ["chain1:"]),
    ("rmat6000", (6000, 150000, 0), dict(chain_wg=5), ["chain1:"], ["(solo:"]),
    ("cora-rmat", (2708, 10556, 0), {}, ["chain1:", "(solo:"], []),
], ids=["lds1-teams", "lds2-windows", "lds4-hubs", "chain-wg5", "chain-solo"])
def test_f1_sequence(gname, gargs, knobs, names, absent):
    """F = 1: LDS row teams (block partials combined), chunk windows and hub teams on the multi-launch
    path, the one-launch chain with 5 workers (tagged granules: the tag is the granule's upper word, so
    a NaN payload must not disturb a wait) and the one-workgroup chain; orders 16 -> 1 -> 32 -> 2 -> 16
    with the reference signal log1p(degree), then with a random one, on the same handle; no wait gives
    up."""
    A = graph_named(gname, *gargs)
    seq = [(1, K) for K in F1_ORDERS]
    L = run_sequence(gname, A, knobs, seq, names, absent=absent, kind="deg", L=make_handle(A, knobs))
    run_sequence(gname, A, knobs, seq + [(1, 16)], names, absent=absent, repeat_at=5, kind="rand", L=L)
    assert not L.chain_status()
    assert "timeouts" not in L.describe(1), L.describe(1)
    L.close()


# ----------------------------------------------------------------- base-model propagation
def _dense_norm(A):
    adj = torch.tensor(A.toarray(), dtype=torch.float32, device="cuda")
    deg = adj.sum(dim=1, keepdim=True)
    deg[deg == 0] = 1
    return adj, adj / deg


def _fwd_bwd(op, x, gy):
    x = x.clone().requires_grad_(True)
    y = wats_hip.propagate(op, x)
    (y * gy).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), x.grad


def test_propagate_sequence_and_flip_view():
    """adj_norm @ x and its x-gradient on one RowNormalizedAdjacency at F = 500 -> 7 -> 64 -> 500 with
    an all-NaN forward before each: equal to a fresh operator's bit for bit and to the dense float64
    product (test_rownorm_spmm_forward_backward_vs_dense_torch).  A with_flips view of the same parent
    (10 flips) propagated between two parent calls leaves the parent's results as they were."""
    g = random_graph(900, 0.01, seed=7, directed=True, weighted=True, self_loop_frac=0.1, isolated_frac=0.05)
    adj, norm = _dense_norm(g.to_scipy())
    op = wats_hip.RowNormalizedAdjacency.from_dense(adj)
    gen = torch.Generator("cuda").manual_seed(3)
    for F in (500, 7, 64, 500):
        x = torch.randn(g.n, F, device="cuda", generator=gen)
        gy = torch.randn(g.n, F, device="cuda", generator=gen)
        yn = wats_hip.propagate(op, nan_like(g.n, F))
        torch.cuda.synchronize()
        # an empty row of adj_norm gives exactly 0, every other row sees the NaN
        assert bool(torch.isnan(yn).any(dim=1).sum() >= 0.9 * g.n)
        y, gx = _fwd_bwd(op, x, gy)
        fresh_op = wats_hip.RowNormalizedAdjacency.from_dense(adj)
        y0, gx0 = _fwd_bwd(fresh_op, x, gy)
        assert torch.equal(y, y0) and torch.equal(gx, gx0), f"F={F}: the reused operator differs from a fresh one"
        assert_parity(_np(y), _np(norm.double() @ x.double()), what=f"propagate reuse F={F}")
        assert_parity(_np(gx), _np(norm.double().t() @ gy.double()), what=f"propagate reuse grad F={F}")
    # a view of the same parent in between
    F = 64
    x = torch.randn(g.n, F, device="cuda", generator=gen)
    gy = torch.randn(g.n, F, device="cuda", generator=gen)
    y1, gx1 = _fwd_bwd(op, x, gy)
    rows = torch.arange(0, 100, 10)
    cols = rows + 301
    view = op.with_flips(rows, cols)
    yv, gxv = _fwd_bwd(view, x, gy)
    adj2 = adj.clone()
    for r, c in zip(rows.tolist(), cols.tolist()):   # calib_fga.py:901-904
        v = 1 - 2 * adj2[r, c]
        adj2[r, c] += v
        adj2[c, r] += v
    deg2 = adj2.sum(dim=1, keepdim=True)
    deg2[deg2 == 0] = 1
    norm2 = adj2 / deg2
    assert_parity(_np(yv), _np(norm2.double() @ x.double()), what="flip view forward")
    assert_parity(_np(gxv), _np(norm2.double().t() @ gy.double()), what="flip view backward")
    y2, gx2 = _fwd_bwd(op, x, gy)
    assert torch.equal(y1, y2) and torch.equal(gx1, gx2), "a view's propagation changed its parent's results"


# ----------------------------------------------------------------- the sharded chain at world 1
def test_sharded_world1_sequence():
    """wg_dist_* at world 1 (its own one-rank RCCL communicator): widths 40 -> 8 -> 1 -> 40 on one
    handle with an all-NaN call before each; the eager, the captured and the replayed call (outputs
    prefilled with NaN each time) all equal a fresh handle's and match the oracle."""
    from wats_hip.dist import ShardedWavelet
    g = rmat_graph(1500, 12000, seed=5)
    A = g.to_scipy()
    K = 8

    def shard():
        return ShardedWavelet(g.indptr, g.indices, g.values, g.n, np.array([0, g.n]), exchange="rccl", device="cuda:0")

    def three(sw, X):
        F = X.shape[1]
        H, S = nan_like(g.n, F), nan_like(g.n, F)
        outs = []
        for _ in range(3):   # eager, captured, replayed
            S.fill_(float("nan"))
            H.fill_(float("nan"))
            sw.wavelet_features(X, k=K, s=0.8, out=(H, S))
            torch.cuda.synchronize()
            outs.append((S.clone(), H.clone()))
        return outs

    sw = shard()
    for F in (40, 8, 1, 40):
        Xh = signal("world1", A, F, K)
        X = torch.from_numpy(Xh).cuda()
        Hn, Sn = sw.wavelet_features(nan_like(g.n, F), k=K, s=0.8)
        torch.cuda.synchronize()
        assert bool(torch.isnan(Sn).all())
        outs = three(sw, X)
        fr = shard()
        S0, H0 = three(fr, X)[0]
        fr.close()
        for i, (S, H) in enumerate(outs):
            assert torch.equal(S, S0) and torch.equal(H, H0), f"world 1 F={F} call {i} differs from a fresh handle's"
        check_oracle(outs[2][0], outs[2][1], oracle("world1", A, F, K), F, f"world 1 F={F}")
    sw.close()
