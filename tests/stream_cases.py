"""The registry of stream-taking entry points of include/wats_hip.h, for tests/test_streams_host.py (every
prototype with a `void* stream` is classified here) and tests/test_streams.py (every case runs off the default
stream and, where the header promises it, from a replayed graph).  Helpers; not a test.

A case names the `wg_*` entries it exercises, its class in the header's own words, `make(seed)` (a dict of input
tensors on the device) and `run(inputs)` (a tuple of output tensors; a SYNCHRONOUS case returns `(tensors, host
values)`).  `run` reads the tensors of `inputs` in place, never copies them aside before the launch and never
writes them (a `stateful` case excepted: it advances the tensors it lists), so the caller may rewrite them between
two calls or between two replays of a captured call.  Graph objects and handles are built once, on the default
stream, by `fixtures()`; signals, weights, masks, ids and upstream gradients are what a seed changes.  Shapes of one
case are the same for every seed (a SYNCHRONOUS case's outputs excepted: their sizes are the host values).

Importing this module touches no GPU.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import torch

import gats_ref

CAPTURABLE, ASYNC, SYNCHRONOUS = "CAPTURABLE", "ASYNC", "SYNCHRONOUS"
WIDTHS = (40, 7)            # one width on the 16-byte loads, one on the dword loads
REPEATS = 3                 # launches of a stateful case per comparison

# Stream-taking prototypes without a case, each with its reason.
_CHAIN = ("the wavelet chain has capture rules of its own (a synchronous first call per width, a replayed graph of "
          "the handle's), held by the capture tests of tests/test_gpu_parity.py and by tests/test_handle_reuse.py")
EXCLUDED = {
    "wg_wavelet_features": _CHAIN,
    "wg_cheb_step": "a per-step entry of the chain: " + _CHAIN,
    "wg_cheb_step_u": "a per-step entry of the chain: " + _CHAIN,
    "wg_scale_dinv": "the prologue of wg_cheb_step_u on the same plan: " + _CHAIN,
    "wg_clenshaw_step": "a per-step entry of the chain: " + _CHAIN,
    "wg_dist_wavelet_features": "csrc/dist.hip is multi-process (one process per GPU) and runs on streams of its own; "
                                "tests/test_dist.py covers it",
}

# Entries that stay ASYNC (asynchronous, not promised capturable), each with its reason; empty when every
# asynchronous case replays from a graph.
ASYNC_REASONS = {
    "wg_log1p_degree": "its only input is the handle, which a captured call binds: no input of a replay can be rewritten, "
                       "so the replay test's rule (every output differs between the two sets of inputs) has nothing to "
                       "hold it to; it is one launch without allocation, and tests/test_streams.py holds its ordering on "
                       "the fixture handle by rewriting the output buffer instead of an input",
}


class Case:
    def __init__(self, name, names, klass, make, run, stateful=(), note=""):
        self.name, self.names, self.klass, self.make, self.run = name, tuple(names), klass, make, run
        self.stateful, self.note = tuple(stateful), note

    def __repr__(self):
        return f"Case({self.name})"


CASES = []


def case(name, names, klass, stateful=(), note=""):
    def register(cls):
        CASES.append(Case(name, names, klass, cls.make, cls.run, stateful, note))
        return cls
    return register


# ------------------------------------------------------------------------------------------------ helpers
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _rng(seed, salt):
    return np.random.default_rng(1000 * salt + seed)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev())


def _normal(rng, *shape, scale=1.0):
    return _f32(rng.standard_normal(shape) * scale)


def _uniform(rng, lo, hi, *shape):
    return _f32(rng.uniform(lo, hi, shape))


def _ints(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev(), dtype=dtype)


def _leaf(t):
    return t.detach().requires_grad_(True)


def _grad(out, leaves, g):
    return torch.autograd.grad(out, leaves, g)


def _detached(outs):
    return tuple(t.detach() for t in outs)


def _stream():
    from wats_hip.laplacian import stream_handle
    return stream_handle(dev())


def _lib():
    from wats_hip import _lib
    return _lib.load()


def _check(rc, what):
    from wats_hip._lib import check
    check(rc, what)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _sorted_sets(rng, n, sizes, exclude=()):
    """ascending id sets of the given sizes drawn from [0, n) without the excluded ids, concatenated"""
    pool = np.setdiff1d(np.arange(n), np.asarray(list(exclude), np.int64))
    return np.concatenate([np.sort(rng.choice(pool, s, replace=False)) for s in sizes] + [np.zeros(0, np.int64)])


def _ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)])


@functools.lru_cache(maxsize=None)
def fixtures():
    """Everything that is built once: the graphs of the families' own tests and the objects on them."""
    from wats_hip.cagcn import SymNormGraph
    from wats_hip.dcgc import EdgeWeightGraph
    from wats_hip.gcn import RowNormalizedAdjacency, propagate
    from wats_hip.laplacian import NormalizedLaplacian
    d = dev()
    fx = SimpleNamespace()
    src, dst, n = gats_ref.star_graph(700, 50)          # a long row on the workgroup kernels beside short ones
    fx.sym_star = SymNormGraph(torch.from_numpy(np.stack([src, dst])).to(d), n, d)
    src, dst, n = gats_ref.random_graph(300, 8, False, 3)
    fx.sym_rand = SymNormGraph(torch.from_numpy(np.stack([src, dst])).to(d), n, d)
    for name in ("star", "rand"):
        sym = getattr(fx, "sym_" + name)
        # the canonical unit CSR (by destination, one self loop per node) as every other family takes it
        setattr(fx, "ewg_" + name, EdgeWeightGraph(SimpleNamespace(n=sym.n, indptr=sym.indptr, indices=sym.indices),
                                                   sym.n, d))
        setattr(fx, "op_" + name, RowNormalizedAdjacency(sym.n, sym.indptr, sym.indices, None, device=d))
    hub = fx.op_star
    fx.view_star = hub.with_flips([0, 0, 710], [5, 720, 2])       # the hub row loses an entry and gains one
    for op in (fx.op_star, fx.view_star):                          # the first call at a width sizes the workspace
        for w in WIDTHS:
            x = torch.zeros(op.n, w, device=d).requires_grad_(True)
            propagate(op, x).sum().backward()
    fx.max_len_rand = int((fx.sym_rand.indptr[1:] - fx.sym_rand.indptr[:-1]).max())
    fx.lap_rand = NormalizedLaplacian(fx.sym_rand.n, fx.sym_rand.indptr, fx.sym_rand.indices, None, device=d)
    torch.cuda.synchronize()
    return fx


def _csr_host(sym):
    return sym.indptr.cpu().numpy(), sym.indices.cpu().numpy()


# ------------------------------------------------------------------------------------------------ ingestion
@case("dense_to_csr", ["wg_dense_to_csr_count", "wg_dense_to_csr_fill"], SYNCHRONOUS)
class _DenseToCsr:
    @staticmethod
    def make(seed):
        rng = _rng(seed, 1)
        n = 300
        return dict(adj=_f32(rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.05)))

    @staticmethod
    def run(I):
        from wats_hip.laplacian import dense_to_csr
        indptr, indices, values = dense_to_csr(I["adj"])
        return (indptr, indices, values), (int(indices.numel()),)


@case("coo_to_csr", ["wg_coo_to_csr"], SYNCHRONOUS)
class _CooToCsr:
    @staticmethod
    def make(seed):
        rng = _rng(seed, 2)
        return dict(edge_index=_ints(rng.integers(0, 300, (2, 3000)), torch.int64), weights=_uniform(rng, 0.5, 2.0, 3000))

    @staticmethod
    def run(I):
        from wats_hip.ingest import edge_index_to_csr
        g = edge_index_to_csr(I["edge_index"], 300, I["weights"], duplicates="sum", symmetric=True)
        return (g.indptr, g.indices, g.values), (int(g.indices.numel()),)


@case("column_degree", ["wg_column_degree"], CAPTURABLE,
      note="float64 atomic adds: the values are small integers, so every order of the sum gives the same bits")
class _ColumnDegree:
    @staticmethod
    def make(seed):
        fx = fixtures()
        return dict(values=_f32(_rng(seed, 3).integers(1, 9, fx.sym_rand.nnz)))

    @staticmethod
    def run(I):
        sym = fixtures().sym_rand
        colsum = torch.zeros(sym.n, dtype=torch.float64, device=dev())
        diag = torch.zeros(sym.n, dtype=torch.float64, device=dev())
        _check(_lib().wg_column_degree(sym.n, 0, _ptr(sym.indptr), _ptr(sym.indices), _ptr(I["values"]), _ptr(colsum),
                                       _ptr(diag), _stream()), "column_degree")
        return colsum, diag


@case("laplacian_create", ["wg_laplacian_create", "wg_laplacian_export"], SYNCHRONOUS,
      note="the handle is the input of the export, so the two run as one unit")
class _LaplacianCreate:
    @staticmethod
    def make(seed):
        fx = fixtures()
        return dict(values=_f32(_rng(seed, 4).integers(1, 5, fx.sym_rand.nnz)))

    @staticmethod
    def run(I):
        from wats_hip.laplacian import NormalizedLaplacian
        sym = fixtures().sym_rand
        L = NormalizedLaplacian(sym.n, sym.indptr, sym.indices, I["values"], device=dev())
        values = torch.from_numpy(np.ascontiguousarray(L.export()[2]))     # the pattern is the fixed graph's
        host = (L.info["nnz"], L.info["n_isolated"], L.info["max_row_nnz"])
        L.close()
        return (values,), host


@case("log1p_degree", ["wg_log1p_degree"], ASYNC, note="behind a handle made from the seed's values (the creation waits for the stream, so this orders nothing by "
           "itself: test_log1p_degree_is_ordered_on_the_given_stream does); see ASYNC_REASONS")
class _Log1pDegree:
    make = _LaplacianCreate.make

    @staticmethod
    def run(I):
        from wats_hip.laplacian import NormalizedLaplacian
        sym = fixtures().sym_rand
        L = NormalizedLaplacian(sym.n, sym.indptr, sym.indices, I["values"], device=dev())
        x0 = L.log1p_degree()
        torch.cuda.current_stream().synchronize()      # the handle's memory is freed next
        L.close()
        return (x0,)


@case("operator_create", ["wg_operator_create"], SYNCHRONOUS,
      note="read back through one literal step (wg_permute_rows, wg_cheb_step) on the new handle")
class _OperatorCreate:
    @staticmethod
    def make(seed):
        rng = _rng(seed, 5)
        fx = fixtures()
        return dict(values=_normal(rng, fx.sym_rand.nnz), x=_normal(rng, fx.sym_rand.n, 7))

    @staticmethod
    def run(I):
        from wats_hip.laplacian import NormalizedLaplacian
        sym = fixtures().sym_rand
        L = NormalizedLaplacian.literal(sym.indptr, sym.indices, I["values"], sym.n, device=dev())
        out = torch.empty_like(I["x"])
        L.step(1, L.permute(I["x"], True), None, out)
        y = L.permute(out, False)
        host = (L.info["nnz"], L.info["max_row_nnz"])
        L.close()
        return (y,), host


@case("rownorm_create", ["wg_rownorm_create"], SYNCHRONOUS, note="read back through wg_spmm on both new handles")
class _RownormCreate:
    @staticmethod
    def make(seed):
        rng = _rng(seed, 6)
        fx = fixtures()
        return dict(values=_uniform(rng, 0.5, 2.0, fx.sym_rand.nnz), x=_normal(rng, fx.sym_rand.n, 7))

    @staticmethod
    def run(I):
        from wats_hip.gcn import RowNormalizedAdjacency
        sym = fixtures().sym_rand
        op = RowNormalizedAdjacency(sym.n, sym.indptr, sym.indices, I["values"], device=dev())
        return (op.fwd.apply(I["x"]), op.bwd.apply(I["x"]), op.deg), ()


@case("handle_rows", ["wg_permute_rows", "wg_laplacian_map_rows", "wg_gather_rows", "wg_row_l1_normalize"], CAPTURABLE)
class _HandleRows:
    @staticmethod
    def make(seed):
        rng = _rng(seed, 7)
        n = fixtures().lap_rand.n
        return dict(x=_normal(rng, n, 7), rows=_ints(rng.integers(0, n, n), torch.int32), S=_normal(rng, n, 40))

    @staticmethod
    def run(I):
        from wats_hip.wavelet import row_l1_normalize
        L = fixtures().lap_rand
        n = L.n
        lib = _lib()
        ids = [torch.empty(n, dtype=torch.int32, device=dev()) for _ in range(2)]
        for direction in (0, 1):
            _check(lib.wg_laplacian_map_rows(L.handle, direction, _ptr(I["rows"]), n, _ptr(ids[direction]), _stream()),
                   "laplacian_map_rows")
        picked = torch.empty_like(I["x"])
        _check(lib.wg_gather_rows(_ptr(I["x"]), _ptr(I["rows"]), n, 7, _ptr(picked), _stream()), "gather_rows")
        return L.permute(I["x"], True), L.permute(I["x"], False), ids[0], ids[1], picked, row_l1_normalize(I["S"])


# ------------------------------------------------------------------------------------------------ the base model's propagation
def _signals(seed, salt, n):
    rng = _rng(seed, salt)
    I = {}
    for w in WIDTHS:
        I[f"x{w}"] = _normal(rng, n, w)
        I[f"g{w}"] = _normal(rng, n, w)
    return I


def _propagate_both(op, I):
    from wats_hip.gcn import propagate
    outs = []
    for w in WIDTHS:
        x = _leaf(I[f"x{w}"])
        y = propagate(op, x)
        outs += [y, *_grad(y, [x], I[f"g{w}"])]
    return _detached(outs)


@case("spmm", ["wg_spmm"], CAPTURABLE, note="after one call at each width (fixtures): the first one sizes the workspace")
class _Spmm:
    @staticmethod
    def make(seed):
        return _signals(seed, 8, fixtures().op_star.n)

    @staticmethod
    def run(I):
        return _propagate_both(fixtures().op_star, I)


@case("flip_view", ["wg_flip_rows", "wg_flip_cols"], CAPTURABLE)
class _FlipView:
    @staticmethod
    def make(seed):
        return _signals(seed, 9, fixtures().view_star.n)

    @staticmethod
    def run(I):
        return _propagate_both(fixtures().view_star, I)


@case("sddmm_rowdot", ["wg_sddmm", "wg_rowdot"], CAPTURABLE)
class _Sddmm:
    @staticmethod
    def make(seed):
        rng = _rng(seed, 10)
        n, P = 300, 1000
        I = dict(rows=_ints(rng.integers(0, n, P), torch.int32), cols=_ints(rng.integers(0, n, P), torch.int32),
                 scale=_uniform(rng, 0.5, 2.0, n))
        for w in WIDTHS:
            I[f"A{w}"], I[f"B{w}"] = _normal(rng, n, w), _normal(rng, n, w)
        return I

    @staticmethod
    def run(I):
        from wats_hip.gcn import rowdot, sddmm
        outs = []
        for w in WIDTHS:
            term = rowdot(I[f"A{w}"], I[f"B{w}"])
            outs += [term, sddmm(I["rows"], I["cols"], I[f"A{w}"], I[f"B{w}"], row_term=term, row_scale=I["scale"],
                                 validate=False)]
        return tuple(outs)


def _overlay(seed):
    """One overlay of 12 positions in 12 distinct rows and columns of the unit random graph, a seed-dependent number of
    them on stored entries (which the flip deletes), as the device arrays `with_flips` makes of it."""
    fx = fixtures()
    rng = _rng(seed, 11)
    indptr, indices = _csr_host(fx.sym_rand)
    n, P = fx.sym_rand.n, 12
    present = 3 + seed % 5
    rows = rng.choice(np.flatnonzero(np.diff(indptr) >= 3), P, replace=False)
    cols, used = [], set()
    for i, r in enumerate(rows):
        stored = indices[indptr[r]:indptr[r + 1]]
        pool = stored[stored != r] if i < present else np.setdiff1d(np.arange(n), np.append(stored, r))
        c = next(int(c) for c in rng.permutation(pool) if int(c) not in used)
        used.add(c)
        cols.append(c)
    view = fx.op_rand.with_flips(rows.tolist(), cols, symmetric=False)
    assert view.n_positions == P and view.n_touched == P
    d = view._dev
    return {k: d[k].clone() for k in ("t_rows", "seg", "cols", "a_new", "base_pos")}


@case("flip_resolve", ["wg_flip_resolve"], CAPTURABLE, note="the wrapper reads the result to the host: direct ABI")
class _FlipResolve:
    make = staticmethod(_overlay)

    @staticmethod
    def run(I):
        op = fixtures().op_rand
        P, T = I["cols"].numel(), I["t_rows"].numel()
        a_old = torch.empty(P, dtype=torch.float32, device=dev())
        base_pos = torch.empty(P, dtype=torch.int64, device=dev())
        row_sum = torch.empty(T, dtype=torch.float64, device=dev())
        _check(_lib().wg_flip_resolve(op.n, _ptr(op.indptr), _ptr(op.indices), None, T, _ptr(I["t_rows"]), _ptr(I["seg"]),
                                      P, _ptr(I["cols"]), _ptr(a_old), _ptr(base_pos), _ptr(row_sum), _stream()),
               "flip_resolve")
        return a_old, base_pos, row_sum


@case("csr_patch", ["wg_csr_patch"], SYNCHRONOUS, note="the overlay is the input: direct ABI")
class _CsrPatch:
    make = staticmethod(_overlay)

    @staticmethod
    def run(I):
        op = fixtures().op_rand
        P, T = I["cols"].numel(), I["t_rows"].numel()
        capacity = op.nnz + P
        indptr = torch.empty(op.n + 1, dtype=torch.int64, device=dev())
        indices = torch.empty(capacity, dtype=torch.int32, device=dev())
        values = torch.empty(capacity, dtype=torch.float32, device=dev())
        nnz = ctypes.c_int64(0)
        _check(_lib().wg_csr_patch(op.n, op.nnz, _ptr(op.indptr), _ptr(op.indices), None, T, _ptr(I["t_rows"]),
                                   _ptr(I["seg"]), P, _ptr(I["cols"]), _ptr(I["a_new"]), _ptr(I["base_pos"]),
                                   _ptr(indptr), _ptr(indices), _ptr(values), capacity, ctypes.byref(nnz), _stream()),
               "csr_patch")
        return (indptr, indices[:nnz.value], values[:nnz.value]), (int(nnz.value),)


# ------------------------------------------------------------------------------------------------ GATS
@case("gat", ["wg_gat_forward", "wg_gat_backward"], CAPTURABLE)
class _Gat:
    @staticmethod
    def make(seed):
        rng = _rng(seed, 12)
        n = fixtures().sym_star.n
        I = dict(t=_normal(rng, n, 8), conf=_uniform(rng, 0.1, 1.0, n), g=_normal(rng, n, 8))
        for w in WIDTHS:
            I[f"a{w}"] = _normal(rng, n, w, scale=0.4)
        return I

    @staticmethod
    def run(I):
        from wats_hip.gats import edge_softmax_attention
        ag = fixtures().sym_star.ag
        outs = []
        for w in WIDTHS:
            a, t = _leaf(I[f"a{w}"]), _leaf(I["t"])
            sim, dconf = edge_softmax_attention(ag, a, t, I["conf"])
            outs += [sim, dconf, *_grad(sim, [a, t], I["g"])]
        return _detached(outs)


@case("csr_transpose_map", ["wg_csr_transpose_map"], SYNCHRONOUS, note="the structure is this entry's input")
class _TransposeMap:
    @staticmethod
    def make(seed):
        n, m = 300, 2400
        keys = np.sort(_rng(seed, 13).choice(n * n, m, replace=False))
        indptr = np.concatenate([[0], np.cumsum(np.bincount(keys // n, minlength=n))])
        return dict(indptr=_ints(indptr, torch.int64), indices=_ints(keys % n, torch.int32))

    @staticmethod
    def run(I):
        from wats_hip.gats import csr_transpose_map
        return csr_transpose_map(I["indptr"], I["indices"]), ()


@case("bfs_levels", ["wg_bfs_levels"], CAPTURABLE)
class _Bfs:
    @staticmethod
    def make(seed):
        n = fixtures().sym_rand.n
        return dict(mask=torch.from_numpy(_rng(seed, 14).random(n) < 0.03).to(dev()))

    @staticmethod
    def run(I):
        return (fixtures().sym_rand.ag.bfs(I["mask"], 3),)


# ------------------------------------------------------------------------------------------------ CaGCN, GETS
@case("symnorm_aggregate", ["wg_symnorm_aggregate"], CAPTURABLE)
class _SymNorm:
    @staticmethod
    def make(seed):
        I = _signals(seed, 15, fixtures().sym_star.n)
        rng = _rng(seed, 16)
        for w in WIDTHS:
            I[f"bias{w}"] = _normal(rng, w)
        return I

    @staticmethod
    def run(I):
        from wats_hip.cagcn import sym_norm_aggregate
        outs = []
        for w in WIDTHS:
            x, b = _leaf(I[f"x{w}"]), _leaf(I[f"bias{w}"])
            out = sym_norm_aggregate(fixtures().sym_star, x, b, relu=True)
            outs += [out, *_grad(out, [x, b], I[f"g{w}"])]
        return _detached(outs)


@case("gated_symnorm", ["wg_gated_symnorm_forward", "wg_gets_head_backward", "wg_gated_symnorm_transposed"], CAPTURABLE)
class _Gets:
    E, K = 3, 2

    @staticmethod
    def make(seed):
        rng = _rng(seed, 17)
        n, E, K = fixtures().sym_star.n, _Gets.E, _Gets.K
        I = dict(sel=_ints(np.argsort(rng.random((n, E)), 1)[:, :K], torch.int32), gate=_uniform(rng, 0.1, 0.9, n, K))
        for w in WIDTHS:
            I[f"z{w}"], I[f"bias{w}"] = _normal(rng, n, E, w), _normal(rng, E, w)
            I[f"logits{w}"], I[f"g{w}"] = _normal(rng, n, w, scale=2.0), _normal(rng, n, w)
        return I

    @staticmethod
    def run(I):
        from wats_hip.gets import gated_sym_norm_head
        outs = []
        for w in WIDTHS:
            z, gate, logits = _leaf(I[f"z{w}"]), _leaf(I["gate"]), _leaf(I[f"logits{w}"])
            out = gated_sym_norm_head(fixtures().sym_star, z, I["sel"], gate, I[f"bias{w}"], logits, check_selection=False)
            outs += [out, *_grad(out, [z, gate, logits], I[f"g{w}"])]
        return _detached(outs)


# ------------------------------------------------------------------------------------------------ SimCalib
@case("simcalib", ["wg_simcalib_forward", "wg_simcalib_backward"], CAPTURABLE)
class _SimCalib:
    @staticmethod
    def make(seed):
        rng = _rng(seed, 18)
        n, m = 300, 70
        I = dict(inv_conf=1.0 / _uniform(rng, 0.3, 1.0, m), g=_normal(rng, n))
        for d in WIDTHS:
            I[f"x{d}"] = _normal(rng, n, d)
            I[f"bank{d}"] = torch.nn.functional.normalize(_normal(rng, m, d), dim=1).contiguous()
        return I

    @staticmethod
    def run(I):
        from wats_hip.simcalib import similarity_temperature
        outs = []
        for d in WIDTHS:
            x = _leaf(I[f"x{d}"])
            t = similarity_temperature(x, I[f"bank{d}"], I["inv_conf"], tau=0.1)
            outs += [t, *_grad(t, [x], I["g"])]
        return _detached(outs)


# ------------------------------------------------------------------------------------------------ DCGC
@case("edge_mlp", ["wg_edge_mlp_forward", "wg_edge_mlp_backward"], CAPTURABLE,
      note="C = 8 and 33: either side of an instantiation edge, p = 0; the wrapper takes its scratch per call")
class _EdgeMlp:
    CS = (8, 33)

    @staticmethod
    def make(seed):
        rng = _rng(seed, 19)
        g = fixtures().ewg_rand
        I = dict(g=_normal(rng, g.nnz))
        for C in _EdgeMlp.CS:
            shapes = ((4 * C, 2 * C), (4 * C,), (2 * C, 4 * C), (2 * C,), (1, 2 * C), (1,))
            I[f"emb{C}"] = _normal(rng, g.n, C)
            for k, s in enumerate(shapes):
                I[f"p{C}_{k}"] = _normal(rng, *s, scale=1.0 / np.sqrt(s[-1])) + (0.5 if k == 5 else 0.0)
        return I

    @staticmethod
    def run(I):
        from wats_hip.dcgc import edge_mlp_weights
        outs = []
        for C in _EdgeMlp.CS:
            emb = _leaf(I[f"emb{C}"])
            params = [_leaf(I[f"p{C}_{k}"]) for k in range(6)]
            w = edge_mlp_weights(fixtures().ewg_rand, emb, tuple(params))
            outs += [w, *_grad(w, [emb] + params, I["g"])]
        return _detached(outs)


@case("edge_aggregate", ["wg_edge_aggregate"], CAPTURABLE, note="with wg_sddmm and wg_rowdot in its backward")
class _EdgeAggregate:
    @staticmethod
    def make(seed):
        I = _signals(seed, 20, fixtures().ewg_star.n)
        I["w"] = _uniform(_rng(seed, 21), 0.5, 1.5, fixtures().ewg_star.nnz)
        return I

    @staticmethod
    def run(I):
        from wats_hip.dcgc import weighted_propagate
        outs = []
        for width in WIDTHS:
            w, x = _leaf(I["w"]), _leaf(I[f"x{width}"])
            y = weighted_propagate(fixtures().ewg_star, w, x)
            outs += [y, *_grad(y, [w, x], I[f"g{width}"])]
        return _detached(outs)


@case("edge_pair_inv_distance", ["wg_edge_pair_inv_distance"], CAPTURABLE)
class _PairInvDistance:
    @staticmethod
    def make(seed):
        return dict(q=_normal(_rng(seed, 22), fixtures().ewg_star.n, 7))

    @staticmethod
    def run(I):
        from wats_hip.dcgc import pair_inv_distance
        return (pair_inv_distance(fixtures().ewg_star, I["q"], 0.5),)


# ------------------------------------------------------------------------------------------------ the attacks' kernels
C_ATTACK, T_ATTACK, B_ATTACK, TOPK = 7, 5, 3, 4


def _model(rng, n, Hd, nfeat=None):
    I = dict(z=_normal(rng, n, Hd), h=torch.relu(_normal(rng, n, Hd)), b1=_normal(rng, Hd, scale=0.1),
             W2=_normal(rng, C_ATTACK, Hd, scale=0.3), b2=_normal(rng, C_ATTACK, scale=0.1))
    if nfeat:
        I["W1"] = _normal(rng, Hd, nfeat, scale=0.3)
    return I


def _models(seed, salt, nfeat=None):
    rng = _rng(seed, salt)
    n = fixtures().sym_rand.n
    return rng, n, {f"{k}{Hd}": v for Hd in WIDTHS for k, v in _model(rng, n, Hd, nfeat).items()}


@case("flip_select", ["wg_flip_select"], CAPTURABLE, note="n = 300: two workgroups and the merging launch")
class _FlipSelect:
    @staticmethod
    def make(seed):
        rng = _rng(seed, 23)
        n = fixtures().sym_rand.n
        return dict(grad_loss=_normal(rng, 2 * n), grad_pmax=_normal(rng, 2 * n), grad_psmax=_normal(rng, 2 * n),
                    p_top2=_f32([0.6, 0.3]) + _uniform(rng, 0.0, 0.05, 2),
                    toggled=_ints(_sorted_sets(rng, n, [4], [T_ATTACK]), torch.int32))

    @staticmethod
    def run(I):
        from wats_hip.attack import flip_select
        sym = fixtures().sym_rand
        return flip_select(sym.n, T_ATTACK, I["grad_loss"], sym.indptr, sym.indices, None, I["toggled"], I["grad_pmax"],
                           I["grad_psmax"], I["p_top2"], topk=TOPK, return_scores=True)


@case("target_logits", ["wg_target_logits"], CAPTURABLE)
class _TargetLogits:
    SIZES = (0, 2, 3)

    @staticmethod
    def make(seed):
        rng, n, I = _models(seed, 24)
        I["cand_ptr"] = _ints(_ptr_of(_TargetLogits.SIZES), torch.int32)
        I["cand_ids"] = _ints(_sorted_sets(rng, n, _TargetLogits.SIZES, [T_ATTACK]), torch.int32)
        return I

    @staticmethod
    def run(I):
        from wats_hip.attack import target_logits
        sym = fixtures().sym_rand
        return tuple(target_logits(sym.n, sym.indptr, sym.indices, I[f"z{Hd}"], I[f"b1{Hd}"], I[f"W2{Hd}"], I[f"b2{Hd}"],
                                   T_ATTACK, (I["cand_ptr"], I["cand_ids"])) for Hd in WIDTHS)


@case("trial_logits", ["wg_trial_logits"], CAPTURABLE)
class _TrialLogits:
    SIZES, FEATS, NFEAT = (1, 2, 0), (2, 0, 1), 12

    @staticmethod
    def make(seed):
        rng, n, I = _models(seed, 25, _TrialLogits.NFEAT)
        I["trial_t"] = _ints(rng.integers(0, n, B_ATTACK), torch.int32)
        I["cand_ptr"] = _ints(_ptr_of(_TrialLogits.SIZES), torch.int32)
        I["cand_ids"] = _ints(_sorted_sets(rng, n, _TrialLogits.SIZES), torch.int32)
        I["feat_ptr"] = _ints(_ptr_of(_TrialLogits.FEATS), torch.int32)
        I["feat_ids"] = _ints(_sorted_sets(rng, _TrialLogits.NFEAT, _TrialLogits.FEATS), torch.int32)
        I["feat_delta"] = _normal(rng, sum(_TrialLogits.FEATS))
        return I

    @staticmethod
    def run(I):
        from wats_hip.attack import trial_logits
        sym = fixtures().sym_rand
        trials = tuple(I[k] for k in ("trial_t", "cand_ptr", "cand_ids", "feat_ptr", "feat_ids", "feat_delta"))
        return tuple(trial_logits(sym.n, sym.indptr, sym.indices, I[f"z{Hd}"], I[f"b1{Hd}"], I[f"W2{Hd}"], I[f"b2{Hd}"],
                                  trials, W1=I[f"W1{Hd}"]) for Hd in WIDTHS)


@case("fga_scores", ["wg_fga_scores"], CAPTURABLE,
      note="the scores, not the gradient rows: the header leaves the two (t, t) slots of a gradient row undefined")
class _FgaScores:
    SIZES = (0, 2, 1)

    @staticmethod
    def make(seed):
        rng, n, I = _models(seed, 26)
        targets = rng.choice(n, B_ATTACK, replace=False)
        I["targets"] = _ints(targets, torch.int32)
        I["tog_ptr"] = _ints(_ptr_of(_FgaScores.SIZES), torch.int32)
        I["tog_ids"] = _ints(_sorted_sets(rng, n, _FgaScores.SIZES, targets), torch.int32)
        I["g_logits"] = _normal(rng, B_ATTACK, 3, C_ATTACK)
        I["rerank"] = _ints([1, 0, 1], torch.int32)
        I["p_top2"] = _uniform(rng, 0.2, 0.6, B_ATTACK, 2)
        return I

    @staticmethod
    def run(I):
        from wats_hip.attack import fga_scores
        sym = fixtures().sym_rand
        cap = B_ATTACK * fixtures().max_len_rand + sum(_FgaScores.SIZES)
        outs = ()
        for Hd in WIDTHS:
            outs += fga_scores(sym.n, sym.indptr, sym.indices, I[f"z{Hd}"], I[f"h{Hd}"], I[f"b1{Hd}"], I[f"W2{Hd}"],
                               I["targets"], (I["tog_ptr"], I["tog_ids"]), I["g_logits"], rerank=I["rerank"],
                               p_top2=I["p_top2"], topk=TOPK, return_scores=True, local_cap=cap)
        return outs


@case("iga", ["wg_iga_path_logits", "wg_iga_scores"], CAPTURABLE)
class _Iga:
    STEPS = 3

    @staticmethod
    def make(seed):
        rng, n, I = _models(seed, 27)
        I["targets"] = _ints(rng.integers(0, n, B_ATTACK), torch.int32)
        I["g_logits"] = _normal(rng, B_ATTACK, 2 * (_Iga.STEPS + 1), C_ATTACK)
        for Hd in WIDTHS:
            I[f"zsum{Hd}"], I[f"hsum{Hd}"] = I[f"z{Hd}"].double().sum(0), I[f"h{Hd}"].double().sum(0)
        return I

    @staticmethod
    def run(I):
        from wats_hip.attack import iga_path_logits, iga_scores
        sym = fixtures().sym_rand
        outs = ()
        for Hd in WIDTHS:
            z, h, b1, W2 = I[f"z{Hd}"], I[f"h{Hd}"], I[f"b1{Hd}"], I[f"W2{Hd}"]
            logits, state = iga_path_logits(sym.n, sym.indptr, sym.indices, z, h, I[f"zsum{Hd}"], I[f"hsum{Hd}"], b1, W2,
                                            I[f"b2{Hd}"], I["targets"], _Iga.STEPS)
            outs += (logits, state) + iga_scores(sym.n, sym.indptr, sym.indices, z, h, b1, W2, I["targets"], _Iga.STEPS,
                                                 I["g_logits"], state, topk=TOPK, return_scores=True, return_coeffs=True)
        return outs


# ------------------------------------------------------------------------------------------------ TS, VS, MS, ETS
C_SCALE, N_SCALE, ROWS_SCALE, EPOCHS = 7, 700, 600, 6      # 600 listed rows: three chunks, so three arrivals


def _scale_params(rng, mode):
    C = C_SCALE
    if mode == 0:
        return [_uniform(rng, 0.5, 1.5, 1)]
    if mode == 1:
        return [_uniform(rng, 0.5, 1.5, C)]
    if mode == 2:
        return [_f32(np.eye(C)) + _normal(rng, C, C, scale=0.1), _normal(rng, C, scale=0.1)]
    return [_uniform(rng, 0.5, 1.5, 1), _uniform(rng, 0.5, 0.7, 1), _uniform(rng, 0.2, 0.3, 1), _uniform(rng, 0.05, 0.1, 1)]


def _scale_inputs(seed, salt):
    rng = _rng(seed, salt)
    I = dict(logits=_normal(rng, N_SCALE, C_SCALE, scale=2.0),
             rows=_ints(rng.permutation(N_SCALE)[:ROWS_SCALE], torch.int32),     # no repeats: see scaled_log_probs
             labels=_ints(rng.integers(0, C_SCALE, N_SCALE), torch.int64))
    return rng, I


@case("scale_row_map", ["wg_scale_forward", "wg_scale_backward"], CAPTURABLE,
      note="all four modes at C = 7 with a row list; below scaled_log_probs, whose check of the list reads the host")
class _ScaleRowMap:
    @staticmethod
    def make(seed):
        rng, I = _scale_inputs(seed, 28)
        I["g"] = _normal(rng, ROWS_SCALE, C_SCALE)
        for mode in range(4):
            for k, p in enumerate(_scale_params(rng, mode)):
                I[f"p{mode}_{k}"] = p
        return I

    @staticmethod
    def run(I):
        from wats_hip.scaling import _ScaledLogProbs
        outs = []
        for mode in range(4):
            logits = _leaf(I["logits"])
            params = [_leaf(I[k]) for k in sorted(I) if k.startswith(f"p{mode}_")]
            out = _ScaledLogProbs.apply(logits, I["rows"], mode, 1 if mode == 2 else 0, *params)
            outs += [out, *_grad(out, [logits] + params, I["g"])]
        return _detached(outs)


def _training_state(mode, block=None, init=None):
    from wats_hip.scaling import _TrainingState
    if block is None:
        return _TrainingState(mode, C_SCALE, EPOCHS, ROWS_SCALE, 3, mode == 2, dev(), init=init)
    st = object.__new__(_TrainingState)
    st.mode, st.C, st.epochs, st.flags, st.device, st.max_rows = mode, C_SCALE, EPOCHS, int(mode == 2), dev(), ROWS_SCALE
    st.block = block
    return st


@case("scale_state", ["wg_scale_state_init", "wg_scale_state_read"], CAPTURABLE,
      note="_TrainingState's constructor; one epoch, so that the traces depend on the seed; then the read without its "
           "copy to the host")
class _ScaleState:
    @staticmethod
    def make(seed):
        rng, I = _scale_inputs(seed, 29)
        I.update({f"p{mode}_{k}": p for mode in range(3) for k, p in enumerate(_scale_params(rng, mode))})
        return I

    @staticmethod
    def run(I):
        outs = []
        for mode in range(3):
            st = _training_state(mode, init=[I[k] for k in sorted(I) if k.startswith(f"p{mode}_")])
            fresh = st.block.clone()
            st.epoch(I["logits"], I["rows"], I["labels"])
            flat = torch.empty({0: 1, 1: C_SCALE, 2: C_SCALE * C_SCALE + C_SCALE}[mode], dtype=torch.float32, device=dev())
            info = torch.empty(5 + 2 * EPOCHS, dtype=torch.float64, device=dev())
            _check(_lib().wg_scale_state_read(_ptr(st.block), mode, C_SCALE, EPOCHS, _ptr(flat), _ptr(info), _stream()),
                   "scale_state_read")
            outs += [fresh, flat, info]
        return tuple(outs)


@case("scale_epoch", ["wg_scale_epoch"], CAPTURABLE, stateful=("block0", "block1", "block2"),
      note="one epoch per mode is the unit; compared: the whole state blocks after three of them")
class _ScaleEpoch:
    @staticmethod
    def make(seed):
        rng, I = _scale_inputs(seed, 30)
        for mode in range(3):
            I[f"block{mode}"] = _training_state(mode, init=_scale_params(rng, mode)).block
        return I

    @staticmethod
    def run(I):
        for mode in range(3):
            _training_state(mode, I[f"block{mode}"]).epoch(I["logits"], I["rows"], I["labels"])
        return tuple(I[f"block{mode}"] for mode in range(3))


@case("ets_label_probs", ["wg_ets_label_probs"], CAPTURABLE, note="with a row list, whose check in the wrapper reads "
                                                                   "the host: direct ABI")
class _EtsLabelProbs:
    @staticmethod
    def make(seed):
        rng, I = _scale_inputs(seed, 31)
        I["tau"] = _uniform(rng, 0.5, 1.5, 1)
        return I

    @staticmethod
    def run(I):
        p0 = torch.empty(ROWS_SCALE, dtype=torch.float64, device=dev())
        p1 = torch.empty(ROWS_SCALE, dtype=torch.float64, device=dev())
        _check(_lib().wg_ets_label_probs(N_SCALE, ROWS_SCALE, C_SCALE, _ptr(I["logits"]), _ptr(I["rows"]), _ptr(I["labels"]),
                                         _ptr(I["tau"]), _ptr(p0), _ptr(p1), _stream()), "ets_label_probs")
        return p0, p1


# ------------------------------------------------------------------------------------------------ evaluation, the WATS head
@case("calib_eval", ["wg_calib_bins", "wg_calib_ece"], CAPTURABLE,
      note="G = 2; 288 table words (kept in LDS) and 8118 (above kLdsCells = 5120: added to in place)")
class _CalibEval:
    SHAPES = ((7, 10, 2), (40, 64, 0))        # C, n_bins, kind (logits, probabilities)

    @staticmethod
    def make(seed):
        rng = _rng(seed, 32)
        n = 600
        I = dict(rows=_ints(rng.integers(0, n, 500), torch.int64))
        for C, _, kind in _CalibEval.SHAPES:
            out = _normal(rng, 2, n, C, scale=2.0)
            I[f"out{C}"] = out if kind == 2 else torch.softmax(out, dim=2).contiguous()
            I[f"labels{C}"] = _ints(rng.integers(0, C, n), torch.int64)
        return I

    @staticmethod
    def run(I):
        from wats_hip.metrics import _calib_launch
        return tuple(_calib_launch(I[f"out{C}"], I[f"labels{C}"], I["rows"], kind, n_bins, 4)[0]
                     for C, n_bins, kind in _CalibEval.SHAPES)


@case("wats_head", ["wg_wats_head_forward", "wg_wats_head_backward"], CAPTURABLE)
class _WatsHead:
    F, HID = 3, 16

    @staticmethod
    def make(seed):
        rng = _rng(seed, 33)
        n, F, hid = 300, _WatsHead.F, _WatsHead.HID
        I = dict(H=_normal(rng, n, F), W1=_normal(rng, hid, F, scale=0.5), b1=_normal(rng, hid, scale=0.1),
                 W2=_normal(rng, 1, hid, scale=0.3), b2=_normal(rng, 1, scale=0.1))
        for w in WIDTHS:
            I[f"logits{w}"], I[f"g{w}"] = _normal(rng, n, w, scale=2.0), _normal(rng, n, w)
        return I

    @staticmethod
    def run(I):
        from wats_hip.head import _WATSHead
        outs = []
        for w in WIDTHS:
            leaves = [_leaf(I[k]) for k in (f"logits{w}", "W1", "b1", "W2", "b2")]
            out = _WATSHead.apply(I["H"], *leaves)
            outs += [out, *_grad(out, leaves, I[f"g{w}"])]
        return _detached(outs)


# ------------------------------------------------------------------------------------------------ (c): the two direct-ABI probes
def abi_rowdot(I, stream):
    A, B = I["A40"], I["B40"]
    out = torch.empty(A.shape[0], dtype=torch.float32, device=dev())
    _check(_lib().wg_rowdot(A.shape[0], A.shape[1], _ptr(A), _ptr(B), _ptr(out), stream), "rowdot")
    return (out,)


def abi_symnorm(I, stream):
    sym = fixtures().sym_star
    x = I["x40"]
    out = torch.empty_like(x)
    _check(_lib().wg_symnorm_aggregate(sym.n, sym.nnz, _ptr(sym.indptr), _ptr(sym.indices), int(sym.long_rows.numel()),
                                       _ptr(sym.long_rows), _ptr(sym.dinv), x.shape[1], _ptr(x), _ptr(I["bias40"]), 1,
                                       _ptr(out), stream), "symnorm_aggregate")
    return (out,)


ABI_PROBES = {"sddmm_rowdot": abi_rowdot, "symnorm_aggregate": abi_symnorm}


# ------------------------------------------------------------------------------------------------ (d): whole calibrators
CALIBRATORS = ("WATS", "GATS", "CaGCN", "SimCalib", "DCGC", "GETS", "TS", "VS", "MS", "ETS")
N_CAL, F_CAL, C_CAL = 500, 12, 5


@functools.lru_cache(maxsize=None)
def calibrator_data():
    """A 500-node graph as the dense adjacency every calibrator takes (symmetric, self loops), a frozen sparse base
    model, labels and a validation mask; all on the default stream."""
    import wats_hip
    rng = np.random.default_rng(77)
    src, dst, n = gats_ref.random_graph(N_CAL, 8, False, 11)
    adj = np.zeros((n, n), np.float32)
    adj[src, dst] = 1.0
    np.fill_diagonal(adj, 1.0)
    torch.manual_seed(5)
    base = wats_hip.SparseCompatibleGCN(F_CAL, nclass=C_CAL, nhid=16).to(dev()).eval()
    val = torch.from_numpy(rng.random(n) < 0.3).to(dev())
    d = SimpleNamespace(adj=torch.from_numpy(adj).to(dev()), base=base, val=val,
                        y=_ints(rng.integers(0, C_CAL, n), torch.int64), x=_normal(rng, n, F_CAL))
    torch.cuda.synchronize()
    return d


def calibrator_features(seed):
    return _normal(_rng(seed, 40), N_CAL, F_CAL)


@functools.lru_cache(maxsize=None)
def calibrator(name):
    """One calibrator built with a single training epoch on the default stream, in eval mode."""
    import wats_hip
    d = calibrator_data()
    torch.manual_seed(6)
    args = (d.base, d.x, d.y, d.adj, d.val)
    if name == "WATS":
        cal = wats_hip.WATS(*args, verbose=False, fused_head=True)
    elif name == "GATS":
        cal = wats_hip.GATSCalibrator(*args, epochs=1, verbose=False)
    elif name == "CaGCN":
        cal = wats_hip.CaGCN(*args, epochs=1, verbose=False)
    elif name == "SimCalib":
        cal = wats_hip.SimCalib(*args)
    elif name == "DCGC":
        cal = wats_hip.DCGC(*args, epochs=1)
    elif name == "GETS":
        cal = wats_hip.GETSCalibrator(d.base, C_CAL, hidden_dim=16, feature_hidden_dim=8, degree_hidden_dim=4)
        cal.fit(d.adj, d.x, d.y, [~d.val, d.val, ~d.val], train=False)
        cal.calib_train(epochs=1)
    elif name in ("TS", "VS", "MS"):
        cal = getattr(wats_hip, name)(*args, verbose=False, epochs=1)
    else:
        assert name == "ETS", name
        cal = wats_hip.ETS(*args, verbose=False, epochs=1).fit([~d.val, d.val, ~d.val])
    cal.eval()
    torch.cuda.synchronize()
    return cal
