"""GPU tests of the fused temperature head (csrc/head.hip) through its C ABI, against tests/head_ref.py.

t_save has to EQUAL the bit-level model of head_mlp.  out, g_logits and the four parameter gradients are held to
per-element units counted from the documented arithmetic (head_ref's module docstring), c <= 1, on the kernel's own
float32 t_save and out; no bound comes from a kernel's output.  Every case prints c, the bound and the c of the float32
host model on the same inputs.  The paths of the ABI are run bitwise against each other: t_save NULL in the forward
and in the backward, grad_logits NULL, a second run.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import head_ref as R  # noqa: E402
import wats_hip  # noqa: E402
from wats_hip._lib import check, load, ptr  # noqa: E402

DEV = "cuda"
WG_ERR_INVALID, WG_ERR_UNSUPPORTED = -1, -4
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    load()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(DEV).contiguous()


def host(t):
    return t.detach().cpu().numpy()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class Device:
    """the float32 inputs of a head_ref case on the device; `views`: H, logits and g as views 4 bytes past a 16-byte
    boundary"""

    def __init__(self, I, views=False):
        self.n, self.C, self.hid, self.F = I["n"], I["C"], I["hid"], I["F"]
        self.keep = []
        place = self.view_at_4 if views else dev
        self.H, self.logits, self.g = place(I["H"]), place(I["logits"]), place(I["g"])
        self.W1, self.b1, self.W2, self.b2 = (dev(I[k]) for k in ("W1", "b1", "W2", "b2"))

    def view_at_4(self, a):
        buf = torch.zeros(a.size + 8, dtype=torch.float32, device=DEV)
        off = ((4 - buf.data_ptr()) % 16) // 4
        v = buf[off:off + a.size].view(a.shape)
        v.copy_(torch.as_tensor(np.ascontiguousarray(a, np.float32)))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        self.keep.append(buf)
        return v

    def shape_args(self):
        return (self.n, self.F, self.C, self.hid, ptr(self.H), ptr(self.logits), ptr(self.W1), ptr(self.b1),
                ptr(self.W2), ptr(self.b2))

    def forward_rc(self, t_save=True):
        out = torch.full((max(self.n, 1), self.C), NAN, dtype=torch.float32, device=DEV)
        t = torch.full((max(self.n, 1),), NAN, dtype=torch.float32, device=DEV) if t_save else None
        rc = load().wg_wats_head_forward(*self.shape_args(), ptr(out), ptr(t), stream())
        torch.cuda.synchronize()
        return rc, out[:self.n], (t[:self.n] if t_save else None)

    def forward(self, t_save=True):
        rc, out, t = self.forward_rc(t_save)
        check(rc, "wats_head_forward")
        return out, t

    def backward_rc(self, out, t, g=None, glogits=True):
        """(rc, dict over head_ref.GRADS of numpy arrays); every output buffer is pre-filled with NaN"""
        nbytes = ctypes.c_int64(0)
        check(load().wg_wats_head_workspace(self.n, self.F, self.hid, ctypes.byref(nbytes)), "wats_head_workspace")
        ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=DEV)
        full = lambda *s: torch.full(s, NAN, dtype=torch.float32, device=DEV)   # noqa: E731
        gl = full(max(self.n, 1), self.C) if glogits else None
        gW1, gb1, gW2, gb2 = full(self.hid, self.F), full(self.hid), full(self.hid), full(1)
        g = self.g if g is None else g
        rc = load().wg_wats_head_backward(*self.shape_args(), ptr(out), ptr(t), ptr(g), ptr(gl), ptr(gW1), ptr(gb1),
                                          ptr(gW2), ptr(gb2), ptr(ws), stream())
        torch.cuda.synchronize()
        grads = dict(W1=host(gW1), b1=host(gb1), W2=host(gW2), b2=host(gb2))
        if glogits:
            grads["g_logits"] = host(gl[:self.n])
        return rc, grads

    def backward(self, out, t, g=None, glogits=True):
        rc, grads = self.backward_rc(out, t, g, glogits)
        check(rc, "wats_head_backward")
        return grads


def hold(I, D, label, g=None):
    """the whole list of assertions of one input: returns (out, t, grads) as numpy"""
    out_d, t_d = D.forward()
    out, t = host(out_d), host(t_d)
    assert same_bits(t, I["t"]), f"{label}: t_save differs from the bit-level model in " \
        f"{np.count_nonzero(bits(t) != bits(I['t']))} of {t.size} rows"
    c_model = R.forward_c(I["logits"], t, R.model_forward(I["logits"], t), "model out")
    R.C.report(f"{label} out", R.forward_c(I["logits"], t, out), R.BOUND, f"host model c={c_model:.3f}")
    assert same_bits(host(D.forward(t_save=False)[0]), out), f"{label}: out differs with t_save = NULL"
    assert same_bits(host(D.forward()[0]), out), f"{label}: a second forward differs"

    g_d = None if g is None else dev(g)
    grads = D.backward(out_d, t_d, g_d)
    truth = R.backward_truth(I, t, I["pre"], out, g)
    c_model = R.backward_c(I, t, I["pre"], out, R.model_backward(I, t, I["pre"], out, g=g), truth=truth)
    for k, c in R.backward_c(I, t, I["pre"], out, grads, truth=truth).items():
        R.C.report(f"{label} {k}", c, R.BOUND, f"host model c={c_model[k]:.3f}")
    again = D.backward(out_d, t_d, g_d)
    assert all(same_bits(again[k], grads[k]) for k in R.GRADS), f"{label}: a second backward differs"
    null = D.backward(out_d, None, g_d)
    assert all(same_bits(null[k], grads[k]) for k in R.GRADS), f"{label}: the backward differs with t_save = NULL"
    bare = D.backward(out_d, t_d, g_d, glogits=False)
    assert all(same_bits(bare[k], grads[k]) for k in R.PARAMS), f"{label}: the backward differs with grad_logits = NULL"
    if I["dead"] is not None:
        assert not grads["W1"][I["dead"]].any() and grads["b1"][I["dead"]] == 0 and grads["W2"][I["dead"]] == 0
    return out, t, grads


@pytest.mark.parametrize("case", R.cases(), ids=R.case_id)
def test_head_holds_its_bounds(case):
    I = R.case_inputs(case)
    hold(I, Device(I), R.case_id(case))


@pytest.mark.parametrize("r", [0, 4095, 4096])
def test_one_row_of_grad_out(r):
    """grad_out in one row alone, before, at and after the grid's wrap: the parameter gradients are held to that single
    row's unit, and every other row of g_logits is exactly 0"""
    case = (4097, 7, 16, 1, 1, "randn")
    I = R.case_inputs(case)
    g = np.zeros_like(I["g"])
    g[r] = I["g"][r]
    _, _, grads = hold(I, Device(I), f"{R.case_id(case)} row {r} alone", g=g)
    others = np.arange(case[0]) != r
    assert not grads["g_logits"][others].any() and grads["g_logits"][r].any()


def test_caller_buffers_four_bytes_past_a_boundary():
    case = (4097, 65, 16, 7, 1, "randn")
    I = R.case_inputs(case)
    out, t, grads = hold(I, Device(I, views=True), f"{R.case_id(case)} views")
    D = Device(I)
    o2, t2 = D.forward()
    g2 = D.backward(o2, t2)
    assert same_bits(out, host(o2)) and all(same_bits(grads[k], g2[k]) for k in R.GRADS)


def test_largest_lds_shape_and_the_refusal_beyond_it():
    """hid = 64, F = 29 (P = 1985, 63 520 bytes of dynamic LDS) runs and holds its bounds (it is among the cases; here at
    n = 3); hid = 64, F = 30 is refused by the backward, which writes nothing; its forward still runs"""
    I = R.inputs(3, 7, 64, 29, 1)
    I["t"], I["pre"] = R.model_t(I)
    hold(I, Device(I), "n3-C7-hid64-F29")
    I = R.inputs(5, 7, 64, 30, 1)
    I["t"], I["pre"] = R.model_t(I)
    D = Device(I)
    out_d, t_d = D.forward()
    assert same_bits(host(t_d), I["t"])
    R.C.report("hid64-F30 out", R.forward_c(I["logits"], I["t"], host(out_d)), R.BOUND)
    rc, grads = D.backward_rc(out_d, t_d)
    assert rc == WG_ERR_UNSUPPORTED
    assert all(np.isnan(v).all() for v in grads.values()), "a refused backward wrote to a gradient buffer"


def test_invalid_arguments_and_no_rows():
    I = R.inputs(5, 7, 16, 1, 1)
    D = Device(I)
    out_d, t_d = D.forward()
    D.hid = 65
    assert D.forward_rc()[0] == WG_ERR_INVALID and D.backward_rc(out_d, t_d)[0] == WG_ERR_INVALID
    D.hid, D.n = 16, -1
    assert D.forward_rc()[0] == WG_ERR_INVALID
    # wg_wats_head_workspace refuses n < 0 as well: the backward is called with a workspace of its own
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    gW1, gb1, gW2, gb2 = (torch.full((k,), NAN, device=DEV) for k in (16, 16, 16, 1))
    rc = load().wg_wats_head_backward(*D.shape_args(), ptr(out_d), ptr(t_d), ptr(D.g), None, ptr(gW1), ptr(gb1),
                                      ptr(gW2), ptr(gb2), ptr(ws), stream())
    assert rc == WG_ERR_INVALID
    D.n = 0
    rc, out, _ = D.forward_rc()
    assert rc == 0
    grads = D.backward(out_d, t_d, glogits=False)
    assert all(not bits(grads[k]).any() for k in R.PARAMS), "n = 0: the parameter gradients are not exactly 0"


def nonfinite_case():
    case = (300, 65, 16, 7, 1, "randn")
    I = R.inputs(*case)
    I["t"], I["pre"] = R.model_t(I)
    D = Device(I)
    out_d, t_d = D.forward()
    return I, host(out_d), D.backward(out_d, t_d)


@pytest.mark.parametrize("where", ["H", "logits"])
def test_a_nan_stays_in_its_row(where):
    """a NaN in one row of H or of logits: every other row of out and g_logits is bitwise what it is without it; the
    row itself is NaN in out (head_relu hands the NaN on, as torch's ReLU), and so are g_b2 and g_W2"""
    I, out0, grads0 = nonfinite_case()
    r = 137
    bad = dict(I)
    bad[where] = I[where].copy()
    bad[where][r, 0] = np.nan
    D = Device(bad)
    out_d, t_d = D.forward()
    grads = D.backward(out_d, t_d)
    out = host(out_d)
    others = np.arange(I["n"]) != r
    assert same_bits(out[others], out0[others]) and same_bits(grads["g_logits"][others], grads0["g_logits"][others])
    assert np.isnan(out[r]).all() and np.isnan(grads["g_logits"][r]).all()
    assert np.isnan(grads["b2"]).all() and np.isnan(grads["W2"]).all()
    if where == "H":
        assert np.isnan(host(t_d)[r])


def test_a_row_whose_exp_overflows():
    """t > 88.8, expf(t) = inf, T = inf: the row of out is finite and constant (-log C), its g_logits row is 0, every
    other row is untouched, and the parameter gradients are non-finite where torch's float32 expression on the device
    has them non-finite"""
    I0, out0, grads0 = nonfinite_case()
    r = 41
    I = R.inputs(300, 65, 16, 7, 1, hot_row=r)
    I["t"], I["pre"] = R.model_t(I)
    assert I["t"][r] > 88.8 and np.count_nonzero(I["t"] > 88) == 1
    D = Device(I)
    out_d, t_d = D.forward()
    out, grads = host(out_d), D.backward(out_d, t_d)
    assert same_bits(host(t_d), I["t"])
    assert np.isfinite(out[r]).all() and (out[r] == out[r, 0]).all()
    assert abs(out[r, 0] + np.log(65)) <= (1 + 2 * R.LOGF_ULP) * R.EPS * np.log(65)      # s = 65 exactly, then logf
    assert not grads["g_logits"][r].any()
    others = np.arange(300) != r
    assert same_bits(out[others], out0[others]) and same_bits(grads["g_logits"][others], grads0["g_logits"][others])
    net = torch.nn.Sequential(torch.nn.Linear(7, 16), torch.nn.ReLU(), torch.nn.Linear(16, 1)).to(DEV)
    with torch.no_grad():
        net[0].weight.copy_(D.W1), net[0].bias.copy_(D.b1), net[2].weight.copy_(D.W2.view(1, -1)), net[2].bias.copy_(D.b2)
    ref = torch.log_softmax(D.logits / torch.log(torch.exp(net(D.H)) + 1.1), dim=1)
    rg = torch.autograd.grad(ref, list(net.parameters()), grad_outputs=D.g)
    assert torch.isfinite(ref[r]).all()
    for k, v in zip(R.PARAMS, rg):
        got, want = np.isfinite(grads[k]).reshape(-1), np.isfinite(host(v)).reshape(-1)
        print(f"t = {I['t'][r]:.1f}: g_{k}: {np.count_nonzero(~got)} of {got.size} non-finite (torch: "
              f"{np.count_nonzero(~want)})")
        assert np.array_equal(got, want), f"g_{k} is non-finite in other places than torch's"


def test_through_wats_head():
    """the autograd function: saved tensors, needs_input_grad with and without the logits' gradient"""
    case = (4097, 7, 16, 1, 1, "randn")
    I = R.case_inputs(case)
    D = Device(I)
    net = torch.nn.Sequential(torch.nn.Linear(1, 16), torch.nn.ReLU(), torch.nn.Linear(16, 1)).to(DEV)
    with torch.no_grad():
        net[0].weight.copy_(D.W1), net[0].bias.copy_(D.b1), net[2].weight.copy_(D.W2.view(1, -1)), net[2].bias.copy_(D.b2)
    logits = D.logits.clone().requires_grad_(True)
    out_t = wats_hip.wats_head(D.H, logits, net)
    got = torch.autograd.grad(out_t, [logits] + list(net.parameters()), grad_outputs=D.g)
    out = host(out_t)
    grads = {k: host(v).reshape(np.shape(I[k]) if k in I else v.shape) for k, v in zip(R.GRADS, got)}
    label = R.case_id(case) + " wats_head"
    R.C.report(f"{label} out", R.forward_c(I["logits"], I["t"], out), R.BOUND)
    for k, c in R.backward_c(I, I["t"], I["pre"], out, grads).items():
        R.C.report(f"{label} {k}", c, R.BOUND)
    direct_out, direct_t = D.forward()
    direct = D.backward(direct_out, direct_t)
    assert same_bits(out, host(direct_out)) and all(same_bits(grads[k], direct[k]) for k in R.GRADS)
    bare = torch.autograd.grad(wats_hip.wats_head(D.H, D.logits, net), list(net.parameters()), grad_outputs=D.g)
    assert all(same_bits(host(v).reshape(-1), grads[k].reshape(-1)) for k, v in zip(R.PARAMS, bare))
