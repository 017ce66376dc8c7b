"""GPU tests of the header's stream and capture promise (include/wats_hip.h, "Conventions"): every stream-taking
entry point of tests/stream_cases.py does its work on the stream it is given, and the ones documented as "may be
captured" give the same bits from a replayed graph whose inputs were rewritten.

For each case, inputs A and B come from two seeds and `base_A`, `base_B` are eager results on the default stream;
every output differs between them (asserted: otherwise a stale result could pass).  All comparisons are bitwise.

(a) replay, CAPTURABLE cases: the case is warmed and captured on a side stream over static inputs that hold A.  With
    the outputs filled with NaN before each replay: replay -> base_A; inputs rewritten to B, replay -> base_B;
    replay once more -> base_B again (an accumulator or an arrival counter that a replay does not reset shows here).
    A stateful case (wg_scale_epoch) advances its state block: it is reset and replayed three times per comparison,
    against three eager launches from the same initial block.
(b) ordering, every case: the static inputs hold A and the device is idle; on a side stream a delay is enqueued,
    then the copy of B into the inputs, then the case; only the side stream is waited for.  Work that reached any
    other stream runs during the delay and reads A; a result read back after a sync of another stream is returned
    before B is written (the host values of the SYNCHRONOUS cases are compared as well).  Blind spot: a launch on a
    wrong stream that shares the side stream's hardware queue waits for the delay too and passes.
(c) the detector detects: (b) with NULL (the legacy stream) handed to two direct-ABI calls while the side stream is
    torch's current one gives base_A, not base_B.  This is the wrong-stream mutant without a rebuild; it also pins
    the assumption of (b) that torch's side streams do not block against the legacy stream.
(d) ordering of the ten calibrators' eval-mode forward, the features being the rewritten input.

Streams that the runtime maps onto one hardware queue run in order whatever their flags, so behind such a side stream
the legacy stream waits for the delay too and (b) would pass a wrong stream: the `side` fixture takes a stream that the
legacy stream is seen to overtake, and (c) asserts on every run that the detector still detects.

The delay of (b) - (d) is a condition of the harness, not a tolerance: at least 20 ms and at least 20 times the host
time of the slowest registered call, both measured by the `delay` fixture and printed; above 500 ms the fixture fails
instead of shortening the margin.
"""
import functools
import time

import pytest
import torch

from stream_cases import (ABI_PROBES, CALIBRATORS, CAPTURABLE, CASES, REPEATS, SYNCHRONOUS, calibrator,
                          calibrator_data, calibrator_features, fixtures)

pytestmark = pytest.mark.gpu

SEED_A, SEED_B = 1, 2
MIN_DELAY_MS, MARGIN, MAX_DELAY_MS = 20.0, 20.0, 500.0
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------------ comparing
def same(a, b):
    """bitwise, shape and dtype included"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def assert_same(got, want, what):
    assert len(got) == len(want), what
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if not same(a, b)]
    assert not bad, f"{what}: outputs {bad} of {len(want)} differ from the eager result on the default stream"


def poison(outs):
    for t in outs:
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(171)
        elif t.dtype == torch.bool:
            t.fill_(True)
        else:
            t.fill_(-123456789)


def call(case, inputs):
    """(output tensors, host values); a stateful case takes its REPEATS steps"""
    for _ in range(REPEATS if case.stateful else 1):
        result = case.run(inputs)
    return result if case.klass == SYNCHRONOUS else (tuple(result), ())


def rewrite(static, inputs, keys=None):
    for k in (static if keys is None else keys):
        static[k].copy_(inputs[k])


def clones(inputs):
    return {k: v.clone() for k, v in inputs.items()}


# ------------------------------------------------------------------------------------------------ baselines, the delay
_BASE = {}


def baseline(case):
    """inputs and eager results of both seeds on the default stream, made once and left unchanged"""
    if case.name not in _BASE:
        fixtures()
        b = {}
        for tag, seed in (("A", SEED_A), ("B", SEED_B)):
            inputs = case.make(seed)
            pristine = clones(inputs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs, host = call(case, inputs)
            b["host_ms_" + tag] = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            b[tag] = pristine
            b["base_" + tag] = tuple(t.clone() for t in outs)
            b["host_" + tag] = host
        # the second call is the warm one: no plan, no import, no first allocation
        b["host_ms"] = b["host_ms_B"]
        differs = [not same(a, c) for a, c in zip(b["base_A"], b["base_B"])]
        assert all(differs) and differs, f"{case.name}: outputs {[i for i, d in enumerate(differs) if not d]} are " \
                                         f"the same for both seeds and prove nothing"
        _BASE[case.name] = b
    return _BASE[case.name]


@functools.lru_cache(maxsize=None)
def _sleep_ms():
    """(fn, measure, ms per unit): fn(units) enqueues a delay on the current stream, measure times it with a pair of
    events; the unit is calibrated on a delay of at least 10 ms"""
    def measure(fn, units):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn(units)
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    if hasattr(torch.cuda, "_sleep"):
        fn, units = (lambda units: torch.cuda._sleep(int(units))), 250_000
    else:       # a chain of matrix products sized the same way
        a = torch.randn(2048, 2048, device="cuda")

        def fn(units):
            b = a
            for _ in range(int(units)):
                b = (a @ b) * 1e-3
        units = 2
    measure(fn, units)
    while True:
        ms = measure(fn, units)
        if ms >= 10.0 or units > 1e12:
            return fn, measure, ms / units
        units *= 4


@pytest.fixture(scope="module")
def delay():
    """enqueues the delay of (b) - (d) on the current stream"""
    slow_name, slow_ms = max(((c.name, baseline(c)["host_ms"]) for c in CASES), key=lambda p: p[1])
    data = calibrator_data()
    for name in CALIBRATORS:
        cal, x = calibrator(name), calibrator_features(SEED_B)
        with torch.no_grad():
            cal(x, data.adj)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cal(x, data.adj)
            ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        if ms > slow_ms:
            slow_name, slow_ms = name, ms
    want = max(MIN_DELAY_MS, MARGIN * slow_ms)
    print("\nstreams: host ms per call: " + ", ".join(f"{c.name} {baseline(c)['host_ms']:.2f}" for c in CASES))
    print(f"\nstreams: slowest host call {slow_name} {slow_ms:.3f} ms; delay wanted {want:.1f} ms")
    assert want <= MAX_DELAY_MS, f"the slowest call ({slow_name}, {slow_ms:.2f} ms on the host) needs a delay of " \
                                 f"{want:.0f} ms, above the cap of {MAX_DELAY_MS:.0f} ms: shorten the call, not the margin"
    fn, measure, ms_per_unit = _sleep_ms()
    units = 1.25 * want / ms_per_unit
    got = measure(fn, units)
    print(f"streams: delay measured {got:.1f} ms ({units:.3g} units of {ms_per_unit:.3g} ms)")
    assert got >= want, f"the delay took {got:.1f} ms, {want:.1f} ms were wanted"
    return lambda: fn(units)


@pytest.fixture(autouse=True)
def stop_after_a_device_error():
    """a device error ends the module: nothing more is started on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further test is started: {e}", returncode=3)


def legacy_runs_ahead_of(stream):
    """whether work on the legacy stream overtakes a delay on `stream`.  Streams that the runtime maps onto one
    hardware queue run in order, whatever their flags: behind such a side stream a launch on the legacy stream waits
    for the delay like a launch on the right stream, and (b) would pass it."""
    fn, _, ms_per_unit = _sleep_ms()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        fn(10.0 / ms_per_unit)
    marker = torch.zeros(1, device="cuda").add_(1)
    done = torch.cuda.Event()
    done.record()
    t0 = time.perf_counter()
    while not done.query() and time.perf_counter() - t0 < 3e-3:
        pass
    ahead = done.query()
    torch.cuda.synchronize()
    return ahead and float(marker) == 1.0


@pytest.fixture(scope="module")
def side():
    """the side stream of every test here: one that the legacy stream does not queue behind"""
    tried = 0
    for tried in range(1, 17):
        stream = torch.cuda.Stream()
        if legacy_runs_ahead_of(stream):
            print(f"\nstreams: side stream found at attempt {tried}")
            return stream
    pytest.fail(f"the legacy stream waited behind each of {tried} side streams: (b) cannot see a wrong stream here")


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("case", [c for c in CASES if c.klass == CAPTURABLE], ids=lambda c: c.name)
def test_replay_follows_rewritten_inputs_and_resets_what_it_accumulates(case, side):
    b = baseline(case)
    static = clones(b["A"])
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        case.run(static)                         # warms the allocator and any plan
        with torch.cuda.graph(graph, stream=side):
            outs = tuple(case.run(static))
    torch.cuda.synchronize()
    for step, tag in enumerate("ABB"):
        if case.stateful:                        # the outputs are the state: back to the initial block
            rewrite(static, b[tag])
        else:
            if step == 1:
                rewrite(static, b[tag])
            poison(outs)
        for _ in range(REPEATS if case.stateful else 1):
            graph.replay()
        torch.cuda.synchronize()
        assert_same(outs, b["base_" + tag], f"{case.name}, replay {step + 1} (inputs {tag})")


# ------------------------------------------------------------------------------------------------ (b)
def ordered_run(fn, static, inputs_b, delay, side):
    """the static inputs hold A; on the side stream: the delay, the copy of B, fn(static); the side stream alone is
    waited for"""
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        delay()
        rewrite(static, inputs_b)
        result = fn(static)
    side.synchronize()
    return result


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_work_is_ordered_on_the_given_stream(case, delay, side):
    b = baseline(case)
    outs, host = ordered_run(lambda static: call(case, static), clones(b["A"]), b["B"], delay, side)
    try:
        assert host == b["host_B"], f"{case.name}: host values {host}, {b['host_B']} after a sync of the right stream"
        assert_same(outs, b["base_B"], f"{case.name} on a side stream")
    finally:
        torch.cuda.synchronize()


def test_log1p_degree_is_ordered_on_the_given_stream(delay, side):
    """wg_log1p_degree reads nothing but its handle, so the output is what is rewritten: behind the delay the side stream
    fills x0 with NaN, then the entry runs.  On the right stream it overwrites the NaN; on another one (NULL here) it runs
    during the delay and the fill lands on top of it."""
    from stream_cases import _check, _lib, _ptr
    from wats_hip.laplacian import stream_handle
    L = fixtures().lap_rand
    base = L.log1p_degree()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(base).all()) and float(base.max()) > 0

    def on(stream_of):
        x0 = torch.zeros_like(base)
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            delay()
            x0.fill_(float("nan"))
            _check(_lib().wg_log1p_degree(L.handle, _ptr(x0), stream_of()), "log1p_degree")
        side.synchronize()
        result = x0.clone()
        torch.cuda.synchronize()
        return result

    assert same(on(lambda: stream_handle(base.device)), base)
    assert bool(torch.isnan(on(lambda: None)).all()), "a launch on the legacy stream was not seen"


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("name", sorted(ABI_PROBES))
def test_the_legacy_stream_is_seen_as_a_wrong_stream(name, delay, side):
    from wats_hip.laplacian import stream_handle
    case, probe = BY_NAME[name], ABI_PROBES[name]
    b = baseline(case)
    base = {}
    for tag in "AB":
        base[tag] = probe(b[tag], stream_handle(torch.device("cuda", torch.cuda.current_device())))
        torch.cuda.synchronize()
    assert not same(base["A"][0], base["B"][0])
    right = ordered_run(lambda static: probe(static, stream_handle(torch.device("cuda", torch.cuda.current_device()))),
                        clones(b["A"]), b["B"], delay, side)
    torch.cuda.synchronize()
    assert_same(right, base["B"], f"{name} with the side stream")
    wrong = ordered_run(lambda static: probe(static, None), clones(b["A"]), b["B"], delay, side)
    torch.cuda.synchronize()
    share = {tag: float((wrong[0] == base[tag][0]).float().mean()) for tag in "AB"}
    print(f"streams: {name} on the legacy stream: share of elements equal to base_A {share['A']:.3f}, base_B {share['B']:.3f}")
    assert same(wrong[0], base["A"][0]) and not same(wrong[0], base["B"][0]), \
        f"{name}: a launch on the legacy stream did not run ahead of the side stream's copy ({share}): (b) cannot see a " \
        f"wrong stream"


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("name", CALIBRATORS)
def test_calibrator_forward_is_ordered_on_the_current_stream(name, delay, side):
    data, cal = calibrator_data(), calibrator(name)
    x = {tag: calibrator_features(seed) for tag, seed in (("A", SEED_A), ("B", SEED_B))}
    with torch.no_grad():
        base = {tag: cal(x[tag], data.adj).clone() for tag in "AB"}
        torch.cuda.synchronize()
        assert not same(base["A"], base["B"])
        out = ordered_run(lambda static: cal(static["x"], data.adj), dict(x=x["A"].clone()), dict(x=x["B"]), delay, side)
    try:
        assert_same((out,), (base["B"],), f"{name}.forward on a side stream")
    finally:
        torch.cuda.synchronize()
