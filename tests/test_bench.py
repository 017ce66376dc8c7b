"""The bench.py contract the driver parses: one JSON line on stdout with the
required keys, a roofline object (bound, achieved, peak, unit, frac,
traffic) and, at N = 1, a cpu_baseline object -- run on a small workload."""
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO


def _run(args, timeout=600):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, capture_output=True, text=True,
                         timeout=timeout, cwd=REPO)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, f"stdout must be exactly one JSON line, got {len(lines)}: {out.stdout[:2000]}"
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_line_schema_small():
    d = _run(["--full", "--config", "pubmed", "--F", "8", "--steps", "3", "--warmup", "1", "--cpu-seconds", "1",
              "--sharded-extra", "pubmed", "--sharded-steps", "2", "--exchange", "ipc,rccl", "--cold-reps", "1"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["higher_is_better"] is True and d["value"] > 0
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and 0 < r["frac"] < 1.5
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["check"]["ok"], c["check"]          # the benchmarked S vs the C oracle (all columns)
    assert "connected_companion" not in d          # only for the ogbn-arxiv headline
    assert d["prologue"]["create_ms"] > 0 and d["prologue"]["log1p_degree_ms"] > 0
    assert d["cpu_baseline"]["prologue_s"] > 0
    for key in ("sharded", "sharded_pubmed_rccl"):
        sh = d[key]
        assert "error" not in sh, sh
        assert sh["value"] > 0 and sh["check"]["ok"], sh["check"]


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A run without --full: the headline keys only (no roofline, CPU baseline,
    companions or sharded extras), --steps timed steps, and --dump-outputs
    writes the last timed pass's H and S (float32) -- checked against the
    oracle on the same inputs, rebuilt here from the bench's seeds."""
    import numpy as np

    from conftest import assert_parity
    from oracle import wats_oracle as O
    from wats_hip.graphgen import named_graph

    d = _run(["--config", "pubmed", "--F", "8", "--steps", "4", "--warmup", "1", "--settle-s", "0.05",
              "--dump-outputs", str(tmp_path / "dump")], timeout=120)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype"):
        assert k in d, k
    assert d["steps"] == 4 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "edges*K/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    # value = edges * K per second of the timed steps
    assert abs(d["value"] - d["config"]["nnz"] * d["config"]["K"] / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    for k in ("roofline", "cpu_baseline", "prologue", "cold", "f1_companion", "sharded", "pubmed_companion",
              "connected_companion"):
        assert k not in d, k
    assert sorted(os.listdir(tmp_path / "dump")) == ["H.npy", "S.npy"]
    H, S = np.load(tmp_path / "dump" / "H.npy"), np.load(tmp_path / "dump" / "S.npy")
    g = named_graph("pubmed", seed=0)
    X = np.random.default_rng(1).standard_normal((g.n, 8)).astype(np.float32)
    assert H.dtype == np.float32 and S.dtype == np.float32 and H.shape == S.shape == (g.n, 8)
    ref = O.graph_wavelet_features(g.to_scipy(), k=d["config"]["K"], s=0.8, X0=X, return_all=True)
    assert_parity(S, ref["S"], what="dumped S")
    assert_parity(H, ref["H"], what="dumped H")


def test_dump_outputs_sample_cpu(tmp_path, monkeypatch):
    """bench.dump_outputs (no GPU): float32 .npy files; an array over its share
    of the budget is cut to the same seeded rows in every call."""
    import numpy as np
    sys.path.insert(0, REPO)
    import bench
    a = np.arange(1000 * 6, dtype=np.float64).reshape(1000, 6)
    bench.dump_outputs(str(tmp_path / "a"), {"H": a, "S": -a})
    got = np.load(tmp_path / "a" / "H.npy")
    assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * (4096 + 100 * 24))   # room for 100 rows of each
    for sub in ("b", "c"):
        bench.dump_outputs(str(tmp_path / sub), {"H": a, "S": -a})
    hb, sb, hc = (np.load(tmp_path / p / f) for p, f in (("b", "H.npy"), ("b", "S.npy"), ("c", "H.npy")))
    assert hb.shape == (100, 6) and np.array_equal(hb, hc) and np.array_equal(hb, -sb)
    rows = (hb[:, 0] / 6).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(hb, a[rows].astype(np.float32))
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in ("H.npy", "S.npy")) <= bench.DUMP_BUDGET


@pytest.mark.gpu
def test_bench_multi_rank_headline_rehearsal():
    """The N > 1 code path (headline = one graph row-sharded over the ranks,
    strong scaling; replicas as an extra) with 2 ranks sharing the one GPU:
    gloo process group, IPC exchange (RCCL refuses two ranks per device)."""
    env = dict(os.environ, WATS_BENCH_PG="gloo", WATS_BENCH_DEVICE="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={29500 + os.getpid() % 1000}", os.path.join(REPO, "bench.py"),
           "--gpus", "2", "--full", "--steps", "3", "--warmup", "1", "--scale-config", "pubmed", "--F", "8",
           "--exchange", "ipc", "--sharded-extra", "none", "--config", "pubmed"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO, env=env)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    assert d["config"]["parallelism"] == "rows x2" and d["check"]["ok"], d.get("check")
    assert d["replicas"]["value"] > 0


@pytest.mark.gpu
def test_bench_multi_rank_picks_the_faster_exchange():
    """N > 1 with two exchanges: the headline is timed with both and the line is
    the faster one whose check passed; the other is attached in full."""
    env = dict(os.environ, WATS_BENCH_PG="gloo", WATS_BENCH_DEVICE="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={30500 + os.getpid() % 1000}", os.path.join(REPO, "bench.py"),
           "--gpus", "2", "--full", "--steps", "3", "--warmup", "1", "--scale-config", "pubmed", "--F", "8",
           "--exchange", "ipc,host", "--sharded-extra", "none", "--config", "pubmed", "--replicas", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO, env=env)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    cmp = d["exchange_compare"]
    assert set(cmp) == {"ipc", "host"} and all(v["check_ok"] for v in cmp.values()), cmp
    best = max(cmp, key=lambda x: cmp[x]["value"])
    assert d["config"]["exchange"] == best and d["value"] == cmp[best]["value"]
    other = "host" if best == "ipc" else "ipc"
    assert d[f"sharded_pubmed_{other}"]["value"] == cmp[other]["value"]


def test_byte_models_cpu():
    """bench.py's byte models (no GPU): SURVEY 8(d)'s forward-recurrence B_step
    and the Clenshaw form, which drops the S read + write (8 B) and adds the
    X0 read (4 B) per row and column."""
    sys.path.insert(0, REPO)
    import bench
    n, nnz, F = 93_861, 2_315_600, 40
    assert bench.algorithmic_bytes(n, nnz, F) == 8 * nnz + 4 * (n + 1) + 20 * n * F
    assert bench.algorithmic_bytes(n, nnz, F) - bench.clenshaw_bytes(n, nnz, F) == 4 * n * F
    assert bench.algorithmic_bytes(n, nnz, F) == 93_989_048   # the active-row B_step quoted in DESIGN.md 4.1
    # unweighted: no CSR values (4 B/nnz), plus the float64 dinv of each row
    assert bench.clenshaw_bytes(n, nnz, F) - bench.clenshaw_bytes(n, nnz, F, unit=True) == 4 * nnz - 8 * n
