"""Generate the Calib_Random / Calib_RND fixtures FROM THE REFERENCE (``calib_attack/calib_random.py`` and
``calib_attack/calib_rnd.py`` over ``calibration/TS.py`` on ``src/gnn/model.py``'s ``CompatibleGCN``), on the CPU.

Run only in the build container, where the reference is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_random.py

The reference's packages are imported through stub packages with the pinned CPU code path, as
``tools/gen_golden_fga.py`` does.  The reference's own classes then run ``attack`` after ``random.seed``; a forward hook
on the surrogate records, for EVERY trial, the output row of the target and the rows of the adjacency and of the
features it was called with, from which the trial's kind, add / remove and index follow.  Outputs are DATA only
(``allow_pickle=False``): ``tests/golden/random/*.npz`` and ``manifest.json`` (versions, seeds, sha256, distances).

Each file holds one graph in the attack convention (the adjacency of ``tests/golden/fga``'s file of the same name:
symmetric, self loops), binary features ``x`` (n, 24), ``y``, ``val_idx``, the trained model ``p__<name>``, the
temperature ``ts__temperature`` and the runs ``r<i>__<field>``: per trial ``step``, ``kind`` (0 edge, 1 feature),
``add``, ``index``, ``logits`` (the surrogate's output row), ``label``, ``conf``, ``accepted``; per run ``orig_logits``,
``n_perturb``, ``best_conf``, ``toggles`` (the final toggle set), ``features`` (the final row t) and ``next_random``
(``random.random()`` after the run: the stream's position).

Conditions, checked here (exit status 1 if a case cannot meet them) and again by tests/test_random_attack_host.py:
the float64 restatement of the loop (tests/trial_ref.py) draws and accepts the same trials and ends at the same
stream position; for every evaluated trial ``|conf - best_conf|`` and the top-2 gap of the output row exceed
100 x the case's float32-vs-float64 distance of the confidences / of the rows -- except a trial whose output row is,
bit for bit, the row of the accepted state (a feature flip of a target that no row gathers: the tie the strict
comparison rejects, equal in every precision because the same numbers are summed); at least 12 runs per case over
both classes, the three strategies and the three modes; and per case a tried self-loop removal, a trial rejected for
a changed label, a step in which all 50 trials fail, an accepted feature flip, a feature flipped back, and in iso120 a
run on a node without any entry (only additions are possible there: no add / remove draw).
"""
from __future__ import annotations

import contextlib
import hashlib
import importlib
import importlib.util
import io
import json
import math
import os
import random
import sys
import types

os.environ["MKL_ENABLE_INSTRUCTIONS"] = "AVX2"
os.environ["ATEN_CPU_CAPABILITY"] = "avx2"

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "random")
FGA = os.path.join(REPO, "tests", "golden", "fga")
for p in (os.path.join(REPO, "efficient-gnn_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import trial_ref as T  # noqa: E402

BUDGET, MAX_TRIALS, NFEAT = 5, 50, 24
MODES = {"structure": (True, False), "features": (False, True), "both": (True, True)}
STRATEGIES = ("under", "over", "under_kl")
EVENTS = ("self_loop_removal", "label_reject", "all_fail_step", "feature_accept", "feature_back")
FACTOR = 100.0


def import_reference():
    ue = types.ModuleType("utils.ece")
    ue.calculate_average_ece = lambda *a, **k: (_ for _ in ()).throw(NotImplementedError("a placeholder"))
    u = types.ModuleType("utils")
    u.__path__ = []
    u.ece = ue
    sys.modules.update({"utils": u, "utils.ece": ue})
    for name in ("calib_attack", "calibration"):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, name)]
        sys.modules[name] = pkg
    rnd = importlib.import_module("calib_attack.calib_rnd")
    ran = importlib.import_module("calib_attack.calib_random")
    ts = importlib.import_module("calibration.TS")
    spec = importlib.util.spec_from_file_location("ref_gnn_model", os.path.join(REF, "src", "gnn", "model.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    return dict(Calib_Random=ran.Calib_Random, Calib_RND=rnd.Calib_RND), ts, M


def train_model(M, seed, x, adj, ncls, nhid):
    torch.manual_seed(seed)
    teacher = M.CompatibleGCN(nfeat=x.shape[1], nclass=ncls, nhid=nhid, dropout=0.0)
    teacher.eval()
    with torch.no_grad():
        y = (3 * teacher(x, adj)).argmax(1)
    model = M.CompatibleGCN(nfeat=x.shape[1], nclass=ncls, nhid=nhid, dropout=0.5)
    opt = torch.optim.Adam(model.parameters(), lr=0.02, weight_decay=5e-4)
    model.train()
    for _ in range(400):
        opt.zero_grad()
        F.cross_entropy(model(x, adj), y).backward()
        opt.step()
    model.eval()
    return model, y


def run_reference(cls, surrogate, x, adj, t, strategy, mode, seed, P, scale):
    """One reference run, recorded: (arrays, meta) or (None, why)."""
    structure, features = MODES[mode]
    calls = []

    def hook(_m, inputs, out):
        calls.append((out[t].detach().clone(), inputs[1][t].detach().clone(), inputs[0][t].detach().clone()))
    handle = surrogate.register_forward_hook(hook)
    kw = dict(n_perturb=[], best_conf=[])
    random.seed(seed)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            atk = cls(surrogate, attack_structure=structure, attack_features=features, device="cpu")
            atk.attack(x if cls.__name__ == "Calib_Random" else x.numpy(), adj if cls.__name__ == "Calib_Random"
                       else adj.numpy(), t, BUDGET, strategy=strategy, max_trials=MAX_TRIALS, **kw)
    finally:
        handle.remove()
    next_random = random.random()
    better = (lambda a, b: a > b) if strategy == "over" else (lambda a, b: a < b)
    out0 = calls[0][0]
    label0 = int(out0.argmax())
    best = F.softmax(out0[None], dim=1)[0, label0].item()
    cur_adj, cur_x = adj[t].clone(), x[t].clone()
    last_row = out0
    rec = dict(step=[], kind=[], add=[], index=[], logits=[], label=[], conf=[], accepted=[], tie=[], best_before=[])
    events = set()
    step, in_step, accepted_n = 0, 0, 0
    for out, arow, xrow in calls[1:]:
        da, dx = torch.nonzero(arow != cur_adj).flatten(), torch.nonzero(xrow != cur_x).flatten()
        assert len(da) + len(dx) == 1, (len(da), len(dx))
        if len(da):
            kind, index = 0, int(da[0])
            add = int(arow[index] > cur_adj[index])
            if not add and index == t:
                events.add("self_loop_removal")
        else:
            kind, index = 1, int(dx[0])
            add = int(xrow[index] > cur_x[index])
            if cur_x[index] != x[t, index]:
                events.add("feature_back")
        label = int(out.argmax())
        conf = F.softmax(out[None], dim=1)[0, label].item()
        ok = label == label0 and better(conf, best)
        if label != label0:
            events.add("label_reject")
        tie = bool(torch.equal(out, last_row))
        for k, v in zip(rec, (step, kind, add, index, out, label, conf, ok, tie, best)):
            rec[k].append(v)
        in_step += 1
        if ok:
            best, cur_adj, cur_x, last_row = conf, arow, xrow, out
            accepted_n += 1
            if kind == 1:
                events.add("feature_accept")
        if ok or in_step == MAX_TRIALS:
            if not ok:
                events.add("all_fail_step")
            step, in_step = step + 1, 0
    assert accepted_n == kw["n_perturb"][0] and best == kw["best_conf"][0], "the replay of the acceptances is off"
    # the float64 restatement
    rng = random.Random(seed)
    truth = T.random_loop(P, x, adj, t, BUDGET, strategy, MAX_TRIALS, rng, structure, features, scale=scale)
    if len(truth["trials"]) != len(rec["kind"]):
        return None, "float64 loop: another number of trials"
    d_logits = d_conf = 0.0
    for k, tr in enumerate(truth["trials"]):
        if (tr["kind"], tr["index"], tr["accepted"], tr["step"]) != (rec["kind"][k], rec["index"][k], rec["accepted"][k],
                                                                    rec["step"][k]) or int(tr["add"]) != rec["add"][k]:
            return None, f"float64 loop: trial {k} differs"
        d_logits = max(d_logits, float((rec["logits"][k].double() - tr["logits"]).abs().max()))
        d_conf = max(d_conf, abs(rec["conf"][k] - tr["conf"]))
        if rec["tie"][k] and tr["conf"] != tr["best_before"]:
            return None, f"trial {k}: a tie in float32 only"
    if rng.random() != next_random or truth["n_perturb"] != accepted_n:
        return None, "float64 loop: another stream position"
    d_conf = max(d_conf, abs(best - truth["best_conf"]))
    toggles = sorted(int(j) for j in torch.nonzero(cur_adj != adj[t]).flatten())
    if toggles != truth["toggles"]:
        return None, "float64 loop: another toggle set"
    top2 = torch.topk(torch.stack(rec["logits"]), 2, dim=1).values
    arrays = dict(step=np.asarray(rec["step"], np.int32), kind=np.asarray(rec["kind"], np.int8),
                  add=np.asarray(rec["add"], np.int8), index=np.asarray(rec["index"], np.int32),
                  logits=torch.stack(rec["logits"]).numpy(), label=np.asarray(rec["label"], np.int32),
                  conf=np.asarray(rec["conf"], np.float64), accepted=np.asarray(rec["accepted"], np.bool_),
                  tie=np.asarray(rec["tie"], np.bool_), orig_logits=out0.numpy(), n_perturb=np.int64(accepted_n),
                  best_conf=np.float64(best), toggles=np.asarray(toggles, np.int64), features=cur_x.numpy(),
                  next_random=np.float64(next_random))
    gaps = np.abs(np.asarray(rec["conf"]) - np.asarray(rec["best_before"]))
    live = ~arrays["tie"]
    meta = dict(cls=cls.__name__, strategy=strategy, mode=mode, target=int(t), seed=int(seed), trials=len(rec["kind"]),
                n_perturb=accepted_n, events=sorted(events), ties=int(arrays["tie"].sum()),
                f32_vs_f64=dict(logits=d_logits, conf=d_conf),
                min_conf_gap=float(gaps[live].min()) if live.any() else float("inf"),
                min_top2_gap=float((top2[:, 0] - top2[:, 1]).min()))
    return (arrays, meta), "ok"


def gaps_hold(meta, worst):
    return meta["min_conf_gap"] > FACTOR * worst["conf"] and meta["min_top2_gap"] > FACTOR * worst["logits"]


def make_case(classes, ts, M, name, seed, ncls, nhid):
    with np.load(os.path.join(FGA, name + ".npz"), allow_pickle=False) as d:
        adj = torch.from_numpy(d["adj"].astype(np.float32))
        isolated = [int(i) for i in d["isolated"]]
    n = adj.shape[0]
    torch.manual_seed(seed)
    x = (torch.rand(n, NFEAT) < 0.3).float()
    model, y = train_model(M, seed, x, adj, ncls, nhid)
    val_idx = torch.randperm(n)[:n // 3]
    with contextlib.redirect_stdout(io.StringIO()):
        cal = ts.TemperatureScaling(model, x, y, adj, val_idx)
    cal.eval()
    temperature = cal.temperature.detach().clone()
    scale = math.log(math.exp(float(temperature.double())) + float(torch.tensor(1.1).double()))
    P = {k: v.detach().clone() for k, v in model.state_dict().items()}
    deg = adj.sum(1)
    order = [int(i) for i in torch.argsort(deg, stable=True)]
    pool = [i for i in order if i not in isolated][::5] + [int(deg.argmax())]
    runs = []

    def attempt(cls_name, strategy, mode, targets, base_seed):
        for k, t in enumerate(targets):
            res, why = run_reference(classes[cls_name], cal, x, adj, t, strategy, mode, base_seed + k, P, scale)
            if res is not None and gaps_hold(res[1], res[1]["f32_vs_f64"]) and res[1]["trials"] >= 5:
                return res
        return None

    combo = 0
    for cls_name in ("Calib_Random", "Calib_RND"):
        for strategy in STRATEGIES:
            for mode in MODES:
                combo += 1
                rot = pool[combo % len(pool):] + pool[:combo % len(pool)]
                res = attempt(cls_name, strategy, mode, rot, 1000 * combo + seed)
                if res is not None:
                    runs.append(res)
    if isolated:            # a node without any entry: only additions are possible; its feature trials are ties
        res = attempt("Calib_Random", "under", "both", isolated, 77000 + seed)
        if res is None:
            raise SystemExit(f"{name}: no run on an isolated node meets the conditions")
        res[1]["events"] = sorted(set(res[1]["events"]) | {"isolated_target"})
        runs.append(res)
    have = lambda: set(e for _, m in runs for e in m["events"])
    extra = 0
    while set(EVENTS) - have() and extra < 400:      # more runs until every event is covered
        extra += 1
        cls_name = ("Calib_Random", "Calib_RND")[extra % 2]
        strategy, mode = STRATEGIES[extra % 3], list(MODES)[(extra // 3) % 3]
        res = attempt(cls_name, strategy, mode, [pool[extra % len(pool)]], 50000 + extra)
        if res is not None and set(res[1]["events"]) - have():
            runs.append(res)
    while True:             # the gaps against the case's distances (the largest of its runs)
        worst = {k: max(m["f32_vs_f64"][k] for _, m in runs) for k in ("logits", "conf")}
        kept = [r for r in runs if gaps_hold(r[1], worst)]
        if len(kept) == len(runs):
            break
        runs = kept
    missing = set(EVENTS) - have()
    covered = (len(runs) >= 12 and {m["cls"] for _, m in runs} == set(classes) and
               {m["strategy"] for _, m in runs} == set(STRATEGIES) and {m["mode"] for _, m in runs} == set(MODES))
    if missing or not covered:
        raise SystemExit(f"{name}: {len(runs)} runs kept, events missing: {sorted(missing)}, coverage {covered}")
    arrays = dict(x=x.numpy(), y=y.numpy(), val_idx=val_idx.numpy(), isolated=np.asarray(isolated, np.int64),
                  ts__temperature=temperature.numpy())
    arrays.update({"p__" + k: v.numpy() for k, v in P.items()})
    metas = []
    for i, (arr, meta) in enumerate(runs):
        arrays.update({f"r{i}__{k}": v for k, v in arr.items()})
        meta["run"] = i
        metas.append(meta)
    print(f"{name}: {len(runs)} runs, {sum(m['trials'] for m in metas)} trials, distances {worst}")
    return arrays, dict(seed=seed, n=n, adjacency=f"tests/golden/fga/{name}.npz", budget=BUDGET, max_trials=MAX_TRIALS,
                        scale=scale, runs=metas, f32_vs_f64=worst)


def save(name, manifest, arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    limit = max(os.path.getsize(os.path.join(FGA, f)) for f in os.listdir(FGA))
    assert size < limit, f"{path}: {size} B, the largest file of tests/golden/fga has {limit} B"
    with open(path, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    manifest["files"][name + ".npz"] = dict(sha256=digest, keys=sorted(arrays.keys()))
    print(f"wrote {path} ({size} B)")


def main():
    os.makedirs(OUT, exist_ok=True)
    classes, ts, M = import_reference()
    manifest = dict(generator="tools/gen_golden_random.py",
                    reference="calib_attack/calib_random.py + calib_attack/calib_rnd.py + calibration/TS.py + "
                              "src/gnn/model.py (2026-02-06)",
                    numpy=np.__version__, torch=torch.__version__, python=sys.version.split()[0],
                    cpu_code_path=dict(MKL_ENABLE_INSTRUCTIONS="AVX2", ATEN_CPU_CAPABILITY="avx2"), cases={}, files={})
    for name, seed, ncls, nhid in (("iso120", 5, 5, 32), ("hub96", 9, 4, 24)):
        for s in range(seed, seed + 8):
            try:
                arrays, meta = make_case(classes, ts, M, name, s, ncls, nhid)
                break
            except SystemExit as e:
                print(f"seed {s}: {e}")
        else:
            raise SystemExit(f"{name}: no seed meets the conditions")
        manifest["cases"][name] = meta
        save(name, manifest, arrays)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("manifest written")


if __name__ == "__main__":
    main()
