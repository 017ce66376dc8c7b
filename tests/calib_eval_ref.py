"""numpy model of the documented arithmetic of csrc/calib.hip -- TEST INFRASTRUCTURE ONLY.

``probabilities`` gives the float32 ``p`` of every element (np.longdouble exp / softmax, rounded once), ``bin_table``
the integer table exactly as documented in include/wats_hip.h (np.digitize on the caller's edges, fixed point with
quantum 2^-40), ``scalar_truth`` the np.longdouble sums of the scalars with the sum of their absolute terms (the
yardstick of the float64 bound), ``ece_from_table`` the float64 arithmetic of wg_calib_ece, ``curves_from_table``
sklearn's calibration_curve from the same table, ``fragile`` the elements whose float32 rounding a float64
evaluation may not reproduce.  ``MUTANTS`` names the deliberate mistakes tests/test_calib_eval_host.py must catch.
"""
import json
import os

import numpy as np

LD = np.longdouble
Q40 = 2 ** 40
KINDS = ("probs", "exp", "logits")


# the kind="exp" / "logits" inputs of tests/test_calib_eval.py: tests/test_calib_eval_host.py asserts that none of
# their elements is fragile (below), for every width and bin count in use
GPU_SEEDS = (11, 12, 13)
GPU_ROWS = 2 * 256 + 1
GPU_WIDTHS = (1, 2, 7, 40, 41, 64, 65, 256)
GPU_BINS = (1, 10, 15, 64)


def gpu_logits(C, seed, n=GPU_ROWS):
    """float32 logits at a moderate scale (no softmax entry rounds to 0 or 1)"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, C)) * 1.5 - 1.0).astype(np.float32)


def load_fixture_cases():
    """tests/golden/evaluation (tools/gen_golden_evaluation.py): name -> the manifest entry plus the arrays"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluation")
    with open(os.path.join(here, "manifest.json")) as f:
        manifest = json.load(f)
    with np.load(os.path.join(here, "evaluation_cases.npz"), allow_pickle=False) as d:
        data = {k: d[k] for k in d.files}
    cases = {}
    for name, info in manifest["cases"].items():
        c = dict(info)
        c["rows_form"] = c.pop("rows")
        for key in ("outputs", "labels", "rows", "triple", "per_class", "curve_lens", "curve_true", "curve_pred"):
            if f"{name}__{key}" in data:
                c[key] = data[f"{name}__{key}"]
        cases[name] = c
    return cases


def unflatten_curves(c):
    out, at = [], 0
    for ln in c["curve_lens"]:
        out.append((c["curve_true"][at:at + ln], c["curve_pred"][at:at + ln]))
        at += ln
    return out


def edges_of(n_bins):
    return np.linspace(0, 1, n_bins + 1)


def row_list(rows, n):
    if rows is None:
        return np.arange(n)
    rows = np.asarray(rows)
    return np.flatnonzero(rows) if rows.dtype == bool else rows.astype(np.int64)


def probabilities_ld(out, kind):
    """p of every element in np.longdouble, before the rounding to float32 (probs: the float32 itself)"""
    x = np.asarray(out, np.float32).astype(LD)
    if kind == "probs":
        return x
    with np.errstate(all="ignore"):
        if kind == "exp":
            return np.exp(x)
        e = np.exp(x - np.max(x, axis=1, keepdims=True))
        return e / np.sum(e, axis=1, keepdims=True)


def probabilities(out, kind):
    with np.errstate(all="ignore"):
        return probabilities_ld(out, kind).astype(np.float32)


def fragile(out, kind, n_bins=(10,), rel=2.0 ** -50):
    """Mask of the elements of a kind="exp" / "logits" input whose float32 p a float64 evaluation may round the other
    way: the longdouble p within `rel` (relative) of a float32 rounding midpoint, or the rounded p on a bin edge (of
    any of the bin counts n_bins)."""
    n_bins = (n_bins,) if np.isscalar(n_bins) else n_bins
    pl = probabilities_ld(out, kind)
    p32 = pl.astype(np.float32)
    with np.errstate(all="ignore"):
        up = np.nextafter(p32, np.float32(np.inf)).astype(LD)
        dn = np.nextafter(p32, np.float32(-np.inf)).astype(LD)
        p = p32.astype(LD)
        near = np.minimum(np.abs(pl - (p + up) / 2), np.abs(pl - (p + dn) / 2)) <= rel * np.abs(pl)
    on_edge = np.isin(p32.astype(np.float64), np.concatenate([edges_of(b) for b in n_bins]))
    return np.isfinite(p32) & (near | on_edge)


def _slots(p64, edges, right=True):
    n_bins = len(edges) - 1
    idx = np.digitize(p64, edges, right=right) - 1          # NaN -> n_bins
    return np.where(idx < 0, n_bins, np.where(idx >= n_bins, n_bins + 1, idx))


def bin_table(p32, labels, rows=None, n_bins=10, edges=None):
    """(C + 1, n_bins + 2, 3) uint64 of one set: include/wats_hip.h, wg_calib_bins."""
    p32 = np.asarray(p32, np.float32)
    n, C = p32.shape
    edges = edges_of(n_bins) if edges is None else edges
    idx = row_list(rows, n)
    p = p32[idx]
    y = np.asarray(labels)[idx]
    with np.errstate(all="ignore"):
        top = np.max(p, axis=1) if len(idx) else np.zeros(0, np.float32)          # a NaN wins, as torch.max
    arg = np.argmax(p, axis=1) if len(idx) else np.zeros(0, np.int64)            # first maximum, a NaN first
    cols = np.concatenate([p, top[:, None]], axis=1)
    lab = np.concatenate([y[:, None] == np.arange(C)[None, :], (arg == y)[:, None]], axis=1)
    slot = _slots(cols.astype(np.float64), edges)
    with np.errstate(all="ignore"):
        fixed = np.rint(cols.astype(np.float64) * Q40)
    third = np.where(slot < n_bins, fixed, np.where(slot == n_bins, cols == 0, np.isnan(cols) | (cols == np.inf)))
    third = np.where(np.isfinite(third), third, 0).astype(np.uint64)
    table = np.zeros((C + 1, n_bins + 2, 3), np.uint64)
    cc = np.broadcast_to(np.arange(C + 1)[None, :], slot.shape)
    np.add.at(table[..., 0], (cc, slot), np.uint64(1))
    np.add.at(table[..., 1], (cc, slot), lab.astype(np.uint64))
    np.add.at(table[..., 2], (cc, slot), third)
    return table


def ece_from_table(table, n_rows, min_count=4, mutant=None):
    """wg_calib_ece: float64, bins ascending; returns (ece_class (C), ece_top)"""
    C1, nb2, _ = table.shape
    n_bins = nb2 - 2
    out = np.zeros(C1)
    for c in range(C1):
        ece = 0.0
        for b in range(n_bins):
            cnt = int(table[c, b, 0])
            skip = cnt <= min_count if mutant == "le_min_count" else cnt < min_count
            if skip or cnt == 0:
                continue
            conf = (np.float64(table[c, b, 2]) / np.float64(Q40)) / np.float64(cnt)
            acc = np.float64(table[c, b, 1]) / np.float64(cnt)
            in_bins = float(table[c, :n_bins, 0].sum())
            weight = np.float64(cnt) / np.float64(in_bins if mutant == "weight_in_bins" else n_rows)
            ece += abs(conf - acc) * weight
        out[c] = ece
    return out[:-1], out[-1]


MUTANTS = ("right_false", "le_min_count", "weight_in_bins", "zero_binned", "drop_bad_labels", "logits_for_exp")


def model_report(out, labels, rows=None, kind="probs", n_bins=10, min_count=4, mutant=None):
    """The triple and the per-class ECE as the documented arithmetic gives them (mutant: one deliberate mistake)."""
    out = np.asarray(out, np.float32)
    labels = np.asarray(labels)
    idx = row_list(rows, out.shape[0])
    C = out.shape[1]
    if mutant == "logits_for_exp" and kind == "exp":
        kind = "logits"
    if mutant == "drop_bad_labels":
        idx = idx[(labels[idx] >= 0) & (labels[idx] < C)]
    p = probabilities(out, kind)
    edges = edges_of(n_bins)
    if mutant == "right_false":
        sub, y = p[idx], labels[idx]
        table = np.zeros((C + 1, n_bins + 2, 3), np.uint64)
        slot = _slots(sub.astype(np.float64), edges, right=False)
        for c in range(C):
            for b in range(n_bins + 2):
                m = slot[:, c] == b
                table[c, b] = (m.sum(), (m & (y == c)).sum(), int(np.rint(sub[m, c].astype(np.float64) * Q40).sum())
                               if b < n_bins else 0)
    else:
        table = bin_table(p, labels, idx, n_bins, edges)
    if mutant == "zero_binned":        # sklearn's rule used for the ECE: p == 0 in bin 0
        table = table.copy()
        zeros = table[:, n_bins, 2].copy()
        table[:, 0, 0] += zeros
        # the label count of the zeros is not kept apart: every p <= 0 of the fixtures is an exact zero
        table[:, 0, 1] += table[:, n_bins, 1]
    n = len(idx)
    ece_class, ece_top = ece_from_table(table, max(n, 1), min_count, mutant)
    sub = p[idx]
    with np.errstate(all="ignore"):
        acc = float(np.mean(np.argmax(sub, axis=1) == labels[idx])) if n else float("nan")
        conf = float(np.mean(np.max(sub, axis=1).astype(np.float64))) if n else float("nan")
    return {"acc": acc, "conf": conf, "ece": float(np.mean(ece_class)), "ece_class": ece_class, "ece_top": ece_top,
            "table": table, "n": n}


def curves_from_table(table, n_classes):
    """sklearn's calibration_curve per class from the table (p == 0 joins bin 0; empty bins dropped)"""
    n_bins = table.shape[1] - 2
    curves = []
    for c in range(n_classes):
        cnt = table[c, :n_bins, 0].astype(np.float64)
        true = table[c, :n_bins, 1].astype(np.float64)
        cnt[0] += float(table[c, n_bins, 0])
        true[0] += float(table[c, n_bins, 1])
        nz = cnt != 0
        curves.append((true[nz] / cnt[nz], (table[c, :n_bins, 2].astype(np.float64) / Q40)[nz] / cnt[nz]))
    return curves


def scalar_truth(out, labels, rows=None, kind="probs"):
    """np.longdouble truths of scalars [0 .. 6] and the sum of the absolute terms of each (the bound's yardstick)."""
    out = np.asarray(out, np.float32)
    labels = np.asarray(labels)
    idx = row_list(rows, out.shape[0])
    C = out.shape[1]
    p = probabilities(out, kind)[idx]
    x = out[idx].astype(LD)
    y = labels[idx]
    fin = np.all(np.isfinite(p), axis=1)
    p, x, y = p[fin], x[fin], y[fin]
    pl = p.astype(LD)
    ok = (y >= 0) & (y < C)
    r = np.flatnonzero(ok)
    py = p[r, y[r]]
    use = py > 0
    r, py = r[use], py[use]
    with np.errstate(all="ignore"):
        if kind == "logits":
            m = np.max(x[r], axis=1)
            terms = -((x[r, y[r]] - m) - np.log(np.sum(np.exp(x[r] - m[:, None]), axis=1)))
        elif kind == "exp":
            terms = -x[r, y[r]]
        else:
            terms = -np.log(py.astype(LD))
    onehot = (y[:, None] == np.arange(C)[None, :]).astype(LD)
    brier_terms = (pl - onehot) ** 2
    top = np.max(pl, axis=1) if len(p) else np.zeros(0, LD)
    arg = np.argmax(p, axis=1) if len(p) else np.zeros(0, np.int64)
    val = [len(idx), int(fin.sum()), int((arg == y).sum()), top.sum(), terms.sum(), len(r), brier_terms.sum()]
    mag = [0, 0, 0, np.abs(top).sum(), np.abs(terms).sum(), 0, brier_terms.sum()]
    return np.array(val, LD), np.array(mag, LD)
