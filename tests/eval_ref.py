"""numpy / Python restatement of the evaluation's per-alpha reduction (include/cpr_hip.h
cpr_eval_net): what a record adds to a cpr_summary, and the documented order of the f64
statistics. Python floats are IEEE doubles with one rounding per operation, so the results can
be compared bit for bit with the device's and with tests/native_eval."""

import math

import numpy as np

from cpr_amd import _lib as L

THREADS = 256
SUM_FIELDS = ["episodes", "steps", "activations", "reward_attacker_fx", "reward_defender_fx",
              "progress_fx", "rel_revenue_fx", "rel_revenue_sq_fx", "orphans", "status_tie",
              "status_overlap", "status_other", "invalid"]


def alpha_slots(n_alpha, first, n_set):
    """Slots of table entry j, for every j: the s with (first + s) mod n_alpha = j, in order."""
    return [[s for s in range(n_set) if (first + s) % n_alpha == j] for j in range(n_alpha)]


def summary(recs):
    """cpr_summary of records as {field: int, "hist": [64 ints]}: the rule of every other
    summary, an episode with CPR_ST_INVALID bits in steps / activations / invalid only."""
    s = {f: 0 for f in SUM_FIELDS}
    hist = [0] * L.HIST_BINS
    for r in recs:
        st = int(r["status"])
        steps, acts = int(r["episode_n_steps"]), int(r["episode_n_activations"])
        s["steps"] += steps
        s["activations"] += acts
        if st & L.ST_INVALID:
            s["invalid"] += 1
            continue
        ra, rd = float(r["reward_attacker"]), float(r["reward_defender"])
        rel = ra / (ra + rd) if (ra + rd) != 0.0 else 0.0
        s["episodes"] += 1
        s["reward_attacker_fx"] += int(np.rint(ra * 1048576.0))
        s["reward_defender_fx"] += int(np.rint(rd * 1048576.0))
        s["progress_fx"] += int(np.rint(float(r["episode_progress"]) * 1048576.0))
        s["rel_revenue_fx"] += int(np.rint(rel * 4294967296.0))
        s["rel_revenue_sq_fx"] += int(np.rint(rel * rel * 4294967296.0))
        s["orphans"] += acts - int(r["height"])
        s["status_tie"] += 1 if st & L.ST_TIE else 0
        s["status_overlap"] += 1 if st & L.ST_OVERLAP else 0
        s["status_other"] += 1 if st & ~(L.ST_TIE | L.ST_OVERLAP | L.ST_EXACT_RERUN) else 0
        hist[min(L.HIST_BINS - 1, max(0, int(rel * L.HIST_BINS)))] += 1
    s["hist"] = hist
    return s


def summary_of(cs):
    """A ctypes Summary in ``summary``'s form."""
    d = {f: int(getattr(cs, f)) for f in SUM_FIELDS}
    d["hist"] = [int(x) for x in cs.hist]
    return d


def _ordered_sum(values):
    """p_t = 0 + its values t, t + 256, ... in order; then the tree off = 128, 64, ..., 1."""
    p = [0.0] * THREADS
    for t in range(THREADS):
        for k in range(t, len(values), THREADS):
            if values[k] is not None:
                p[t] = p[t] + values[k]
    off = THREADS // 2
    while off > 0:
        for t in range(off):
            p[t] = p[t] + p[t + off]
        off //= 2
    return p[0]


def stats(recs):
    """(n, mean[5], std[5]) of an alpha's records (in slot order) in the documented order; an
    invalid record keeps its position k and adds nothing."""
    valid = [(int(r["status"]) & L.ST_INVALID) == 0 for r in recs]
    n = sum(valid)
    mean, std = [], []
    for name in L.EVAL_COLUMNS:
        x = [float(r[name]) if v else None for r, v in zip(recs, valid)]
        m = _ordered_sum(x) / n if n > 0 else float("nan")
        dev = [None if v is None else (v - m) * (v - m) for v in x]
        sd = math.sqrt(_ordered_sum(dev) / (n - 1)) if n > 1 else float("nan")
        mean.append(m)
        std.append(sd)
    return n, mean, std


def same_bits(a, b):
    """Equal as bit patterns, any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
