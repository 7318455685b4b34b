"""oracle_py.reduce_records, the oracle side of tests/test_gpu_sweep_oracle.py, without a GPU.

1. Hand-written records whose summary words are written out by hand: no payout (rel 0,
   bin 0), rel exactly 1.0 (bin 64 clipped to 63), rel 63/64 (bin 63 unclipped), a reward whose
   2^20 multiple lies exactly between two integers (rint rounds to even: a reduction that
   rounds half away from zero gives other words), an invalid episode, and the status rule.
2. 512 real oracle episodes against the second restatement, eval_ref.summary (a per-episode
   Python loop written for cpr_eval_net), and the identities the device's summary kernels
   rely on: reward_attacker + reward_defender = head_height = progress.
"""

import numpy as np

import eval_ref as E
import oracle_py as O
from cpr_amd import _lib as L
from cpr_amd import device

# (reward_attacker, reward_defender, progress, n_steps, n_activations, head_height, status)
H = 0.5 + 2.0 ** -21  # H * 2^20 = 524288.5, (1.5 - 2^-21) * 2^20 = 1572863.5
EPISODES = [
    (0.0, 0.0, 0.0, 3, 4, 0, 0),                                    # rel 0, bin 0
    (5.0, 0.0, 5.0, 10, 11, 5, 0),                                  # rel 1.0, bin 64 -> 63
    (1.0, 3.0, 4.0, 7, 8, 4, L.ST_TIE | L.ST_EXACT_RERUN),          # rel .25, bin 16
    (3.0, 1.0, 4.0, 9, 10, 4, L.ST_DEEP_FORK),                      # rel .75, bin 48, other
    (100.0, 100.0, 200.0, 50, 60, 200, L.ST_CAPACITY | L.ST_TIE),   # invalid
    (1.0, 2.0, 3.0, 5, 6, 3, L.ST_OVERLAP | L.ST_EXACT_RERUN),      # rel 1/3, bin 21
    (H, 1.5 - 2.0 ** -21, 2.0, 2, 3, 2, 0),                         # rel .25 + 2^-22, bin 16
    (63.0, 1.0, 64.0, 100, 130, 64, 0),                             # rel 63/64, bin 63
]


def _records(rows):
    r = np.zeros(len(rows), dtype=L.RECORD_DTYPE)
    for i, (ra, rd, pr, ns, na, hh, st) in enumerate(rows):
        r[i]["reward_attacker"], r[i]["reward_defender"], r[i]["progress"] = ra, rd, pr
        r[i]["n_steps"], r[i]["n_activations"], r[i]["head_height"], r[i]["status"] = ns, na, hh, st
    return r


def _hist(**bins):
    h = [0] * 64
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


def test_hand_written_episodes():
    got = O.reduce_records(_records(EPISODES))
    want = {
        "episodes": 7,
        "steps": 3 + 10 + 7 + 9 + 50 + 5 + 2 + 100,
        "activations": 4 + 11 + 8 + 10 + 60 + 6 + 3 + 130,
        # 5 + 1 + 3 + 1 + 63 whole rewards, and 524288.5 rounded to even
        "reward_attacker_fx": 73 * 1048576 + 524288,
        # 3 + 1 + 2 + 1 whole rewards, and 1572863.5 rounded to even
        "reward_defender_fx": 7 * 1048576 + 1572864,
        "progress_fx": (5 + 4 + 4 + 3 + 2 + 64) * 1048576,
        # 1, 1/4, 3/4, 1/3 (2^32 / 3 = 1431655765.33), 1/4 + 2^-22, 63/64
        "rel_revenue_fx": 4294967296 + 1073741824 + 3221225472 + 1431655765 + (1073741824 + 1024)
        + 4227858432,
        # 1, 1/16, 9/16, 1/9 (2^32 / 9 = 477218588.44), 2^-4 + 2^-23 + 2^-44, 3969/4096
        "rel_revenue_sq_fx": 4294967296 + 268435456 + 2415919104 + 477218588 + (268435456 + 512)
        + 4161798144,
        "orphans": 4 + 6 + 4 + 6 + 3 + 1 + 66,
        "status_tie": 1,      # the invalid episode's TIE bit is not counted
        "status_overlap": 1,
        "status_other": 1,    # DEEP_FORK; TIE | EXACT_RERUN and OVERLAP | EXACT_RERUN are not
        "invalid": 1,
        "hist": _hist(b0=1, b16=2, b21=1, b48=1, b63=2),
    }
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    assert all(type(v) is int for k, v in got.items() if k != "hist")
    assert set(got) - {"hist"} == set(L.Summary.FIELDS)


def test_status_rule_one_bit_at_a_time():
    base = (1.0, 1.0, 2.0, 4, 5, 2)
    for st, field in [(L.ST_TIE, "status_tie"), (L.ST_OVERLAP, "status_overlap"),
                      (L.ST_EXACT_RERUN, None), (L.ST_TIE | L.ST_EXACT_RERUN, "status_tie"),
                      (L.ST_DEEP_FORK, "status_other"), (L.ST_TIE_UNRESOLVED, "status_other"),
                      (L.ST_STALE_TIME, "status_other")]:
        got = O.reduce_records(_records([base + (st,)]))
        for f in ("status_tie", "status_overlap", "status_other"):
            assert got[f] == (1 if f == field else 0), (st, f)
        assert got["episodes"] == 1 and got["invalid"] == 0
    for st in (L.ST_CAPACITY, L.ST_REFERENCE_RAISES, L.ST_TRACE_MISS):
        got = O.reduce_records(_records([base + (st | L.ST_DEEP_FORK,)]))
        assert got["invalid"] == 1 and got["steps"] == 4 and got["activations"] == 5
        assert all(v == 0 for k, v in got.items()
                   if k not in ("invalid", "steps", "activations", "hist"))
        assert sum(got["hist"]) == 0


def test_empty():
    got = O.reduce_records(np.zeros(0, dtype=L.RECORD_DTYPE))
    assert all(v == 0 for k, v in got.items() if k != "hist") and got["hist"] == [0] * 64


def _as_eval_columns(rec):
    names = {"n_steps": "episode_n_steps", "n_activations": "episode_n_activations",
             "progress": "episode_progress", "head_height": "height"}
    out = np.zeros(len(rec), dtype=[(names.get(n, n), rec.dtype[n]) for n in rec.dtype.names])
    for n in rec.dtype.names:
        out[names.get(n, n)] = rec[n]
    return out


def test_oracle_episodes_against_the_second_restatement():
    cfg, _ = device.make_config(alpha=0.4, gamma=0.5, max_steps=500, seed=0x5EED0000)
    rec = O.run_episodes(cfg, 0, 512, threads=8)
    got = O.reduce_records(rec)
    assert got == E.summary(_as_eval_columns(rec))
    assert got["episodes"] == 512 and got["steps"] == 512 * 500
    assert 0 < got["reward_attacker_fx"] < got["progress_fx"]
    # what the device's summary kernels assume of a Nakamoto gym episode
    assert np.array_equal(rec["reward_attacker"] + rec["reward_defender"], rec["progress"])
    assert np.array_equal(rec["progress"], rec["head_height"].astype(np.float64))
    # the same after mixing in hand-written episodes (an invalid one, rel 0 and rel 1)
    mixed = np.concatenate([rec, _records(EPISODES)])
    assert O.reduce_records(mixed) == E.summary(_as_eval_columns(mixed))
