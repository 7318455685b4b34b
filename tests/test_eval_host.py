"""The evaluation's host-compilable rules (cpr_amd/csrc/eval.h, lane_env.h), without a GPU.

tests/native_eval/eval_host.cpp compiles the headers for the host, plain and with
AddressSanitizer + UBSan, as a stand-alone program:

1. the cyclic schedule's table entry against e % n_alpha, around 2^32 too;
2. record -> summary and the documented order of the statistics against the restatement in
   eval_ref.py on scripted records, bit for bit: an invalid episode, n = 1 (std NaN) and
   n = 257 (the strided part and the tree both have work);
3. the restated mean against math.fsum within the bound every summation order keeps.
"""

import math
import pathlib
import subprocess

import numpy as np
import pytest

import eval_ref as E
from cpr_amd import _lib as L

ROOT = pathlib.Path(__file__).resolve().parent.parent
DIR = ROOT / "tests" / "native_eval"
EXES = ["eval_host", "eval_host_asan"]


def _run(exe, *args):
    subprocess.run(["make", "-s", "-C", str(DIR)], check=True)
    p = subprocess.run([str(DIR / "build" / exe), *[str(a) for a in args]], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


@pytest.mark.parametrize("exe", EXES)
def test_cycle_entry_is_the_episode_id_modulo_the_table(exe):
    for n_alpha in (1, 3, 4, 4096):
        for first in (0, 2**32 - 50, 2**32, 2**63 + 11, 2**64 - 100):
            got = [int(x) for x in _run(exe, "cycle", n_alpha, first, 100).split()]
            assert got == [(first + i) % n_alpha for i in range(100)], (n_alpha, first)


def scripted_records(n_alpha, per_alpha, first, seed, invalid=()):
    """Records with awkward floats: slot s is episode first + s; `invalid` slots carry a
    CPR_ST_INVALID bit; some episodes pay nothing (rel = 0), some carry other status bits."""
    rng = np.random.default_rng(seed)
    n = n_alpha * per_alpha
    r = np.zeros(n, dtype=L.EVAL_RECORD_DTYPE)
    r["episode"] = first + np.arange(n, dtype=np.uint64)
    r["alpha_index"] = (first + np.arange(n)) % n_alpha
    r["alpha"] = (r["alpha_index"] + 1) / 16.0
    r["reward_attacker"] = rng.integers(0, 40, n) * rng.choice([1.0, 0.1, 1 / 3], n)
    r["reward_defender"] = rng.integers(0, 60, n) * rng.choice([1.0, 0.7], n)
    r["episode_progress"] = rng.integers(0, 100, n) * rng.choice([1.0, 0.5], n)
    r["episode_reward"] = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, n)
    r["episode_sim_time"] = rng.exponential(100.0, n)
    r["episode_chain_time"] = r["episode_sim_time"] * rng.uniform(0.5, 1.0, n)
    r["episode_n_activations"] = rng.integers(1, 300, n)
    r["episode_n_steps"] = rng.integers(1, 128, n)
    r["height"] = rng.integers(0, 100, n)
    r["status"] = rng.choice([0, 0, L.ST_TIE, L.ST_OVERLAP | L.ST_EXACT_RERUN, L.ST_DEEP_FORK], n)
    for s in invalid:
        r["status"][s] |= L.ST_CAPACITY
    return r


CASES = {
    # name: (n_alpha, per_alpha, first, invalid slots)
    "n1": (3, 1, 0, ()),                      # one record per alpha: std NaN
    "invalid": (4, 24, 5, (0, 6, 7, 95)),     # a first episode that is no multiple of the table
    "all_invalid": (2, 1, 0, (0,)),           # n = 0 for entry 0: mean NaN too
    "n257": (2, 257, 2**32 - 3, (100,)),      # thread 0 adds two records, then the tree
    "n600": (1, 600, 7, (256, 511)),
}


@pytest.mark.parametrize("exe", EXES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_reduction_equals_the_restatement_bit_for_bit(exe, case, tmp_path):
    n_alpha, per_alpha, first, invalid = CASES[case]
    recs = scripted_records(n_alpha, per_alpha, first, seed=len(case), invalid=invalid)
    path = tmp_path / "records.bin"
    recs.tofile(path)
    lines = _run(exe, "reduce", path, n_alpha, first).strip().split("\n")
    assert len(lines) == n_alpha
    slots = E.alpha_slots(n_alpha, first, len(recs))
    for j, line in enumerate(lines):
        w = line.split()
        mine = recs[slots[j]]
        assert len(mine) == per_alpha and np.all(mine["alpha_index"] == j)
        want = E.summary(mine)
        n, mean, std = E.stats(mine)
        assert int(w[0]) == j and int(w[1]) == n == want["episodes"]
        got = [int(x) for x in w[2:15]]
        got[6] %= 2**64  # printed as signed
        got[7] %= 2**64
        assert got == [want[f] for f in E.SUM_FIELDS], case
        assert [int(x) for x in w[15:15 + L.HIST_BINS]] == want["hist"]
        bits = [int(x, 16) for x in w[15 + L.HIST_BINS:]]
        got_mean = np.array(bits[0::2], dtype=np.uint64).view(np.float64)
        got_std = np.array(bits[1::2], dtype=np.uint64).view(np.float64)
        assert E.same_bits(got_mean, mean), (case, j, got_mean, mean)
        assert E.same_bits(got_std, std), (case, j, got_std, std)
        assert np.all(np.isnan(got_std)) == (n < 2)
        assert np.all(np.isnan(got_mean)) == (n < 1)
    if case == "invalid":
        assert [E.summary(recs[s])["invalid"] for s in slots] == [2, 1, 0, 1]


def test_restated_mean_is_within_the_bound_of_any_summation_order():
    # |sum_in_any_order - exact| <= (n - 1) u sum|x| to first order with u = 2^-53; fsum is the
    # correctly rounded exact sum. Guards against a wrong order (a dropped or doubled
    # record), not a sloppy one.
    for case, (n_alpha, per_alpha, first, invalid) in CASES.items():
        recs = scripted_records(n_alpha, per_alpha, first, seed=len(case), invalid=invalid)
        for mine in (recs[s] for s in E.alpha_slots(n_alpha, first, len(recs))):
            n, mean, _ = E.stats(mine)
            ok = mine[(mine["status"] & L.ST_INVALID) == 0]
            assert n == len(ok)
            if n == 0:
                continue
            for c, name in enumerate(L.EVAL_COLUMNS):
                x = [float(v) for v in ok[name]]
                bound = (n - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in x) / n
                assert abs(mean[c] - math.fsum(x) / n) <= bound, (case, name)


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cpr_hip.h"\n'
        'int main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(cpr_eval_opts), '
        'sizeof(cpr_eval_record), sizeof(cpr_eval_alpha), offsetof(cpr_eval_record, alpha_index), '
        'offsetof(cpr_eval_alpha, std), offsetof(cpr_eval_opts, check_every));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    import ctypes

    assert got == [ctypes.sizeof(L.EvalOptsC), ctypes.sizeof(L.EvalRecord),
                   ctypes.sizeof(L.EvalAlpha), L.EvalRecord.alpha_index.offset,
                   L.EvalAlpha.std.offset, L.EvalOptsC.check_every.offset]
    assert L.EVAL_RECORD_DTYPE.fields["alpha_index"][1] == L.EvalRecord.alpha_index.offset
    assert L.EVAL_ALPHA_DTYPE.fields["std"][1] == L.EvalAlpha.std.offset
