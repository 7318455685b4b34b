"""The lane over packed tips (NakLanePacked, nakamoto_lane.h PTip), on the CPU.

tests/native_tips/packed_vs_refs.cpp runs it beside the lane over BRef tips (NakLane) through
fused_reset, fused_step and fused_verify_races on the same keyed stream and compares, after
every step, every word of NakLane::pack except the tips' k, tinf, esum, qn and rw of every
point, at gamma = .5 the race lists, and at the end the heads: the four built-in policies x
ARR {0, 1} x alphas {.05, .33, .5, t_att = 2^32} x max_steps {16, 300, 2016, 16384} x delays
{1e-9, 1e-3}, every third episode with a clock uniform forced to zero. The packed lane's
assertion that no height carries into the attacker count is live in the host build.
"""

import json
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent
DIR = ROOT / "tests" / "native_tips"


def _run(exe, *args, timeout=900):
    subprocess.run(["make", "-s", "-C", str(DIR)], check=True)
    p = subprocess.run([str(DIR / "build" / exe), *args], capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _episodes(per_case):
    # per policy and delay: two alpha pairs x (16, 300: per_case; 2016: per_case / 2 + 1;
    # 16384: 1); per policy once more 16384 steps x 3
    return 4 * (2 * 2 * (2 * per_case + per_case // 2 + 1 + 1) + 2 * 3)


def test_packed_lane_equals_lane_over_refs():
    both = _run("packed_vs_refs", "6")
    for net in ("gamma0", "gamma05"):
        out = both[net]
        assert out["mismatches"] == 0
        assert out["episodes"] == _episodes(6)
        # a path that never ran cannot pass
        assert out["inf_clock_episodes"] > 0
        assert out["overlap_points"] > 0
        assert out["deep_fork_points"] > 0  # t_att = 2^32: the private chain reaches cap
        assert out["max_private"] == 4095
        assert out["max_height"] > 2 ** 13  # both halves of the word well past 2^8
    out = both["gamma05"]
    assert out["races"] > 10000 and out["drains"] > 1000
    assert out["redo_points"] > 0  # 1e-9: races too close to decide without the clock


def test_packed_lane_under_host_sanitizers():
    # the same stand-alone program built with AddressSanitizer and UBSan, at a small size
    both = _run("packed_vs_refs_asan", "2")
    for net in ("gamma0", "gamma05"):
        out = both[net]
        assert out["mismatches"] == 0
        assert out["episodes"] == _episodes(2)
        assert out["inf_clock_episodes"] > 0
