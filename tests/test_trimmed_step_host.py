"""The fused lanes' trimmed step (nakamoto_lane.h policy_flags, apply_flags, LaneMem::cap_test),
on the CPU.

tests/native_step/step_vs_lane.cpp checks policy_flags against the decoding of nak_policy's
action (four built-in policies, h and a in 0..40), and steps NakLanePacked through fused_step
with the capacity test off and cap = max_steps + 2 beside one NakLane per point through
policy_action, apply, resolve and activate with the test on: every NakLane::pack word, rw,
tinf, the listed races and the heads, four policies x ARR {0, 1} x alphas {.05, .33, .5,
t_att = 2^32} x max_steps {1, 16, 62, 300} x delays {1e-9, 1e-3}. The lane's host assertions on
the step's one released tip are live in that build and abort it.
"""

import json
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent
DIR = ROOT / "tests" / "native_step"


def _run(exe, *args, timeout=900):
    subprocess.run(["make", "-s", "-C", str(DIR)], check=True)
    p = subprocess.run([str(DIR / "build" / exe), *args], capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _episodes(per_case):
    # per policy: two delays x four lengths x two alpha pairs
    return 4 * 2 * 4 * 2 * per_case


def _check(out, per_case):
    fl = out["flags"]
    assert fl["mismatches"] == 0
    assert fl["checked"] == 4 * 41 * 41 * 2
    # every decision occurs, and exactly one per observation
    assert min(fl["adopt"], fl["match"], fl["override"], fl["wait"]) > 0
    assert fl["adopt"] + fl["match"] + fl["override"] + fl["wait"] == fl["checked"]
    for net in ("gamma0", "gamma05"):
        o = out[net]
        assert o["mismatches"] == 0
        assert o["episodes"] == _episodes(per_case)
        assert o["deep_fork_points"] == 0
        # t_att = 2^32 under a policy that never releases: n reaches max_steps + 1 = cap - 1
        assert o["max_private"] == 301 and o["cap_minus_private_min"] == 1
        # a path that never ran cannot pass: the shared tip reached A or pub, p0 moved
        assert o["releases"] > 0 and o["deliveries"] > 0 and o["adopts"] > 0
        assert o["inf_clock_episodes"] > 0
    assert out["gamma0"]["races"] == 0
    assert out["gamma05"]["races"] > 100 * per_case and out["gamma05"]["drains"] > 0


def test_trimmed_step_equals_lane_over_refs():
    out = _run("step_vs_lane", "6")
    _check(out, 6)
    assert out["gamma05"]["redo_points"] > 0  # 1e-9: races too close to decide without the clock


def test_trimmed_step_under_host_sanitizers():
    # the same stand-alone program built with AddressSanitizer and UBSan, at a small size
    _check(_run("step_vs_lane_asan", "3"), 3)
