"""The closed-form rollout step on the CPU, beside the oracle's gym.

tests/native_rollout/nak_rollout_vs_oracle.cpp compiles cpr_amd/csrc/nak_rollout.h (policy,
action log, step, done rule, reward, auto-reset at episode id + n_lanes) for the host and
runs 32 lanes x 300 steps of it per configuration (4 policies x alpha {.25, .42} x gamma
{0, .5}, max_steps 70) beside sequential oracle episodes on the same keyed stream. The GPU
runs the same header inside k_nak_rollout (tests/test_gpu_nak_rollout.py).
"""

import json
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_rollout_step_matches_oracle_gym():
    d = ROOT / "tests" / "native_rollout"
    subprocess.run(["make", "-s", "-C", str(d)], check=True)
    p = subprocess.run([str(d / "build" / "nak_rollout_vs_oracle"), "32", "300", "70"],
                       capture_output=True, text=True, timeout=600)
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert p.returncode == 0, p.stderr[-2000:]
    assert out["mismatches"] == 0, p.stderr[-2000:]
    assert out["episodes"] > 1000
    assert out["steps"] == 16 * 32 * 300
