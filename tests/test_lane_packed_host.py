"""The lane as the two timed summary-only kernels configure it, on the CPU.

tests/native_packed/summary_lane_vs_eager.cpp compiles cpr_amd/csrc/nakamoto_lane.h for the
host twice over: once as k_run_episodes' gamma = 0 and gamma = .5 summary instantiations set
it up (no block times, lazy clock with the high-word skip test, 32-bit miner draw, 32-bit
masks at d = 2, deferred races over an emulated wave's list) and once as the general eager
lane, and compares observation, head, activation count and status after every step:
alpha {.05, .33, .45, .5} x (gamma 0 with d {2, 3, 5}, gamma .5 with d 2) x SM1, ES'14,
honest, random actions x delays {1e-9, 1e-5, 1e-3} x max_steps {300, 16384}, zero clock
uniforms (+inf delays), and alpha = 1. Every draw's miner is checked against the 64-bit
formula as well.
"""

import json
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent
DIR = ROOT / "tests" / "native_packed"


def _run(exe, *args, timeout=900):
    subprocess.run(["make", "-s", "-C", str(DIR)], check=True)
    p = subprocess.run([str(DIR / "build" / exe), *args], capture_output=True, text=True,
                       timeout=timeout)
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert p.returncode == 0, p.stderr[-2000:]
    return out


def test_timed_lane_equals_eager_lane():
    out = _run("summary_lane_vs_eager", "24", "4")
    assert out["mismatches"] == 0 and out["miner_mismatches"] == 0
    assert out["episodes"] == 192 * 24 + 192 * 4 + 3 * 8
    # a path that never ran cannot pass
    assert out["exact_branch_entries"] > 1000
    assert out["overlap_episodes"] > 100
    assert out["tie_episodes"] > 0
    assert out["redo_episodes"] > 0
    assert out["inf_clock_episodes"] > 0
    assert out["races"] > 10000 and out["drains"] > 1000
    assert out["alpha1_draws"] == 3 * 8 * 300


def test_timed_lane_under_host_sanitizers():
    # the same stand-alone program built with AddressSanitizer and UBSan, at a small size
    out = _run("summary_lane_vs_eager_asan", "4", "0")
    assert out["mismatches"] == 0 and out["miner_mismatches"] == 0
    assert out["episodes"] == 192 * 4 + 3 * 8
