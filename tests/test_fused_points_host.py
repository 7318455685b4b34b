"""The multi-point lane of k_run_episodes_fused, on the CPU.

tests/native_fused/fused_vs_single.cpp compiles cpr_amd/csrc/nak_fused.h for the host and
runs NA = 2 .. NAmax sweep points in one lane beside NA single lanes set up as the one-point
timed summary kernels set them up (gamma = 0: lazy clock; gamma = .5: lazy clock and deferred
races, a wave of one lane), on the same keyed stream with the same actions, and compares
every state word, the status bits and the lazy clock's +inf flag after every step (at
gamma = .5 the bits a race verification sets once the last verification has run): the four
built-in policies x delays {1e-9, 1e-3, .05} x max_steps 300 (and one episode of 16384),
alphas from (.05, .25, .35, .45, .5, .10), every fifth episode with a clock uniform forced
to zero.
"""

import json
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent
DIR = ROOT / "tests" / "native_fused"


def _run(exe, *args, timeout=900):
    subprocess.run(["make", "-s", "-C", str(DIR)], check=True)
    p = subprocess.run([str(DIR / "build" / exe), *args], capture_output=True, text=True,
                       timeout=timeout)
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert p.returncode == 0, p.stderr[-2000:]
    return out


def _episodes(out, per_case):
    sizes = out["fuse_max"] - 1  # group sizes 2 .. NAmax
    return 4 * (3 * sizes * per_case + 2)


def test_fused_lane_equals_single_lanes():
    both = _run("fused_vs_single", "20")
    for net in ("gamma0", "gamma05"):
        out = both[net]
        assert out["fuse_max"] >= 2
        assert out["mismatches"] == 0
        assert out["episodes"] == _episodes(out, 20)
        # a path that never ran cannot pass
        assert out["exact_branch_entries"] > 1000
        assert out["overlap_points"] > 100
        assert out["split_episodes"] > 0  # some points of a lane flagged, their siblings not
        assert out["inf_clock_episodes"] > 0
    out = both["gamma05"]
    assert out["races"] > 10000 and out["drains"] > 1000
    assert out["redo_points"] > 0


def test_fused_lane_under_host_sanitizers():
    # the same stand-alone program built with AddressSanitizer and UBSan, at a small size
    both = _run("fused_vs_single_asan", "5")
    for net in ("gamma0", "gamma05"):
        out = both[net]
        assert out["mismatches"] == 0
        assert out["episodes"] == _episodes(out, 5)
        assert out["inf_clock_episodes"] > 0
