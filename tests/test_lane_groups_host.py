"""A lane group of k_run_episodes_fused, on the CPU.

tests/native_lane_groups/lane_groups_vs_single.cpp compiles cpr_amd/csrc/nak_fused.h for the
host and models a group as G lane objects stepped in lockstep: each holds NA sweep points,
refills its held TAG_ACT block where the activation count is a multiple of G (the kernel's
group_fill), and the exchange, a function over the array of held blocks, hands every lane
the block of lane k mod G. Beside it run NA * G single lanes set up as the one-point timed
summary kernels set them up, on the same keyed stream with the same actions; every state
word, the status bits and the lazy clock's +inf flag of every point are compared after every
step (at gamma = .5 the bits a race verification sets once the last verification has run).
G in {2, 4} x NA in {2, 5} at gamma = 0 and NA = 2 at gamma = .5, the four built-in policies
x delays {1e-9, 1e-3, .05} x max_steps {299, 300, 301, 302} (the activation count modulo G
takes every residue), one episode of 16384 steps per shape, every fifth episode with a clock
uniform forced to zero.
"""

import json
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent
DIR = ROOT / "tests" / "native_lane_groups"


def _run(exe, *args, timeout=900):
    subprocess.run(["make", "-s", "-C", str(DIR)], check=True)
    p = subprocess.run([str(DIR / "build" / exe), *args], capture_output=True, text=True,
                       timeout=timeout)
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert p.returncode == 0, p.stderr[-2000:]
    return out


def _episodes(shapes, per_case):
    # per policy and shape: 3 delays x 4 episode lengths; SM1 adds the 16384-step episode
    return shapes * (4 * 3 * 4 * per_case + 1)


def _check(both, per_case):
    for net, shapes in (("gamma0", 4), ("gamma05", 2)):
        out = both[net]
        assert out["mismatches"] == 0
        assert out["block_errors"] == 0
        assert out["episodes"] == _episodes(shapes, per_case)
        # one block per lane per G activations, rounded up: counted where the stream
        # computes them
        assert out["blocks"] == out["blocks_expected"] > 0
        assert out["inf_clock_episodes"] > 0


def test_lane_group_equals_single_lanes():
    both = _run("lane_groups_vs_single", "10")
    _check(both, 10)
    for net in ("gamma0", "gamma05"):
        out = both[net]
        # a path that never ran cannot pass
        assert out["exact_branch_entries"] > 0
        assert out["overlap_points"] > 0
        assert out["split_episodes"] > 0  # some points of a group flagged, their siblings not
        assert out["split_lanes"] > 0     # ... and some lanes of a group, the others not
    out = both["gamma05"]
    assert out["races"] > 0 and out["drains"] > 0
    assert out["redo_points"] > 0


def test_lane_group_under_host_sanitizers():
    # the same stand-alone program built with AddressSanitizer and UBSan, at a small size
    # (five episodes per case: the fifth has its clock uniform forced to zero)
    both = _run("lane_groups_vs_single_asan", "5")
    _check(both, 5)
