"""The lane env's two host-compilable rules (cpr_amd/csrc/lane_env.h), without a GPU.

tests/native_laneenv/lane_env_host.cpp compiles the header for the host, plain and with
AddressSanitizer + UBSan, as a stand-alone program:

1. the per-episode alpha index against the rule stated in include/cpr_hip.h, computed here
   from the oracle's keyed stream (oracle_py.keyed_block / u53), never from the library;
2. the reward wrappers and shapes against cpr_amd/wrappers.py and ppo.py's `cut`
   (lane_env_ref.py) driven with the same synthetic step infos, bit for bit.
"""

import pathlib
import struct
import subprocess

import numpy as np
import pytest

import lane_env_ref as R

ROOT = pathlib.Path(__file__).resolve().parent.parent
DIR = ROOT / "tests" / "native_laneenv"
EXES = ["lane_env_host", "lane_env_host_asan"]


def _run(exe, *args):
    subprocess.run(["make", "-s", "-C", str(DIR)], check=True)
    p = subprocess.run([str(DIR / "build" / exe), *[str(a) for a in args]], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout.split()


# ------------------------------------------------------------------------- 1. the index rule

@pytest.mark.parametrize("exe", EXES)
@pytest.mark.parametrize("seed", [2024, 99])
def test_alpha_index_follows_the_keyed_stream(exe, seed):
    u = [R.alpha_u(seed, e) for e in range(4096)]
    for n_alpha in (1, 3, 4, 4096):
        want = [min(n_alpha - 1, int(x * n_alpha)) for x in u]
        got = [int(x) for x in _run(exe, "index", seed, n_alpha, 4096)]
        assert got == want, n_alpha
        if n_alpha in (3, 4):  # every entry is in use
            assert set(want) == set(range(n_alpha))


def test_alpha_index_of_the_gpu_tests_table():
    # the GPU tests' shape: 32 lanes, four alphas, seed 2024 -> the first 32 episodes use
    # the entries 6, 7, 9 and 10 times
    got = [R.alpha_index(2024, e, 4) for e in range(32)]
    assert sorted(np.bincount(got, minlength=4).tolist()) == [6, 7, 9, 10]


# ------------------------------------------------------------------- 2. the reward wrappers

TARGET = 8
ALPHA = 0.3


def scripted_episodes():
    """Episodes with awkward floats, ending with: total == 0 (and progress == 0), progress == 0
    with rewards, progress == target, overshoot, undershoot, and pairs around cut's 1.05."""
    rng = np.random.default_rng(5)
    ends = [
        (0.0, 0.0, 0.0, 5),              # total == 0, progress == 0
        (1.7, 0.3, 0.0, 9),              # progress == 0, rewards paid
        (3.3, 4.7, float(TARGET), 9),    # progress == target
        (2.9, 7.1, 10.0, 14),            # overshoot
        (0.1, 6.2, 7.0, 7),              # undershoot, no orphans (cut: the 0.9 branch)
        (5.0, 5.5, 10.0, 10),            # n_activations / progress == 1 <= 1.05
        (4.0, 6.0, 10.0, 11),            # 1.1 > 1.05
        (21.0 / 20.0, 19.0, 20.0, 21),   # 1.05 exactly
        (0.0, 9.0, 9.0, 12),             # the attacker got nothing
    ]
    eps = []
    for ra, rd, prog, acts in ends:
        n = int(rng.integers(1, 7))
        parts = rng.random(n)
        parts = parts / parts.sum() * ra  # step rewards, none of them round numbers
        steps = []
        for t in range(n):
            f = 1.0 if t == n - 1 else (t + 1) / n
            steps.append((float(parts[t]), t == n - 1, ra * f, rd * f, prog * f, int(acts * f)))
        eps.append((ALPHA, steps))
    return eps


@pytest.mark.filterwarnings("ignore:observed too")
@pytest.mark.parametrize("exe", EXES)
@pytest.mark.parametrize("shape", range(3))
@pytest.mark.parametrize("scheme", range(4))
def test_wrapper_header_equals_python_wrappers_bit_for_bit(tmp_path, exe, scheme, shape):
    eps = scripted_episodes()
    ends = [steps[-1] for _, steps in eps]
    if R.SCHEMES[scheme] == "dense_per_progress":
        # the dense wrapper divides by the progress at done: the reference raises at 0, and
        # the header documents that it adds no correction there
        eps = [e for e in eps if e[1][-1][4] != 0.0]
        assert any(s[4] == TARGET for s in ends) and any(s[4] > TARGET for s in ends)
        assert any(0 < s[4] < TARGET for s in ends)
    else:
        assert any(s[2] + s[3] == 0 for s in ends) and any(s[4] == 0 and s[2] > 0 for s in ends)
    want = R.wrapped_rewards(eps, R.SCHEMES[scheme], R.SHAPES[shape], TARGET)
    lines = []
    for _, steps in eps:
        lines.append("reset")
        for r, d, ra, rd, prog, acts in steps:
            lines.append(" ".join([float(r).hex(), str(int(d)), float(ra).hex(), float(rd).hex(),
                                   float(prog).hex(), str(acts)]))
    path = tmp_path / "steps.txt"
    path.write_text("\n".join(lines) + "\n")
    got = _run(exe, "wrap", scheme, shape, float(TARGET).hex(), float(ALPHA).hex(), path)
    got = [struct.unpack("<d", struct.pack("<Q", int(x, 16)))[0] for x in got]
    assert len(got) == len(want)
    bits = lambda v: [struct.pack("<d", x) for x in v]  # noqa: E731
    assert bits(got) == bits(want)
    assert any(x != 0.0 for x in want)
