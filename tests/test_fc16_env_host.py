"""The FC'16 model as an environment (CPR_PROTO_FC16_ENV), without a GPU.

(a) tests/fc16_env_ref.py, the pure-Python env that the GPU tests compare the device lanes
    with, driven with the index of the action that honest play, SM1 and a random table name:
    it reproduces the pinned episode oracle (oracle_py.fc16_episode).
(b) tests/native_fc16/fc16_host.cpp compiles cpr_amd/csrc/fc16_lane.h for the host, plain
    and with AddressSanitizer + UBSan, as a stand-alone program: fc16_start / fc16_step /
    the action rule / the observation under random index sequences equal the Python env
    step by step, observations bit for bit.
"""

import pathlib
import struct
import subprocess

import numpy as np
import pytest

import fc16_env_ref as R
import oracle_py as O

ROOT = pathlib.Path(__file__).resolve().parent.parent
DIR = ROOT / "tests" / "native_fc16"
EXES = ["fc16_host", "fc16_host_asan"]


# ------------------------------------------------ (a) the reference env against the oracle

def _random_table(dim, seed):
    return np.random.default_rng(seed).integers(0, 4, dim * dim * 3).astype(np.uint8)


@pytest.mark.parametrize("policy", ["honest", "sm1", "table"])
def test_reference_env_reproduces_the_episode_oracle(policy):
    seed, alpha, gamma, horizon, max_steps = 11, 0.35, 0.5, 10, 50
    pid = {"honest": 0, "sm1": 1, "table": 2}[policy]
    table = _random_table(6, 3) if policy == "table" else None
    env = R.Fc16EnvRef(seed, alpha, gamma, horizon, max_steps)
    n_trunc = n_term = 0
    for e in range(500):
        want = O.fc16_episode(seed, e, alpha, gamma, horizon, pid, table, max_steps=max_steps)
        env.reset(e)
        while True:
            name = O.fc16_policy(pid, env.a, env.h, env.fork, table, 6)
            _, _, term, trunc = env.step(R.index_of(env.a, env.h, name))
            if term or trunc:
                break
        assert (env.reward, env.progress, env.steps, trunc) == tuple(want), e
        n_trunc += trunc
        n_term += term
    assert n_term > 0
    if policy != "honest":  # honest play makes progress at every other step
        assert n_trunc > 0


def test_action_rule_table():
    # index 2: Override if a > h, Match if a = h, Wait if a < h; index 3: Match if a > h
    assert [R.action_name(2, 1, i) for i in range(5)] == [R.WAIT, R.ADOPT, R.OVERRIDE, R.MATCH,
                                                          R.WAIT]
    assert [R.action_name(1, 1, i) for i in range(4)] == [R.WAIT, R.ADOPT, R.MATCH, R.WAIT]
    assert [R.action_name(0, 1, i) for i in range(4)] == [R.WAIT, R.ADOPT, R.WAIT, R.WAIT]


# ------------------------------------------------------ (b) fc16_lane.h on the host

def _run(exe, *args):
    subprocess.run(["make", "-s", "-C", str(DIR)], check=True)
    p = subprocess.run([str(DIR / "build" / exe), *[str(a) for a in args]], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return [ln.split() for ln in p.stdout.splitlines()]


def _bits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


@pytest.mark.parametrize("exe", EXES)
def test_lane_header_equals_reference_env_step_by_step(tmp_path, exe):
    seed, alpha, gamma, horizon = 77, 0.4, 0.6, 8
    env = R.Fc16EnvRef(seed, alpha, gamma, horizon)
    rng = np.random.default_rng(1)
    cmds, want, seen = [], [], set()
    for e in list(range(40)) + [(1 << 40) + 5]:
        obs = env.reset(e)
        cmds.append(f"reset {e}")
        want.append([env.a, env.h, env.fork, 0, 0, 0, 0] + [_bits(x) for x in obs])
        for _ in range(60):
            index = int(rng.integers(0, 5))  # 4: beyond every list
            before = (env.reward, env.progress)
            obs, r, term, _ = env.step(index)
            seen.add((index, env.last_name))
            cmds.append(f"step {index}")
            want.append([env.a, env.h, env.fork, int(r), env.progress - before[1], int(term),
                         env.steps] + [_bits(x) for x in obs])
            if term:
                break
    path = tmp_path / "cmds.txt"
    path.write_text("\n".join(cmds) + "\n")
    got = _run(exe, env.ta, env.tg, env.tt, seed, path)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert [int(x) for x in g[:7]] == w[:7], (i, cmds[i])
        assert g[7:] == w[7:], (i, cmds[i])
    # every row of the action rule was exercised
    assert {(2, R.OVERRIDE), (2, R.MATCH), (2, R.WAIT), (3, R.MATCH), (3, R.WAIT),
            (4, R.WAIT), (1, R.ADOPT), (0, R.WAIT)} <= seen
