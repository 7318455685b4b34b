"""The generic release/consider env over Nakamoto (CPR_PROTO_GENERIC_NAKAMOTO), without a GPU.

(a) tests/generic_env_ref.py, the literal pure-Python env the GPU tests compare the device
    lanes with, equals two counter models that follow from the keyed draws alone (honest play
    and always Continue; derivations in that module's docstring).
(b) The reference's test_rust.py::test_actions on the action codec, in Python and in the
    host-compiled generic_lane.h.
(c) tests/native_generic/generic_host.cpp compiles cpr_amd/csrc/generic_lane.h for the host,
    plain and with AddressSanitizer + UBSan, as a stand-alone program: a fuzz of resets and
    integer actions equals the Python env line for line, also when the lane's memory starts
    out as garbage, and the fuzz reaches every event of the coverage list.
"""

import os
import pathlib
import struct
import subprocess

import numpy as np
import pytest

import generic_env_ref as R

ROOT = pathlib.Path(__file__).resolve().parent.parent
DIR = ROOT / "tests" / "native_generic"
EXES = ["generic_host", "generic_host_asan"]


# ------------------------------------------------ (a) the reference against the counter models

def _play(env, ep, policy):
    env.reset(ep)
    while True:
        f = env.fields()
        _, _, term, trunc = env.step(policy(f))
        if term or trunc:
            return dict(reward_attacker=env.era, reward_defender=env.erd, progress=env.eprog,
                        steps=env.steps, rewrite=env.last["rewrite"], terminated=term,
                        truncated=trunc)


@pytest.mark.parametrize("model", ["honest", "continue"])
def test_reference_equals_counter_model(model):
    seed, alpha, gamma, horizon, max_steps = 5, 0.4, 0.6, 8, 200
    env = R.GenericNakamotoRef(seed, alpha, gamma, horizon, max_steps)
    if model == "honest":
        counter, policy = R.honest_counter, lambda f: R.honest_action(f[3], f[4])
    else:
        counter, policy = R.continue_counter, lambda f: 0
    n_switch = n_term = 0
    for e in range(500):
        got = _play(env, e, policy)
        want = counter(seed, e, alpha, gamma, horizon, max_steps)
        assert got == want, (e, got, want)
        n_term += got["terminated"]
        n_switch += got["rewrite"] > 0
    assert n_term > 400
    if model == "continue":  # both outcomes of shutdown were seen
        assert 0 < n_switch < n_term
        assert {("shutdown", True, True), ("shutdown", False, True)} <= env.events


# ------------------------------------------------ (b) test_rust.py::test_actions

def _bits32(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _host_codec(exe, floats):
    subprocess.run(["make", "-s", "-C", str(DIR)], check=True)
    p = subprocess.run([str(DIR / "build" / exe), "codec"], capture_output=True, text=True,
                       input="".join(_bits32(x) + "\n" for x in floats), timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split("\n")
    table = [ln.split() for ln in lines[:513]]
    return table, [ln for ln in lines[513:] if ln]


PROBES = [0.0, 0.1, -0.1, 1.0, -1.0, 1.5, -1.5, float("nan")]


def _check_actions(encode, decode):
    # continue = 0, release < 0, consider > 0
    assert encode(0) == 0.0
    seq = [encode(-(i + 1)) for i in range(255, -1, -1)] + [encode(i + 1) for i in range(256)]
    assert all(x < 0 for x in seq[:256]) and all(x > 0 for x in seq[256:])
    # strictly monotonic over Release(255) ... Release(0), Consider(0) ... Consider(255)
    assert all(a < b for a, b in zip(seq, seq[1:]))
    # round trip for all 512 (and Continue)
    for a in range(-256, 257):
        assert decode(encode(a)) == a, a
    for x in (0.0, 0.1, -0.1):
        assert decode(x) == 0
    assert decode(1.0) == 256 and decode(-1.0) == -256  # index 255
    for x in (1.5, -1.5, float("nan")):
        with pytest.raises(ValueError):
            decode(x)


def test_actions_python():
    from cpr_amd import envs

    _check_actions(R.encode_action, R.decode_action)
    _check_actions(envs.generic_encode_action, envs.generic_decode_action)  # the public codec
    floats = np.random.default_rng(0).uniform(-1, 1, 5000).astype(np.float32)
    for x in floats:
        assert envs.generic_decode_action(x) == R.decode_action(x), x


@pytest.mark.parametrize("exe", EXES)
def test_actions_host(exe):
    table, probes = _host_codec(exe, PROBES)
    enc = {int(a): struct.unpack("<f", struct.pack("<I", int(b, 16)))[0] for a, b, _ in table}
    dec = {_bits32(enc[int(a)]): int(d) for a, _, d in table}
    dec.update({_bits32(x): (None if p == "raises" else int(p)) for x, p in zip(PROBES, probes)})

    def decode(x):
        d = dec[_bits32(x)]
        if d is None:
            raise ValueError(x)
        return d

    _check_actions(lambda a: enc[a], decode)
    # bit for bit the Python codec
    for a in range(-256, 257):
        assert _bits32(enc[a]) == _bits32(R.encode_action(a)), a
    # ... and the same decoding of arbitrary floats, half-way cases of the rounding included
    floats = list(np.random.default_rng(0).uniform(-1, 1, 2000).astype(np.float32))
    floats += [np.float32(k + 0.5) / (np.float32(k + 1.5)) for k in range(0, 300, 7)]
    floats += [-x for x in floats[-43:]]
    _, got = _host_codec(exe, floats)
    assert [int(g) for g in got] == [R.decode_action(x) for x in floats]


# ------------------------------------------------ (c) generic_lane.h on the host

ACTIONS = [0, 1, -1, 2, -2, 3, -3, 256, -256]
FUZZ = dict(seed=1, alpha=0.4, gamma=0.6, horizon=6, max_steps=48, rng=1)
# (kind, True) is the release list, (kind, False) the consider list; ("shutdown", fast, wire).
# A step with negative attacker reward is not in the set: over Nakamoto no sequence of actions
# reaches one (DESIGN.md §4.10a proves it), and test_no_step_pays_the_attacker_less_than_zero
# keeps watch.
COVERAGE = {"release>=2", "consider>=2", ("clamped", True), ("clamped", False),
            ("empty", True), ("empty", False), "rewrite",
            ("shutdown", True, True), ("shutdown", False, True), "truncated"}


def fuzz_script():
    """(commands, expected lines, events reached) of the fuzz: 60 episodes plus one episode id
    above 2^40, actions uniform over ACTIONS."""
    c = FUZZ
    env = R.GenericNakamotoRef(c["seed"], c["alpha"], c["gamma"], c["horizon"], c["max_steps"])
    rng = np.random.default_rng(c["rng"])
    cmds, want = [], []
    for e in list(range(60)) + [(1 << 40) + 5]:
        obs = env.reset(e)
        cmds.append(f"reset {e}")
        want.append(env.fields() + [0, 0, 0, 0, 0] + [_bits32(x) for x in obs])
        while True:
            a = ACTIONS[int(rng.integers(0, len(ACTIONS)))]
            obs, r, term, trunc = env.step(a)
            cmds.append(f"step {a}")
            want.append(env.fields() + [int(r), env.last["progress"], int(term), int(trunc),
                                        env.status] + [_bits32(x) for x in obs])
            if term or trunc:
                break
    return cmds, want, env


def test_fuzz_reaches_every_event():
    _, _, env = fuzz_script()
    assert COVERAGE <= env.events, COVERAGE - env.events


def test_no_step_pays_the_attacker_less_than_zero():
    _, _, env = fuzz_script()
    assert "negative" not in env.events


@pytest.mark.parametrize("garbage", [None, "3"])
@pytest.mark.parametrize("exe", EXES)
def test_lane_header_equals_reference_line_for_line(tmp_path, exe, garbage):
    cmds, want, env = fuzz_script()
    path = tmp_path / "cmds.txt"
    path.write_text("\n".join(cmds) + "\n")
    subprocess.run(["make", "-s", "-C", str(DIR)], check=True)
    envv = dict(os.environ)
    envv.pop("GARBAGE", None)
    if garbage:
        envv["GARBAGE"] = garbage
    c = FUZZ
    p = subprocess.run([str(DIR / "build" / exe), str(env.ta), str(env.tg), str(env.tt),
                        str(c["max_steps"]), str(c["seed"]), str(path)], capture_output=True,
                       text=True, timeout=300, env=envv)
    assert p.returncode == 0, p.stderr[-2000:]
    got = [ln.split() for ln in p.stdout.splitlines()]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert [int(x) for x in g[:12]] == w[:12], (i, cmds[i])
        assert g[12:] == w[12:], (i, cmds[i])
