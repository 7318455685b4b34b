"""Host side of policy evaluation over explicit MDPs (cpr_amd.mdp.reachable_states /
policy_evaluation / mdp_policy_from_table, the ctypes mirrors of cpr_mdp_pe*, the library's
argument checks): no GPU needed. The golden file holds the reference toolbox's own results
(tests/golden/make_mdp_pe_fixture.py)."""

import ctypes
import json
import pathlib
import subprocess

import numpy as np
import pytest

from cpr_amd import _lib as L
from cpr_amd import mdp

ROOT = pathlib.Path(__file__).resolve().parent.parent
CASES = json.loads((ROOT / "tests" / "golden" / "mdp_policy_eval.json").read_text())["cases"]


def _tab(alpha, gamma, mfl, horizon):
    _states, tab = mdp.compile_mdp(mdp.BitcoinSM(alpha, gamma, mfl))
    return mdp.ptmdp(tab, horizon)


def _case_id(c):
    return f"c{c['maximum_fork_length']}-h{c['horizon']}-a{c['alpha']}-g{c['gamma']}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_host_restatement_is_the_reference_bit_for_bit(case):
    assert len(CASES) == 12
    tab = _tab(case["alpha"], case["gamma"], case["maximum_fork_length"], case["horizon"])
    assert len(tab) == case["n_states"]
    start = [tuple(x) for x in case["start"]]
    assert [s for s, _ in start] == [0, 1]
    packed = mdp.pack(tab)
    for name, ev in case["evals"].items():
        policy = np.array(ev["policy"])
        assert sorted(mdp.reachable_states(tab, policy, start)) == ev["reachable"], name
        assert sorted(mdp.reachable_states(packed, policy)) == ev["reachable"], name
        for t in (tab, packed):
            pe = mdp.policy_evaluation(t, policy, theta=case["theta"], start=start,
                                       states=ev["states"], max_iter=ev["max_iter"])
            assert pe["pe_iter"] == ev["pe_iter"], name
            assert [float(x).hex() for x in pe["pe_reward"]] == ev["pe_reward"], name
            assert [float(x).hex() for x in pe["pe_progress"]] == ev["pe_progress"], name
    assert case["evals"]["vi_max5"]["pe_iter"] == 5


def stay(p=0.5, reward=1.0):
    """One state: stay with probability p, reward 1 (the rest of the probability is lost)."""
    return dict(dst=np.zeros((1, 1, 1), np.int64), prb=np.full((1, 1, 1), p),
                rew=np.full((1, 1, 1), reward), prg=np.ones((1, 1, 1)),
                used=np.ones((1, 1, 1), bool), valid=np.ones((1, 1), bool))


def test_the_stop_is_strict():
    # reward after sweep i: 1 - 2^-i, so the deltas are 1/2, 1/4, 1/8, ... exactly
    m = stay()
    for i in range(1, 8):
        pe = mdp.policy_evaluation(m, [0], theta=1e-300, max_iter=i, start=[(0, 1.0)])
        assert pe["pe_delta"] == 0.5 ** i and pe["pe_reward"][0] == 1.0 - 0.5 ** i
    # sweep 2 has delta == theta, which does not stop it
    pe = mdp.policy_evaluation(m, [0], theta=0.25, start=[(0, 1.0)])
    assert pe["pe_iter"] == 3 and pe["pe_delta"] == 0.125
    # with reward 2 the deltas are 1, .5, .25, ...: theta = .25 stops after sweep 4, not 3
    m = stay(reward=2.0)
    pe = mdp.policy_evaluation(m, [0], theta=0.25, start=[(0, 1.0)])
    assert pe["pe_iter"] == 4 and pe["pe_delta"] == 0.125
    assert mdp.value_iteration(m, stop_delta=0.25)["vi_iter"] == 3  # `<=` there
    # max_iter is asked after the delta; 0 stops after the first sweep, as in the reference
    assert mdp.policy_evaluation(m, [0], theta=0.25, max_iter=0)["pe_iter"] == 1
    assert mdp.policy_evaluation(m, [0], theta=0.25, max_iter=9)["pe_iter"] == 4


@pytest.mark.parametrize("mfl", [4, 6, 10])
def test_evaluating_the_optimum_gives_its_value(mfl):
    # the reference's library gave at most 4.3e-7 at cut-offs 4, 6, 10 and 20; 20 x that
    tab = _tab(0.3, 0.5, mfl, 100)
    vi = mdp.value_iteration(tab, stop_delta=1e-6)
    start = [(0, 0.3), (1, 0.7)]
    pe = mdp.policy_evaluation(tab, vi["vi_policy"], theta=1e-6, start=start)
    reach = sorted(mdp.reachable_states(tab, vi["vi_policy"], start))
    err = np.abs(pe["pe_reward"] - vi["vi_value"])[reach].max()
    print(f"cut-off {mfl}: {len(reach)} reachable states, max |pe_reward - vi_value| = {err:.3g}")
    assert err <= 1e-5
    out = np.setdiff1d(np.arange(len(tab)), reach)
    assert not pe["pe_reward"][out].any() and not pe["pe_progress"][out].any()


def test_a_table_round_trips_to_the_policy_it_was_made_from():
    mfl = 8
    model, states, vi = mdp.solve(0.4, 0.7, maximum_fork_length=mfl, horizon=50)
    tab = mdp.ptmdp(mdp.compile_mdp(model)[1], 50)
    reach = mdp.reachable_states(tab, vi["vi_policy"], [(0, 0.4), (1, 0.6)])
    assert len(reach) > 20
    fc16 = mdp._fc16_table_of(model, states, vi, mfl + 1)
    back = mdp.mdp_policy_from_table(model, states, fc16, "fc16")
    assert back.shape == vi["vi_policy"].shape and back[-1] == -1
    assert back.tolist() == vi["vi_policy"].tolist()  # every state, reached or not
    nak = mdp._policy_table_of(model, states, vi, mfl + 1)
    back = mdp.mdp_policy_from_table(model, states, nak, "nakamoto")
    # the Nakamoto table has no entry of its own for an active match (it shares ProofOfWork's)
    seen = [s for s in sorted(reach) if s < len(states) and states[s][2] != mdp.ACTIVE]
    assert len(seen) > 15
    assert back[seen].tolist() == vi["vi_policy"][seen].tolist()
    # honest play and SM1 are tables too; what the model does not offer becomes Override or Adopt
    honest = mdp.mdp_policy_from_table(model, states, mdp.fc16_honest_table(mfl + 1), "fc16")
    sm1 = mdp.mdp_policy_from_table(model, states, mdp.fc16_sm1_table(mfl + 1), "fc16")
    for sid, s in enumerate(states):
        a, h, fork = s
        acts = model.actions(s)
        assert acts[honest[sid]] == (mdp.OVERRIDE if a > h else mdp.ADOPT if h > a else
                                     mdp.WAIT if mdp.WAIT in acts else mdp.ADOPT)
        if model.truncated(s) and not (h == a - 1 and h >= 1) and not h > a:
            assert acts[sm1[sid]] == (mdp.OVERRIDE if a > h else mdp.ADOPT)
    assert acts_of(model, states, sm1, (1, 1, mdp.RELEVANT)) == mdp.MATCH
    assert acts_of(model, states, sm1, (2, 1, mdp.RELEVANT)) == mdp.OVERRIDE
    assert acts_of(model, states, sm1, (1, 1, mdp.IRRELEVANT)) == mdp.ADOPT  # no Match
    with pytest.raises(ValueError, match="kind"):
        mdp.mdp_policy_from_table(model, states, fc16, "bitcoin")
    with pytest.raises(ValueError, match="entries"):
        mdp.mdp_policy_from_table(model, states, fc16[:-1], "fc16")


def acts_of(model, states, policy, s):
    return model.actions(s)[policy[states.index(s)]]


def test_bad_policies_raise():
    tab = _tab(0.3, 0.5, 4, 10)
    n = len(tab)
    ok = np.array([0] * (n - 1) + [-1])
    mdp.policy_evaluation(tab, ok, theta=1e-3)
    for bad in (ok[:-1], ok.astype(float), np.where(np.arange(n) == 3, 9, ok),
                np.where(np.arange(n) == n - 1, 0, ok),  # the terminal state offers nothing
                np.where(np.arange(n) == 0, len(tab[0]), ok)):
        with pytest.raises(ValueError, match="policy"):
            mdp.policy_evaluation(tab, bad, theta=1e-3)
        with pytest.raises(ValueError, match="policy"):
            mdp.reachable_states(tab, bad)
        with pytest.raises(ValueError, match="policy"):
            mdp.policy_evaluation_device(tab, [bad], theta=1e-3)  # before any device call
    with pytest.raises(ValueError, match="start"):
        mdp.policy_evaluation(tab, ok, theta=1e-3, start=[(n, 1.0)])
    with pytest.raises(ValueError, match="states"):
        mdp.policy_evaluation(tab, ok, theta=1e-3, states="some")
    with pytest.raises(ValueError, match="theta"):
        mdp.policy_evaluation(tab, ok, theta=-1.0)
    with pytest.raises(ValueError, match="infinite"):
        mdp.policy_evaluation(tab, ok, theta=0.0)
    with pytest.raises(ValueError, match="pair"):
        mdp.policy_evaluation_device(tab, [ok], pairs=[(0, 1)], theta=1e-3)
    with pytest.raises(ValueError, match="max_iter"):
        mdp.policy_evaluation_device(tab, [ok], theta=1e-3, max_iter=0)


def test_the_library_checks_its_arguments_before_it_needs_a_device():
    # with ctx = NULL a call that passes every check ends at "ctx is NULL"; one that does not
    # names its own complaint, so each check is seen to come before anything touches a device
    lib = L.lib()
    m = mdp.pack(_tab(0.3, 0.5, 4, 10))
    a = {k: np.ascontiguousarray(m[k], dt) for k, dt in
         [("dst", np.int32), ("used", np.uint8), ("valid", np.uint8), ("rew", np.float64),
          ("prg", np.float64), ("prb", np.float64)]}
    S, A, T = a["dst"].shape
    E = 2
    out = [np.zeros((E, S)), np.zeros((E, S)), np.zeros(E, np.int64), np.zeros(E),
           np.zeros(E, np.int32)]
    res = L.MdpPeResultC(*(x.ctypes.data for x in out))
    opts = L.MdpPeOptsC()
    L.check(lib.cpr_mdp_pe_opts_default(ctypes.byref(opts)))
    assert (opts.theta, opts.discount, opts.max_iter, opts.path) == (1e-6, 1.0, 0, 0)
    assert lib.cpr_mdp_pe_opts_default(None) == L.CPR_E_INVALID_ARG

    def rc(sizes=(S, A, T, 1), point=(0, 0), policy=None, states=L.MDP_PE_REACHABLE,
           start=((0, 1), (0, 1)), n_start=2, e=E, **o):
        c = L.MdpC(*sizes, *(a[k].ctypes.data for k in ("dst", "used", "valid", "rew", "prg",
                                                         "prb")))
        pt = np.array(point, np.int32)
        pol = np.zeros((E, S), np.int32)
        pol[:, -1] = -1
        if policy is not None:
            pol[1, policy[0]] = policy[1]
        ss = np.array(start, np.int32)
        sp = np.full(ss.shape, 0.5)
        job = L.MdpPeC(e, pt.ctypes.data, pol.ctypes.data, states, n_start, ss.ctypes.data,
                       sp.ctypes.data)
        ops = L.MdpPeOptsC(o.get("theta", 1e-6), o.get("discount", 1.0), o.get("max_iter", 0),
                           o.get("path", 0))
        code = lib.cpr_mdp_policy_evaluation(None, ctypes.byref(c), ctypes.byref(job),
                                             ctypes.byref(ops), ctypes.byref(res))
        return code, lib.cpr_last_error().decode()

    assert rc() == (L.CPR_E_INVALID_ARG, "ctx is NULL")
    assert rc(states=L.MDP_PE_ALL, n_start=0) == (L.CPR_E_INVALID_ARG, "ctx is NULL")
    for kw, word in [(dict(sizes=(0, A, T, 1)), "at least 1"), (dict(point=(0, 1)), "point"),
                     (dict(point=(-1, 0)), "point"), (dict(policy=(3, A)), "policy"),
                     (dict(policy=(S - 1, 0)), "policy"),  # valid == 0: the terminal state
                     (dict(theta=-1e-9), "theta"), (dict(theta=float("nan")), "theta"),
                     (dict(theta=0.0), "infinite"), (dict(max_iter=-1), "max_iter"),
                     (dict(discount=0.0), "discount"), (dict(discount=1.5), "discount"),
                     (dict(start=((0, 1), (0, S))), "start state"),
                     (dict(start=((-1, 1), (0, 1))), "start state"),
                     (dict(n_start=0), "n_start"), (dict(states=2), "states"),
                     (dict(e=0), "E must"), (dict(path=3), "path")]:
        code, msg = rc(**kw)
        assert code == L.CPR_E_INVALID_ARG and word in msg, (kw, msg)
    assert rc(theta=0.0, max_iter=3) == (L.CPR_E_INVALID_ARG, "ctx is NULL")
    # the checks of cpr_mdp are value iteration's
    arr = a["dst"].copy()
    a["dst"][tuple(np.argwhere(a["used"])[3])] = S
    code, msg = rc()
    a["dst"] = arr
    assert code == L.CPR_E_INVALID_ARG and "dst" in msg


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cpr_hip.h"\n'
        'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(cpr_mdp_pe),'
        ' sizeof(cpr_mdp_pe_opts), sizeof(cpr_mdp_pe_result), offsetof(cpr_mdp_pe, states),'
        ' offsetof(cpr_mdp_pe, start_prob), offsetof(cpr_mdp_pe_opts, path),'
        ' offsetof(cpr_mdp_pe_result, path_used), offsetof(cpr_mdp_pe_result, kernel_ms));'
        'printf("%d %d %d %d\\n", CPR_MDP_PE_REACHABLE, CPR_MDP_PE_ALL, CPR_MDP_PE_MAX_ITER,'
        ' CPR_MDP_PE_NOT_CONVERGED);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(L.MdpPeC), ctypes.sizeof(L.MdpPeOptsC), ctypes.sizeof(L.MdpPeResultC),
            L.MdpPeC.states.offset, L.MdpPeC.start_prob.offset, L.MdpPeOptsC.path.offset,
            L.MdpPeResultC.path_used.offset, L.MdpPeResultC.kernel_ms.offset,
            L.MDP_PE_REACHABLE, L.MDP_PE_ALL, L.MDP_PE_MAX_ITER, L.MDP_PE_NOT_CONVERGED]
    assert got == want
