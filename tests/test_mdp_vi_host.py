"""Host side of the device value iteration (cpr_amd.mdp.pack / value_iteration_device /
solve(device=False), the ctypes mirrors of cpr_mdp*): no GPU needed."""

import ctypes
import json
import pathlib
import subprocess

import numpy as np
import pytest

from cpr_amd import _lib as L
from cpr_amd import mdp

ROOT = pathlib.Path(__file__).resolve().parent.parent
CASES = json.loads((ROOT / "tests" / "golden" / "mdp_fc16_vi.json").read_text())["cases"]


def _tab(alpha, gamma, mfl, horizon):
    _states, tab = mdp.compile_mdp(mdp.BitcoinSM(alpha, gamma, mfl))
    return mdp.ptmdp(tab, horizon)


def test_pack_round_trips_the_tables():
    tab = _tab(0.33, 0.5, 6, 20)
    m = mdp.pack(tab)
    S, A, T = m["dst"].shape
    assert S == len(tab) and m["valid"].shape == (S, A) and not m["valid"][-1].any()
    back = [[[(int(m["dst"][s, i, j]), m["prb"][s, i, j], m["rew"][s, i, j], m["prg"][s, i, j])
              for j in range(T) if m["used"][s, i, j]]
             for i in range(A) if m["valid"][s, i]] for s in range(S)]
    assert back == [[[(d, float(p), float(r), float(g)) for d, p, r, g in lst] for lst in acts]
                    for acts in tab]
    # used slots are a prefix of every action's slots, valid actions a prefix of every state's
    assert (np.diff(m["used"].astype(int), axis=2) <= 0).all()
    assert (np.diff(m["valid"].astype(int), axis=1) <= 0).all()
    assert not m["prb"][~m["used"]].any() and not m["dst"][~m["used"]].any()


@pytest.mark.parametrize("case", CASES[:2], ids=lambda c: f"a{c['alpha']:.3f}-g{c['gamma']}")
def test_value_iteration_over_a_packed_mdp_is_the_golden(case):
    m = mdp.pack(_tab(case["alpha"], case["gamma"], case["maximum_fork_length"],
                      case["horizon"]))
    # garbage in the padding slots changes nothing
    m["dst"][~m["used"]] = 10 ** 9
    m["prb"][~m["used"]] = 1e300
    m["rew"][~m["used"]] = -7.0
    vi = mdp.value_iteration(m, stop_delta=case["stop_delta"])
    assert vi["vi_iter"] == case["vi_iter"]
    assert vi["vi_policy"].tolist() == case["vi_policy"]
    assert vi["vi_value"].tolist() == case["vi_value"]  # bit for bit


def test_topology_mismatch_raises_before_any_device_call():
    a = mdp.pack(_tab(0.33, 0.5, 4, 10))
    with pytest.raises(ValueError, match="topology"):
        mdp.value_iteration_device([a, mdp.pack(_tab(0.33, 0.5, 5, 10))], stop_delta=1e-6)
    b = {k: v.copy() for k, v in a.items()}
    b["rew"][tuple(np.argwhere(b["used"])[0])] += 1.0
    with pytest.raises(ValueError, match="topology"):
        mdp.value_iteration_device([a, b], stop_delta=1e-6)
    c = {k: v.copy() for k, v in a.items()}
    c["dst"][tuple(np.argwhere(c["used"])[5])] = 0
    with pytest.raises(ValueError, match="topology"):
        mdp.value_iteration_device([a, c], stop_delta=1e-6)
    with pytest.raises(ValueError, match="no MDP"):
        mdp.value_iteration_device([], stop_delta=1e-6)
    with pytest.raises(ValueError, match="packed MDP without"):
        mdp.value_iteration_device({"dst": a["dst"]}, stop_delta=1e-6)


def test_one_mdp_is_told_from_a_list_by_its_nesting():
    tab = _tab(0.33, 0.5, 4, 10)
    as_lists = json.loads(json.dumps(tab))  # transitions as lists, as a JSON file gives them
    late = [[], []] + as_lists  # the first states offer no action
    for one in (tab, as_lists, late, tuple(tab), mdp.pack(tab)):
        assert mdp._is_single(one)
    for many in ([tab, tab], [as_lists], (tab,), [mdp.pack(tab)], [mdp.pack(tab), tab], []):
        assert not mdp._is_single(many)
    for bad in ([[], []], [[[]]], 7, [[[[[[1.0]]]]]]):
        with pytest.raises(ValueError, match="expected a tab"):
            mdp._is_single(bad)


def test_solve_without_device_is_unchanged():
    case = CASES[0]
    kw = dict(maximum_fork_length=case["maximum_fork_length"], horizon=case["horizon"],
              stop_delta=case["stop_delta"])
    for extra in ({}, {"device": False}):
        model, states, vi = mdp.solve(case["alpha"], case["gamma"], **kw, **extra)
        assert [list(s) for s in states] == case["states"]
        assert sorted(vi) == ["vi_delta", "vi_iter", "vi_policy", "vi_progress", "vi_value"]
        assert vi["vi_iter"] == case["vi_iter"]
        assert vi["vi_value"].tolist() == case["vi_value"]
    t = mdp.policy_table(case["alpha"], case["gamma"], **kw)
    assert t.tolist() == mdp.policy_table(case["alpha"], case["gamma"], device=False, **kw).tolist()
    f = mdp.fc16_table(case["alpha"], case["gamma"], **kw)
    assert f.size == 3 * (case["maximum_fork_length"] + 1) ** 2


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cpr_hip.h"\n'
        'int main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(cpr_mdp),'
        ' sizeof(cpr_mdp_vi_opts), sizeof(cpr_mdp_vi_result), offsetof(cpr_mdp, dst),'
        ' offsetof(cpr_mdp_vi_opts, path), offsetof(cpr_mdp_vi_result, path_used),'
        ' offsetof(cpr_mdp_vi_result, kernel_ms));'
        'printf("%d %d %d\\n", CPR_MDP_VI_RESIDENT, CPR_MDP_VI_GLOBAL,'
        ' CPR_MDP_VI_NOT_CONVERGED);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(L.MdpC), ctypes.sizeof(L.MdpViOptsC), ctypes.sizeof(L.MdpViResultC),
            L.MdpC.dst.offset, L.MdpViOptsC.path.offset, L.MdpViResultC.path_used.offset,
            L.MdpViResultC.kernel_ms.offset, L.MDP_VI_RESIDENT, L.MDP_VI_GLOBAL,
            L.MDP_VI_NOT_CONVERGED]
    assert got == want
