"""Policy evaluation on the device (cpr_mdp_policy_evaluation, kernels_mdp.hip)
— needs an MI355X. Every result is compared with cpr_amd.mdp.policy_evaluation on the same
packed MDP and must equal it in reward and progress bit for bit, in iter and in delta, on the
resident path (one workgroup per evaluation, vectors in LDS) and on the global path (one launch
per sweep)."""

import numpy as np
import pytest

from cpr_amd import _lib as L
from cpr_amd import device, mdp

pytestmark = pytest.mark.gpu

PATHS = ["resident", "global"]
POINTS = [(0.3, 0.5), (0.1, 0.0), (0.45, 0.9)]


@pytest.fixture(scope="module")
def ctx():
    return device.default_context()


def ssz(alpha, gamma, mfl, horizon):
    _states, tab = mdp.compile_mdp(mdp.BitcoinSM(alpha, gamma, mfl))
    return mdp.pack(mdp.ptmdp(tab, horizon))


def start_of(alpha):
    return [(0, alpha), (1, 1 - alpha)]


def same(dev, host, path=None):
    assert dev["pe_iter"] == host["pe_iter"]
    assert dev["pe_delta"] == host["pe_delta"]
    assert dev["pe_reward"].tobytes() == host["pe_reward"].tobytes()
    assert dev["pe_progress"].tobytes() == host["pe_progress"].tobytes()
    if path is not None:
        assert dev["pe_path"] == path


_cache = {}


def once(key, make):
    """A host result computed once and shared by the tests and paths that need it."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def first_action(m):
    """Slot 0 wherever a state offers an action (pack puts valid actions first), else -1."""
    return np.where(np.asarray(m["valid"])[:, 0], 0, -1)


def small():
    """Cut-off 4, horizon 10 at three points; the optimum of each, and the first-action
    policy; the host evaluation of every policy at every point."""
    def make():
        ms = [ssz(a, g, 4, 10) for a, g in POINTS]
        assert ms[0]["dst"].shape[0] == 40  # 39 states and the terminal one
        pols = [mdp.value_iteration(m, stop_delta=1e-6)["vi_policy"] for m in ms[:2]]
        pols.append(first_action(ms[0]))
        starts = [start_of(a) for a, _g in POINTS]
        hosts = {(q, p): mdp.policy_evaluation(ms[p], pols[q], theta=1e-6, start=starts[p])
                 for q in range(3) for p in range(3)}
        return ms, pols, starts, hosts
    return once("small", make)


@pytest.mark.parametrize("path", PATHS)
def test_one_evaluation(ctx, path):
    ms, pols, starts, hosts = small()
    dev = mdp.policy_evaluation_device(ms[0], [pols[0]], theta=1e-6, start=starts[0], path=path,
                                       ctx=ctx)
    assert len(dev) == 1 and hosts[0, 0]["pe_iter"] == 120
    same(dev[0], hosts[0, 0], path)
    assert dev[0]["pe_status"] == L.MDP_PE_CONVERGED


@pytest.mark.parametrize("path", PATHS)
def test_cross_product_and_independent_stops(ctx, path):
    ms, pols, starts, hosts = small()
    devs = mdp.policy_evaluation_device(ms, pols, theta=1e-6, start=starts, path=path, ctx=ctx)
    assert len(devs) == 9
    # policy-major; the evaluations of one call stop at sweeps of their own
    iters = [hosts[q, p]["pe_iter"] for q in range(3) for p in range(3)]
    assert len(set(iters)) >= 6 and max(iters) > 1.5 * min(iters)
    for e, dev in enumerate(devs):
        same(dev, hosts[divmod(e, 3)], path)
        assert dev["pe_status"] == L.MDP_PE_CONVERGED


@pytest.mark.parametrize("path", PATHS)
def test_ragged_pairs(ctx, path):
    ms, pols, starts, hosts = small()
    pairs = [(2, 2), (0, 0), (1, 2), (2, 2), (0, 2)]  # point 2 four times, point 1 never
    devs = mdp.policy_evaluation_device(ms, pols, pairs, theta=1e-6, start=starts, path=path,
                                        ctx=ctx)
    for dev, pair in zip(devs, pairs):
        same(dev, hosts[pair], path)


@pytest.mark.parametrize("path", PATHS)
def test_more_evaluations_than_compute_units(ctx, path):
    ms, pols, starts, hosts = small()
    pairs = [((7 * e) % 3, (5 * e + e // 9) % 3) for e in range(300)]
    assert len(set(pairs)) == 9
    devs = mdp.policy_evaluation_device(ms, pols, pairs, theta=1e-6, start=starts, path=path,
                                        ctx=ctx)
    assert len(devs) == 300
    for dev, pair in zip(devs, pairs):
        same(dev, hosts[pair], path)


@pytest.mark.parametrize("path", PATHS)
def test_more_sweeps_than_one_bounded_launch(ctx, path):
    # 1,544 sweeps: two bounded launches of the resident kernel (1,024 sweeps each) with the
    # vectors carried through global memory, 25 status reads of the global path
    m = once("h100", lambda: ssz(0.3, 0.5, 4, 100))
    pol = once("h100-pol", lambda: mdp.value_iteration(m, stop_delta=1e-6)["vi_policy"])
    host = once("h100-pe", lambda: mdp.policy_evaluation(m, pol, theta=1e-6,
                                                         start=start_of(0.3)))
    assert host["pe_iter"] == 1544
    dev = mdp.policy_evaluation_device(m, [pol], theta=1e-6, start=start_of(0.3), path=path,
                                       ctx=ctx)[0]
    same(dev, host, path)
    reach = mdp.reachable_states(m, pol, start_of(0.3))
    assert len(reach) == 14
    out = np.setdiff1d(np.arange(40), sorted(reach))
    assert not dev["pe_reward"][out].any() and not dev["pe_progress"][out].any()
    assert dev["pe_reward"][sorted(reach)[:2]].all()


def random_mdp(S, A, T, seed):
    rng = np.random.default_rng(seed)
    used = rng.random((S, A, T)) < 0.8
    valid = rng.random((S, A)) < 0.9
    prb = rng.random((S, A, T))
    prb /= np.maximum((prb * used).sum(axis=2, keepdims=True), 1e-9)
    return dict(dst=rng.integers(0, S, (S, A, T)), prb=prb, rew=rng.random((S, A, T)) * 4 - 1,
                prg=rng.random((S, A, T)), used=used, valid=valid)


def random_policy(m, seed):
    """A valid slot per state where there is one (not always the first), else -1."""
    rng = np.random.default_rng(seed)
    valid = np.asarray(m["valid"])
    pick = np.argmax(valid * rng.random(valid.shape), axis=1)
    return np.where(valid.any(axis=1), pick, -1)


# Resident instantiations: 1, 2, 4 and 10 states per thread (state counts as
# tests/test_gpu_mdp_vi.py takes them), with the slots kept in registers (T <= 4 and at most 2
# states per thread) and read again in every sweep (T = 5, or more states per thread).
def _many_states(name):
    if name == "ssz-cutoff-40":  # 3,982 states: 4 per thread
        m = ssz(0.33, 0.5, 40, 100)
        return m, first_action(m), dict(theta=1e-6, max_iter=12, start=start_of(0.33))
    S, T = {"random-700": (700, 4), "random-700-t5": (700, 5), "random-1500": (1500, 4),
            "random-1500-t5": (1500, 5), "random-9999": (9999, 4)}[name]
    m = random_mdp(S, 3, T, seed=S + T)
    return m, random_policy(m, S), dict(theta=1e-6, max_iter=6, discount=0.95,
                                        start=[(3, 0.5), (S - 1, 0.5)])


@pytest.mark.parametrize("name,per_thread,keeps", [
    ("random-700", 1, True), ("random-700-t5", 1, False), ("random-1500", 2, True),
    ("random-1500-t5", 2, False), ("ssz-cutoff-40", 4, False), ("random-9999", 10, False)])
def test_resident_states_per_thread(ctx, name, per_thread, keeps):
    m, pol, kw = _many_states(name)
    S, _A, T = m["dst"].shape
    threads = min(1024, -(-S // 64) * 64)
    assert min(p for p in (1, 2, 4, 10) if p * threads >= S) == per_thread
    assert S % 64 != 0 and (T <= 4 and per_thread <= 2) == keeps
    host = mdp.policy_evaluation(m, pol, **kw)
    assert host["pe_iter"] == kw["max_iter"] and host["pe_delta"] > 0
    assert len(mdp.reachable_states(m, pol, kw["start"])) > S // 3
    # a second point and a second policy in the same launch
    other = dict(m, prb=np.where(m["used"], m["prb"] * 0.75, m["prb"]))
    pol2 = np.where(np.arange(S) % 7 == 3, -1, pol)
    host2 = mdp.policy_evaluation(other, pol2, **kw)
    for path in PATHS:
        devs = mdp.policy_evaluation_device([m, other], [pol, pol2], [(0, 0), (1, 1)], path=path,
                                            ctx=ctx, **kw)
        same(devs[0], host, path)
        same(devs[1], host2, path)
        assert devs[0]["pe_status"] == L.MDP_PE_MAX_ITER


def test_reread_hook_gives_the_same(ctx, monkeypatch):
    # CPR_MDP_PE_REREAD=1 (the measurement hook) takes the re-reading kernels where the
    # register-keeping ones would run
    monkeypatch.setenv("CPR_MDP_PE_REREAD", "1")
    ms, pols, starts, hosts = small()
    devs = mdp.policy_evaluation_device(ms, pols, theta=1e-6, start=starts, path="resident",
                                        ctx=ctx)
    for e, dev in enumerate(devs):
        same(dev, hosts[divmod(e, 3)], "resident")


def test_auto_path_and_the_guard(ctx):
    ms, pols, starts, hosts = small()
    dev = mdp.policy_evaluation_device(ms[0], [pols[0]], theta=1e-6, start=starts[0], ctx=ctx)[0]
    assert dev["pe_path"] == "resident"
    # 10,104 states are the most whose reward and progress fit a workgroup's LDS (16 bytes a
    # state and 128 bytes of reduction words in 160 KiB less 2 KiB); one more does not
    S = 10_105
    m = random_mdp(S, 2, 3, seed=0x504531)
    pol = random_policy(m, 1)
    kw = dict(theta=1e-6, max_iter=4, start=[(0, 1.0)])
    host = mdp.policy_evaluation(m, pol, **kw)
    same(mdp.policy_evaluation_device(m, [pol], ctx=ctx, **kw)[0], host, "global")
    with pytest.raises(L.CprError) as e:
        mdp.policy_evaluation_device(m, [pol], path="resident", ctx=ctx, **kw)
    assert e.value.code == L.CPR_E_CAPACITY


@pytest.mark.parametrize("path", PATHS)
def test_leaves_all_states_and_unreachable_states(ctx, path):
    ms, pols, starts, _hosts = small()
    m, pol, start = ms[2], pols[2], starts[2]
    # -1 at reachable non-terminal states: they are leaves and stay 0, and so does what only
    # they led to
    full = mdp.reachable_states(m, pol, start)
    leaves = [s for s in sorted(full) if s > 1 and s != 39][2::7][:3]
    cut = np.where(np.isin(np.arange(40), leaves), -1, pol)
    reach = mdp.reachable_states(m, cut, start)
    assert len(leaves) == 3 and set(leaves) <= reach <= full and len(full) == 34
    host = once("cut", lambda: mdp.policy_evaluation(m, cut, theta=1e-6, start=start))
    dev = mdp.policy_evaluation_device(m, [cut], theta=1e-6, start=start, path=path, ctx=ctx)[0]
    same(dev, host, path)
    out = sorted(set(range(40)) - reach) + leaves
    assert not dev["pe_reward"][out].any() and not dev["pe_progress"][out].any()
    assert dev["pe_reward"][0] > 0
    # every state: the states nothing reaches are evaluated too
    opt = pols[0]
    some = mdp.reachable_states(ms[0], opt, starts[0])
    host_all = once("all", lambda: mdp.policy_evaluation(ms[0], opt, theta=1e-6, states="all"))
    dev = mdp.policy_evaluation_device(ms[0], [opt], theta=1e-6, states="all", path=path,
                                       ctx=ctx)[0]
    same(dev, host_all, path)
    assert np.count_nonzero(dev["pe_reward"]) > len(some) == 4
    # a start state with probability 0 does not count
    only1 = [(0, 0.0), (1, 1.0)]
    host1 = once("only1", lambda: mdp.policy_evaluation(m, cut, theta=1e-6, start=only1))
    same(mdp.policy_evaluation_device(m, [cut], theta=1e-6, start=only1, path=path, ctx=ctx)[0],
         host1, path)


def stay(reward):
    return dict(dst=np.zeros((1, 1, 1), np.int64), prb=np.full((1, 1, 1), 0.5),
                rew=np.full((1, 1, 1), reward), prg=np.ones((1, 1, 1)),
                used=np.ones((1, 1, 1), bool), valid=np.ones((1, 1), bool))


@pytest.mark.parametrize("path", PATHS)
def test_the_stop_is_strict(ctx, path):
    # stay with probability .5: reward 1 has deltas .5, .25, .125, reward 2 has 1, .5, .25, ...
    # exactly; a delta equal to theta does not stop the evaluation
    for reward, sweeps in [(1.0, 3), (2.0, 4)]:
        dev = mdp.policy_evaluation_device(stay(reward), [[0]], theta=0.25, start=[(0, 1.0)],
                                           path=path, ctx=ctx)[0]
        assert dev["pe_iter"] == sweeps and dev["pe_delta"] == 0.125
        assert dev["pe_reward"][0] == reward * (1 - 0.5 ** sweeps)
        same(dev, mdp.policy_evaluation(stay(reward), [0], theta=0.25, start=[(0, 1.0)]), path)
        assert dev["pe_status"] == L.MDP_PE_CONVERGED


@pytest.mark.parametrize("path", PATHS)
def test_max_iter_status(ctx, path):
    ms, pols, starts, hosts = small()
    host = once("max7", lambda: mdp.policy_evaluation(ms[0], pols[2], theta=1e-6, max_iter=7,
                                                      start=starts[0]))
    assert host["pe_iter"] == 7
    devs = mdp.policy_evaluation_device(ms[:2], [pols[2]], theta=1e-6, max_iter=7,
                                        start=starts[:2], path=path, ctx=ctx)
    same(devs[0], host, path)
    assert [d["pe_status"] for d in devs] == [L.MDP_PE_MAX_ITER] * 2
    # the second evaluation converges (110 sweeps) before max_iter = 115 stops the first (152)
    assert hosts[1, 1]["pe_iter"] == 110 and hosts[2, 0]["pe_iter"] == 152
    devs = mdp.policy_evaluation_device(ms[:2], pols, [(2, 0), (1, 1)], theta=1e-6, max_iter=115,
                                        start=starts[:2], path=path, ctx=ctx)
    assert [d["pe_status"] for d in devs] == [L.MDP_PE_MAX_ITER, L.MDP_PE_CONVERGED]
    assert [d["pe_iter"] for d in devs] == [115, 110]
    same(devs[1], hosts[1, 1], path)
    # theta = 0 never converges: max_iter ends it
    dev = mdp.policy_evaluation_device(stay(1.0), [[0]], theta=0.0, max_iter=2000, path=path,
                                       ctx=ctx)[0]
    assert dev["pe_iter"] == 2000 and dev["pe_delta"] == 0.0 and dev["pe_reward"][0] == 1.0
    assert dev["pe_status"] == L.MDP_PE_MAX_ITER


@pytest.mark.parametrize("path", PATHS)
def test_the_cap_ends_an_evaluation_that_cannot_converge(ctx, path, monkeypatch):
    # a two-state cycle with reward 1 and discount 1 grows for ever; the library's cap of 2^20
    # sweeps is lowered for this call (CPR_MDP_PE_SWEEP_CAP): three resident launches
    monkeypatch.setenv("CPR_MDP_PE_SWEEP_CAP", "2500")
    cycle = dict(dst=np.array([[[1]], [[0]]]), prb=np.ones((2, 1, 1)), rew=np.ones((2, 1, 1)),
                 prg=np.ones((2, 1, 1)), used=np.ones((2, 1, 1), bool),
                 valid=np.ones((2, 1), bool))
    # a second evaluation, of the policy without any action, converges at once
    devs = mdp.policy_evaluation_device(cycle, [[0, 0], [-1, -1]], theta=1e-6, path=path,
                                        ctx=ctx)
    assert devs[0]["pe_status"] == L.MDP_PE_NOT_CONVERGED
    assert devs[0]["pe_iter"] == 2500 and devs[0]["pe_delta"] == 1.0
    assert devs[0]["pe_reward"].tolist() == [2500.0, 2500.0]
    assert devs[1]["pe_status"] == L.MDP_PE_CONVERGED and devs[1]["pe_iter"] == 1
    assert devs[1]["pe_reward"].tolist() == [0.0, 0.0]
    same(devs[0], mdp.policy_evaluation(cycle, [0, 0], theta=1e-6, max_iter=2500))


def test_revenue_matrix(ctx):
    alphas, gammas = (0.2, 0.33, 0.45), (0.0, 0.9)
    r = mdp.revenue_matrix(alphas, gammas, maximum_fork_length=6, horizon=100, ctx=ctx)
    rev, vi = r["revenue"], r["vi_revenue"]
    assert rev.shape == (8, 6) and len(r["policies"]) == 8 and r["policies"][6:] == ["honest",
                                                                                    "sm1"]
    assert r["points"] == [(a, g) for a in alphas for g in gammas]
    assert (r["pe_status"] == L.MDP_PE_CONVERGED).all()
    for p in range(6):
        print(f"point {r['points'][p]}: vi {vi[p]:.9f} own {rev[p, p]:.9f} "
              f"rel {abs(rev[p, p] - vi[p]) / vi[p]:.3g} "
              f"best other {np.delete(rev[:, p], p).max():.9f}")
    # 1e-5: the bound of tests/test_mdp_pe_host.py on |pe_reward - vi_value| (20 x the 4.3e-7
    # that the reference's library gave), here relative to the revenue
    for p in range(6):
        assert abs(rev[p, p] - vi[p]) <= 1e-5 * vi[p]
        assert (rev[:, p] <= rev[p, p] + 1e-5 * vi[p]).all()
    # honest play earns alpha, whatever gamma is
    assert np.allclose(rev[6], [a for a in alphas for _g in gammas], rtol=1e-5)
    # the host evaluation of one entry is the device's
    model = mdp.BitcoinSM(0.33, 0.9, 6)
    states, tab = mdp.compile_mdp(model)
    sm1 = mdp.mdp_policy_from_table(model, states, mdp.fc16_sm1_table(7), "fc16")
    pe = mdp.policy_evaluation(mdp.ptmdp(tab, 100), sm1, theta=1e-6, start=start_of(0.33))
    want = (0.33 * pe["pe_reward"][0] + 0.67 * pe["pe_reward"][1]) / \
        (0.33 * pe["pe_progress"][0] + 0.67 * pe["pe_progress"][1])
    assert rev[7, 3] == want and r["pe_iter"][7, 3] == pe["pe_iter"]


def test_revenue_matrix_labels_every_given_policy(ctx):
    # a given policy keeps its label and its row, also one named like a built-in row
    given = {"honest": (mdp.fc16_honest_table(5), "fc16"), "mine": (mdp.fc16_sm1_table(5), "fc16")}
    r = mdp.revenue_matrix([0.4], [0.5], given, maximum_fork_length=4, horizon=10, ctx=ctx)
    assert r["policies"] == ["optimum(0.4,0.5)", "honest", "sm1", "honest", "mine"]
    assert r["revenue"].shape == (5, 1)
    assert r["revenue"][3, 0] == r["revenue"][1, 0] and r["revenue"][4, 0] == r["revenue"][2, 0]


def test_value_iteration_is_untouched_by_an_evaluation(ctx):
    m = ssz(0.33, 0.5, 4, 10)
    ms, pols, starts, _hosts = small()
    for path in PATHS:
        before = mdp.value_iteration_device(m, stop_delta=1e-6, path=path, ctx=ctx)
        for pe_path in PATHS:
            mdp.policy_evaluation_device(ms, pols, theta=1e-6, start=starts, path=pe_path, ctx=ctx)
        after = mdp.value_iteration_device(m, stop_delta=1e-6, path=path, ctx=ctx)
        assert before["vi_iter"] == after["vi_iter"] == 147
        for k in ("vi_value", "vi_progress", "vi_policy"):
            assert before[k].tobytes() == after[k].tobytes()
        assert before["vi_delta"] == after["vi_delta"]
