"""Per-episode alpha schedules and cpr-v0 rewards on the device lanes (cpr_lane_env_set) —
needs an MI355X.

All runs: 32 lanes, the table {0.125, 0.25, 0.375, 0.5}, gamma 0.5. The alpha an episode is
expected to run at comes from the oracle's keyed stream (lane_env_ref.alpha_index), never
from the library; every oracle env is made with its own episode's alpha.

1. the step path, all four protocols: reset / step / masked reset against one oracle gym env
   per episode, every output bit for bit, lane_alpha() at every step;
2. the network rollout (Nakamoto with the exact-engine hand-over, B_k): an integer network
   fed with the lane's alpha against oracle envs driven by forward_f64, bit for bit;
3. every reward scheme x shape of that rollout against the oracle run passed through
   cpr_amd/wrappers.py and ppo.py's cut, bit for bit;
4. consistency, all four protocols: chunked calls, a host-driven replay through step, and a
   one-entry table against a batch without a lane env;
5. refusals.
"""

import ctypes
import functools

import numpy as np
import pytest

import lane_env_ref as R
import oracle_py as O
from cpr_amd import _lib as L
from cpr_amd import device

pytestmark = pytest.mark.gpu

N = 32
TABLE = (0.125, 0.25, 0.375, 0.5)
GAMMA = 0.5
CFG_ALPHA = 0.33  # the batch's own alpha: no episode may run at it once a table is set
PROTO = {
    "nakamoto": dict(protocol=L.PROTO_NAKAMOTO),
    "bk": dict(protocol=L.PROTO_BK, k=2),
    "ethereum": dict(protocol=L.PROTO_ETHEREUM, reward_scheme=L.REWARD_DISCOUNT),
    "tailstorm": dict(protocol=L.PROTO_TAILSTORM, k=2, reward_scheme=L.REWARD_DISCOUNT,
                      subblock_selection=L.SELECT_HEURISTIC),
}
SHAPE = {"nakamoto": (4, 4), "bk": (8, 8), "ethereum": (10, 24), "tailstorm": (10, 8)}
ENV = {"nakamoto": O.GymEnv, "bk": O.BkGymEnv, "ethereum": O.EthGymEnv, "tailstorm": O.TsGymEnv}
POLICY = {"nakamoto": L.POLICY_SAPIRSHTEIN_2016_SM1, "bk": L.BK_POLICY_GET_AHEAD,
          "ethereum": L.ETH_POLICY_FN19, "tailstorm": L.TS_POLICY_AVOID_LOSS}
INFO = ["episode_reward_attacker", "episode_reward_defender", "episode_progress",
        "episode_chain_time", "episode_sim_time", "episode_n_steps", "episode_n_activations",
        "head_height", "head_miner"]


@pytest.fixture(scope="module")
def ctx():
    return device.default_context()


def make_cfg(proto, alpha=CFG_ALPHA, **kw):
    return device.make_config(**dict(PROTO[proto], alpha=alpha, gamma=GAMMA, n_lanes=N, **kw))


def _batch(ctx, proto, **kw):
    cfg, keep = make_cfg(proto, **kw)
    return cfg, device.Batch(cfg, ctx=ctx, keep=keep)


def ep_alpha(seed, episode):
    return TABLE[R.alpha_index(seed, episode, len(TABLE))]


class Oracles:
    """One oracle gym env per episode, made with that episode's alpha."""

    def __init__(self, proto, **kw):
        self.proto, self.seed = proto, kw["seed"]
        self.cfgs = {a: make_cfg(proto, alpha=a, **kw)[0] for a in TABLE}
        self.diag = 0

    def start(self, episode):
        a = ep_alpha(self.seed, episode)
        env = ENV[self.proto](self.cfgs[a], episode=int(episode))
        return env, a, env.reset()

    def finish(self, env):
        if self.proto == "nakamoto":
            self.diag |= env.diag()


# --------------------------------------------------------------------------- 1. the step path

@pytest.mark.parametrize("proto", ["nakamoto", "bk", "ethereum", "tailstorm"])
def test_step_path_runs_every_episode_at_its_own_alpha(ctx, proto):
    T = 96
    kw = dict(max_steps=32, seed=2024)
    if proto == "nakamoto":
        kw["propagation_delay"] = 0.05  # lanes leave the closed form for the exact engine
    _, b = _batch(ctx, proto, **kw)
    assert np.array_equal(b.lane_alpha(), np.full(N, CFG_ALPHA))
    b.set_lane_env(alphas=TABLE)
    orc = Oracles(proto, **kw)
    ids = np.arange(N, dtype=np.uint64)
    envs, alphas, ref = map(list, zip(*[orc.start(e) for e in ids]))
    obs = b.reset()
    assert np.array_equal(obs, np.array(ref))
    assert np.array_equal(b.lane_alpha(), np.array(alphas))
    seen, dones = set(alphas), 0
    keys = [k for k in INFO if not (proto == "tailstorm" and k == "head_miner")]
    for t in range(T):
        acts = b.policy_actions(POLICY[proto], obs)
        obs, rew, done, info = b.step(acts)
        for i in range(N):
            o, r, d, inf = envs[i].step(int(acts[i]))
            assert np.array_equal(obs[i], o), (t, i, obs[i], o)
            assert rew[i] == r and done[i] == d, (t, i)
            for k in keys:
                assert info[k][i] == inf[k], (t, i, k)
        st = info["status"]
        assert not ((st & L.ST_LOCKSTEP_INEXACT != 0) & (st & L.ST_EXACT_RERUN == 0)).any()
        if done.any():
            dones += int(done.sum())
            ids[done] += N
            for i in np.flatnonzero(done):
                orc.finish(envs[i])
                envs[i], alphas[i], ref[i] = orc.start(ids[i])
                seen.add(alphas[i])
            obs = b.reset(mask=done, episode_ids=ids)
            assert np.array_equal(obs[done], np.array(ref)[done]), t
        assert np.array_equal(b.lane_alpha(), np.array(alphas)), t
    for e in envs:
        orc.finish(e)
    # preconditions, on the oracle's run
    assert dones > 0 and len(seen) >= 2
    if proto == "nakamoto":
        assert orc.diag & 2  # DIAG_OVERLAP: the exact-engine hand-over ran per lane alpha


# ------------------------------------------- 2. the network rollout, exact integers, bit for bit

def int_net(seed, n_in, n_act, extra):
    """Weights in {-1, 0, 1}, three layers of 32 units (test_gpu_policy_net.py's network)."""
    rng = np.random.default_rng(seed)

    def lin(n_out, fan_in):
        return (rng.integers(-1, 2, size=(n_out, fan_in)).astype(np.float32),
                rng.integers(-1, 2, size=n_out).astype(np.float32))

    def trunk():
        return [lin(32, n_in if i == 0 else 32) for i in range(3)]

    return device.PolicyNet(pi=trunk(), pi_head=lin(n_act, 32), vf=trunk(), vf_head=lin(1, 32),
                            extra=extra)


def magnitude_bound(net, x):
    """max over layers and rows of sum |w||x| + |b| (an upper bound of every partial sum);
    x holds the whole input rows, extras included."""
    worst = 0.0
    for trunk, head in ((net.pi, net.pi_head), (net.vf, net.vf_head)):
        h = np.abs(x)
        for w, b in list(trunk) + [head]:
            h = h @ np.abs(w.astype(np.float64)).T + np.abs(b.astype(np.float64))
            worst = max(worst, h.max())
    return worst


EXACT = {
    # (config, weight seed chosen on the CPU so that the reference run is non-trivial)
    "nakamoto": (dict(max_steps=32, propagation_delay=0.05, seed=2024, unit_observation=False), 3),
    "bk": (dict(max_steps=32, seed=2024, unit_observation=False), 3),
}
DENSE = dict(max_steps=800, max_progress=8)
DENSE_TARGET = 8


@functools.lru_cache(maxsize=None)
def net_reference(proto, dense=False, T=96):
    """The oracle's rollout: per lane one env per episode at its alpha, driven by forward_f64
    of the network whose extras are (that alpha, gamma). Also every lane's recorded episodes
    [(alpha, [(reward, done, era, erd, progress, n_activations), ...]), ...]."""
    kw, wseed = EXACT[proto]
    if dense:
        kw = dict(kw, **DENSE)
    ol, na = SHAPE[proto]
    nets = {a: int_net(wseed, ol + 2, na, (a, GAMMA)) for a in TABLE}
    orc = Oracles(proto, **kw)
    out = dict(obs0=np.zeros((N, ol)), obs=np.zeros((T, N, ol)), action=np.zeros((T, N), np.int32),
               reward=np.zeros((T, N)), done=np.zeros((T, N), bool), value=np.zeros((T + 1, N)),
               alpha0=np.zeros(N), alpha=np.zeros((T, N)))
    lanes = []
    for i in range(N):
        ep = i
        env, a, o = orc.start(ep)
        out["obs0"][i], out["alpha0"][i] = o, a
        episodes = [(a, [])]
        for t in range(T):
            lg, v = nets[a].forward_f64(o[None])
            act = int(np.argmax(lg[0]))  # the lowest index of the maximum
            out["value"][t, i], out["action"][t, i] = v[0], act
            o, r, d, inf = env.step(act)
            episodes[-1][1].append((r, d, inf["episode_reward_attacker"],
                                    inf["episode_reward_defender"], inf["episode_progress"],
                                    int(inf["episode_n_activations"])))
            if d:
                orc.finish(env)
                ep += N
                env, a, o = orc.start(ep)
                episodes.append((a, []))
            out["obs"][t, i], out["reward"][t, i], out["done"][t, i] = o, r, d
            out["alpha"][t, i] = a
        out["value"][T, i] = nets[a].forward_f64(o[None])[1][0]
        orc.finish(env)
        lanes.append([e for e in episodes if e[1]])
    return nets[TABLE[0]], out, lanes, orc.diag


def check_reference_is_exact_and_not_trivial(proto, net, ref, diag):
    ol = SHAPE[proto][0]
    obs = np.concatenate([ref["obs0"][None], ref["obs"]]).reshape(-1, ol)
    alpha = np.concatenate([ref["alpha0"][None], ref["alpha"]]).reshape(-1)
    rows = np.concatenate([obs, alpha[:, None], np.full((len(obs), 1), GAMMA)], axis=1)
    # exactness: inputs are multiples of 1/8 and every partial sum is below 2^21, so f32
    # arithmetic (24 bits) is exact in any order
    assert np.array_equal(rows * 8, np.rint(rows * 8))
    assert magnitude_bound(net, rows) < 2 ** 21
    assert len(np.unique(ref["action"])) >= 3
    assert ref["done"].any()
    assert len(np.unique(ref["alpha"])) >= 2
    if proto == "nakamoto":
        assert diag & 2  # DIAG_OVERLAP: a lane left the closed form


def net_batch(ctx, proto, dense=False, **env):
    kw, _ = EXACT[proto]
    if dense:
        kw = dict(kw, **DENSE)
    _, b = _batch(ctx, proto, **kw)
    b.set_lane_env(alphas=TABLE, alpha_column=0, **env)
    return b


@pytest.mark.parametrize("proto", ["nakamoto", "bk"])
def test_integer_network_rollout_with_lane_alpha_equals_oracle(ctx, proto):
    T = 96
    net, ref, _, diag = net_reference(proto)
    check_reference_is_exact_and_not_trivial(proto, net, ref, diag)
    b = net_batch(ctx, proto)
    b.set_policy_net(net)  # its alpha extra is the table's first entry: never the input
    s, got = b.rollout_net(T, deterministic=True)
    for f in ("obs0", "obs", "action", "reward", "done", "value", "alpha0", "alpha"):
        bad = np.argwhere(got[f] != ref[f])
        assert len(bad) == 0, (f, bad[0], got[f][tuple(bad[0])], ref[f][tuple(bad[0])])
    assert np.array_equal(got["engine_reward"], ref["reward"])
    assert s.steps == T * N and s.episodes == int(ref["done"].sum())
    assert np.array_equal(b.lane_alpha(), ref["alpha"][-1])


# ------------------------------------------------------------------------------- 3. rewards

@pytest.mark.filterwarnings("ignore:observed too")
@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("scheme", R.SCHEMES)
@pytest.mark.parametrize("proto", ["nakamoto", "bk"])
def test_wrapped_rewards_equal_the_python_wrappers(ctx, proto, scheme, shape):
    T = 96
    dense = scheme == "dense_per_progress"
    net, ref, lanes, diag = net_reference(proto, dense)
    check_reference_is_exact_and_not_trivial(proto, net, ref, diag)
    want = np.zeros((T, N))
    for i, episodes in enumerate(lanes):
        want[:, i] = R.wrapped_rewards(episodes, scheme, shape, DENSE_TARGET)
    assert np.any(want != 0.0)
    if dense:
        ends = [steps[-1] for eps in lanes for _, steps in eps if steps[-1][1]]
        assert ends and all(s[4] != 0 for s in ends)  # at 0 the reference would have raised
        # a done with progress != target, so that the overshoot correction runs. Nakamoto's
        # run has five. B_k (k = 2, progress in steps of 2) has none under this configuration
        # with any weight seed in 0..499 (searched on the CPU): its run checks the scaling,
        # the accumulator across resets and the branch without a correction.
        if proto == "nakamoto":
            assert any(s[4] != DENSE_TARGET for s in ends)
    b = net_batch(ctx, proto, dense, reward=scheme, shape=shape,
                  dense_target=DENSE_TARGET if dense else None)
    b.set_policy_net(net)
    _, got = b.rollout_net(T, deterministic=True)
    for f in ("obs", "action", "done", "alpha"):
        assert np.array_equal(got[f], ref[f]), f
    assert np.array_equal(got["engine_reward"], ref["reward"])
    bad = np.argwhere(got["reward"].view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (bad[0], got["reward"][tuple(bad[0])], want[tuple(bad[0])])


# --------------------------------------------------------------------------- 4. consistency

CONSIST = dict(max_steps=20, seed=99)
SUM_FIELDS = ["episodes", "steps", "activations", "reward_attacker_fx", "reward_defender_fx",
              "progress_fx", "rel_revenue_fx", "rel_revenue_sq_fx", "orphans", "status_tie",
              "status_overlap", "status_other", "invalid"]
NET_OUT = ("obs", "action", "reward", "done", "logp")


def float_net(seed, n_in, depth, wpi, wvf, n_act, extra=()):
    rng = np.random.default_rng(seed)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    def trunk(w):
        return [lin(w, n_in if i == 0 else w) for i in range(depth)]

    return device.PolicyNet(pi=trunk(wpi), pi_head=lin(n_act, wpi), vf=trunk(wvf),
                            vf_head=lin(1, wvf), extra=extra)


def consist_net(proto, extra=(0.4, GAMMA)):
    ol, na = SHAPE[proto]
    return float_net(7, ol + 2, 2, 48, 32, na, extra=extra)


@pytest.mark.parametrize("proto", ["nakamoto", "bk", "ethereum", "tailstorm"])
def test_sampled_rollout_with_a_table_is_consistent(ctx, proto):
    T = 48
    net = consist_net(proto)
    env = dict(alphas=TABLE, alpha_column=0, reward="sparse_relative", shape="per_alpha")

    def fresh():
        _, b = _batch(ctx, proto, **CONSIST)
        b.set_lane_env(**env)
        b.set_policy_net(net)
        return b

    sa, A = fresh().rollout_net(T, deterministic=False)
    assert A["done"].any() and len(np.unique(A["action"])) >= 3
    assert len(np.unique(A["alpha"])) >= 2
    # the alpha outputs follow the assignment rule
    ep = np.arange(N)
    assert np.array_equal(A["alpha0"], [ep_alpha(99, e) for e in ep])
    for t in range(T):
        ep = ep + N * A["done"][t]
        assert np.array_equal(A["alpha"][t], [ep_alpha(99, e) for e in ep]), t

    # (a) one 48-step call equals three 16-step calls
    b = fresh()
    parts = [b.rollout_net(16, deterministic=False) for _ in range(3)]
    assert np.array_equal(parts[0][1]["obs0"], A["obs0"])
    assert np.array_equal(parts[0][1]["alpha0"], A["alpha0"])
    for k in NET_OUT + ("alpha", "engine_reward"):
        assert np.array_equal(np.concatenate([p[1][k] for p in parts]), A[k]), k
    for j in range(3):
        assert np.array_equal(parts[j][1]["value"][:16], A["value"][16 * j:16 * j + 16])
    assert np.array_equal(parts[2][1]["value"][16], A["value"][T])
    for f in SUM_FIELDS:
        assert sum(getattr(p[0], f) for p in parts) == getattr(sa, f), f

    # (b) a host-driven replay through step with the rollout's actions
    _, b2 = _batch(ctx, proto, **CONSIST)
    b2.set_lane_env(**env)
    obs = b2.reset()
    assert np.array_equal(obs, A["obs0"]) and np.array_equal(b2.lane_alpha(), A["alpha0"])
    ids = np.arange(N, dtype=np.uint64)
    for t in range(T):
        obs, rew, d, _ = b2.step(A["action"][t])
        if d.any():
            ids[d] += N
            obs = b2.reset(mask=d, episode_ids=ids)
        assert np.array_equal(obs, A["obs"][t]), t
        assert np.array_equal(rew, A["engine_reward"][t]), t  # step's reward stays the engine's
        assert np.array_equal(d, A["done"][t]), t
        assert np.array_equal(b2.lane_alpha(), A["alpha"][t]), t


@pytest.mark.parametrize("proto", ["nakamoto", "bk", "ethereum", "tailstorm"])
def test_one_entry_table_equal_to_cfg_alpha_changes_nothing(ctx, proto):
    T = 48
    net = consist_net(proto, extra=(0.4, GAMMA))
    kw = dict(CONSIST, alpha=0.4)
    if proto == "nakamoto":
        kw["propagation_delay"] = 0.05
    _, plain = _batch(ctx, proto, **kw)
    plain.set_policy_net(net)
    sp, P = plain.rollout_net(T, deterministic=False)
    assert set(P) == {"obs0", "obs", "action", "reward", "done", "logp", "value"}
    _, b = _batch(ctx, proto, **kw)
    b.set_lane_env(alphas=[0.4], alpha_column=None, reward="engine", shape="none")
    b.set_policy_net(net)
    se, E = b.rollout_net(T, deterministic=False)
    assert P["done"].any()
    for k in P:
        assert np.array_equal(P[k], E[k]), k
    assert np.array_equal(E["engine_reward"], P["reward"])
    assert np.all(E["alpha"] == 0.4) and np.all(E["alpha0"] == 0.4)
    for f in SUM_FIELDS:
        assert getattr(sp, f) == getattr(se, f), f
    assert list(sp.hist) == list(se.hist)


def test_device_env_fn_builds_cpr_v0_over_lanes(ctx):
    from cpr_amd import envs

    b, extras = envs.device_env_fn(N, ctx=ctx, seed=2024, protocol="nakamoto", episode_len=32,
                                   alpha=list(TABLE), gamma=GAMMA, reward="sparse_relative")
    assert extras == (TABLE[0], GAMMA)
    assert (b.config.max_steps, b.config.max_progress, b.config.defenders) == (32, 0.0, 2)
    b.reset()
    assert np.array_equal(b.lane_alpha(), [ep_alpha(2024, e) for e in range(N)])
    b.set_policy_net(int_net(3, 4 + 2, 4, extras))
    _, out = b.rollout_net(40, deterministic=True)
    done = out["done"]
    assert done.any() and np.all(out["reward"][~done] == 0.0)  # sparse: paid at the end only
    # normalize_reward: the episode's share over the alpha it ran at (the step's input)
    prev = np.concatenate([out["alpha0"][None], out["alpha"][:-1]])
    assert np.any(out["reward"][done] != 0.0)
    assert np.all(out["reward"][done] * prev[done] <= 1.0 + 1e-12)

    # the dense scheme ends episodes at episode_len progress, within 100 episode_len steps
    b, _ = envs.device_env_fn(N, ctx=ctx, protocol="bk", protocol_args=dict(k=2, reward="constant"),
                              episode_len=8, alpha=0.25, reward="dense_per_progress")
    assert (b.config.max_steps, b.config.max_progress) == (800, 8.0)
    # a callable is sampled into a 4,096-entry table; pretend_alpha keeps the extra constant
    rng = np.random.default_rng(1)
    draws = []

    def schedule():
        draws.append(float(rng.uniform(0.1, 0.4)))
        return draws[-1]

    b, extras = envs.device_env_fn(N, ctx=ctx, seed=5, alpha=schedule, pretend_alpha=0.3,
                                   episode_len=16)
    assert len(draws) == L.LANE_ENV_MAX_ALPHA and extras == (0.3, GAMMA)
    b.reset()
    assert np.array_equal(b.lane_alpha(),
                          [draws[R.alpha_index(5, e, len(draws))] for e in range(N)])


# ------------------------------------------------------------------------------ 5. refusals

def _code(fn):
    with pytest.raises(L.CprError) as e:
        fn()
    return e.value.code


def test_lane_env_after_the_first_reset_or_rollout_is_a_state_error(ctx):
    _, b = _batch(ctx, "nakamoto", **CONSIST)
    b.reset()
    assert _code(lambda: b.set_lane_env(alphas=TABLE)) == L.CPR_E_STATE
    _, b = _batch(ctx, "bk", **CONSIST)
    b.set_policy_net(consist_net("bk"))
    b.rollout_net(2)
    assert _code(lambda: b.set_lane_env(alphas=TABLE)) == L.CPR_E_STATE
    _, b = _batch(ctx, "bk", **CONSIST)
    b.rollout(2)
    assert _code(lambda: b.set_lane_env(alphas=TABLE)) == L.CPR_E_STATE


def test_lane_env_invalid_arguments_are_refused(ctx):
    _, b = _batch(ctx, "nakamoto", **CONSIST)
    bad = L.CPR_E_INVALID_ARG
    # n_alpha out of range
    assert _code(lambda: b.set_lane_env(alphas=[])) == bad
    assert _code(lambda: b.set_lane_env(alphas=np.full(4097, 0.25))) == bad
    e = L.LaneEnvC()
    tab = np.array(TABLE)
    e.n_alpha, e.alpha, e.alpha_column = -1, tab.ctypes.data, -1
    assert L.lib().cpr_lane_env_set(b.handle, ctypes.byref(e)) == bad
    e.n_alpha, e.alpha = 4, None
    assert L.lib().cpr_lane_env_set(b.handle, ctypes.byref(e)) == bad
    # alphas that are NaN or outside [0, 1]
    for a in (float("nan"), -0.125, 1.5):
        assert _code(lambda: b.set_lane_env(alphas=[0.25, a])) == bad
    # alpha 0 with a shape that divides by it (fine without one)
    for shape in ("per_alpha", "cut"):
        assert _code(lambda: b.set_lane_env(alphas=[0.25, 0.0], shape=shape)) == bad
    # dense_target <= 0
    for t in (None, 0.0, -8.0):
        assert _code(lambda: b.set_lane_env(alphas=TABLE, reward="dense_per_progress",
                                            dense_target=t)) == bad
    # alpha_column against the network's extras, whichever setter comes second
    assert _code(lambda: b.set_lane_env(alphas=TABLE, alpha_column=-2)) == bad
    b.set_policy_net(consist_net("nakamoto"))  # two extras
    assert _code(lambda: b.set_lane_env(alphas=TABLE, alpha_column=2)) == bad
    b.set_lane_env(alphas=[0.25, 0.0, 1.0], alpha_column=1)  # none of the above: accepted
    b.set_lane_env(alphas=[0.25, 0.5], alpha_column=1)  # and replaced before the first reset
    assert _code(lambda: b.set_policy_net(float_net(1, 4 + 1, 1, 16, 16, 4, extra=(0.5,)))) == bad
    b.set_policy_net(consist_net("nakamoto"))
    b.rollout_net(2)


def test_lane_env_unsupported_batches_and_calls(ctx):
    cfg, keep = device.make_config(alpha=0.3, gamma=0.5, protocol=L.PROTO_FC16, max_steps=100,
                                   policy=L.FC16_POLICY_HONEST, n_lanes=4)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    assert _code(lambda: b.set_lane_env(alphas=TABLE)) == L.CPR_E_UNSUPPORTED
    cfg, keep = device.make_config(alpha=0.3, gamma=0.5, max_steps=20, n_lanes=0)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    assert _code(lambda: b.set_lane_env(alphas=TABLE)) == L.CPR_E_UNSUPPORTED
    # the built-in rollout runs every lane at cfg.alpha: refused while a table is set
    _, b = _batch(ctx, "bk", **CONSIST)
    b.set_lane_env(alphas=TABLE)
    assert _code(lambda: b.rollout(4)) == L.CPR_E_UNSUPPORTED
    # without a table (cfg.alpha, reward wrappers only) it still runs
    _, b = _batch(ctx, "bk", **CONSIST)
    b.set_lane_env(reward="sparse_relative")
    assert b.rollout(4).steps == 4 * N
