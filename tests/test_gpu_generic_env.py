"""The generic release/consider env over Nakamoto as lockstep lanes
(CPR_PROTO_GENERIC_NAKAMOTO) — needs an MI355X.

Every comparison is against tests/generic_env_ref.py: the literal pure-Python env (tied to
generic_lane.h and to two counter models by test_generic_env_host.py) or the counter models
themselves, never a device path against itself.

1. lockstep parity under the host fuzz's action distribution, on 128 and on 37 lanes;
2. honest play and always-Continue against the counter models;
3. honest play's law: the attacker's reward is Binomial(progress, alpha);
4. networks: rollout_net against a host loop, evaluate_net, one ppo_iterate, one dqn_iterate;
5. envs.Generic, the reference's surface;
6. refusals.
"""

import ctypes
import os

import numpy as np
import pytest
import torch

import dqn_ref
import eval_ref
import generic_env_ref as R
import lane_env_ref
import ppo_ref
from cpr_amd import _lib as L
from cpr_amd import device, envs
from cpr_amd import dqn as Q
from cpr_amd import ppo as P

pytestmark = pytest.mark.gpu

INFO = ["episode_reward_attacker", "episode_reward_defender", "episode_progress",
        "episode_chain_time", "episode_sim_time", "episode_n_steps", "episode_n_activations",
        "head_height", "head_miner", "status"]
ACTIONS = np.array([0, 1, -1, 2, -2, 3, -3, 256, -256], dtype=np.int32)
ALPHAS = [0.2, 0.3, 0.45]


@pytest.fixture(scope="module")
def ctx():
    return device.default_context()


def _batch(ctx, **kw):
    kw.setdefault("k", 2)
    cfg, keep = device.make_config(protocol=L.PROTO_GENERIC_NAKAMOTO, policy=0, **kw)
    return device.Batch(cfg, ctx=ctx, keep=keep)


def _f64(obs32):
    return np.asarray(obs32, dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------ 1. lockstep parity

FUZZ = dict(alpha=0.4, gamma=0.6, horizon=6, max_steps=48)


def _run_parity(ctx, n, T, until=()):
    """The device under fuzz actions against one reference env per lane, every output of every
    step, for T steps and until the episodes `until` are over; lane i plays episodes 500 + i,
    500 + i + n, ... Returns {episode: (era, erd, progress, steps, status)} of the finished
    episodes and the events the references reached."""
    seed = 9
    b = _batch(ctx, seed=seed, n_lanes=n, **FUZZ)
    assert b.observation_spec()[:2] == (5, 5)
    refs = [R.GenericNakamotoRef(seed, FUZZ["alpha"], FUZZ["gamma"], FUZZ["horizon"],
                                 FUZZ["max_steps"]) for _ in range(n)]
    ids = np.arange(n, dtype=np.uint64) + 500
    want = np.array([_f64(e.reset(i)) for e, i in zip(refs, ids)])
    assert b.reset(episode_ids=ids).tobytes() == want.tobytes()
    finished = {}
    t = 0
    while t < T or not set(until) <= set(finished):
        assert t < 1000
        # the action depends on (episode, step) alone, so any lane count plays the same episodes
        acts = np.array([ACTIONS[np.random.default_rng([int(ids[i]), refs[i].steps]).integers(9)]
                         for i in range(n)], dtype=np.int32)
        obs, rew, done, info = b.step(acts)
        out = [e.step(int(a)) for e, a in zip(refs, acts)]
        assert obs.tobytes() == np.array([_f64(o[0]) for o in out]).tobytes(), t
        assert np.array_equal(rew, [o[1] for o in out]), t
        assert np.array_equal(done, [o[2] or o[3] for o in out]), t
        infos = [e.info() for e in refs]
        for k in INFO:
            assert np.array_equal(info[k], [i[k] for i in infos]), (t, k)
        assert np.array_equal(b.observe_fields(), [e.fields() for e in refs]), t
        if done.any():  # the test's own auto-reset: a partial mask, fresh episode ids
            for i in np.flatnonzero(done):
                e = refs[i]
                finished[int(ids[i])] = (e.era, e.erd, e.eprog, e.steps, e.status)
            ids[done] += np.uint64(n)
            want = np.array([_f64(refs[i].reset(ids[i])) if done[i] else _f64(out[i][0])
                             for i in range(n)])
            assert b.reset(mask=done, episode_ids=ids).tobytes() == want.tobytes(), t
        t += 1
    events = set().union(*(e.events for e in refs))
    return finished, events


@pytest.fixture(scope="module")
def parity_128(ctx):
    return _run_parity(ctx, 128, 150)


def test_lockstep_parity_every_output_of_every_step(parity_128):
    finished, events = parity_128
    assert len(finished) > 256
    # terminated and truncated episodes, rewrites, long lists and guarded actions were compared
    assert {"release>=2", "consider>=2", "rewrite", "truncated", ("clamped", True),
            ("clamped", False), ("empty", True), ("empty", False), ("shutdown", True, True),
            ("shutdown", False, True)} <= events
    assert any(not (st & L.ST_CAPACITY) for *_, st in finished.values())


def test_the_same_episodes_on_37_lanes(ctx, parity_128):
    """Lane i of n plays episodes 500 + i, 500 + i + n, ...: on 37 lanes the first 128
    episode ids are played again (by other lanes, at other times) with the same results."""
    first = {e: v for e, v in parity_128[0].items() if e < 500 + 128}
    assert len(first) == 128
    got, _ = _run_parity(ctx, 37, 0, until=first)
    for e in first:
        assert got[e] == first[e], e


# ------------------------------------------------------------ 2. the counter models

def _play(b, policy, max_iter):
    """Every lane plays its first episode under policy(fields) -> actions; returns the infos
    at each lane's done step and that step's rewrite field."""
    n = b.n_lanes
    b.reset()
    live = np.ones(n, dtype=bool)
    res = {k: np.zeros(n) for k in INFO}
    rewrite = np.zeros(n, dtype=np.int64)
    for _ in range(max_iter):
        obs, rew, done, info = b.step(policy(b.observe_fields()))
        f = b.observe_fields()
        end = done & live
        for k in INFO:
            res[k][end] = info[k][end]
        rewrite[end] = f[end, 6]
        live &= ~done
        if not live.any():
            break
    assert not live.any()
    return res, rewrite


@pytest.mark.parametrize("model", ["honest", "continue"])
def test_counter_models_on_the_device(ctx, model):
    n, seed = 256, 31
    kw = dict(alpha=0.4, gamma=0.6, horizon=8, max_steps=200)
    b = _batch(ctx, seed=seed, n_lanes=n, **kw)
    if model == "honest":
        counter = R.honest_counter
        policy = lambda f: np.array([envs.generic_honest_action(r) for r in f],  # noqa: E731
                                    dtype=np.int32)
    else:
        counter = R.continue_counter
        policy = lambda f: np.zeros(len(f), dtype=np.int32)  # noqa: E731
    res, rewrite = _play(b, policy, 200)
    want = [counter(seed, e, 0.4, 0.6, 8, 200) for e in range(n)]
    assert np.array_equal(res["episode_reward_attacker"], [w["reward_attacker"] for w in want])
    assert np.array_equal(res["episode_reward_defender"], [w["reward_defender"] for w in want])
    assert np.array_equal(res["episode_progress"], [w["progress"] for w in want])
    assert np.array_equal(res["episode_n_steps"], [w["steps"] for w in want])
    assert np.array_equal(rewrite, [w["rewrite"] for w in want])
    trunc = (res["status"].astype(np.uint32) & L.ST_CAPACITY) != 0
    assert np.array_equal(trunc, [w["truncated"] for w in want])
    if model == "continue":
        assert (rewrite > 0).any() and (rewrite == 0).any()


# ------------------------------------------------------------ 3. honest play's law

def test_honest_play_pays_binomial_progress_alpha(ctx):
    """Under honest play every mined block ends on the defenders' chain and the termination
    words are independent of the miner words (generic_env_ref's docstring), so given the
    progress the attacker's reward is exactly Binomial(sum of progress, alpha)."""
    n, alpha = 4096, 0.3
    b = _batch(ctx, seed=77, n_lanes=n, alpha=alpha, gamma=0.5, horizon=25, max_steps=1000)
    res, rewrite = _play(b, lambda f: np.where(f[:, 3] > 0, -1, np.where(f[:, 4] > 0, 1, 0))
                         .astype(np.int32), 1000)
    assert not (res["status"].astype(np.uint32) & L.ST_CAPACITY).any()  # no episode truncates
    N, k = res["episode_progress"].sum(), res["episode_reward_attacker"].sum()
    sigma = np.sqrt(N * alpha * (1 - alpha))
    print(f"honest law: progress {N:.0f} attacker {k:.0f} expected {N * alpha:.1f} "
          f"sigma {sigma:.1f} z {(k - N * alpha) / sigma:+.2f}")
    assert abs(k - N * alpha) <= 4 * sigma
    assert N / n == pytest.approx(25 + 1, rel=0.1)  # horizon, plus the block shutdown forces out
    assert not rewrite.any()


# ------------------------------------------------------------ 4. networks

def float_net(seed, depth, wpi, wvf, n_act=5, extra=()):
    rng = np.random.default_rng(seed)
    n_in = 5 + len(extra)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    def trunk(w):
        return [lin(w, n_in if i == 0 else w) for i in range(depth)]

    return device.PolicyNet(pi=trunk(wpi), pi_head=lin(n_act, wpi), vf=trunk(wvf),
                            vf_head=lin(1, wvf), extra=extra)


NET_KW = dict(alpha=0.35, gamma=0.5, horizon=6, max_steps=24)


@pytest.mark.parametrize("deterministic", [True, False])
def test_rollout_net_equals_a_host_loop(ctx, deterministic):
    """rollout_net with a lane env of three alphas against the reference env per lane, the
    network through policy_net_forward, the rewards through cpr_amd/wrappers.py."""
    n, T, seed = 64, 40, 21
    net = float_net(4, 2, 64, 64, extra=(0.375, 0.5))

    def make():
        b = _batch(ctx, seed=seed, n_lanes=n, **NET_KW)
        b.set_lane_env(alphas=ALPHAS, alpha_column=None, reward="sparse_relative",
                       shape="per_alpha")
        b.set_policy_net(net)
        return b

    b, h = make(), make()
    s, A = b.rollout_net(T, deterministic=deterministic)
    refs = [R.GenericNakamotoRef(seed, 0.35, 0.5, 6, 24) for _ in range(n)]
    ids = np.arange(n, dtype=np.uint64)

    def start(i):
        a = ALPHAS[lane_env_ref.alpha_index(seed, int(ids[i]), 3)]
        refs[i].set_alpha(a)
        return a, _f64(refs[i].reset(ids[i]))

    alpha = np.zeros(n)
    obs = np.zeros((n, 5))
    for i in range(n):
        alpha[i], obs[i] = start(i)
    assert obs.tobytes() == A["obs0"].tobytes() and np.array_equal(alpha, A["alpha0"])
    episodes = [[(alpha[i], [])] for i in range(n)]  # per lane, for wrappers.py
    n_done = 0
    for t in range(T):
        act, logp, val, lg = h.policy_net_forward(obs, deterministic=True, logits=True)
        assert np.array_equal(val, A["value"][t]), t
        if deterministic:
            assert np.array_equal(act, A["action"][t]) and np.array_equal(logp, A["logp"][t]), t
        else:
            act = A["action"][t]
            lg64 = lg.astype(np.float64)
            m = lg64.max(axis=1)
            ref_logp = lg64[np.arange(n), act] - m - np.log(np.exp(lg64 - m[:, None]).sum(axis=1))
            assert np.allclose(A["logp"][t], ref_logp, rtol=1e-12, atol=1e-15), t
        for i in range(n):
            o, r, term, trunc = refs[i].step(R.head_action(int(act[i]), 2))
            done = term or trunc
            e = refs[i]
            episodes[i][-1][1].append((r, done, float(e.era), float(e.erd), float(e.eprog),
                                       e.mined + 1))
            assert A["engine_reward"][t, i] == r and A["done"][t, i] == done, (t, i)
            if done:
                n_done += 1
                ids[i] += n
                alpha[i], obs[i] = start(i)
                episodes[i].append((alpha[i], []))
            else:
                obs[i] = _f64(o)
        assert obs.tobytes() == A["obs"][t].tobytes(), t
        assert np.array_equal(alpha, A["alpha"][t]), t
    assert np.array_equal(h.policy_net_forward(obs)[2], A["value"][T])
    for i in range(n):
        eps = [e for e in episodes[i] if e[1]]
        want = lane_env_ref.wrapped_rewards(eps, "sparse_relative", "per_alpha")
        assert np.array_equal(A["reward"][:, i], want), i
    assert n_done > n and len(np.unique(A["action"])) >= (2 if deterministic else 4)
    assert len(np.unique(A["alpha"])) == 3 and np.any(A["reward"] != A["engine_reward"])
    assert s.steps == T * n and s.episodes + s.invalid == n_done


def test_evaluate_net_equals_the_reference(ctx):
    E, seed, n = 60, 78, 16
    net = float_net(12, 2, 64, 64)
    b = _batch(ctx, seed=seed, n_lanes=n, **NET_KW)
    b.set_policy_net(net)
    res = b.evaluate_net(E, deterministic=True)
    h = _batch(ctx, seed=seed, n_lanes=1, **NET_KW)
    h.set_policy_net(net)
    recs = []
    env = R.GenericNakamotoRef(seed, 0.35, 0.5, 6, 24)
    for e in range(E):
        obs = env.reset(e)
        total = 0.0
        while True:
            act = h.policy_net_forward(_f64(obs)[None], deterministic=True)[0]
            obs, r, term, trunc = env.step(R.head_action(int(act[0]), 2))
            total += r
            if term or trunc:
                break
        i = env.info()
        recs.append(dict(episode=e, alpha=0.35, episode_reward=total, episode_sim_time=0.0,
                         episode_chain_time=0.0, episode_progress=i["episode_progress"],
                         reward_attacker=i["episode_reward_attacker"],
                         reward_defender=i["episode_reward_defender"],
                         episode_n_activations=i["episode_n_activations"],
                         episode_n_steps=i["episode_n_steps"], height=i["head_height"],
                         alpha_index=0, status=i["status"]))
    for name in L.EVAL_RECORD_DTYPE.names:
        assert np.array_equal(res.records[name], [r[name] for r in recs]), name
    cnt, mean, std = eval_ref.stats(recs)
    assert int(res.stats["n"][0]) == cnt
    assert eval_ref.same_bits(res.stats["mean"][0], mean)
    assert eval_ref.same_bits(res.stats["std"][0], std)
    assert eval_ref.summary_of(res.total) == eval_ref.summary(recs)
    assert 0 < cnt < E  # terminated and truncated episodes


def _stat_close(st, s64, s32, keys):
    for key in keys:
        print(f"{key}: device {st[key]!r} f64 {s64[key]!r} torch-f32 {s32[key]!r}")
        # test_gpu_ppo.py / test_gpu_dqn.py: rtol 1e-5 against float64, or 8x torch-f32's error
        tol = max(1e-5 * abs(s64[key]), 8 * abs(s32[key] - s64[key]))
        assert abs(st[key] - s64[key]) <= tol, (key, st[key], s64[key], s32[key])


def test_one_ppo_iterate_equals_the_reference_loss(ctx):
    n, T, seed = 64, 16, 41
    net = float_net(18, 2, 64, 64)

    def make():
        b = _batch(ctx, seed=seed, n_lanes=n, **NET_KW)
        b.set_policy_net(net)
        return b

    opts = P.PPOOptions(n_epochs=1, minibatch=n * T, ent_coef=0.01, lr=1e-3)
    b, twin = make(), make()
    s, st = b.ppo_iterate(T, opts)
    s2, a = twin.rollout_net(T, deterministic=False)
    assert bytes(s) == bytes(s2) and a["done"].any() and (a["reward"] != 0).any()
    assert st["n_minibatches"] == 1
    adv, ret = ppo_ref.gae_ref(a["reward"], a["done"], a["value"], opts.gae_gamma,
                               opts.gae_lambda)
    obs = np.concatenate([a["obs0"][None], a["obs"][:-1]]).reshape(T * n, -1)
    x = ppo_ref.net_input(net, obs, None, None)
    args = (a["action"].ravel(), a["logp"].ravel(), adv.ravel(), ret.ravel(), opts)
    s64, _, _ = ppo_ref.ppo_loss(net, x, *args, torch.float64)
    s32, _, _ = ppo_ref.ppo_loss(net, x, *args, torch.float32)
    _stat_close(st, s64, s32, ("policy_loss", "value_loss", "entropy_loss", "approx_kl",
                               "clip_fraction", "loss", "grad_norm"))
    # the update itself: the same data through ppo_update on the twin, bit for bit
    st2 = twin.ppo_update(dict(obs=obs, action=a["action"].ravel(), old_logp=a["logp"].ravel(),
                               advantage=adv.ravel(), ret=ret.ravel()), opts)
    assert st == st2
    w = P.flatten_params(b.get_policy_net())
    assert w.tobytes() == P.flatten_params(twin.get_policy_net()).tobytes()
    assert np.any(w != P.flatten_params(net))


def test_one_dqn_iterate_equals_the_reference_loss(ctx):
    n, T, seed, batch = 64, 12, 43, 130
    net = float_net(19, 2, 64, 64)
    b = _batch(ctx, seed=seed, n_lanes=n, **NET_KW)
    b.set_policy_net(net)
    b.dqn_init(T)
    opts = Q.DQNOptions(batch=batch, gradient_steps=1, lr=1e-3, gamma=0.95, learning_starts=0,
                        target_update_interval=10 ** 9)
    s, st = b.dqn_iterate(T, 0.5, opts)
    assert st["n_steps"] == 1 and s.steps == T * n
    rep = b.dqn_replay()
    idx = b.dqn_last_indices(1, batch)[0]
    assert np.array_equal(idx, dqn_ref.sample_indices(seed, opts.sample_seed, 0, 1, batch,
                                                      T * n)[0])
    flat = {k: rep[k].reshape((T * n,) + rep[k].shape[2:]) for k in rep}
    assert len(np.unique(flat["action"])) == 5 and flat["done"].any()
    x = ppo_ref.net_input(net, flat["obs"][idx], None, None)
    xn = ppo_ref.net_input(net, flat["next_obs"][idx], None, None)
    args = (x, xn, flat["action"][idx], flat["reward"][idx], flat["done"][idx], 0.95)
    s64, _, _ = dqn_ref.dqn_loss(net, net, *args, torch.float64)
    s32, _, _ = dqn_ref.dqn_loss(net, net, *args, torch.float32)
    _stat_close(st, s64, s32, ("loss", "abs_td", "q", "target", "grad_norm"))
    assert np.any(P.flatten_params(b.get_policy_net()) != P.flatten_params(net))
    assert P.flatten_params(b.get_target_net()).tobytes() == P.flatten_params(net).tobytes()


# ------------------------------------------------------------ 5. envs.Generic

def test_generic_env_has_the_references_surface(ctx):
    seed, alpha, horizon = 3, 0.35, 6
    env = envs.Generic("nakamoto", alpha=alpha, gamma=0.5, horizon=horizon, max_steps=30,
                       seed=seed, ctx=ctx)
    ref = R.GenericNakamotoRef(seed, alpha, 0.5, horizon, 30)
    # test_rust.py: the action codec and its descriptions
    assert env.encode_action_continue() == 0.0
    assert env.encode_action_release(0) < 0 < env.encode_action_consider(0)
    assert env.describe_action([env.encode_action_continue()]) == "Continue"
    for i in (0, 1, 7, 255):
        assert env.describe_action([env.encode_action_release(i)]) == f"Release({i})"
        assert env.describe_action([env.encode_action_consider(i)]) == f"Consider({i})"
    assert env.describe_action([0.1]) == env.describe_action([-0.1]) == "Continue"
    with pytest.raises(ValueError):
        env.describe_action([1.5])
    assert list(env.low()) == [0, 0, 0, -1, 0]
    assert list(env.high()) == [np.finfo(np.float32).max, np.finfo(np.float32).max, 1, 0, 1]
    rng = np.random.default_rng(5)
    n_term = n_trunc = 0
    for ep in range(12):
        obs, info = env.reset()
        assert info == {} and obs.dtype == np.float32
        assert obs.tobytes() == ref.reset(ep).tobytes()
        while True:
            a = float(R.encode_action(int(ACTIONS[rng.integers(9)]) if rng.random() < 0.7 else 0))
            obs, r, term, trunc, info = env.step([a])
            o, ra, t2, tr2 = ref.step(R.decode_action(a))
            assert obs.tobytes() == o.tobytes() and (term, trunc) == (t2, tr2)
            want = np.float32(np.float32(np.float32(ra) / np.float32(alpha)) / np.float32(horizon))
            assert np.float32(r) == want
            assert info == {k: type(info[k])(v) for k, v in ref.last.items()}
            assert sorted(info) == ["progress", "reward_attacker", "reward_defender", "rewrite",
                                    "time"]
            if term or trunc:
                n_term, n_trunc = n_term + term, n_trunc + trunc
                break
    assert n_term > 0 and n_trunc > 0


def test_device_env_fn_accepts_the_protocol(ctx):
    b, extras = envs.device_env_fn(40, ctx=ctx, seed=9, protocol="generic_nakamoto",
                                   protocol_args=dict(horizon=6, actions=3), episode_len=24,
                                   alpha=ALPHAS, gamma=0.5, reward="sparse_relative")
    assert b.config.protocol == L.PROTO_GENERIC_NAKAMOTO and b.config.horizon == 6.0
    assert b.config.k == 3 and b.config.max_steps == 24
    assert b.observation_spec()[:2] == (5, 7)
    b.set_policy_net(float_net(18, 1, 16, 16, n_act=7, extra=extras))
    s, A = b.rollout_net(30, deterministic=False)
    assert set(np.unique(A["alpha"])) == set(ALPHAS) and s.steps == 30 * 40
    assert A["action"].max() == 6 and A["done"].any()
    with pytest.raises(ValueError):
        envs.device_env_fn(8, ctx=ctx, protocol="generic_nakamoto", reward="dense_per_progress")


# ------------------------------------------------------------ 6. refusals

def test_refusals(ctx):
    kw = dict(alpha=0.35, gamma=0.5, horizon=6, seed=1, n_lanes=8)
    for bad in (None, 0, -3, L.GENERIC_MAX_STEPS + 1):
        with pytest.raises(L.CprError) as e:
            _batch(ctx, max_steps=bad, **kw)
        assert e.value.code == L.CPR_E_INVALID_ARG and "max_steps" in str(e.value)
    assert L.GENERIC_MAX_STEPS >= 1000
    for bad in (0, 12):
        with pytest.raises(L.CprError) as e:
            _batch(ctx, max_steps=20, k=bad, **kw)
        assert e.value.code == L.CPR_E_INVALID_ARG and "1..11" in str(e.value)
    assert _batch(ctx, max_steps=20, k=11, **kw).observation_spec()[1] == 23
    b = _batch(ctx, max_steps=20, **kw)
    with pytest.raises(L.CprError) as e:  # step before reset
        b.step(np.zeros(8, dtype=np.int32))
    assert e.value.code == L.CPR_E_STATE
    with pytest.raises(L.CprError) as e:
        b.run(4)
    assert e.value.code == L.CPR_E_UNSUPPORTED and "cpr_rollout_net" in str(e.value)
    with pytest.raises(L.CprError) as e:
        b.rollout(4)
    assert e.value.code == L.CPR_E_UNSUPPORTED and "cpr_rollout_net" in str(e.value)
    with pytest.raises(L.CprError) as e:
        b.policy_actions(0, np.zeros((1, 5)))
    assert e.value.code == L.CPR_E_UNSUPPORTED
    with pytest.raises(L.CprError) as e:
        b.node_outputs(4)
    assert e.value.code == L.CPR_E_UNSUPPORTED and "no network nodes" in str(e.value)
    with pytest.raises(L.CprError) as e:
        b.set_lane_env(reward="dense_per_progress", dense_target=16)
    assert e.value.code == L.CPR_E_UNSUPPORTED and "progress target" in str(e.value)
    off = np.zeros(5, dtype=np.int64)
    tr = L.CTrace()
    tr.n_episodes = 4
    for k in ("act_offset", "pow_offset", "link_offset"):
        setattr(tr, k, off.ctypes.data)
    s = L.Summary()
    rc = L.lib().cpr_replay(b.handle, ctypes.byref(tr), ctypes.byref(s), None, 0)
    assert rc == L.CPR_E_UNSUPPORTED and b"trace" in L.lib().cpr_last_error()
    # a network with the wrong head width
    with pytest.raises(ValueError) as e:
        b.set_policy_net(float_net(1, 1, 16, 16, n_act=4))
    assert "actions" in str(e.value)
    b.set_policy_net(float_net(1, 1, 16, 16))
    old = os.environ.get("CPR_FC16_ROLLOUT_FUSED")
    os.environ["CPR_FC16_ROLLOUT_FUSED"] = "1"
    try:
        with pytest.raises(L.CprError) as e:
            b.rollout_net(2)
        assert e.value.code == L.CPR_E_UNSUPPORTED and "CPR_FC16_ROLLOUT_FUSED" in str(e.value)
    finally:
        if old is None:
            del os.environ["CPR_FC16_ROLLOUT_FUSED"]
        else:
            os.environ["CPR_FC16_ROLLOUT_FUSED"] = old
    # actions beyond +-256 are clamped, not refused; a finished lane ignores steps
    b.reset()
    obs, rew, done, info = b.step(np.array([10 ** 6, -10 ** 6, 0, 0, 0, 0, 0, 0], dtype=np.int32))
    assert not done.any()
    for _ in range(20):
        obs, rew, done, info = b.step(np.zeros(8, dtype=np.int32))
    assert done.all()
    f = b.observe_fields()
    o2, r2, d2, i2 = b.step(np.zeros(8, dtype=np.int32))
    assert d2.all() and not r2.any() and np.array_equal(b.observe_fields(), f)
    assert o2.tobytes() == obs.tobytes()
