"""The FC'16 model as a lockstep env (CPR_PROTO_FC16_ENV) and its one-kernel network rollout
— needs an MI355X.

Every comparison is against the pure-Python env (fc16_env_ref.py, tied to the pinned episode
oracle by test_fc16_env_host.py) or against the launch sequence (CPR_FC16_ROLLOUT_FUSED=0),
never a device path against itself.

1. reset / step against the reference env, every output;
2. the launch sequence of rollout_net against a host loop of policy_net_forward + step + reset;
3. the fused rollout kernel against the launch sequence, every output bit for bit;
4. ppo_iterate (fused rollout) against rollout_net_env + gae + ppo_update by hand;
5. evaluate_net against fused episodes of the network's table (fc16_table_from_net);
6. refusals.
"""

import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import fc16_env_ref as R
import oracle_py as O
from cpr_amd import _lib as L
from cpr_amd import device, mdp
from cpr_amd import ppo as P

pytestmark = pytest.mark.gpu

INFO = ["episode_reward_attacker", "episode_reward_defender", "episode_progress",
        "episode_chain_time", "episode_sim_time", "episode_n_steps", "episode_n_activations",
        "head_height", "head_miner", "status"]
SUM_FIELDS = ["episodes", "steps", "activations", "reward_attacker_fx", "reward_defender_fx",
              "progress_fx", "rel_revenue_fx", "rel_revenue_sq_fx", "orphans", "status_tie",
              "status_overlap", "status_other", "invalid"]
ALPHAS = [0.2, 0.3, 0.45]


@pytest.fixture(scope="module")
def ctx():
    return device.default_context()


def _batch(ctx, **kw):
    kw.setdefault("policy", L.FC16_POLICY_HONEST)
    cfg, keep = device.make_config(protocol=L.PROTO_FC16_ENV, **kw)
    return device.Batch(cfg, ctx=ctx, keep=keep)


@contextlib.contextmanager
def _rollout_path(value):
    """CPR_FC16_ROLLOUT_FUSED, read by the library at every call."""
    old = os.environ.get("CPR_FC16_ROLLOUT_FUSED")
    os.environ["CPR_FC16_ROLLOUT_FUSED"] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ["CPR_FC16_ROLLOUT_FUSED"]
        else:
            os.environ["CPR_FC16_ROLLOUT_FUSED"] = old


def launch_sequence():
    return _rollout_path("0")


def fused_kernel():
    return _rollout_path("1")


def last_rollout_fused(b):
    return int(b.rollout_net_fused())


def float_net(seed, depth, wpi, wvf, extra=()):
    """Gaussian weights scaled 1/sqrt(fan_in) (test_gpu_policy_net.py's network)."""
    rng = np.random.default_rng(seed)
    n_in = 3 + len(extra)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    def trunk(w):
        return [lin(w, n_in if i == 0 else w) for i in range(depth)]

    return device.PolicyNet(pi=trunk(wpi), pi_head=lin(4, wpi), vf=trunk(wvf),
                            vf_head=lin(1, wvf), extra=extra)


# ------------------------------------------------------------ 1. reset / step against the reference

def test_reset_and_step_equal_the_reference_env(ctx):
    n, T, seed = 300, 200, 5
    kw = dict(alpha=0.35, gamma=0.5, horizon=10, max_steps=50)
    b = _batch(ctx, seed=seed, n_lanes=n, **kw)
    assert b.observation_spec()[:2] == (3, 4)
    envs = [R.Fc16EnvRef(seed, 0.35, 0.5, 10, 50) for _ in range(n)]
    ids = np.arange(n, dtype=np.uint64) + 1000  # explicit episode ids from the first reset on
    ref = np.array([e.reset(i) for e, i in zip(envs, ids)])
    assert b.reset(episode_ids=ids).tobytes() == ref.tobytes()
    rng = np.random.default_rng(9)
    seen, n_term, n_trunc = set(), 0, 0
    for t in range(T):
        acts = rng.integers(0, 4, n).astype(np.int32)
        obs, rew, done, info = b.step(acts)
        want = [e.step(int(a)) for e, a in zip(envs, acts)]
        seen |= {(int(a), e.last_name) for e, a in zip(envs, acts)}
        assert obs.tobytes() == np.array([w[0] for w in want]).tobytes(), t
        assert np.array_equal(rew, [w[1] for w in want]), t
        assert np.array_equal(done, [w[2] or w[3] for w in want]), t
        infos = [e.info() for e in envs]
        for k in INFO:
            assert np.array_equal(info[k], [i[k] for i in infos]), (t, k)
        assert np.array_equal(b.observe_fields(), [(e.a, e.h, e.fork) for e in envs]), t
        n_term += sum(w[2] for w in want)
        n_trunc += sum(w[3] for w in want)
        if done.any():  # the test's own auto-reset: a partial mask, explicit ids
            ids[done] += n
            for i in np.flatnonzero(done):
                ref[i] = envs[i].reset(ids[i])
            for i in np.flatnonzero(~done):
                ref[i] = want[i][0]
            assert b.reset(mask=done, episode_ids=ids).tobytes() == ref.tobytes(), t
    # preconditions, on the reference's run alone
    assert n_term > 0 and n_trunc > 0
    assert {(2, R.OVERRIDE), (2, R.MATCH), (2, R.WAIT), (3, R.MATCH), (3, R.WAIT)} <= seen


# ------------------------------------------------ 2. the launch sequence against a host loop

@pytest.mark.parametrize("deterministic", [True, False])
def test_launch_sequence_equals_a_host_loop(ctx, deterministic):
    n, T, seed = 130, 40, 21
    kw = dict(alpha=0.35, gamma=0.5, horizon=10, max_steps=12, seed=seed, n_lanes=n)
    net = float_net(4, 2, 16, 16)
    b, h = _batch(ctx, **kw), _batch(ctx, **kw)
    b.set_policy_net(net)
    h.set_policy_net(net)
    with launch_sequence():
        s, A = b.rollout_net(T, deterministic=deterministic)
        assert last_rollout_fused(b) == 0
    obs = h.reset()
    assert obs.tobytes() == A["obs0"].tobytes()
    ids = np.arange(n, dtype=np.uint64)
    step = np.zeros(n, dtype=np.int64)
    finished, near = [], 0
    for t in range(T):
        act, logp, val, lg = h.policy_net_forward(obs, deterministic=True, logits=True)
        assert np.array_equal(val, A["value"][t]), t
        if deterministic:
            assert np.array_equal(act, A["action"][t]), t
            assert np.array_equal(logp, A["logp"][t]), t
        else:
            # the sampling rule in float64 on the device's logits, the draw from the oracle's
            # keyed stream at (episode, step, TAG_POLICY); rows within rounding of a CDF edge
            # are left to test 3's bit-for-bit comparison
            act = A["action"][t]
            lg64 = lg.astype(np.float64)
            m = lg64.max(axis=1)
            e = np.exp(lg64 - m[:, None])
            S = e[:, 0] + e[:, 1] + e[:, 2] + e[:, 3]
            cdf = np.cumsum(e, axis=1)
            u = np.array([O.u53(*(int(x) for x in O.keyed_block(seed, int(ids[i]), int(step[i]),
                                                               L.TAG_POLICY)[:2]))
                          for i in range(n)])
            below = (u * S)[:, None] < cdf
            expect = np.where(below.any(axis=1), below.argmax(axis=1), 3)
            close = (np.abs((u * S)[:, None] - cdf) <= 1e-9 * S[:, None]).any(axis=1)
            near += int(close.sum())
            assert np.array_equal(expect[~close], act[~close]), t
            ref_logp = lg64[np.arange(n), act] - m - np.log(S)
            assert np.allclose(A["logp"][t], ref_logp, rtol=1e-12, atol=0.0), t
        obs, rew, done, info = h.step(act)
        assert np.array_equal(rew, A["reward"][t]) and np.array_equal(done, A["done"][t]), t
        step += 1
        if done.any():
            finished += [{k: v[i] for k, v in info.items()} for i in np.flatnonzero(done)]
            ids[done] += n
            step[done] = 0
            obs = h.reset(mask=done, episode_ids=ids)
        assert obs.tobytes() == A["obs"][t].tobytes(), t
    assert np.array_equal(h.policy_net_forward(obs)[2], A["value"][T])
    assert near <= 2 and len(finished) > n and len(np.unique(A["action"])) >= 3
    # the summary: summary.h's fixed-point rule over the finished episodes' step infos
    want = dict.fromkeys(SUM_FIELDS, 0)
    hist = [0] * L.HIST_BINS
    want["steps"] = T * n
    for f in finished:
        ra, rd = float(f["episode_reward_attacker"]), float(f["episode_reward_defender"])
        st = int(f["status"])
        if st & L.ST_INVALID:
            want["invalid"] += 1
            continue
        rel = ra / (ra + rd) if ra + rd != 0 else 0.0
        want["episodes"] += 1
        want["reward_attacker_fx"] += int(np.rint(ra * 2 ** 20))
        want["reward_defender_fx"] += int(np.rint(rd * 2 ** 20))
        want["progress_fx"] += int(np.rint(float(f["episode_progress"]) * 2 ** 20))
        want["rel_revenue_fx"] += int(np.rint(rel * 2 ** 32))
        want["rel_revenue_sq_fx"] += int(np.rint(rel * rel * 2 ** 32))
        want["orphans"] += int(f["episode_n_activations"]) - int(f["head_height"])
        hist[min(L.HIST_BINS - 1, max(0, int(rel * L.HIST_BINS)))] += 1
    # activations: the start block and one per step of every episode, finished or running
    want["activations"] = T * n + n + len(finished)
    assert want["invalid"] > 0 and want["episodes"] > 0  # truncated and terminated episodes
    for f in SUM_FIELDS:
        if f not in ("status_tie", "status_overlap", "status_other"):
            assert getattr(s, f) == want[f], f
    assert list(s.hist) == hist


# ------------------------------------------------ 3. the fused kernel against the launch sequence

NET_OUT = ("obs0", "obs", "action", "reward", "done", "logp", "value")
ENV_OUT = ("alpha0", "alpha", "engine_reward")


def _make(ctx, n, shape, env, seed=31):
    depth, wpi, wvf = shape
    b = _batch(ctx, alpha=0.35, gamma=0.5, horizon=10, max_steps=12, seed=seed, n_lanes=n)
    if env:
        b.set_lane_env(alphas=ALPHAS, alpha_column=0, reward="sparse_relative", shape="per_alpha")
    # seed 18: played greedily, with or without the lane env, episodes of this network
    # terminate, truncate and pay the attacker (checked on the reference env)
    b.set_policy_net(float_net(18, depth, wpi, wvf, extra=(0.375, 0.5)))
    return b


def _device_rollout(b, T, deterministic, env):
    """rollout_net into torch tensors on the device, returned as host arrays."""
    n = b.n_lanes
    dev = torch.device("cuda", b.ctx.device)
    t = {"obs0": torch.zeros((n, 3), dtype=torch.float64, device=dev),
         "obs": torch.zeros((T, n, 3), dtype=torch.float64, device=dev),
         "action": torch.zeros((T, n), dtype=torch.int32, device=dev),
         "reward": torch.zeros((T, n), dtype=torch.float64, device=dev),
         "done": torch.zeros((T, n), dtype=torch.uint8, device=dev),
         "logp": torch.zeros((T, n), dtype=torch.float64, device=dev),
         "value": torch.zeros((T + 1, n), dtype=torch.float64, device=dev)}
    if env:
        t.update(alpha0=torch.zeros(n, dtype=torch.float64, device=dev),
                 alpha=torch.zeros((T, n), dtype=torch.float64, device=dev),
                 engine_reward=torch.zeros((T, n), dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    s, _ = b.rollout_net(T, deterministic=deterministic,
                         device_outputs={k: v.data_ptr() for k, v in t.items()})
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["done"] = out["done"].astype(bool)
    return s, out


def _same(A, B, what):
    assert sorted(A) == sorted(B), what
    for k in A:
        assert A[k].dtype == B[k].dtype and A[k].tobytes() == B[k].tobytes(), (what, k)


@pytest.mark.parametrize("shape", [(1, 16, 16), (3, 64, 64), (3, 64, 16)])
@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_fused_rollout_equals_the_launch_sequence(ctx, n, shape):
    T = 40
    episodes = invalid = wrapped = 0
    for env in (False, True):
        for deterministic in (False, True):
            what = (env, deterministic)
            f, q = _make(ctx, n, shape, env), _make(ctx, n, shape, env)
            with fused_kernel():
                sf, F = f.rollout_net(T, deterministic=deterministic)
            assert last_rollout_fused(f) == 1, what
            with launch_sequence():
                sq, Q = q.rollout_net(T, deterministic=deterministic)
                assert last_rollout_fused(q) == 0, what
            _same(F, Q, what)
            assert bytes(sf) == bytes(sq), what
            assert sorted(F) == sorted(NET_OUT + ENV_OUT if env else NET_OUT)
            assert F["done"].any()
            assert deterministic or len(np.unique(F["action"])) >= 2
            episodes += sf.episodes
            invalid += sf.invalid
            if env:
                assert len(np.unique(F["alpha"])) == 3
                wrapped += int(np.any(F["reward"] != F["engine_reward"]))
    # terminated and truncated episodes and wrapped rewards were compared
    assert episodes > 0 and invalid > 0 and wrapped > 0


@pytest.mark.parametrize("env", [False, True])
def test_fused_rollout_continues_across_calls_steps_and_resets(ctx, env):
    n, shape = 130, (3, 64, 16)
    # device outputs, and a 40-step call against two 20-step calls of the launch sequence
    f, q = _make(ctx, n, shape, env), _make(ctx, n, shape, env)
    with fused_kernel():
        sf, F = _device_rollout(f, 40, False, env)
    assert last_rollout_fused(f) == 1
    with launch_sequence():
        s1, Q1 = q.rollout_net(20, deterministic=False)
        s2, Q2 = q.rollout_net(20, deterministic=False)
    for k in F:
        if k in ("obs0", "alpha0"):
            want = Q1[k]
        elif k == "value":
            want = np.concatenate([Q1[k][:20], Q2[k]])
        else:
            want = np.concatenate([Q1[k], Q2[k]])
        assert F[k].tobytes() == want.tobytes(), k
    for fld in SUM_FIELDS:
        assert getattr(sf, fld) == getattr(s1, fld) + getattr(s2, fld), fld
    assert [x + y for x, y in zip(s1.hist, s2.hist)] == list(sf.hist)
    # two fused calls equal the one as well
    g = _make(ctx, n, shape, env)
    with fused_kernel():
        _, G1 = g.rollout_net(20, deterministic=False)
        _, G2 = g.rollout_net(20, deterministic=False)
    assert last_rollout_fused(g) == 1
    _same(G1, Q1, "first half")
    _same(G2, Q2, "second half")
    # a step and a partial reset between two calls are honoured by both paths
    acts = (np.arange(n) % 4).astype(np.int32)
    mask = (np.arange(n) % 3 == 0)
    ids = np.arange(n, dtype=np.uint64) + 7000
    outs = []
    for b, fused in ((g, True), (q, False)):
        o1 = b.step(acts)
        o2 = b.reset(mask=mask, episode_ids=ids)
        with fused_kernel() if fused else launch_sequence():
            s, X = b.rollout_net(20, deterministic=False)
        assert last_rollout_fused(b) == int(fused)
        outs.append((o1, o2, s, X))
    assert outs[0][0][0].tobytes() == outs[1][0][0].tobytes()
    assert outs[0][1].tobytes() == outs[1][1].tobytes()
    assert outs[0][3]["obs0"].tobytes() == outs[0][1].tobytes()
    _same(outs[0][3], outs[1][3], "after step and reset")
    assert bytes(outs[0][2]) == bytes(outs[1][2])


# ------------------------------------------------------------------ 4. ppo_iterate

def _weights(b):
    return P.flatten_params(b.get_policy_net())


def test_iterate_on_the_fused_rollout_equals_the_three_calls(ctx):
    def make():
        b = _batch(ctx, alpha=0.35, gamma=0.5, horizon=10, max_steps=12, seed=41, n_lanes=64)
        b.set_lane_env(alphas=ALPHAS, alpha_column=0, reward="sparse_relative", shape="per_alpha")
        b.set_policy_net(float_net(18, 2, 32, 32, extra=(0.375, 0.5)))
        return b

    T, n = 32, 64
    opts = P.PPOOptions(n_epochs=2, minibatch=256, ent_coef=0.01, lr=1e-3)
    b, twin = make(), make()
    for it in range(2):  # the second iteration continues from the lanes' state
        with fused_kernel():
            s, st = b.ppo_iterate(T, opts)
        assert last_rollout_fused(b) == 1
        with launch_sequence():
            s2, a = twin.rollout_net(T, deterministic=False)
        obs = np.concatenate([a["obs0"][None], a["obs"][:-1]]).reshape(T * n, -1)
        alpha = np.concatenate([a["alpha0"][None], a["alpha"][:-1]]).ravel()
        adv, ret = twin.gae(a["reward"], a["done"], a["value"], opts.gae_gamma, opts.gae_lambda)
        st2 = twin.ppo_update(dict(obs=obs, alpha=alpha, action=a["action"].ravel(),
                                   old_logp=a["logp"].ravel(), advantage=adv.ravel(),
                                   ret=ret.ravel()), opts)
        assert bytes(s) == bytes(s2), it
        assert s.steps == T * n and s.episodes > 0
        assert st == st2, it
        assert st["n_minibatches"] == 2 * 8
        assert _weights(b).tobytes() == _weights(twin).tobytes(), it
        assert np.any(a["done"]) and np.any(a["reward"] != 0)
    assert np.any(_weights(b) != P.flatten_params(b._net))


# ------------------------------------------------ 5. evaluation against fused episodes

def _fused_records(ctx, table, alpha, seed, n):
    cfg, keep = device.make_config(protocol=L.PROTO_FC16_ENV, alpha=alpha, gamma=0.5, horizon=10,
                                   max_steps=60, seed=seed, table=table)
    return device.Batch(cfg, ctx=ctx, keep=keep).run(n, records=True)[1]


def _check_records(ev, rec, sel, what):
    for a, b in (("reward_attacker", "reward_attacker"), ("episode_progress", "progress"),
                 ("episode_n_steps", "n_steps"), ("status", "status")):
        assert np.array_equal(ev[a][sel], rec[b][sel]), (what, a)


def test_evaluation_equals_fused_episodes_of_the_networks_table(ctx):
    E, seed = 512, 77
    net = float_net(12, 2, 32, 16)
    b = _batch(ctx, alpha=0.35, gamma=0.5, horizon=10, max_steps=60, seed=seed, n_lanes=96)
    b.set_policy_net(net)
    ev = b.evaluate_net(E, deterministic=True).records
    table = mdp.fc16_table_from_net(net, 62, ctx=ctx)
    assert table.shape == (62 * 62 * 3,) and len(np.unique(table)) >= 3
    rec = _fused_records(ctx, table, 0.35, seed, E)
    _check_records(ev, rec, slice(None), "one alpha")
    assert np.array_equal(ev["episode"], np.arange(E))
    assert (rec["status"] & L.ST_CAPACITY).any() and not (rec["status"] & L.ST_CAPACITY).all()


def test_evaluation_per_alpha_equals_one_table_batch_per_alpha(ctx):
    E, seed = 512, 78
    net = float_net(14, 2, 32, 16, extra=(0.0, 0.5))
    b = _batch(ctx, alpha=0.35, gamma=0.5, horizon=10, max_steps=60, seed=seed, n_lanes=96)
    b.set_lane_env(alphas=ALPHAS, alpha_column=0, schedule="cycle")
    b.set_policy_net(net)
    ev = b.evaluate_net(E // 3 + 1, deterministic=True).records[:E]
    assert np.array_equal(ev["alpha_index"], np.arange(E) % 3)
    tables = []
    for j, alpha in enumerate(ALPHAS):
        # the network sees (float)alpha in column 0, as the lane env feeds it
        tables.append(mdp.fc16_table_from_net(net, 62, extra=(alpha, 0.5), ctx=ctx))
        rec = _fused_records(ctx, tables[j], alpha, seed, E)
        _check_records(ev, rec, np.arange(E) % 3 == j, alpha)
    assert any(not np.array_equal(tables[0], t) for t in tables[1:])


# ------------------------------------------------------------------ 6. refusals

def test_refusals(ctx):
    b = _batch(ctx, alpha=0.35, gamma=0.5, horizon=10, max_steps=20, seed=1, n_lanes=8)
    with pytest.raises(L.CprError) as e:
        b.rollout(4)
    assert e.value.code == L.CPR_E_UNSUPPORTED and "cpr_rollout_net" in str(e.value)
    with pytest.raises(L.CprError) as e:
        b.policy_actions(0, np.zeros((1, 3)))
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
    b.reset()
    for bad in (4, -1):
        with pytest.raises(L.CprError) as e:
            b.step(np.array([0, 1, 2, 3, bad, 0, 0, 0], dtype=np.int32))
        assert e.value.code == L.CPR_E_INVALID_ARG
    # the env wrapper: gymnasium's call shape, truncation from the capacity status
    from cpr_amd import envs

    env = envs.FC16SSZwPT(alpha=0.35, gamma=0.5, horizon=1000, max_steps=5, seed=3, ctx=ctx)
    ref = R.Fc16EnvRef(3, 0.35, 0.5, 1000, 5)
    obs, info = env.reset()
    assert info == {} and list(obs) == ref.reset(0)
    for t in range(5):
        obs, r, term, trunc, info = env.step(t % 4)
        assert (list(obs), r, term, trunc) == ref.step(t % 4) and info == {}
    assert trunc and not term
    assert list(env.reset()[0]) == ref.reset(1)


def test_device_env_fn_builds_the_env_with_the_lane_env(ctx):
    from cpr_amd import envs

    b, extras = envs.device_env_fn(70, ctx=ctx, seed=9, protocol="fc16",
                                   protocol_args=dict(horizon=10), episode_len=12,
                                   alpha=ALPHAS, gamma=0.5, reward="sparse_relative")
    assert b.config.protocol == L.PROTO_FC16_ENV and b.config.horizon == 10.0
    assert b.config.max_steps == 12 and extras == (ALPHAS[0], 0.5)
    b.set_policy_net(float_net(18, 1, 16, 16, extra=extras))
    s, A = b.rollout_net(30, deterministic=False)
    assert last_rollout_fused(b) == 0  # the one-kernel path is off unless asked for
    assert set(np.unique(A["alpha"])) == set(ALPHAS) and s.steps == 30 * 70
    # the alpha an episode runs at follows the keyed choice of lane_env_ref
    import lane_env_ref

    assert np.array_equal(A["alpha0"], [ALPHAS[lane_env_ref.alpha_index(9, e, 3)]
                                        for e in range(70)])
    with pytest.raises(ValueError):
        envs.device_env_fn(8, ctx=ctx, protocol="fc16", reward="dense_per_progress")
