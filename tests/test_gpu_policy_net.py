"""Neural-network policies on the device (k_policy_forward, cpr_rollout_net) — needs an MI355X.

1. the forward against a numpy float64 forward, within the f32 dot-product error bound
   propagated through the layers;
2. integer weights and raw observations, where f32 arithmetic is exact: a whole rollout
   against oracle gym envs driven by the same integer network, bit for bit;
3. float weights, sampled actions, all four protocols: the rollout against the forward entry,
   the sampling rule, a host-driven replay through Batch.step and the summary rule;
4. refusals.
"""

import functools

import numpy as np
import pytest

import oracle_py as O
from cpr_amd import _lib as L
from cpr_amd import device

pytestmark = pytest.mark.gpu

PROTO = {
    "nakamoto": dict(protocol=L.PROTO_NAKAMOTO),
    "bk": dict(protocol=L.PROTO_BK, k=2),
    "ethereum": dict(protocol=L.PROTO_ETHEREUM, reward_scheme=L.REWARD_DISCOUNT),
    "tailstorm": dict(protocol=L.PROTO_TAILSTORM, k=2, reward_scheme=L.REWARD_DISCOUNT,
                      subblock_selection=L.SELECT_HEURISTIC),
}
SHAPE = {"nakamoto": (4, 4), "bk": (8, 8), "ethereum": (10, 24), "tailstorm": (10, 8)}
ENV = {"nakamoto": O.GymEnv, "bk": O.BkGymEnv, "ethereum": O.EthGymEnv, "tailstorm": O.TsGymEnv}


@pytest.fixture(scope="module")
def ctx():
    return device.default_context()


def _batch(ctx, proto, **kw):
    cfg, keep = device.make_config(**dict(PROTO[proto], **kw))
    return cfg, device.Batch(cfg, ctx=ctx, keep=keep)


def float_net(seed, n_in, depth, wpi, wvf, n_act, extra=()):
    """Gaussian weights scaled 1/sqrt(fan_in): asymmetric, so an operand or C-write swap shows."""
    rng = np.random.default_rng(seed)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    def trunk(w):
        return [lin(w, n_in if i == 0 else w) for i in range(depth)]

    return device.PolicyNet(pi=trunk(wpi), pi_head=lin(n_act, wpi), vf=trunk(wvf),
                            vf_head=lin(1, wvf), extra=extra)


def forward_with_bound(net, obs):
    """(logits, value, logits bound, value bound) in float64: the reference forward on the
    f32-rounded inputs and, per output, the standard f32 dot-product bound propagated through
    the layers: err_out <= |W| err_in + gamma_{K+1} (|W| (|x| + err_in) + |b|), gamma_k =
    k 2^-24 / (1 - k 2^-24); ReLU is 1-Lipschitz."""
    u = 2.0 ** -24
    x = np.asarray(obs, dtype=np.float64).astype(np.float32).astype(np.float64)
    x = np.concatenate([x, np.tile(np.float32(net.extra).astype(np.float64), (len(x), 1))], axis=1)
    outs = []
    for trunk, head in ((net.pi, net.pi_head), (net.vf, net.vf_head)):
        h, e = x, np.zeros_like(x)
        layers = [(w, b, True) for w, b in trunk] + [(head[0], head[1], False)]
        for w, b, relu in layers:
            W, B = w.astype(np.float64), b.astype(np.float64)
            k = W.shape[1] + 1
            gam = k * u / (1 - k * u)
            y = h @ W.T + B
            e = e @ np.abs(W).T + gam * ((np.abs(h) + e) @ np.abs(W).T + np.abs(B))
            h = np.maximum(y, 0.0) if relu else y
        outs.append((h, e))
    return outs[0][0], outs[1][0][:, 0], outs[0][1], outs[1][1][:, 0]


def softmax_f64(logits):
    """(m, e, S) of the kernel's epilogue, S summed in index order."""
    lg = logits.astype(np.float64)
    m = lg.max(axis=-1, keepdims=True)
    e = np.exp(lg - m)
    S = np.zeros(lg.shape[:-1])
    for i in range(lg.shape[-1]):
        S = S + e[..., i]
    return m[..., 0], e, S


# ------------------------------------------------------------------ 1. forward against float64

@pytest.fixture(scope="module")
def obs_pool(ctx):
    """Per protocol: a batch and 257 observation rows (what reset and a few steps return,
    plus random rows within the unit observation box)."""
    pool = {}
    for proto in ("nakamoto", "bk", "ethereum"):
        cfg, b = _batch(ctx, proto, alpha=0.4, gamma=0.5, max_steps=64, seed=17, n_lanes=48)
        rng = np.random.default_rng(3)
        rows = [rng.random((257 - 4 * 48, SHAPE[proto][0])), b.reset()]
        for _ in range(3):
            rows.append(b.step(rng.integers(0, SHAPE[proto][1], size=48))[0])
        pool[proto] = (b, np.concatenate(rows))
        assert pool[proto][1].shape == (257, SHAPE[proto][0])
    return pool


@pytest.mark.parametrize("widths", [(16, 16), (48, 64), (256, 256)])
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("n_extra", [0, 2])
@pytest.mark.parametrize("proto", ["nakamoto", "bk", "ethereum"])
def test_forward_within_f32_bound_of_float64(obs_pool, proto, n_extra, depth, widths):
    b, rows = obs_pool[proto]
    ol, na = SHAPE[proto]
    net = float_net(100 + depth + widths[0], ol + n_extra, depth, widths[0], widths[1], na,
                    extra=(0.375, 0.7)[:n_extra])
    b.set_policy_net(net)
    for n in (1, 31, 64, 257):
        obs = rows[257 - n:]  # the lanes' observations; at 257 the random rows too
        act, logp, val, lg = b.policy_net_forward(obs, deterministic=True, logits=True)
        rl, rv, el, ev = forward_with_bound(net, obs)
        dl, dv = np.abs(lg.astype(np.float64) - rl), np.abs(val - rv)
        print(f"{proto} extra {n_extra} depth {depth} widths {widths} n {n}: "
              f"logit err/bound max {np.max(dl / el):.3f}, value {np.max(dv / ev):.3f}")
        assert np.all(dl <= el), (n, np.argwhere(dl > el)[0], dl.max(), el.max())
        assert np.all(dv <= ev), (n, np.argwhere(dv > ev)[0], dv.max(), ev.max())
        # the epilogue, from the device's own logits
        assert np.array_equal(act, np.argmax(lg, axis=1))  # numpy: the first maximum
        m, e, S = softmax_f64(lg)
        ref_logp = lg[np.arange(n), act].astype(np.float64) - m - np.log(S)
        assert np.allclose(logp, ref_logp, rtol=1e-12, atol=0.0)


# ------------------------------------------------------ 2. exact integers against the oracle

def int_net(seed, n_in, n_act, extra):
    rng = np.random.default_rng(seed)

    def lin(n_out, fan_in):
        return (rng.integers(-1, 2, size=(n_out, fan_in)).astype(np.float32),
                rng.integers(-1, 2, size=n_out).astype(np.float32))

    def trunk():
        return [lin(32, n_in if i == 0 else 32) for i in range(3)]

    return device.PolicyNet(pi=trunk(), pi_head=lin(n_act, 32), vf=trunk(), vf_head=lin(1, 32),
                            extra=extra)


def magnitude_bound(net, x):
    """max over layers and rows of sum |w||x| + |b| (an upper bound of every partial sum)."""
    x = np.abs(np.concatenate([x, np.tile(np.abs(net.extra), (len(x), 1))], axis=1))
    worst = 0.0
    for trunk, head in ((net.pi, net.pi_head), (net.vf, net.vf_head)):
        h = x
        for w, b in list(trunk) + [head]:
            h = h @ np.abs(w.astype(np.float64)).T + np.abs(b.astype(np.float64))
            worst = max(worst, h.max())
    return worst


EXACT = {
    # (config, weight seed chosen on the CPU so that the reference run is non-trivial)
    "nakamoto": (dict(alpha=0.33, gamma=0.5, max_steps=32, propagation_delay=0.05, seed=2024,
                      unit_observation=False, n_lanes=32), 3),
    "bk": (dict(alpha=0.33, gamma=0.5, max_steps=32, seed=2024, unit_observation=False,
                n_lanes=32), 2),
}
EXTRA_INT = (1.0, -2.0)


@functools.lru_cache(maxsize=None)
def exact_reference(proto, T=96):
    kw, wseed = EXACT[proto]
    cfg, _ = device.make_config(**dict(PROTO[proto], **kw))
    n, (ol, na) = kw["n_lanes"], SHAPE[proto]
    net = int_net(wseed, ol + 2, na, EXTRA_INT)
    R = dict(obs0=np.zeros((n, ol)), obs=np.zeros((T, n, ol)), action=np.zeros((T, n), np.int32),
             reward=np.zeros((T, n)), done=np.zeros((T, n), bool), value=np.zeros((T + 1, n)))
    diag = 0
    for i in range(n):
        ep = i
        env = ENV[proto](cfg, episode=ep)
        o = R["obs0"][i] = env.reset()
        for t in range(T):
            lg, v = net.forward_f64(o[None])
            a = int(np.argmax(lg[0]))  # the lowest index of the maximum
            R["value"][t, i], R["action"][t, i] = v[0], a
            o, r, d, _ = env.step(a)
            if d:
                if proto == "nakamoto":
                    diag |= env.diag()
                ep += n
                env = ENV[proto](cfg, episode=ep)
                o = env.reset()
            R["obs"][t, i], R["reward"][t, i], R["done"][t, i] = o, r, d
        R["value"][T, i] = net.forward_f64(o[None])[1][0]
        if proto == "nakamoto":
            diag |= env.diag()
    return net, R, diag


@pytest.mark.parametrize("proto", ["nakamoto", "bk"])
def test_integer_network_rollout_equals_oracle_bit_for_bit(ctx, proto):
    T = 96
    net, R, diag = exact_reference(proto, T)
    # preconditions: integer observations; every partial sum below 2^24, so that f32
    # arithmetic is exact in any order
    inputs = np.concatenate([R["obs0"][None], R["obs"]]).reshape(-1, SHAPE[proto][0])
    assert np.array_equal(inputs, np.rint(inputs))
    assert magnitude_bound(net, inputs) < 2 ** 24
    # the reference run is not trivial
    assert len(np.unique(R["action"])) >= 3
    assert R["done"].any()
    if proto == "nakamoto":
        assert diag & 2  # DIAG_OVERLAP: a lane left the closed form
    kw, _ = EXACT[proto]
    _, b = _batch(ctx, proto, **kw)
    b.set_policy_net(net)
    s, got = b.rollout_net(T, deterministic=True)
    for f in ("obs0", "obs", "action", "reward", "done", "value"):
        bad = np.argwhere(got[f] != R[f])
        assert len(bad) == 0, (f, bad[0], got[f][tuple(bad[0])], R[f][tuple(bad[0])])
    assert s.steps == T * kw["n_lanes"] and s.episodes == int(R["done"].sum())
    # greedy actions have probability <= 1
    assert np.all(got["logp"] <= 0.0) and np.all(np.isfinite(got["logp"]))


# ------------------------------------------- 3. rollout consistency, float weights, sampling

CONSIST = dict(alpha=0.4, gamma=0.5, max_steps=20, seed=99, n_lanes=32)
SUM_FIELDS = ["episodes", "steps", "reward_attacker_fx", "reward_defender_fx", "progress_fx",
              "rel_revenue_fx", "rel_revenue_sq_fx", "orphans", "status_tie", "status_overlap",
              "status_other", "invalid"]


def consist_net(proto):
    ol, na = SHAPE[proto]
    return float_net(7, ol + 2, 2, 48, 32, na, extra=(0.4, 0.5))


@pytest.mark.parametrize("proto", ["nakamoto", "bk", "ethereum", "tailstorm"])
def test_sampled_rollout_is_consistent(ctx, proto):
    n, T = 32, 64
    ol, na = SHAPE[proto]
    net = consist_net(proto)
    cfg, b = _batch(ctx, proto, **CONSIST)
    b.set_policy_net(net)
    sa, A = b.rollout_net(40, deterministic=False)
    sb, B = b.rollout_net(24, deterministic=False)
    assert np.array_equal(B["obs0"], A["obs"][-1])  # the second call continues the first
    assert np.array_equal(B["value"][0], A["value"][40])
    G = {k: np.concatenate([A[k], B[k]]) for k in ("obs", "action", "reward", "done", "logp")}
    G["value"] = np.concatenate([A["value"][:40], B["value"]])
    done = G["done"]
    assert done.any() and len(np.unique(G["action"])) >= 3

    # (a) the forward entry on the rollout's own policy inputs
    X = np.concatenate([A["obs0"][None], G["obs"]])  # X[t] = input of step t; X[T] = final
    _, _, val, lg = b.policy_net_forward(X.reshape(-1, ol), logits=True)
    assert np.array_equal(val.reshape(T + 1, n), G["value"])
    lg = lg.reshape(T + 1, n, na)[:T]
    # its sampled mode draws row r at (episode episode0 + r, step 0): the rollout's first step
    a0, lp0, _ = b.policy_net_forward(A["obs0"], deterministic=False, episode0=0)
    assert np.array_equal(a0, G["action"][0]) and np.array_equal(lp0, G["logp"][0])

    # (b) the sampling rule, recomputed in float64 from the device's logits
    ep = np.zeros((T, n), dtype=np.uint64)
    step = np.zeros((T, n), dtype=np.int64)
    u = np.zeros((T, n))
    for i in range(n):
        e, t0 = i, 0
        for t in range(T + 1):
            if t == T or done[t, i]:  # steps t0 .. t are one episode's, indices 0 ..
                if t0 <= min(t, T - 1):
                    cnt = min(t, T - 1) - t0 + 1
                    w = ctx.stream_fill(cfg.seed, e, 0, L.TAG_POLICY, cnt)
                    u[t0:t0 + cnt, i] = [O.u53(int(a), int(c)) for a, c in w[:, :2]]
                    ep[t0:t0 + cnt, i], step[t0:t0 + cnt, i] = e, np.arange(cnt)
                e, t0 = e + n, t + 1
    m, e, S = softmax_f64(lg)
    cdf = np.cumsum(e, axis=-1)  # sequential, index order
    below = (u * S)[..., None] < cdf
    expect = np.where(below.any(axis=-1), below.argmax(axis=-1), na - 1)
    near = (np.abs((u * S)[..., None] - cdf) <= 1e-9 * S[..., None]).any(axis=-1)
    assert near.mean() <= 1e-3
    bad = np.argwhere((expect != G["action"]) & ~near)
    assert len(bad) == 0, (bad[0], expect[tuple(bad[0])], G["action"][tuple(bad[0])])
    tt, ii = np.meshgrid(np.arange(T), np.arange(n), indexing="ij")
    ref_logp = lg[tt, ii, G["action"]].astype(np.float64) - m - np.log(S)
    assert np.allclose(G["logp"], ref_logp, rtol=1e-12, atol=0.0)

    # (c) a second batch driven through Batch.step with the reported actions
    _, b2 = _batch(ctx, proto, **CONSIST)
    obs = b2.reset()
    assert np.array_equal(obs, A["obs0"])
    ids = np.arange(n, dtype=np.uint64)
    finished = []
    for t in range(T):
        obs, rew, d, info = b2.step(G["action"][t])
        if d.any():
            finished += [{k: v[i] for k, v in info.items()} for i in np.flatnonzero(d)]
            ids[d] += n
            obs = b2.reset(mask=d, episode_ids=ids)
        assert np.array_equal(obs, G["obs"][t]), t
        assert np.array_equal(rew, G["reward"][t]), t
        assert np.array_equal(d, done[t]), t

    # (d) the summary: summary.h's fixed-point rule over the finished episodes' step infos
    want = dict.fromkeys(SUM_FIELDS, 0)
    hist = [0] * L.HIST_BINS
    want["steps"] = T * n
    for f in finished:
        ra, rd = float(f["episode_reward_attacker"]), float(f["episode_reward_defender"])
        acts, st = int(f["episode_n_activations"]), int(f["status"])
        assert not st & L.ST_INVALID
        rel = ra / (ra + rd) if ra + rd != 0 else 0.0
        height = f["episode_progress"] if proto in ("bk", "tailstorm") else f["head_height"]
        want["episodes"] += 1
        want["reward_attacker_fx"] += int(np.rint(ra * 2 ** 20))
        want["reward_defender_fx"] += int(np.rint(rd * 2 ** 20))
        want["progress_fx"] += int(np.rint(float(f["episode_progress"]) * 2 ** 20))
        want["rel_revenue_fx"] += int(np.rint(rel * 2 ** 32))
        want["rel_revenue_sq_fx"] += int(np.rint(rel * rel * 2 ** 32))
        want["orphans"] += acts - int(height)
        want["status_tie"] += 1 if st & L.ST_TIE else 0
        want["status_overlap"] += 1 if st & L.ST_OVERLAP else 0
        want["status_other"] += 1 if st & ~(L.ST_TIE | L.ST_OVERLAP | L.ST_EXACT_RERUN) else 0
        hist[min(L.HIST_BINS - 1, max(0, int(rel * L.HIST_BINS)))] += 1
    assert want["episodes"] == int(done.sum())
    for f in SUM_FIELDS:
        assert getattr(sa, f) + getattr(sb, f) == want[f], f
    assert [x + y for x, y in zip(sa.hist, sb.hist)] == hist
    assert sa.activations + sb.activations > 0


@pytest.mark.parametrize("proto", ["nakamoto", "bk"])
def test_rollout_net_interleaves_with_rollout_and_step(ctx, proto):
    n = 32
    ol, na = SHAPE[proto]
    net = consist_net(proto)
    cfg, b = _batch(ctx, proto, **CONSIST)
    b.set_policy_net(net)
    _, o1, r1, d1 = b.rollout(10, outputs=True)  # the built-in policy
    _, N = b.rollout_net(30, deterministic=True)
    assert np.array_equal(N["obs0"], o1[-1])
    o3, r3, d3, _ = b.step(np.full(n, na - 1, dtype=np.int32))
    got_obs = np.concatenate([o1, N["obs"], o3[None]])
    got_rew = np.concatenate([r1, N["reward"], r3[None]])
    got_done = np.concatenate([d1, N["done"], d3[None]])
    assert N["done"].any()
    # the same sequence through step alone
    _, b2 = _batch(ctx, proto, **CONSIST)
    b2.set_policy_net(net)
    obs = b2.reset()
    ids = np.arange(n, dtype=np.uint64)
    for t in range(41):
        if t < 10:
            a = b2.policy_actions(cfg.policy, obs)
        elif t < 40:
            a = b2.policy_net_forward(obs, deterministic=True)[0]
            assert np.array_equal(a, N["action"][t - 10])
        else:
            a = np.full(n, na - 1, dtype=np.int32)
        obs, rew, d, _ = b2.step(a)
        if d.any() and t < 40:  # the rollouts reset finished lanes, step does not
            ids[d] += n
            obs = b2.reset(mask=d, episode_ids=ids)
        assert np.array_equal(obs, got_obs[t]), t
        assert np.array_equal(rew, got_rew[t]) and np.array_equal(d, got_done[t]), t


# ------------------------------------------------------------------------------ 4. refusals

def test_rollout_net_before_set_policy_net_is_a_state_error(ctx):
    _, b = _batch(ctx, "nakamoto", **CONSIST)
    with pytest.raises(L.CprError) as e:
        b.rollout_net(4)
    assert e.value.code == L.CPR_E_STATE
    with pytest.raises(L.CprError) as e:
        b.policy_net_forward(np.zeros((1, 4)))
    assert e.value.code == L.CPR_E_STATE


def test_width_512_beyond_the_lds_budget_is_refused_without_a_launch(ctx):
    _, b = _batch(ctx, "nakamoto", **CONSIST)
    # two hidden tiles of 64 rows x 512 units do not fit the CU's LDS: refused when set
    with pytest.raises(L.CprError) as e:
        b.set_policy_net(float_net(1, 4, 2, 512, 512, 4))
    assert e.value.code == L.CPR_E_UNSUPPORTED and "LDS" in str(e.value)
    with pytest.raises(L.CprError) as e:  # nothing was set, so nothing can launch
        b.rollout_net(4)
    assert e.value.code == L.CPR_E_STATE
    # one hidden layer needs one tile, which fits: the widest supported configuration
    net = float_net(2, 4, 1, 512, 16, 4)
    b.set_policy_net(net)
    obs = np.random.default_rng(0).random((65, 4))
    _, _, val, lg = b.policy_net_forward(obs, logits=True)
    rl, rv, el, ev = forward_with_bound(net, obs)
    assert np.all(np.abs(lg - rl) <= el) and np.all(np.abs(val - rv) <= ev)


def test_fc16_batch_is_unsupported(ctx):
    cfg, keep = device.make_config(alpha=0.3, gamma=0.5, protocol=L.PROTO_FC16, max_steps=100,
                                   policy=L.FC16_POLICY_HONEST, n_lanes=4)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    net = float_net(1, 3, 1, 16, 16, 4)
    with pytest.raises(L.CprError) as e:
        import ctypes

        L.check(L.lib().cpr_policy_net_set(b.handle, ctypes.byref(net.cstruct())))
    assert e.value.code == L.CPR_E_UNSUPPORTED
    with pytest.raises(L.CprError) as e:
        b.rollout_net(4)
    assert e.value.code == L.CPR_E_UNSUPPORTED


def test_set_policy_net_names_the_wrong_shape(ctx):
    _, b = _batch(ctx, "bk", **CONSIST)
    with pytest.raises(ValueError, match="input width 9"):
        b.set_policy_net(float_net(1, 9, 1, 16, 16, 8, extra=(0.5, 0.5)))
    with pytest.raises(ValueError, match="pi_head: 4 actions"):
        b.set_policy_net(float_net(1, 8, 1, 16, 16, 4))
    b.set_policy_net(float_net(1, 8, 1, 16, 16, 8))
    with pytest.raises(ValueError, match=r"obs: expected \[n, 8\]"):
        b.policy_net_forward(np.zeros((3, 4)))
