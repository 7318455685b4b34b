"""Q-learning on the device (cpr_dqn_*; DESIGN.md §4.14 "Q-learning") — needs an MI355X.

 1. epsilon = 0: dqn_collect is rollout_net(deterministic=True) bit for bit, and the ring holds
    exactly those rows;
 2. epsilon = 1 and 0.3: every action is the restated random draw or the greedy action, as the
    restated coin says;
 3. chunking: 40 steps equal 13 + 27;
 4. the ring wraps, and nothing is written behind it;
 5. sampling: the keyed indices, a caller's indices, never an unwritten slot;
 6. the minibatch gradient against torch's float64 autograd of dqn_ref.dqn_loss: per parameter
    tensor the device's relative L2 error may be at most 8x the error of torch's own float32
    CPU autograd on the same inputs (the learner's measure, tests/test_gpu_ppo.py); the vf
    trunk's gradient is exactly zero;
 7. calls repeat bit for bit;
 8. an update equals hand-driven steps of gradient, clip and Adam;
 9. the target's Polyak update bit for bit;
10. dqn_iterate equals collect -> (sync) -> (update) by hand;
11. evaluation and the FC16 table after training;
12. refusals.

Lanes are 96 or 100 (no multiple of 64), n_steps 40. Hidden widths are multiples of 16
(cpr_policy_net_set), so the narrow single-layer network runs at widths 16 and 32, the two
neighbours of 24 that the library accepts. Measured gradient errors (worst device / torch-f32
ratio per network) go to profiles/dqn_grad_error.json (CPR_DQN_GRAD_ERROR_OUT).
"""

import ctypes
import json
import os

import numpy as np
import pytest
import torch

import dqn_ref
import ppo_ref
from cpr_amd import _lib as L
from cpr_amd import device, mdp
from cpr_amd import dqn as Q
from cpr_amd import ppo as P

pytestmark = pytest.mark.gpu

PROTO = {
    "fc16": dict(protocol=L.PROTO_FC16_ENV, policy=L.FC16_POLICY_HONEST, horizon=10),
    "nakamoto": dict(protocol=L.PROTO_NAKAMOTO),
    "bk": dict(protocol=L.PROTO_BK, k=2),
}
ALPHAS = [0.15, 0.2, 0.3, 0.4, 0.45]
EXTRA = (0.375, 0.7)
SEED = 0x5EED000000D0
T = 40


@pytest.fixture(scope="module")
def ctx():
    return device.default_context()


def float_net(seed, n_in, depth, wpi, wvf, n_act, extra=(), tie=False):
    """Gaussian weights scaled 1/sqrt(fan_in); ``tie``: the head's rows 0 and 1 are equal, so
    that Q(s, 0) = Q(s, 1) for every s."""
    rng = np.random.default_rng(seed)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    def trunk(w):
        return [lin(w, n_in if i == 0 else w) for i in range(depth)]

    pi, head = trunk(wpi), lin(n_act, wpi)
    if tie:
        head[0][1], head[1][1] = head[0][0], head[1][0]
    return device.PolicyNet(pi=pi, pi_head=head, vf=trunk(wvf), vf_head=lin(1, wvf), extra=extra)


def make(ctx, proto, n_lanes=96, seed=SEED, env=False, arch=(2, 32, 48), capacity=None,
         net_seed=3, tie=False, max_steps=12):
    cfg, keep = device.make_config(**dict(PROTO[proto], alpha=0.35, gamma=0.5, max_steps=max_steps,
                                          seed=seed, n_lanes=n_lanes))
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    if env:
        b.set_lane_env(alphas=ALPHAS, alpha_column=0, reward="sparse_relative", shape="per_alpha")
    ol, na = b.observation_spec()[:2]
    b.set_policy_net(float_net(net_seed, ol + len(EXTRA), *arch, na, EXTRA, tie=tie))
    if capacity is not None:
        b.dqn_init(capacity)
    return b


def weights(b):
    return P.flatten_params(b.get_policy_net())


def n_pi(net):
    """parameters of the pi trunk and its head: the Q-network, first in the flat order"""
    return sum(a.size for _, a in P.param_arrays(net)[:2 * (net.depth + 1)])


def target_weights(b):
    return P.flatten_params(b.get_target_net())


def same_replay(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in device.Batch.DQN_DATA)


def lane_keys(done, n):
    """(episode, episode step index before the step) of every (t, lane) of a fresh batch's
    first T steps, from the done flags: lane i starts at episode i and moves on by n."""
    ep = np.zeros(done.shape, dtype=np.uint64)
    st = np.zeros(done.shape, dtype=np.int64)
    e, s = np.arange(n, dtype=np.uint64), np.zeros(n, dtype=np.int64)
    for t in range(done.shape[0]):
        ep[t], st[t] = e, s
        d = done[t].astype(bool)
        e = np.where(d, e + np.uint64(n), e)
        s = np.where(d, 0, s + 1)
    return ep, st


CASES = [("fc16", False), ("nakamoto", False), ("bk", True)]


# ------------------------------------------------------------------ 1. epsilon = 0

@pytest.mark.parametrize("proto,env", CASES)
def test_greedy_collect_is_the_deterministic_rollout(ctx, proto, env):
    b = make(ctx, proto, env=env, capacity=T)
    twin = make(ctx, proto, env=env)
    s = b.dqn_collect(T, 0.0)
    assert not b.rollout_net_fused()
    s2, a = twin.rollout_net(T, deterministic=True)
    assert bytes(s) == bytes(s2)
    assert s.steps == T * 96 and s.episodes > 0
    rep = b.dqn_replay()
    assert b.dqn_replay_state() == (T, 0, T)
    inputs = np.concatenate([a["obs0"][None], a["obs"][:-1]])
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    assert np.array_equal(rep["obs"], f32(inputs))
    assert np.array_equal(rep["next_obs"], f32(a["obs"]))
    assert np.array_equal(rep["action"], a["action"])
    assert np.array_equal(rep["reward"], a["reward"])
    assert np.array_equal(rep["done"].astype(bool), a["done"])
    assert a["done"].any() and (a["reward"] != 0).any()
    if env:
        alpha = np.concatenate([a["alpha0"][None], a["alpha"][:-1]])
        assert np.array_equal(rep["alpha"], alpha) and len(np.unique(alpha)) == len(ALPHAS)
    else:
        assert np.all(rep["alpha"] == 0.35)
    # the stored input gives the Q-values of the original row bit for bit
    lg0 = b.policy_net_forward(inputs.reshape(-1, b.obs_len), logits=True)[3]
    lg1 = b.policy_net_forward(rep["obs"].reshape(-1, b.obs_len), logits=True)[3]
    assert lg0.tobytes() == lg1.tobytes()
    # ... and the lanes stand where the rollout left them
    n1, n2 = b.rollout_net(3, deterministic=True)[1], twin.rollout_net(3, deterministic=True)[1]
    assert all(n1[k].tobytes() == n2[k].tobytes() for k in n1)


# ------------------------------------------------------------------ 2. epsilon > 0

@pytest.mark.parametrize("proto,env,eps", [c + (1.0,) for c in CASES] +
                         [("fc16", False, 0.3), ("nakamoto", False, 0.3), ("bk", False, 0.3)])
def test_exploration_follows_the_restated_draws(ctx, proto, env, eps):
    n = 100
    b = make(ctx, proto, n_lanes=n, env=env, capacity=T)
    b.dqn_collect(T, eps)
    rep = b.dqn_replay()
    na = b.observation_spec()[1]
    ep, st = lane_keys(rep["done"], n)
    u1 = np.zeros((T, n))
    rnd = np.zeros((T, n), dtype=np.int32)
    for t in range(T):
        for i in range(n):
            u1[t, i], rnd[t, i] = dqn_ref.explore(SEED, ep[t, i], st[t, i], na)
    coin = u1 < eps
    if eps == 1.0:
        assert coin.all()
        want = rnd
    else:
        greedy = b.policy_net_forward(rep["obs"].reshape(-1, b.obs_len),
                                      deterministic=True)[0].reshape(T, n)
        want = np.where(coin, rnd, greedy)
        assert coin.any() and not coin.all()  # of the restatement: both kinds are checked
        assert (rnd != greedy)[coin].any()
    assert np.array_equal(rep["action"], want)
    assert rep["done"].any() and len(np.unique(rnd)) == na


# ------------------------------------------------------------------ 3. chunking

@pytest.mark.parametrize("proto,env", [("nakamoto", False), ("bk", True)])
def test_chunked_collect_changes_nothing(ctx, proto, env):
    one, two = (make(ctx, proto, env=env, capacity=T) for _ in range(2))
    s1 = one.dqn_collect(T, 0.3)
    s2 = L.Summary()
    two.dqn_collect(13, 0.3, summary=s2)
    assert two.dqn_replay_state() == (13, 13, T)
    two.dqn_collect(27, 0.3, summary=s2)
    assert one.dqn_replay_state() == two.dqn_replay_state() == (T, 0, T)
    assert same_replay(one.dqn_replay(), two.dqn_replay())
    for f in ("episodes", "steps", "reward_attacker_fx", "reward_defender_fx", "progress_fx"):
        assert getattr(s1, f) == getattr(s2, f), f
    n1, n2 = one.rollout_net(3, deterministic=True)[1], two.rollout_net(3, deterministic=True)[1]
    assert all(n1[k].tobytes() == n2[k].tobytes() for k in n1)


# ------------------------------------------------------------------ 4. ring wrap

def test_ring_wraps_and_writes_nothing_behind_it(ctx):
    cap = 16
    b = make(ctx, "fc16", capacity=cap)
    full = make(ctx, "fc16", capacity=T)
    guard0 = b.dqn_replay(cap, 1)
    assert np.all(guard0["done"] == 0xA5)
    assert guard0["action"].tobytes() == b"\xa5" * guard0["action"].nbytes
    b.dqn_collect(T, 0.3)
    full.dqn_collect(T, 0.3)
    assert b.dqn_replay_state() == (cap, T % cap, cap)
    ring, hist = b.dqn_replay(0, cap), full.dqn_replay()
    for s in range(cap):
        step = 24 + ((s - 24) % cap)
        for k in device.Batch.DQN_DATA:
            assert ring[k][s].tobytes() == hist[k][step].tobytes(), (s, k)
    assert same_replay(guard0, b.dqn_replay(cap, 1))
    with pytest.raises(L.CprError) as e:
        b.dqn_replay(cap, 2)
    assert e.value.code == L.CPR_E_INVALID_ARG


# ------------------------------------------------------------------ 5. sampling

def test_sampling_is_the_keyed_stream(ctx):
    cap, filled, n = 16, 10, 96
    opts = Q.DQNOptions(batch=65, gradient_steps=3, sample_seed=5, lr=1e-3)

    def fresh():
        b = make(ctx, "nakamoto", capacity=cap)
        b.dqn_collect(filled, 1.0)
        return b

    b = fresh()
    for update in range(2):
        b.dqn_update(options=opts)
        want = dqn_ref.sample_indices(SEED, 5, update, 3, 65, filled * n)
        assert np.array_equal(b.dqn_last_indices(3, 65), want)
        assert want.max() < filled * n  # never an unwritten slot
    assert len(np.unique(want // n)) == filled
    # a caller's indices are honoured: the same update from the restated draws, given by hand
    twin = fresh()
    for update in range(2):
        idx = dqn_ref.sample_indices(SEED, 5, update, 3, 65, filled * n)
        twin.dqn_update(options=opts, idx=idx)
        assert np.array_equal(twin.dqn_last_indices(3, 65), idx)
    assert weights(b).tobytes() == weights(twin).tobytes()
    other = fresh()
    other.dqn_update(options=opts, idx=np.flip(idx, axis=1).copy())
    assert weights(other).tobytes() != weights(fresh()).tobytes()
    # an index into an unwritten slot is refused
    bad = idx.copy()
    bad[2, 64] = filled * n
    with pytest.raises(L.CprError) as e:
        twin.dqn_update(options=opts, idx=bad)
    assert e.value.code == L.CPR_E_INVALID_ARG


# ------------------------------------------------------------------ 6. gradient

NETS = {"1x16": (1, 16, 16), "1x32": (1, 32, 32), "2x64": (2, 64, 64), "3x64": (3, 64, 64),
        "2x256-64": (2, 256, 64)}
ROWS = (1, 63, 65, 130, 2113)
N_DATA = 2200
GAMMA = 0.97
GRAD_ERRORS = {}
GRAD_OVER = []


def rel_err(a, ref):
    """relative L2 error, absolute where the reference tensor vanishes"""
    n = np.linalg.norm(ref)
    return np.linalg.norm(a - ref) / (n if n >= 1e-30 else 1.0)


def trained_pair(ctx, proto, env, arch, net_seed):
    """A batch whose online network has moved away from its target (three large steps on a few
    collected transitions); the target's head has two equal rows, so its maximum is tied
    wherever one of them is the maximum."""
    b = make(ctx, proto, env=env, arch=arch, capacity=4, net_seed=net_seed, tie=True)
    start = P.flatten_params(b._net)
    b.dqn_collect(4, 1.0)
    b.dqn_update(options=Q.DQNOptions(batch=64, gradient_steps=3, lr=0.02, gamma=GAMMA))
    net, tgt = b.get_policy_net(), b.get_target_net()
    assert P.flatten_params(tgt).tobytes() == start.tobytes()
    k = n_pi(net)  # most of the Q-network has moved (units that never fire keep their weights)
    assert np.mean(P.flatten_params(net)[:k] != start[:k]) > 0.3
    return b, net, tgt


def transitions(b, net, tgt, seed, env):
    """N_DATA synthetic transitions whose rewards put a third of the rows at |delta| < 1, a
    third at delta > 1 and a third at delta < -1 (0.1 away from the kinks); a quarter done.
    Inputs of both signs, so that which action is the target's maximum depends on the row."""
    rng = np.random.default_rng(seed)
    ol, na = b.observation_spec()[:2]
    d = dict(obs=1.5 * rng.standard_normal((N_DATA, ol)),
             next_obs=1.5 * rng.standard_normal((N_DATA, ol)),
             action=rng.integers(0, na, N_DATA).astype(np.int32),
             done=(rng.random(N_DATA) < 0.25).astype(np.uint8))
    col = None
    if env:
        d["alpha"] = rng.choice(ALPHAS, N_DATA)
        col = 0
    x = ppo_ref.net_input(net, d["obs"], d.get("alpha"), col)
    xn = ppo_ref.net_input(net, d["next_obs"], d.get("alpha"), col)
    with torch.no_grad():
        q = ppo_ref.torch_forward(net, ppo_ref.torch_params(net, torch.float64),
                                  torch.tensor(x))[0].numpy()
        qn = ppo_ref.torch_forward(tgt, ppo_ref.torch_params(tgt, torch.float64),
                                   torch.tensor(xn))[0].numpy()
    grp = np.arange(N_DATA) % 3
    mag = rng.uniform(1.1, 3.0, N_DATA)
    want = np.where(grp == 0, rng.uniform(-0.9, 0.9, N_DATA), np.where(grp == 1, mag, -mag))
    qa = q[np.arange(N_DATA), d["action"]]
    d["reward"] = qa - want - GAMMA * qn.max(axis=1) * (1.0 - d["done"])
    return d, x, xn, qn, col


@pytest.mark.parametrize("netname,proto,env", [(k, "nakamoto", False) for k in NETS] +
                         [("2x64", "bk", True)])
def test_gradient_against_float64_autograd(ctx, netname, proto, env):
    arch = NETS[netname]
    b, net, tgt = trained_pair(ctx, proto, env, arch, 7 + sum(arch))
    data, x, xn, qn, col = transitions(b, net, tgt, 31, env)
    perm = np.random.default_rng(5).permutation(N_DATA)
    # The single row of B = 1 is a clamped one (delta > 1, not done). An unclamped row's whole
    # gradient is delta times the Jacobian of q_a, so at B = 1 every tensor's relative error
    # would be that of the one number delta = q_a - y: the ratio of two f32 forwards' rounding
    # noise at a single scalar (measured: 9.1x on 3x64, 1.0x - 3.5x on the other networks),
    # which measures neither. Unclamped rows are measured from B = 63 on.
    first = next(i for i in perm if i % 3 == 1 and not data["done"][i])
    perm = np.concatenate([[first], perm[perm != first]])
    sizes = [a.size for _, a in P.param_arrays(net)]
    names = [n for n, _ in P.param_arrays(net)]
    k_pi = n_pi(net)
    opts = Q.DQNOptions(gamma=GAMMA)
    worst, over = 0.0, []
    for B in ROWS:
        rows = perm[:B]
        assert B == 1 or not np.array_equal(rows, np.sort(rows))  # a real gather
        args = (x[rows], xn[rows], data["action"][rows], data["reward"][rows], data["done"][rows],
                GAMMA)
        s64, g64, info = dqn_ref.dqn_loss(net, tgt, *args, torch.float64)
        s32, g32, _ = dqn_ref.dqn_loss(net, tgt, *args, torch.float32)
        if B >= 63:  # the inputs reach every branch (asserted on the reference)
            dl = info["delta"]
            assert (np.abs(dl) < 0.95).any() and (dl > 1.05).any() and (dl < -1.05).any()
            assert not ((np.abs(np.abs(dl) - 1.0) < 0.05).any())
            assert data["done"][rows].any() and not data["done"][rows].all()
            top = np.sort(info["q_next"], axis=1)
            assert (top[:, -1] == top[:, -2]).any() and (top[:, -1] != top[:, -2]).any()
        grad, st = b.dqn_gradients(data, rows, opts)
        assert grad.dtype == np.float32 and grad.size == g64.size == sum(sizes)
        assert np.all(grad[k_pi:] == 0.0) and np.all(g64[k_pi:] == 0.0)  # the vf trunk
        o = 0
        for name, k in zip(names[:2 * (net.depth + 1)], sizes):
            ed = rel_err(grad[o:o + k].astype(np.float64), g64[o:o + k])
            et = rel_err(g32[o:o + k], g64[o:o + k])
            print(f"{proto} {netname} B {B} {name}: device {ed:.3e} torch-f32 {et:.3e} "
                  f"ratio {ed / et if et else float('inf') if ed else 0.0:.2f}")
            if et > 0:
                worst = max(worst, ed / et)
            if not ed <= 8 * et:  # every figure first; the assertion is at the end
                over.append(dict(case=f"{proto}/{netname}", rows=B, tensor=name, device=ed,
                                 torch_f32=et))
            o += k
        for key in ("loss", "abs_td", "q", "target", "grad_norm"):
            print(f"{proto} {netname} B {B} {key}: device {st[key]!r} f64 {s64[key]!r} "
                  f"torch-f32 {s32[key]!r}")
            tol = max(1e-5 * abs(s64[key]), 8 * abs(s32[key] - s64[key]))
            assert abs(st[key] - s64[key]) <= tol, (B, key, st[key], s64[key], s32[key])
        assert st["n_steps"] == 1
    GRAD_ERRORS[f"{proto}/{netname}"] = worst
    GRAD_OVER.extend(over)
    out = os.environ.get("CPR_DQN_GRAD_ERROR_OUT")
    if out:  # the measurement behind profiles/dqn_grad_error.json
        with open(out, "w") as f:
            json.dump({"bound": 8.0, "rows": list(ROWS),
                       "worst_device_over_torch_f32": GRAD_ERRORS, "above_bound": GRAD_OVER},
                      f, indent=1)
    assert not over, over


# ------------------------------------------------------------------ 7. repeatability

def test_calls_repeat_bit_for_bit(ctx):
    b, net, tgt = trained_pair(ctx, "nakamoto", False, (2, 64, 64), 11)
    data = transitions(b, net, tgt, 9, False)[0]
    rows = np.random.default_rng(1).permutation(N_DATA)[:2113]
    g1, s1 = b.dqn_gradients(data, rows, Q.DQNOptions(gamma=GAMMA))
    g2, s2 = b.dqn_gradients(data, rows, Q.DQNOptions(gamma=GAMMA))
    assert g1.tobytes() == g2.tobytes() and np.any(g1 != 0) and s1 == s2
    opts = Q.DQNOptions(batch=130, gradient_steps=4, lr=1e-3, sample_seed=2)
    got = []
    for _ in range(2):
        u = make(ctx, "bk", env=True, capacity=8)
        u.dqn_collect(8, 0.5)
        st = u.dqn_update(options=opts)
        got.append((weights(u).tobytes(), st))
    assert got[0] == got[1] and got[0][1]["n_steps"] == 4


# ------------------------------------------------------------------ 8. update

def test_update_equals_hand_driven_steps(ctx):
    opts = Q.DQNOptions(batch=130, gradient_steps=3, lr=1e-3, gamma=0.95, max_grad_norm=0.05)
    one = Q.DQNOptions(**dict(vars(opts), gradient_steps=1))

    def fresh():
        b = make(ctx, "bk", env=True, capacity=8)
        b.dqn_collect(8, 0.5)
        return b

    b, twin = fresh(), fresh()
    n = 8 * 96
    idx = np.random.default_rng(4).integers(0, n, (3, 130))
    before, tb = weights(b), target_weights(b)
    st = b.dqn_update(options=opts, idx=idx)
    assert st["n_steps"] == 3
    rep = twin.dqn_replay()
    data = {k: v.reshape((n,) + v.shape[2:]) for k, v in rep.items()}
    net = twin._net
    shapes = [a.shape for _, a in P.param_arrays(net)]
    ref = ppo_ref.TorchAdam([a for _, a in P.param_arrays(net)], opts)
    assert opts.adam_eps == 1e-8
    sums = dict.fromkeys(st, 0.0)
    for g in range(3):
        grad, gs = twin.dqn_gradients(data, idx[g], opts)
        assert gs["grad_norm"] > opts.max_grad_norm  # the clip acts
        us = twin.dqn_update(options=one, idx=idx[g:g + 1])
        assert us["loss"] == gs["loss"] and us["grad_norm"] == gs["grad_norm"]
        for k in sums:
            sums[k] += us[k]
        new, step = ref.step(list(P.unflatten_grads(net, grad).values()))
        got = P.unflatten_grads(net, weights(twin))
        for (name, w), want, s, shp in zip(got.items(), new, step, shapes):
            assert w.shape == shp
            tol = np.spacing(np.abs(want)).astype(np.float64) + 1e-6 * np.abs(s)
            diff = np.abs(w.astype(np.float64) - want.astype(np.float64))
            assert np.all(diff <= tol), (g, name, float(np.max(diff / tol)))
        with torch.no_grad():  # torch continues from the device's weights
            for p, w in zip(ref.ps, got.values()):
                p.copy_(torch.tensor(w))
    after = weights(b)
    assert after.tobytes() == weights(twin).tobytes()
    for k in ("loss", "abs_td", "q", "target", "grad_norm"):
        assert st[k] == pytest.approx(sums[k] / 3, rel=1e-14, abs=1e-300)
    k_pi = n_pi(net)
    assert np.mean(after[:k_pi] != before[:k_pi]) > 0.5
    assert after[k_pi:].tobytes() == before[k_pi:].tobytes()  # the vf trunk
    assert target_weights(b).tobytes() == tb.tobytes() == before.tobytes()


# ------------------------------------------------------------------ 9. target sync

def test_target_sync_is_polyak_in_f32(ctx):
    b = make(ctx, "nakamoto", capacity=4)
    b.dqn_collect(4, 1.0)
    b.dqn_update(options=Q.DQNOptions(batch=64, gradient_steps=2, lr=0.01))
    p, t = weights(b), target_weights(b)
    k = n_pi(b._net)
    assert np.mean(p[:k] != t[:k]) > 0.3 and p[k:].tobytes() == t[k:].tobytes()
    tau = 0.01
    b.dqn_target_sync(tau)
    omt, tf = np.float32(1.0 - tau), np.float32(tau)
    want = (t * omt) + (p * tf)
    assert want.dtype == np.float32
    t1 = target_weights(b)
    assert t1.tobytes() == want.tobytes() and t1.tobytes() != t.tobytes()
    assert weights(b).tobytes() == p.tobytes()
    b.dqn_target_sync(tau)
    assert target_weights(b).tobytes() == ((t1 * omt) + (p * tf)).tobytes()
    b.dqn_target_sync(1.0)
    assert target_weights(b).tobytes() == p.tobytes()
    tn, pn = b.get_target_net(), b.get_policy_net()
    for (_, x), (_, y) in zip(P.param_arrays(tn), P.param_arrays(pn)):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------ 10. iterate

@pytest.mark.parametrize("proto,env", [("fc16", False), ("bk", True)])
def test_iterate_equals_the_calls_by_hand(ctx, proto, env):
    n, steps = 96, 7
    # vector steps 7, 14, 21, 28 against an interval of 15: only the third iteration crosses;
    # learning starts with the second
    opts = Q.DQNOptions(batch=130, gradient_steps=2, lr=1e-3, tau=0.5, gamma=0.95,
                        target_update_interval=15 * n + 3, learning_starts=14 * n)
    b, twin = (make(ctx, proto, env=env, capacity=20) for _ in range(2))
    start = weights(b)
    synced = []
    for it in range(4):
        eps = 0.5 - 0.1 * it
        s, st = b.dqn_iterate(steps, eps, opts)
        s2 = twin.dqn_collect(steps, eps)
        total = steps * (it + 1)
        if total // 15 != (total - steps) // 15:
            twin.dqn_target_sync(opts.tau)
            synced.append(it)
        if total * n >= opts.learning_starts:
            st2 = twin.dqn_update(options=opts)
        else:
            st2 = dict.fromkeys(st, 0.0)
            st2["n_steps"] = 0
        assert bytes(s) == bytes(s2), it
        assert st == st2, it
        assert st["n_steps"] == (0 if it == 0 else 2)
        assert weights(b).tobytes() == weights(twin).tobytes(), it
        assert target_weights(b).tobytes() == target_weights(twin).tobytes(), it
        assert (weights(b).tobytes() == start.tobytes()) == (it == 0)
        assert (target_weights(b).tobytes() == start.tobytes()) == (it < 2), it
        assert same_replay(b.dqn_replay(), twin.dqn_replay())
    assert synced == [2]
    assert b.dqn_replay_state() == (20, 28 % 20, 20)


# ------------------------------------------------------------------ 11. evaluation

def test_evaluation_and_table_after_training(ctx):
    opts = Q.DQNOptions(batch=100, gradient_steps=2, lr=1e-3, gamma=1.0, learning_starts=0,
                        target_update_interval=96 * 5, tau=0.01)
    b = make(ctx, "fc16", capacity=16, max_steps=30)
    stats = [st for _, st in Q.train(b, 3, 5, opts, epsilon=Q.epsilon_schedule(1.0, 0.1, 0.5))]
    assert [st["epsilon"] for st in stats] == pytest.approx([1.0, 0.4, 0.1])
    assert all(st["n_steps"] == 2 for st in stats)
    net = b.get_policy_net()
    assert P.flatten_params(net).tobytes() != P.flatten_params(b._net).tobytes()
    ev = b.evaluate_net(64, deterministic=True).records
    fresh = make(ctx, "fc16", max_steps=30)
    fresh.set_policy_net(net)
    ev2 = fresh.evaluate_net(64, deterministic=True).records
    assert ev.tobytes() == ev2.tobytes() and len(ev) == 64
    table = mdp.fc16_table_from_net(net, 32, ctx=ctx)
    assert table.shape == (32 * 32 * 3,)
    assert table.dtype == np.uint8 and table.max() <= L.FC16_MATCH
    # the table is the greedy action of the trained weights: the forward entry on them agrees
    obs = np.array([[a / (1.0 + a), h / (1.0 + h), f / (1.0 + f)]
                    for a in range(3) for h in range(3) for f in range(3)])
    act = b.policy_net_forward(obs, deterministic=True)[0]
    assert act.shape == (27,) and act.min() >= 0


# ------------------------------------------------------------------ 12. refusals

def _code(call):
    with pytest.raises(L.CprError) as e:
        call()
    return e.value.code, str(e.value)


def test_refusals(ctx):
    cfg, keep = device.make_config(**dict(PROTO["nakamoto"], alpha=0.35, gamma=0.5, max_steps=12,
                                          seed=1, n_lanes=96))
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    assert _code(lambda: b.dqn_init(4))[0] == L.CPR_E_STATE  # no network
    b = make(ctx, "nakamoto")
    for call in (lambda: b.dqn_collect(4, 0.1), lambda: b.dqn_update(), lambda: b.dqn_iterate(4, 0.1),
                 lambda: b.dqn_target_sync(1.0), lambda: b.dqn_replay(0, 1),
                 lambda: b.get_target_net(), lambda: b.dqn_replay_state()):
        assert _code(call)[0] == L.CPR_E_STATE  # no dqn_init
    code, msg = _code(lambda: b.dqn_init(0))
    assert code == L.CPR_E_INVALID_ARG and "capacity" in msg
    b.dqn_init(4)
    before = weights(b)
    assert _code(lambda: b.dqn_update())[0] == L.CPR_E_STATE  # an empty ring
    for field, bad in (("batch", 0), ("gradient_steps", -1)):
        code, msg = _code(lambda: b.dqn_update(options=Q.DQNOptions(**{field: bad})))
        assert code == L.CPR_E_INVALID_ARG and field in msg
        code, msg = _code(lambda: b.dqn_iterate(4, 0.1, Q.DQNOptions(**{field: bad})))
        assert code == L.CPR_E_INVALID_ARG and field in msg
    code, msg = _code(lambda: b.dqn_collect(4, 1.5))
    assert code == L.CPR_E_INVALID_ARG and "epsilon" in msg
    assert b.dqn_replay_state() == (0, 0, 4) and weights(b).tobytes() == before.tobytes()
    # a later set_policy_net keeps the ring and makes the target a copy of the new weights
    b.dqn_collect(2, 1.0)
    ol, na = b.observation_spec()[:2]
    new = float_net(99, ol + 2, 2, 32, 48, na, EXTRA)
    b.set_policy_net(new)
    assert b.dqn_replay_state() == (2, 2, 4)
    assert target_weights(b).tobytes() == P.flatten_params(new).tobytes()
    # the widest network cpr_policy_net_set accepts trains (the LDS budget is the rollout's)
    wide = make(ctx, "nakamoto", arch=(1, 512, 512), capacity=2)
    wide.dqn_collect(2, 1.0)
    assert wide.dqn_update(options=Q.DQNOptions(batch=65))["n_steps"] == 1
    # FC16 without lanes' env, and a batch without lanes
    for kw in (dict(protocol=L.PROTO_FC16, policy=L.FC16_POLICY_HONEST, max_steps=100, n_lanes=4),
               dict(protocol=L.PROTO_NAKAMOTO, max_steps=100)):
        cfg, keep = device.make_config(alpha=0.3, gamma=0.5, **kw)
        u = device.Batch(cfg, ctx=ctx, keep=keep)
        assert L.lib().cpr_dqn_init(u.handle, 4) == L.CPR_E_UNSUPPORTED
        o, st, s = Q.DQNOptions().cstruct(), L.DqnStats(), L.Summary()
        assert L.lib().cpr_dqn_iterate(u.handle, 4, 0.1, ctypes.byref(o), ctypes.byref(s),
                                       ctypes.byref(st)) == L.CPR_E_UNSUPPORTED
        assert L.lib().cpr_dqn_update(u.handle, 1, ctypes.byref(o), None,
                                      ctypes.byref(st)) == L.CPR_E_UNSUPPORTED
