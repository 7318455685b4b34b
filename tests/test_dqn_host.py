"""Q-learning's host side (cpr_amd/dqn.py, tests/dqn_ref.py) — no GPU.

1. DQNOptions mirrors cpr_dqn_opts and its defaults; the presets carry dqn.yml's numbers;
2. SB3's linear exploration schedule;
3. the state dict's names, and its round trip;
4. dqn_ref.dqn_loss (torch) against the loss written by hand in numpy float64 and against its
   central differences, on rows with |delta| on both sides of 1 and with done rows;
5. the keyed draws of dqn_ref, restated from the keyed stream's helpers (oracle_py).
"""

import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import dqn_ref
import oracle_py
import ppo_ref
from cpr_amd import _lib as L
from cpr_amd import device
from cpr_amd import dqn as Q
from cpr_amd import ppo as P


def small_net(seed=5, n_in=6, depth=1, wpi=16, wvf=16, n_act=4, extra=(0.25, 0.5)):
    rng = np.random.default_rng(seed)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    return device.PolicyNet(pi=[lin(wpi, n_in if i == 0 else wpi) for i in range(depth)],
                            pi_head=lin(n_act, wpi),
                            vf=[lin(wvf, n_in if i == 0 else wvf) for i in range(depth)],
                            vf_head=lin(1, wvf), extra=extra)


def test_options_default_to_the_reference():
    o = Q.DQNOptions()
    # dqn.yml's default block over SB3's DQN defaults
    assert (o.batch, o.gradient_steps, o.gamma, o.lr) == (32, 1, 0.99, 1e-4)
    assert (o.beta1, o.beta2, o.adam_eps, o.max_grad_norm) == (0.9, 0.999, 1e-8, 10.0)
    assert (o.tau, o.target_update_interval, o.learning_starts, o.sample_seed) == \
        (1.0, 10_000, 50_000, 0)
    c = L.DqnOptsC()
    L.check(L.lib().cpr_dqn_opts_default(ctypes.byref(c)))
    assert Q.DQNOptions.from_cstruct(c) == o
    assert Q.DQNOptions.from_cstruct(o.cstruct()) == o
    assert [f.name for f in dataclasses.fields(o)] == [n for n, _ in L.DqnOptsC._fields_]
    for n, _ in L.DqnOptsC._fields_:
        assert getattr(c, n) == getattr(o, n), n


def test_presets_are_dqn_yml():
    for preset, steps in ((Q.FC16_PRESET, 50_000_000), (Q.NAKAMOTO_PRESET, 10_000_000)):
        o = preset["options"]
        assert (preset["n_envs"], preset["n_timesteps"], preset["buffer_size"],
                preset["train_freq"]) == (24, steps, 5_000_000, 10_000)
        assert (o.batch, o.gradient_steps, o.lr, o.gamma) == (500, 100, 1e-3, 1.0)
        assert (o.learning_starts, o.target_update_interval, o.tau, o.max_grad_norm) == \
            (500_000, 10_000, 0.01, 10.0)
        assert (preset["exploration_fraction"], preset["exploration_initial_eps"],
                preset["exploration_final_eps"], preset["net_arch"]) == (0.1, 1.0, 0.1, (64, 64))
    assert Q.FC16_PRESET["options"] is not Q.NAKAMOTO_PRESET["options"]


def test_epsilon_schedule_is_sb3s_linear_fn():
    eps = Q.epsilon_schedule(1.0, 0.1, 0.1)
    assert eps(0.0) == 1.0
    assert eps(0.05) == pytest.approx(0.55)
    assert eps(0.1) == pytest.approx(0.1)
    assert eps(0.100001) == 0.1 and eps(1.0) == 0.1
    assert Q.epsilon_schedule()(1.0) == 0.05


def test_state_dict_names_and_round_trip():
    net, target = small_net(depth=2, wpi=32, wvf=48), small_net(seed=6, depth=2, wpi=32, wvf=48)
    sd = Q.state_dict(net, target)
    assert list(sd) == [f"{p}.q_net.{i}.{k}" for p in ("q_net", "q_net_target")
                        for i in (0, 2, 4) for k in ("weight", "bias")]
    assert sd["q_net.q_net.4.weight"].shape == (4, 32)       # the head
    assert sd["q_net_target.q_net.2.weight"].shape == (32, 32)
    n2, t2 = Q.nets_from_state_dict(sd, like=net)
    for a, b in ((net, n2), (target, t2)):
        assert P.flatten_params(a)[:sum(x.size for _, x in P.param_arrays(a)[:6])].tobytes() == \
            P.flatten_params(b)[:sum(x.size for _, x in P.param_arrays(b)[:6])].tobytes()
        assert a.extra == b.extra == net.extra
    # the vf trunk comes from `like`
    assert P.flatten_params(t2)[-49:].tobytes() == P.flatten_params(net)[-49:].tobytes()
    assert list(Q.state_dict(n2, t2)) == list(sd)


def _numpy_q(flat, net, x):
    """Q-values of the pi trunk in numpy float64 from a flat parameter vector."""
    ps = list(P.unflatten_grads(net, flat).values())[:2 * (net.depth + 1)]
    h = x
    for l in range(net.depth):
        h = np.maximum(h @ ps[2 * l].T + ps[2 * l + 1], 0.0)
    return h @ ps[2 * net.depth].T + ps[2 * net.depth + 1]


def test_reference_loss_against_numpy_and_finite_differences():
    net, target = small_net(), small_net(seed=9)
    rng = np.random.default_rng(11)
    B = 6
    x = ppo_ref.net_input(net, rng.random((B, 4)))
    xn = ppo_ref.net_input(net, rng.random((B, 4)))
    action = np.array([1, 3, 0, 2, 1, 0])
    done = np.array([0, 0, 1, 0, 1, 0], dtype=np.uint8)
    gamma = 0.9
    flat = P.flatten_params(net).astype(np.float64)
    q = _numpy_q(flat, net, x)
    qn = _numpy_q(P.flatten_params(target).astype(np.float64), target, xn)
    # rewards chosen for delta = q_a - y: two rows inside (-1, 1), two above 1, two below -1;
    # a done row in each of two groups
    want = np.array([0.3, -0.6, 1.7, 2.5, -1.2, -3.0])
    nnt = 1.0 - done
    reward = q[np.arange(B), action] - want - gamma * qn.max(axis=1) * nnt
    stats, grad, info = dqn_ref.dqn_loss(net, target, x, xn, action, reward, done, gamma)
    assert np.allclose(info["delta"], want, rtol=0, atol=1e-12)
    assert np.allclose(info["q_next"], qn, rtol=1e-13)
    hand, dq = dqn_ref.dqn_loss_numpy(q, qn, action, reward, done, gamma)
    row = np.array([0.5 * 0.09, 0.5 * 0.36, 1.2, 2.0, 0.7, 2.5])
    assert hand["loss"] == pytest.approx(row.mean(), rel=1e-12)
    for k in ("loss", "abs_td", "q", "target"):
        assert stats[k] == pytest.approx(hand[k], rel=1e-13, abs=1e-15), k
    assert np.allclose(dq[np.arange(B), action] * B, np.clip(want, -1, 1), atol=1e-12)
    assert np.count_nonzero(dq) == B
    # a done row's target is its reward alone
    y = reward + gamma * qn.max(axis=1) * nnt
    assert np.array_equal(y[done == 1], reward[done == 1])

    def f(p):
        return dqn_ref.dqn_loss_numpy(_numpy_q(p, net, x), qn, action, reward, done, gamma)[0]["loss"]

    assert abs(f(flat) - stats["loss"]) <= 1e-13
    h = 1e-6
    fd = np.zeros_like(flat)
    for i in range(flat.size):
        e = np.zeros_like(flat)
        e[i] = h
        fd[i] = (f(flat + e) - f(flat - e)) / (2 * h)
    assert grad.shape == fd.shape
    # central differences of a piecewise-smooth function: O(h^2) truncation + 1e-16 / h rounding
    assert np.max(np.abs(fd - grad)) <= 1e-8 * max(1.0, np.max(np.abs(grad)))
    assert np.linalg.norm(grad) > 1e-3
    # the vf trunk takes no part; the target's parameters get no gradient (no_grad)
    n_pi = sum(a.size for _, a in P.param_arrays(net)[:4])
    assert np.any(grad[:n_pi] != 0.0) and np.all(grad[n_pi:] == 0.0)
    # float32 agrees to float32
    s32, g32, _ = dqn_ref.dqn_loss(net, target, x, xn, action, reward, done, gamma, torch.float32)
    assert s32["loss"] == pytest.approx(stats["loss"], rel=1e-5)
    assert np.allclose(g32, grad, rtol=1e-3, atol=1e-6)


def test_keyed_draws_of_the_reference_helpers():
    seed = 0x5EED0000DEADBEEF
    for ep, step in ((0, 0), (7, 3), (2**33 + 5, 40)):
        u1, a = dqn_ref.explore(seed, ep, step, 4)
        assert 0.0 <= u1 < 1.0 and 0 <= a < 4
        # the block is the keyed stream's: words 0, 1 the coin, words 2, 3 the action
        w = [int(v) for v in oracle_py.keyed_block(seed, ep, step, 0x90000000)]
        assert u1 == oracle_py.u53(w[0], w[1])
        assert a == min(3, int(oracle_py.u53(w[2], w[3]) * 4))
    a = dqn_ref.sample_indices(seed, 3, 2, 3, 7, 1000)
    assert a.shape == (3, 7) and a.min() >= 0 and a.max() < 1000
    assert len(np.unique(a)) > 15  # draws, not a constant
    assert not np.array_equal(a, dqn_ref.sample_indices(seed, 4, 2, 3, 7, 1000))
    assert not np.array_equal(a, dqn_ref.sample_indices(seed, 3, 1, 3, 7, 1000))
    # rows 2j and 2j + 1 share a block; a longer batch extends a shorter one
    assert np.array_equal(a[:, :5], dqn_ref.sample_indices(seed, 3, 2, 3, 5, 1000))
    key = (seed ^ (3 * 0x9E3779B97F4A7C15)) & ((1 << 64) - 1)
    w = [int(v) for v in oracle_py.philox([2, 1, 3, 0xA0000000], [key & 0xFFFFFFFF, key >> 32])]
    assert a[1, 6] == min(999, int(oracle_py.u53(w[0], w[1]) * 1000))
    # n = 1: every index is 0
    assert not dqn_ref.sample_indices(seed, 0, 0, 1, 5, 1).any()
