"""The learner's host side (no GPU): options, parameter order, the state dict, and the test
reference itself.

``ppo_ref.ppo_loss`` is what the device gradient is measured against (test_gpu_ppo.py), so it
is pinned here against a loss written by hand in numpy float64 and its finite differences:
a sign or 1/B error in the helper cannot hide behind torch's autograd.
"""

import ctypes
import dataclasses

import numpy as np
import torch

import ppo_ref
from cpr_amd import _lib as L
from cpr_amd import device
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
    o = P.PPOOptions()
    # experiments/train/ppo.py:399-417 (clip_range) over SB3's PPO defaults
    assert (o.n_epochs, o.clip_range, o.vf_coef, o.max_grad_norm) == (10, 0.1, 0.5, 0.5)
    assert (o.adam_eps, o.gae_lambda, o.gae_gamma, o.ent_coef) == (1e-5, 0.95, 0.99, 0.0)
    assert (o.minibatch, o.lr, o.beta1, o.beta2, o.normalize_advantage) == \
        (64, 3e-4, 0.9, 0.999, True)
    # the C defaults are the same, field by field
    c = L.PpoOptsC()
    L.check(L.lib().cpr_ppo_opts_default(ctypes.byref(c)))
    assert P.PPOOptions.from_cstruct(c) == o
    assert P.PPOOptions.from_cstruct(o.cstruct()) == o
    assert [f.name for f in dataclasses.fields(o)] == [n for n, _ in L.PpoOptsC._fields_]


def test_state_dict_round_trips():
    net = small_net(depth=2, wpi=32, wvf=48)
    sd = net.state_dict()
    assert list(sd) == ["mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
                        "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias",
                        "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias",
                        "mlp_extractor.value_net.2.weight", "mlp_extractor.value_net.2.bias",
                        "action_net.weight", "action_net.bias", "value_net.weight",
                        "value_net.bias"]
    back = device.PolicyNet.from_state_dict({k: torch.from_numpy(v) for k, v in sd.items()},
                                            extra=net.extra)
    assert back.depth == 2 and (back.width_pi, back.width_vf) == (32, 48)
    for (_, a), (_, b) in zip(P.param_arrays(net), P.param_arrays(back)):
        assert a.dtype == np.float32 and np.array_equal(a, b)


def test_flat_parameter_order():
    net = small_net(depth=2, wpi=16, wvf=32, n_in=5, extra=(0.5,))
    names = [n for n, _ in P.param_arrays(net)]
    assert names == ["mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
                     "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias",
                     "action_net.weight", "action_net.bias",
                     "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias",
                     "mlp_extractor.value_net.2.weight", "mlp_extractor.value_net.2.bias",
                     "value_net.weight", "value_net.bias"]
    flat = P.flatten_params(net)
    sizes = [16 * 5, 16, 16 * 16, 16, 4 * 16, 4, 32 * 5, 32, 32 * 32, 32, 32, 1]
    assert flat.dtype == np.float32 and flat.size == sum(sizes)
    assert np.array_equal(flat[:80].reshape(16, 5), net.pi[0][0])  # W row-major [out][in]
    assert np.array_equal(flat[80:96], net.pi[0][1])
    o = sum(sizes[:6])
    assert np.array_equal(flat[o:o + 160].reshape(32, 5), net.vf[0][0])
    un = P.unflatten_grads(net, np.arange(flat.size, dtype=np.float32))
    assert list(un) == names
    assert un["action_net.bias"].tolist() == [float(sum(sizes[:5]) + i) for i in range(4)]
    assert un["value_net.weight"].shape == (1, 32)


def numpy_loss(flat, net, x, action, old_logp, adv_n, ret, opts):
    """SB3's loss by hand, float64, on a flat parameter vector (depth 1)."""
    shapes = [a.shape for _, a in P.param_arrays(net)]
    ps, o = [], 0
    for s in shapes:
        k = int(np.prod(s))
        ps.append(flat[o:o + k].reshape(s))
        o += k
    W0, b0, Wh, bh, V0, c0, Vh, ch = ps
    B = x.shape[0]
    total = 0.0
    for r in range(B):
        h = np.maximum(W0 @ x[r] + b0, 0.0)
        l = Wh @ h + bh
        g = np.maximum(V0 @ x[r] + c0, 0.0)
        v = (Vh @ g + ch)[0]
        lse = np.log(np.sum(np.exp(l - l.max()))) + l.max()
        lp = l - lse
        rho = np.exp(lp[action[r]] - old_logp[r])
        surr = min(adv_n[r] * rho,
                   adv_n[r] * min(max(rho, 1 - opts.clip_range), 1 + opts.clip_range))
        H = -np.sum(np.exp(lp) * lp)
        total += (-surr + opts.ent_coef * (-H) + opts.vf_coef * (ret[r] - v) ** 2) / B
    return total


def test_reference_loss_against_numpy_and_finite_differences():
    net = small_net()
    rng = np.random.default_rng(11)
    obs = rng.random((2, 4))
    x = ppo_ref.net_input(net, obs)
    action = np.array([1, 3])
    adv = np.array([0.7, -0.4])
    ret = np.array([0.3, 1.1])
    opts = P.PPOOptions(ent_coef=0.02)
    # row 0 inside the clip range, row 1 (A < 0) outside it on the unclipped side (rho > 1 + c)
    s0, _, i0 = ppo_ref.ppo_loss(net, x, action, np.zeros(2), adv, ret, opts)
    logp = np.log(i0["rho"])
    old = logp - np.array([0.03, 0.25])
    stats, grad, info = ppo_ref.ppo_loss(net, x, action, old, adv, ret, opts)
    assert np.allclose(info["rho"], np.exp([0.03, 0.25]))
    adv_n = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    assert np.allclose(info["adv"], adv_n, rtol=1e-14)
    flat = P.flatten_params(net).astype(np.float64)
    f = lambda p: numpy_loss(p, net, x, action, old, adv_n, ret, opts)  # noqa: E731
    assert abs(f(flat) - stats["loss"]) <= 1e-13 * max(1.0, abs(stats["loss"]))
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
    # a clipped row contributes nothing through the policy term: row 1 with A > 0 instead
    adv2 = np.array([-0.7, 0.4])
    _, g2, _ = ppo_ref.ppo_loss(net, x[1:], action[1:], old[1:], adv2[1:], ret[1:],
                                P.PPOOptions(ent_coef=0.0))
    n_pi = sum(a.size for _, a in P.param_arrays(net)[:4])
    assert np.all(g2[:n_pi] == 0.0) and np.any(g2[n_pi:] != 0.0)


def test_gae_reference_matches_the_recursion():
    rng = np.random.default_rng(2)
    r, v = rng.standard_normal((5, 3)), rng.standard_normal((6, 3))
    d = rng.random((5, 3)) < 0.3
    adv, ret = ppo_ref.gae_ref(r, d, v, 0.9, 0.8)
    for i in range(3):
        last = 0.0
        for t in range(4, -1, -1):
            nnt = 0.0 if d[t, i] else 1.0
            last = r[t, i] + 0.9 * v[t + 1, i] * nnt - v[t, i] + 0.9 * 0.8 * nnt * last
            assert abs(adv[t, i] - last) < 1e-12 and abs(ret[t, i] - (last + v[t, i])) < 1e-12
