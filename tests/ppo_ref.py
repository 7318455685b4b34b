"""References for the learner's tests (no test here).

``gae_ref``: SB3's compute_returns_and_advantage in numpy float64, in k_gae's operation order
(include/cpr_hip.h cpr_gae), so that the device result can be compared bit for bit.

``ppo_loss``: SB3's PPO loss (stable_baselines3/ppo/ppo.py train(), without value clipping and
target_kl) written in torch on the CPU, on parameters taken from a ``PolicyNet``, in float64
or float32: the loss terms SB3 logs and the flat gradient in the order of
``cpr_amd.ppo.param_arrays``.
"""

import numpy as np
import torch

from cpr_amd import ppo as P


def gae_ref(reward, done, value, gamma, lam):
    reward = np.asarray(reward, dtype=np.float64)
    value = np.asarray(value, dtype=np.float64)
    n_steps = reward.shape[0]
    adv = np.zeros_like(reward)
    ret = np.zeros_like(reward)
    last = np.zeros(reward.shape[1])
    gl = np.float64(gamma) * np.float64(lam)
    for t in range(n_steps - 1, -1, -1):
        nnt = 1.0 - np.asarray(done[t], dtype=bool).astype(np.float64)
        delta = (reward[t] + (np.float64(gamma) * value[t + 1]) * nnt) - value[t]
        last = delta + (gl * nnt) * last
        adv[t] = last
        ret[t] = last + value[t]
    return adv, ret


def net_input(net, obs, alpha=None, alpha_column=None):
    """The network's f32 input rows as float64: observation and extras rounded to f32, the
    alpha column (if any) from the rows' alphas."""
    x = np.asarray(obs, dtype=np.float64).astype(np.float32)
    ex = np.tile(np.float32(net.extra), (x.shape[0], 1)).reshape(x.shape[0], len(net.extra))
    if alpha is not None and alpha_column is not None and alpha_column >= 0:
        ex[:, alpha_column] = np.asarray(alpha, dtype=np.float64).astype(np.float32)
    return np.concatenate([x, ex], axis=1).astype(np.float64)


def torch_params(net, dtype):
    return [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)
            for _, a in P.param_arrays(net)]


def torch_forward(net, params, x):
    """(logits, value, hidden activations [trunk][layer]) of the two-trunk ReLU MLP."""
    d = net.depth
    outs, hidden = [], []
    for trunk in range(2):
        ps = params[trunk * 2 * (d + 1):(trunk + 1) * 2 * (d + 1)]
        h, hs = x, []
        for l in range(d):
            h = torch.relu(h @ ps[2 * l].T + ps[2 * l + 1])
            hs.append(h)
        outs.append(h @ ps[2 * d].T + ps[2 * d + 1])
        hidden.append(hs)
    return outs[0], outs[1][:, 0], hidden


def ppo_loss(net, x, action, old_logp, advantage, ret, opts, dtype=torch.float64):
    """x: ``net_input`` rows of the minibatch. Returns (stats dict of Python floats, flat
    gradient as float64 numpy, info dict: rho, the normalised advantages, hidden activations)."""
    params = torch_params(net, dtype)
    xt = torch.tensor(x, dtype=dtype)
    a = torch.tensor(np.asarray(action), dtype=torch.int64)
    olp = torch.tensor(np.asarray(old_logp), dtype=dtype)
    adv = torch.tensor(np.asarray(advantage), dtype=dtype)
    R = torch.tensor(np.asarray(ret), dtype=dtype)
    if opts.normalize_advantage and len(adv) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    logits, value, hidden = torch_forward(net, params, xt)
    logp_all = torch.log_softmax(logits, dim=1)
    logp = logp_all.gather(1, a[:, None])[:, 0]
    log_ratio = logp - olp
    ratio = torch.exp(log_ratio)
    c = opts.clip_range
    pl1 = adv * ratio
    pl2 = adv * torch.clamp(ratio, 1 - c, 1 + c)
    policy_loss = -torch.min(pl1, pl2).mean()
    value_loss = torch.nn.functional.mse_loss(R, value)
    entropy = -(torch.exp(logp_all) * logp_all).sum(dim=1)
    entropy_loss = -entropy.mean()
    loss = policy_loss + opts.ent_coef * entropy_loss + opts.vf_coef * value_loss
    loss.backward()
    with torch.no_grad():
        stats = {
            "policy_loss": policy_loss.item(),
            "value_loss": value_loss.item(),
            "entropy_loss": entropy_loss.item(),
            "approx_kl": ((ratio - 1) - log_ratio).mean().item(),
            "clip_fraction": (torch.abs(ratio - 1) > c).to(dtype).mean().item(),
            "loss": loss.item(),
        }
        flat = np.concatenate([p.grad.double().numpy().ravel() for p in params])
        stats["grad_norm"] = float(np.sqrt(np.sum(flat * flat)))
        info = {"rho": ratio.double().numpy(), "adv": adv.double().numpy(),
                "hidden": [[h.double().numpy() for h in hs] for hs in hidden]}
    return stats, flat, info


class TorchAdam:
    """torch.nn.utils.clip_grad_norm_ and torch.optim.Adam in float32 on the CPU over a list of
    f32 numpy parameters; ``step(grads)`` returns (the new parameters, the step taken per
    parameter as float64)."""

    def __init__(self, params, opts):
        self.ps = [torch.nn.Parameter(torch.tensor(np.asarray(p), dtype=torch.float32))
                   for p in params]
        self.opts = opts
        self.opt = torch.optim.Adam(self.ps, lr=opts.lr, betas=(opts.beta1, opts.beta2),
                                    eps=opts.adam_eps)

    def step(self, grads):
        before = [p.detach().numpy().astype(np.float64) for p in self.ps]
        for p, g in zip(self.ps, grads):
            p.grad = torch.tensor(np.asarray(g), dtype=torch.float32).reshape(p.shape)
        torch.nn.utils.clip_grad_norm_(self.ps, self.opts.max_grad_norm)
        self.opt.step()
        new = [p.detach().numpy().copy() for p in self.ps]
        return new, [n.astype(np.float64) - b for n, b in zip(new, before)]
