"""References for the Q-learning tests (no test here).

``dqn_loss``: SB3's DQN loss (stable_baselines3/dqn/dqn.py train(): the target network's row
maximum under no_grad, the TD target, ``smooth_l1_loss``) written in torch on the CPU, on
parameters taken from two ``PolicyNet`` objects (the online network and the target), in float64
or float32: the statistics of cpr_dqn_stats and the flat gradient in the order of
``cpr_amd.ppo.param_arrays`` (the vf trunk's entries are zero: it takes no part).

``dqn_loss_numpy``: the same loss and statistics by hand in numpy float64, from given Q-values.

``explore`` / ``sample_indices``: the keyed draws of cpr_dqn_collect and cpr_dqn_update restated
from the keyed stream's own helpers (oracle_py.keyed_block / philox / u53).
"""

import numpy as np
import torch

import oracle_py
import ppo_ref
from cpr_amd import _lib as L


def dqn_loss(net, target, x, x_next, action, reward, done, gamma, dtype=torch.float64):
    """x, x_next: ``ppo_ref.net_input`` rows of the minibatch. Returns (stats dict of Python
    floats, flat gradient as float64 numpy, info dict: delta, the target's Q-values)."""
    params = ppo_ref.torch_params(net, dtype)
    tparams = ppo_ref.torch_params(target, dtype)
    a = torch.tensor(np.asarray(action), dtype=torch.int64)
    r = torch.tensor(np.asarray(reward), dtype=dtype)
    d = torch.tensor(np.asarray(done).astype(bool).astype(np.float64), dtype=dtype)
    with torch.no_grad():
        qn, _, _ = ppo_ref.torch_forward(target, tparams, torch.tensor(x_next, dtype=dtype))
        y = r + (1 - d) * gamma * qn.max(dim=1).values
    q, _, _ = ppo_ref.torch_forward(net, params, torch.tensor(x, dtype=dtype))
    qa = q.gather(1, a[:, None])[:, 0]
    loss = torch.nn.functional.smooth_l1_loss(qa, y)
    loss.backward()
    with torch.no_grad():
        delta = qa - y
        stats = {"loss": loss.item(), "abs_td": delta.abs().mean().item(),
                 "q": qa.mean().item(), "target": y.mean().item()}
        flat = np.concatenate([(p.grad if p.grad is not None else torch.zeros_like(p))
                               .double().numpy().ravel() for p in params])
        stats["grad_norm"] = float(np.sqrt(np.sum(flat * flat)))
        info = {"delta": delta.double().numpy(), "q_next": qn.double().numpy()}
    return stats, flat, info


def dqn_loss_numpy(q, q_next, action, reward, done, gamma):
    """The loss by hand in float64 from the Q-values q [B, A] of the rows and q_next [B, A] of
    the target on the next rows: (stats dict, dL/dq [B, A])."""
    q, q_next = np.asarray(q, dtype=np.float64), np.asarray(q_next, dtype=np.float64)
    B = q.shape[0]
    qa = q[np.arange(B), action]
    y = reward + (gamma * q_next.max(axis=1)) * (1.0 - np.asarray(done).astype(bool))
    delta = qa - y
    ad = np.abs(delta)
    row = np.where(ad < 1.0, 0.5 * delta * delta, ad - 0.5)
    dq = np.zeros_like(q)
    dq[np.arange(B), action] = np.clip(delta, -1.0, 1.0) / B
    return {"loss": row.mean(), "abs_td": ad.mean(), "q": qa.mean(), "target": y.mean()}, dq


def explore(seed, episode, step, n_actions):
    """(u1, random action) of lane state (episode, episode step index before the step)."""
    w = [int(v) for v in oracle_py.keyed_block(int(seed), int(episode), int(step), L.TAG_EXPLORE)]
    u1, u2 = oracle_py.u53(w[0], w[1]), oracle_py.u53(w[2], w[3])
    return u1, min(n_actions - 1, int(u2 * n_actions))


def sample_indices(seed, sample_seed, update, gradient_steps, batch, n):
    """int64 [gradient_steps, batch] of cpr_dqn_update's draws (idx NULL) over n transitions."""
    key = (int(seed) ^ (int(sample_seed) * 0x9E3779B97F4A7C15)) & ((1 << 64) - 1)
    out = np.zeros((gradient_steps, batch), dtype=np.int64)
    for g in range(gradient_steps):
        for i in range(batch):
            if i % 2 == 0:
                w = [int(v) for v in oracle_py.philox(
                    [update & 0xFFFFFFFF, g, i >> 1, L.TAG_REPLAY], [key & 0xFFFFFFFF, key >> 32])]
            u = oracle_py.u53(w[2], w[3]) if i & 1 else oracle_py.u53(w[0], w[1])
            out[g, i] = min(n - 1, int(u * n))
    return out
