"""Q-learning's Python face (cpr_dqn_*, include/cpr_hip.h; DESIGN.md §4.14 "Q-learning"):
options, the reference's two presets, the exploration schedule, SB3 DQN's state-dict naming
and a short training loop over ``Batch.dqn_iterate``.
"""

import dataclasses

from . import _lib as L
from .ppo import eval_statistics

_MASK64 = (1 << 64) - 1


@dataclasses.dataclass
class DQNOptions:
    """cpr_dqn_opts, in the struct's field order. The defaults are dqn.yml's ``default:`` block
    over SB3's. ``lr`` is per call."""

    batch: int = 32
    gradient_steps: int = 1
    gamma: float = 0.99
    lr: float = 1e-4
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1e-8
    max_grad_norm: float = 10.0
    tau: float = 1.0
    target_update_interval: int = 10_000
    learning_starts: int = 50_000
    sample_seed: int = 0

    _INTS = ("batch", "gradient_steps", "target_update_interval", "learning_starts")

    def cstruct(self):
        c = L.DqnOptsC()
        for f in dataclasses.fields(self):
            v = getattr(self, f.name)
            if f.name in self._INTS:
                v = int(v)
            elif f.name == "sample_seed":
                v = int(v) & _MASK64
            else:
                v = float(v)
            setattr(c, f.name, v)
        return c

    @classmethod
    def from_cstruct(cls, c):
        return cls(**{f.name: getattr(c, f.name) for f in dataclasses.fields(cls)})


def _preset(n_timesteps):
    # dqn.yml's two env blocks carry the same numbers apart from n_timesteps
    return {
        "n_envs": 24,
        "n_timesteps": n_timesteps,
        "buffer_size": 5_000_000,
        "train_freq": 10_000,
        "exploration_fraction": 0.1,
        "exploration_initial_eps": 1.0,
        "exploration_final_eps": 0.1,
        "net_arch": (64, 64),
        "options": DQNOptions(batch=500, gradient_steps=100, gamma=1.0, lr=1e-3, tau=0.01,
                              target_update_interval=10_000, learning_starts=500_000,
                              max_grad_norm=10.0),
    }


FC16_PRESET = _preset(50_000_000)      # dqn.yml FC16SSZwPT-v0
NAKAMOTO_PRESET = _preset(10_000_000)  # dqn.yml Nakamoto-v0


def epsilon_schedule(initial=1.0, final=0.05, fraction=0.1):
    """SB3's get_linear_fn(initial, final, fraction) as a function of the fraction of training
    done (SB3 passes 1 - progress_remaining): linear from ``initial`` to ``final`` over the
    first ``fraction`` of training, ``final`` afterwards."""
    initial, final, fraction = float(initial), float(final), float(fraction)

    def eps(done):
        if done > fraction:
            return final
        return initial + done * (final - initial) / fraction

    return eps


def _names(prefix, depth):
    out = []
    for i in range(depth + 1):
        out += [f"{prefix}.q_net.{2 * i}.weight", f"{prefix}.q_net.{2 * i}.bias"]
    return out


def state_dict(net, target):
    """{name: f32 array} of the Q-network (``net``'s pi trunk and head) and the target in SB3
    DQNPolicy's naming: q_net.q_net.{2i}.weight / bias for the hidden layers i and the head
    (i = depth), and the same under q_net_target."""
    sd = {}
    for prefix, n in (("q_net", net), ("q_net_target", target)):
        arrays = [a for wb in [*n.pi, n.pi_head] for a in wb]
        for name, a in zip(_names(prefix, n.depth), arrays):
            sd[name] = a
    return sd


def nets_from_state_dict(sd, like):
    """(net, target) from ``state_dict``'s naming. The vf trunk, which Q-learning does not
    touch, and the extras come from ``like`` (a ``PolicyNet``)."""
    from .device import PolicyNet

    out = []
    for prefix in ("q_net", "q_net_target"):
        depth = len([k for k in sd if k.startswith(prefix + ".q_net.")]) // 2 - 1
        wb = [(sd[f"{prefix}.q_net.{2 * i}.weight"], sd[f"{prefix}.q_net.{2 * i}.bias"])
              for i in range(depth + 1)]
        out.append(PolicyNet(wb[:-1], wb[-1], like.vf, like.vf_head, extra=like.extra))
    return tuple(out)


def train(batch, iterations, n_steps, options=None, epsilon=None, lr_schedule=None,
          eval_batch=None, eval_freq=1, eval_start=0, eval_episodes_per_alpha=1):
    """``iterations`` DQN iterations of ``n_steps`` steps per lane on ``batch`` (which has a
    network and a ring, ``dqn_init``): yields (summary, statistics dict) per iteration.
    ``epsilon``: a number, or a function of the fraction of training done
    (``epsilon_schedule``); None: SB3's default schedule. ``lr_schedule(x)``, x the fraction
    of training remaining, gives the iteration's learning rate; None keeps ``options.lr``.
    ``eval_batch`` and the ``eval_*`` arguments are ``ppo.train``'s evaluation hook: the greedy
    policy of the current weights on a separate batch, at the start of an iteration."""
    opts = dataclasses.replace(options) if options is not None else DQNOptions()
    if epsilon is None:
        epsilon = epsilon_schedule()
    for it in range(int(iterations)):
        ev = None
        if eval_batch is not None and it >= eval_start and it % eval_freq == 0:
            eval_batch.copy_policy_net_from(batch)
            ev = eval_statistics(eval_batch.evaluate_net(eval_episodes_per_alpha))
        if lr_schedule is not None:
            opts.lr = float(lr_schedule(1.0 - it / float(iterations)))
        eps = float(epsilon(it / float(iterations))) if callable(epsilon) else float(epsilon)
        summary, stats = batch.dqn_iterate(n_steps, eps, opts)
        stats["lr"] = opts.lr
        stats["epsilon"] = eps
        if ev is not None:
            stats.update(ev)
        yield summary, stats
