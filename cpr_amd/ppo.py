"""The learner's Python face (cpr_ppo_*, include/cpr_hip.h; DESIGN.md §4.14 "Learner"):
options, the flat parameter order and a short training loop over ``Batch.ppo_iterate``.
"""

import dataclasses

import numpy as np

from . import _lib as L


@dataclasses.dataclass
class PPOOptions:
    """cpr_ppo_opts. The defaults are the reference's (experiments/train/ppo.py:399-417 over
    SB3's): 10 epochs, clip 0.1, vf 0.5, max-norm 0.5, Adam eps 1e-5, lambda 0.95. ``lr`` is
    per call: ``train`` applies a schedule."""

    n_epochs: int = 10
    minibatch: int = 64
    clip_range: float = 0.1
    ent_coef: float = 0.0
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    lr: float = 3e-4
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1e-5
    normalize_advantage: bool = True
    gae_gamma: float = 0.99
    gae_lambda: float = 0.95
    perm_seed: int = 0

    def cstruct(self):
        c = L.PpoOptsC()
        for f in dataclasses.fields(self):
            v = getattr(self, f.name)
            if f.name in ("n_epochs", "minibatch", "normalize_advantage"):
                v = int(v)
            elif f.name == "perm_seed":
                v = int(v) & ((1 << 64) - 1)
            else:
                v = float(v)
            setattr(c, f.name, v)
        return c

    @classmethod
    def from_cstruct(cls, c):
        o = cls(**{f.name: getattr(c, f.name) for f in dataclasses.fields(cls)})
        o.normalize_advantage = bool(o.normalize_advantage)
        return o


def param_arrays(net):
    """[(name, array)] of a ``PolicyNet`` in the flat order of cpr_ppo_gradients: the pi trunk
    then the vf trunk; per trunk each hidden layer's W then b, then the head's W and b. Names
    follow SB3's state dict (``PolicyNet.state_dict``)."""
    out = []
    for trunk, head, tname, hname in ((net.pi, net.pi_head, "policy_net", "action_net"),
                                      (net.vf, net.vf_head, "value_net", "value_net")):
        for i, (w, b) in enumerate(trunk):
            out.append((f"mlp_extractor.{tname}.{2 * i}.weight", w))
            out.append((f"mlp_extractor.{tname}.{2 * i}.bias", b))
        out.append((f"{hname}.weight", head[0]))
        out.append((f"{hname}.bias", head[1]))
    return out


def flatten_params(net):
    """The network's parameters as one f32 vector in the documented order."""
    return np.concatenate([np.asarray(a, dtype=np.float32).ravel() for _, a in param_arrays(net)])


def unflatten_grads(net, flat):
    """A flat vector in the documented order as {SB3 name: array shaped like the parameter}."""
    flat = np.asarray(flat)
    out, o = {}, 0
    for name, a in param_arrays(net):
        out[name] = flat[o:o + a.size].reshape(a.shape)
        o += a.size
    if o != flat.size:
        raise ValueError(f"flat: {flat.size} values, the network has {o} parameters")
    return out


def eval_statistics(result):
    """EvalCallback's logged numbers (ppo.py:341-374) of an ``EvalResult`` with records: the
    mean and the standard deviation (pandas' ddof = 1; NaN for a single record) of every
    column of ``_lib.EVAL_COLUMNS`` over all valid records, the alpha column dropped, computed
    here on the host: {"eval/mean_<column>": ..., "eval/std_<column>": ...}, and under
    "eval/per_alpha" the per-alpha table (``EvalResult.per_alpha``)."""
    rec = result.records
    rec = rec[(rec["status"] & L.ST_INVALID) == 0]
    out = {}
    for name in L.EVAL_COLUMNS:
        x = rec[name].astype(np.float64)
        out["eval/mean_" + name] = float(np.mean(x)) if x.size else float("nan")
        out["eval/std_" + name] = float(np.std(x, ddof=1)) if x.size > 1 else float("nan")
    out["eval/per_alpha"] = result.per_alpha
    return out


def train(batch, iterations, n_steps, options=None, lr_schedule=None, eval_batch=None,
          eval_freq=1, eval_start=0, eval_episodes_per_alpha=1):
    """``iterations`` PPO iterations of ``n_steps`` steps per lane on ``batch`` (which has a
    network set): yields (summary, statistics dict) per iteration. ``lr_schedule(x)``, x the
    fraction of training remaining (1 at the start; ppo.py:382-387), gives the iteration's
    learning rate; None keeps ``options.lr``.

    ``eval_batch`` (a separate batch on the same context, e.g. ``envs.device_env_fn(...,
    eval=True)``; None: no evaluation, nothing changes): at the start of iteration ``it``
    with ``it >= eval_start and it % eval_freq == 0`` (EvalCallback._on_rollout_start) it
    takes ``batch``'s weights (``copy_policy_net_from``) and evaluates
    ``eval_episodes_per_alpha`` whole episodes per alpha, deterministic, from episode 0 every
    time (common random numbers between evaluations); the iteration's statistics gain
    ``eval_statistics``' keys. The training batch is not touched by it."""
    opts = dataclasses.replace(options) if options is not None else PPOOptions()
    for it in range(int(iterations)):
        ev = None
        if eval_batch is not None and it >= eval_start and it % eval_freq == 0:
            eval_batch.copy_policy_net_from(batch)
            ev = eval_statistics(eval_batch.evaluate_net(eval_episodes_per_alpha))
        if lr_schedule is not None:
            opts.lr = float(lr_schedule(1.0 - it / float(iterations)))
        summary, stats = batch.ppo_iterate(n_steps, opts)
        stats["lr"] = opts.lr
        if ev is not None:
            stats.update(ev)
        yield summary, stats
