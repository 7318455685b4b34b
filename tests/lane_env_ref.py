"""Reference side of the lane-env tests (test_lane_env_host.py, test_gpu_lane_env.py): the
alpha an episode runs at, from the oracle's keyed stream, and recorded steps passed through
cpr_amd/wrappers.py and ppo.py's `cut`. Nothing here calls the library under test."""

import oracle_py as O
from cpr_amd import wrappers

TAG_ASSUME = 0x70000000
SCHEMES = ["engine", "sparse_relative", "sparse_per_progress", "dense_per_progress"]
SHAPES = ["none", "per_alpha", "cut"]


def alpha_u(seed, episode):
    w = O.keyed_block(seed, int(episode), 0, TAG_ASSUME)
    return O.u53(int(w[0]), int(w[1]))


def alpha_index(seed, episode, n_alpha):
    """include/cpr_hip.h: entry min(n_alpha - 1, (int)(u n_alpha))."""
    return min(n_alpha - 1, int(alpha_u(seed, episode) * n_alpha))


class Script:
    """An env that replays recorded steps. episodes = [(alpha, [(reward, done, era, erd,
    progress, n_activations), ...]), ...]; reset() moves to the next episode."""

    action_space = observation_space = None

    def __init__(self, episodes):
        self.episodes, self.i = episodes, -1
        self.core_kwargs = {}

    @property
    def unwrapped(self):
        return self

    def reset(self):
        self.i += 1
        self.t = 0

    def step(self, action):
        alpha, steps = self.episodes[self.i]
        r, d, ra, rd, prog, acts = steps[self.t]
        self.t += 1
        return None, r, d, dict(episode_reward_attacker=ra, episode_reward_defender=rd,
                                episode_progress=prog, episode_n_activations=acts, alpha=alpha)


def cut(r, info):
    """ppo.py:221-232: nothing for an honest-looking episode's reward, 90 % close to it."""
    if r <= 0.0 or info["episode_progress"] <= 0.0:
        return 0.0
    if info["episode_n_activations"] / info["episode_progress"] <= 1.05:
        return r * 0.9 / info["alpha"]
    return r / info["alpha"]


def wrap(env, scheme, shape, target=None):
    if scheme == "sparse_relative":
        env = wrappers.SparseRelativeRewardWrapper(env)
    elif scheme == "sparse_per_progress":
        env = wrappers.SparseRewardPerProgressWrapper(env)
    elif scheme == "dense_per_progress":
        env = wrappers.DenseRewardPerProgressWrapper(env, episode_len=target)
    else:
        assert scheme == "engine"
    if shape == "per_alpha":
        env = wrappers.MapRewardWrapper(env, lambda r, i: r / i["alpha"])
    elif shape == "cut":
        env = wrappers.MapRewardWrapper(env, cut)
    else:
        assert shape == "none"
    return env


def wrapped_rewards(episodes, scheme, shape, target=None):
    """The rewards the wrapped env pays over the recorded episodes, in order, as floats."""
    env = wrap(Script(episodes), scheme, shape, target)
    out = []
    for _, steps in episodes:
        env.reset()
        for _ in steps:
            out.append(float(env.step(0)[1]))
    return out
