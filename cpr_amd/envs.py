"""Gym-style environments over the device engine, mirroring gym/ocaml/cpr_gym/envs.py:
``Core`` (core-v0), ``env_fn`` (cpr-v0, cpr-nakamoto-v0) and a tiny registry. ``gym`` is
not installed in this image, so ``Env``/``Discrete``/``Box`` are minimal local classes
with the same call signatures (reset() -> obs, step(a) -> (obs, r, done, info)).
"""

import warnings

import numpy as np

from . import engine, protocols, wrappers


class Discrete:
    def __init__(self, n, seed=None):
        self.n = int(n)
        self._rng = np.random.default_rng(seed)

    def sample(self):
        return int(self._rng.integers(self.n))

    def contains(self, x):
        return 0 <= int(x) < self.n


class Box:
    def __init__(self, low, high, dtype=np.float64):
        self.low = np.asarray(low, dtype=dtype)
        self.high = np.asarray(high, dtype=dtype)
        self.shape = self.low.shape
        self.dtype = dtype

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))


class Env:
    metadata = {}
    action_space = None
    observation_space = None

    def reset(self):
        raise NotImplementedError

    def step(self, action):
        raise NotImplementedError

    @property
    def unwrapped(self):
        return self


class Core(Env):
    """envs.py:9-96: one episode at a time; each reset builds a fresh engine instance."""

    metadata = {"render.modes": ["ascii"]}

    def __init__(self, proto=None, alpha=0.25, gamma=0.5, activation_delay=1.0, **kwargs):
        if proto is None:
            proto = protocols.nakamoto(unit_observation=True)
        self.core_kwargs = kwargs
        self.core_kwargs["proto"] = proto
        self.core_kwargs["alpha"] = alpha
        self.core_kwargs["gamma"] = gamma
        self.core_kwargs["activation_delay"] = activation_delay
        if not any(k in kwargs for k in ("max_time", "max_progress", "max_steps")):
            raise ValueError(
                "cpr_gym: set at least one of kwargs max_progress, max_steps, and max_time."
            )
        for k in ("max_time", "max_progress", "max_steps"):
            if k in kwargs and kwargs[k] is None:
                kwargs.pop(k)
        self.ocaml_env = None
        Core.reset(self)
        self.action_space = Discrete(engine.n_actions(self.ocaml_env))
        self.observation_space = Box(
            np.array(engine.observation_low(self.ocaml_env)),
            np.array(engine.observation_high(self.ocaml_env)),
        )
        self.version = engine.cpr_lib_version

    def policies(self):
        return engine.policies(self.ocaml_env).keys()

    def policy(self, obs, name="honest"):
        try:
            fn = engine.policies(self.ocaml_env)[name]
        except KeyError:
            raise ValueError(
                name + " is not a valid policy; choose from " + ", ".join(self.policies())
            )
        return fn(obs)

    def reset(self):
        kwargs = dict(self.core_kwargs)
        d = kwargs.pop("defenders", None)
        if d is None:
            g = kwargs["gamma"]
            if g >= 1:
                raise ValueError("gamma must be smaller than 1")
            d = max(2, int(np.ceil(1 / (1 - g))))
            if d >= 100:
                warnings.warn(f"Expensive assumptions: gamma={g} implies defenders>={d}")
        self.ocaml_env = engine.create(defenders=d, **kwargs)
        return np.array(engine.reset(self.ocaml_env))

    def step(self, a):
        obs, r, d, i = engine.step(self.ocaml_env, a)
        return np.array(obs), r, d, i

    def render(self, mode="ascii"):
        print(engine.to_string(self.ocaml_env))


class FC16SSZwPT(Env):
    """gym/rust/cpr_gym_rs/envs.py FC16SSZwPT over one device lane (CPR_PROTO_FC16_ENV), with
    gymnasium's call shape: ``reset() -> (obs, {})``, ``step(a) -> (obs, r, terminated,
    truncated, {})``. Actions index the offered list [Wait, Adopt, Override if a > h, Match if
    a >= h]; an index beyond the list acts as Wait. ``max_steps`` (None: unbounded, as the
    reference env) truncates an episode; ``truncated`` is the lane's capacity status. Episode
    e of the env runs on the keyed stream of (seed, e)."""

    def __init__(self, alpha=0.25, gamma=0.5, horizon=100, max_steps=None, seed=0, ctx=None):
        from . import _lib as L
        from . import device

        cfg, keep = device.make_config(protocol=L.PROTO_FC16_ENV, alpha=alpha, gamma=gamma,
                                       horizon=horizon, max_steps=max_steps, seed=seed,
                                       policy=L.FC16_POLICY_HONEST, n_lanes=1)
        self._capacity = L.ST_CAPACITY
        self.batch = device.Batch(cfg, ctx=ctx, keep=keep)
        self.action_space = Discrete(4)
        self.observation_space = Box(np.zeros(3), np.ones(3))
        self._episode = -1

    def reset(self, *args, seed=None, options=None):
        self._episode += 1
        obs = self.batch.reset(episode_ids=[self._episode])
        return obs[0], {}

    def step(self, action):
        obs, r, done, info = self.batch.step([int(action)])
        truncated = bool(info["status"][0] & self._capacity)
        return obs[0], float(r[0]), bool(done[0]) and not truncated, truncated, {}


def generic_encode_action(a):
    """generic/mod.rs:236-248 on the integer form (0 Continue, -(i+1) Release(i), +(i+1)
    Consider(i)): x / (1 + |x|) in float32, as generic_lane.h generic_encode_action."""
    a = max(-256, min(256, int(a)))
    x = np.float32(a)
    return np.float32(x / np.float32(np.float32(1.0) + abs(x))) if a else np.float32(0.0)


def generic_decode_action(a):
    """generic/mod.rs:250-279: a float32 action in [-1, 1] to the integer form (ValueError
    outside, as the reference asserts), as generic_lane.h generic_decode_action."""
    a = np.float32(a)
    if not (a >= np.float32(-1.0)) or not (a <= np.float32(1.0)):
        raise ValueError(f"invalid action: {a} outside [-1, 1]")
    if abs(a) == np.float32(1.0):
        return 256 if a > 0 else -256
    with np.errstate(divide="ignore", over="ignore"):
        x = np.float32(-a) / np.float32(a - np.float32(1.0)) if a >= 0 else \
            a / np.float32(a + np.float32(1.0))
    r = np.trunc(x)  # f32::round: half away from zero (x - trunc(x) is exact)
    if abs(np.float32(x - r)) >= np.float32(0.5):
        r = r + np.copysign(np.float32(1.0), x)
    return int(max(-256.0, min(256.0, float(r))))


def generic_honest_action(fields):
    """Honest play on one lane's ``Batch.observe_fields`` row: Release(0) while something can
    be released, else Consider(0) while something can be considered, else Continue."""
    return -1 if fields[3] > 0 else (1 if fields[4] > 0 else 0)


class Generic(Env):
    """gym/rust/cpr_gym_rs/envs.py Generic over one device lane (CPR_PROTO_GENERIC_NAKAMOTO),
    with gymnasium's call shape and the reference's surface: ``step([a])`` takes the float
    action of generic/mod.rs:227 (decoded with ``generic_decode_action``), returns the reward
    r / alpha / horizon in float32 (mod.rs:551) and the info keys progress, reward_attacker,
    reward_defender, rewrite and time (mod.rs:542-548). ``max_steps`` truncates an episode
    (the reference registers Nakamoto-v0 with max_episode_steps = 1000); ``truncated`` is the
    lane's capacity status. Episode e of the env runs on the keyed stream of (seed, e)."""

    def __init__(self, protocol="nakamoto", alpha=0.25, gamma=0.5, horizon=25, max_steps=1000,
                 seed=0, ctx=None):
        from . import _lib as L
        from . import device

        if protocol != "nakamoto":
            raise ValueError("Generic: only protocol='nakamoto' runs on the device")
        cfg, keep = device.make_config(protocol=L.PROTO_GENERIC_NAKAMOTO, alpha=alpha,
                                       gamma=gamma, horizon=horizon, max_steps=max_steps,
                                       seed=seed, policy=0, k=1, n_lanes=1)
        self._capacity = L.ST_CAPACITY
        self.alpha, self.horizon = np.float32(alpha), np.float32(horizon)
        self.batch = device.Batch(cfg, ctx=ctx, keep=keep)
        self.action_space = Box(np.float32([-1.0]), np.float32([1.0]))
        self.observation_space = Box(self.low(), self.high())
        self._episode = -1

    def low(self):
        return np.array(self.batch.observation_spec()[2], dtype=np.float32)

    def high(self):
        return np.array(self.batch.observation_spec()[3], dtype=np.float32)

    @staticmethod
    def encode_action_release(i):
        return float(generic_encode_action(-(int(i) + 1)))

    @staticmethod
    def encode_action_consider(i):
        return float(generic_encode_action(int(i) + 1))

    @staticmethod
    def encode_action_continue():
        return 0.0

    @staticmethod
    def describe_action(a):
        a = generic_decode_action(np.asarray(a, dtype=np.float32).reshape(-1)[0])
        return "Continue" if a == 0 else (f"Release({-a - 1})" if a < 0 else f"Consider({a - 1})")

    def reset(self, *args, seed=None, options=None):
        self._episode += 1
        obs = self.batch.reset(episode_ids=[self._episode])
        self._sums, self._n_blocks = np.zeros(3), 1
        return obs[0].astype(np.float32), {}

    def step(self, action):
        a = generic_decode_action(np.asarray(action, dtype=np.float32).reshape(-1)[0])
        obs, r, done, info = self.batch.step([a])
        sums = np.array([info["episode_progress"][0], info["episode_reward_attacker"][0],
                         info["episode_reward_defender"][0]])
        d, self._sums = sums - self._sums, sums
        f = self.batch.observe_fields()[0]
        truncated = bool(info["status"][0] & self._capacity)
        out = dict(progress=float(d[0]), reward_attacker=float(d[1]), reward_defender=float(d[2]),
                   rewrite=int(f[6]), time=int(f[5] > self._n_blocks))
        self._n_blocks = int(f[5])  # every Continue, also a guarded one, mines one block
        rew = np.float32(np.float32(np.float32(r[0]) / self.alpha) / self.horizon)
        return (obs[0].astype(np.float32), float(rew), bool(done[0]) and not truncated, truncated,
                out)


def env_fn(
    protocol="nakamoto",
    protocol_args=None,
    _protocol_args=dict(unit_observation=True),
    activation_delay=1.0,
    episode_len=128,
    alpha=0.45,
    gamma=0.5,
    pretend_alpha=None,
    pretend_gamma=None,
    defenders=None,
    reward="sparse_relative",
    normalize_reward=True,
):
    """envs.py:99-163: Core + AssumptionScheduleWrapper + reward wrapper (+ r/alpha)."""
    ctor = getattr(protocols, protocol)
    args = dict(_protocol_args) if protocol_args is None else {**_protocol_args, **protocol_args}
    reward_wrappers = {
        "sparse_relative": (wrappers.SparseRelativeRewardWrapper, dict(max_steps=episode_len)),
        "sparse_per_progress": (wrappers.SparseRewardPerProgressWrapper, dict(max_steps=episode_len)),
        "dense_per_progress": (
            lambda env: wrappers.DenseRewardPerProgressWrapper(env, episode_len=episode_len),
            dict(max_steps=None),
        ),
    }
    wrap, env_args = reward_wrappers[reward]
    env = Core(proto=ctor(**args), activation_delay=1.0, alpha=0.0, gamma=0.0,
               defenders=defenders, **env_args)
    env = wrappers.AssumptionScheduleWrapper(env, alpha=alpha, gamma=gamma,
                                             pretend_alpha=pretend_alpha,
                                             pretend_gamma=pretend_gamma)
    env.reset()
    env = wrap(env)
    if normalize_reward:
        env = wrappers.MapRewardWrapper(env, lambda r, i: r / i["alpha"])
    return env


def device_env_fn(
    n_envs,
    ctx=None,
    seed=0,
    protocol="nakamoto",
    protocol_args=None,
    _protocol_args=dict(unit_observation=True),
    activation_delay=1.0,
    episode_len=128,
    alpha=0.45,
    gamma=0.5,
    pretend_alpha=None,
    pretend_gamma=None,
    defenders=None,
    reward="sparse_relative",
    normalize_reward=True,
    shape=None,
    eval=False,
):
    """``env_fn`` (cpr-v0) over ``n_envs`` device lanes: returns ``(batch, extras)``, a
    configured ``device.Batch`` whose lane env (``Batch.set_lane_env``) holds the assumption
    schedule and the reward wrapper, and the extras tuple of the ``PolicyNet`` that goes with
    it (``PolicyNet(..., extra=extras)``, then ``batch.rollout_net``).

    Built the way ``env_fn`` builds cpr-v0: max_steps = episode_len for the sparse rewards,
    max_steps = 100 episode_len and max_progress = episode_len for the dense one, defenders
    derived from gamma, ``normalize_reward`` -> r / alpha. ``shape`` ("none", "per_alpha",
    "cut"; ppo.py's raw is "per_alpha") overrides ``normalize_reward``. ``alpha`` is a float,
    a sequence (one entry is chosen per episode, like ppo.py's ``random.choice``; the
    reference's wrapper cycles a sequence instead) or a zero-argument callable. Deviation: a
    callable is sampled 4,096 times into the table here, and episodes choose among those
    draws by (seed, episode). Gamma is fixed, as in ppo.py.

    ``eval=True`` builds ppo.py's eval env for ``Batch.evaluate_net``: a sequence ``alpha``
    cycles (episode e runs at entry e mod len(alpha), the reference wrapper's
    itertools.cycle; ppo.py's Range is the caller's ``numpy.arange`` grid passed as a list),
    and the reward shape is "per_alpha" whatever ``shape`` says (ppo.py:218-219). Give an eval
    batch its own ``seed``, or it replays the training batch's draws."""
    from . import _lib as L
    from . import device

    if callable(gamma) or np.ndim(gamma) != 0:
        raise ValueError("device_env_fn: gamma is fixed per batch (a float)")
    if callable(alpha):
        table = [float(alpha()) for _ in range(L.LANE_ENV_MAX_ALPHA)]
    else:
        table = [float(a) for a in np.atleast_1d(alpha)]
    ctor = getattr(protocols, protocol)
    args = dict(_protocol_args) if protocol_args is None else {**_protocol_args, **protocol_args}
    proto = ctor(**args)
    fc16 = proto.protocol_id == L.PROTO_FC16_ENV
    if fc16 and reward == "dense_per_progress":
        raise ValueError("device_env_fn: the FC16 model has no progress target "
                         "(dense_per_progress)")
    if proto.protocol_id == L.PROTO_GENERIC_NAKAMOTO and reward == "dense_per_progress":
        raise ValueError("device_env_fn: the generic env has no progress target "
                         "(dense_per_progress)")
    if reward not in ("sparse_relative", "sparse_per_progress", "dense_per_progress"):
        raise KeyError(reward)
    dense = reward == "dense_per_progress"
    if eval:
        if callable(alpha):
            raise ValueError("device_env_fn: eval=True needs a float or a sequence of alphas")
        shape = "per_alpha"
    elif shape is None:
        shape = "per_alpha" if normalize_reward else "none"
    cfg, keep = device.make_config(
        protocol=proto.protocol_id,
        k=proto.params.get("k", 8),
        subblock_selection=proto.params.get("selection_id", 1),
        reward_scheme=proto.params.get("reward_scheme", L.REWARD_CONSTANT),
        alpha=table[0],
        gamma=float(gamma),
        defenders=defenders,
        policy=L.POLICY_HONEST,
        horizon=proto.params.get("horizon", 100.0),
        activation_delay=activation_delay,
        max_steps=episode_len * 100 if dense else episode_len,
        max_progress=episode_len if dense else None,
        seed=seed,
        unit_observation=proto.unit_observation,
        n_lanes=n_envs,
    )
    batch = device.Batch(cfg, ctx=ctx, keep=keep)
    batch.set_lane_env(alphas=table, alpha_column=None if pretend_alpha is not None else 0,
                       reward=reward, shape=shape, dense_target=episode_len if dense else None,
                       schedule="cycle" if eval else "choice")
    extras = (table[0] if pretend_alpha is None else float(pretend_alpha),
              float(gamma) if pretend_gamma is None else float(pretend_gamma))
    return batch, extras


_registry = {
    "core-v0": (Core, {}),
    "cpr-v0": (env_fn, {}),
    "cpr-nakamoto-v0": (
        env_fn,
        dict(protocol="nakamoto", _protocol_args=dict(unit_observation=True), reward="sparse_relative"),
    ),
    "cpr-tailstorm-v0": (
        env_fn,
        dict(
            protocol="tailstorm",
            _protocol_args=dict(k=8, reward="discount", subblock_selection="heuristic",
                                unit_observation=True),
            reward="sparse_per_progress",
        ),
    ),
}


def make(env_id, **kwargs):
    """gym.make replacement for the ids registered by envs.py:166-191."""
    env_id = env_id.split(":")[-1]
    ctor, defaults = _registry[env_id]
    return ctor(**{**defaults, **kwargs})
