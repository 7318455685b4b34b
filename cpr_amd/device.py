"""Device contexts and episode batches over libcpr_hip.

A ``Context`` is one HIP device (one process per GPU, see ``cpr_amd.parallel``); a
``Batch`` is one configuration of the episode engine (protocol, network, attack policy,
alpha/gamma, termination) on that device. ``Batch.run`` fuses the reference's Python
reset/step/policy loop (gym/ocaml/test/test_benchmark.py:5-15, rl-eval) into one kernel
launch; ``Batch.reset``/``Batch.step`` expose the per-step gym API over many lanes.
"""

import ctypes
import math
import os
import warnings

import numpy as np

from . import _lib as L

_default_ctx = {}


class Context:
    def __init__(self, device=0):
        self.device = device
        h = ctypes.c_void_p()
        L.check(L.lib().cpr_ctx_create(device, ctypes.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            L.lib().cpr_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rerun_hbm_retries(self):
        """Cumulative exact re-runs whose event heap outgrew LDS (cpr_rerun_hbm_retries)."""
        v = ctypes.c_int64()
        L.check(L.lib().cpr_rerun_hbm_retries(self.handle, ctypes.byref(v)))
        return v.value

    def rerun_stats(self):
        """Cumulative (episodes, flushes, kernel ms) of exact re-runs on this context
        (cpr_rerun_stats): episodes the fused kernels handed to the exact event engine."""
        e, f, ms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        L.check(L.lib().cpr_rerun_stats(self.handle, ctypes.byref(e), ctypes.byref(f),
                                        ctypes.byref(ms)))
        return e.value, f.value, ms.value

    def synchronize(self):
        """Launches what ``Batch.run_async`` deferred, runs the exact re-runs of flagged
        episodes and waits: summaries and records are complete afterwards."""
        L.check(L.lib().cpr_synchronize(self.handle))

    def stream_fill(self, seed, episode, idx0, tag, n, with_exp=False):
        """Keyed-stream Philox blocks computed on the device."""
        out = np.zeros((n, 4), dtype=np.uint32)
        ex = np.zeros(n, dtype=np.float64) if with_exp else None
        L.check(
            L.lib().cpr_stream_fill(
                self.handle, seed, episode, idx0, tag, n, L.ptr(out), L.ptr(ex) if with_exp else None
            )
        )
        return (out, ex) if with_exp else out

    MDP_VI_PATHS = {"auto": L.MDP_VI_AUTO, "resident": L.MDP_VI_RESIDENT,
                    "global": L.MDP_VI_GLOBAL}

    def mdp_value_iteration(self, dst, used, valid, rew, prg, prb, *, stop_delta, discount=1.0,
                            max_iter=0, path="auto"):
        """Value iteration on the device (cpr_mdp_value_iteration) for P points that share one
        topology in the dense padded form: dst, used, rew, prg [S][A][T], valid [S][A], prb
        [P][S][A][T] (or [S][A][T] for one point). Returns a dict of value, progress, policy
        [P][S], iter, delta, status [P], path_used ("resident" / "global") and kernel_ms.
        Invalid input raises ``CprError`` before anything is launched."""
        m, keep = self._mdp_c(dst, used, valid, rew, prg, prb)
        S, P = m.S, m.P
        if path not in self.MDP_VI_PATHS:
            raise ValueError(f"path: expected one of {sorted(self.MDP_VI_PATHS)}")
        o = L.MdpViOptsC(float(stop_delta), float(discount), int(max_iter),
                         self.MDP_VI_PATHS[path])
        out = dict(value=np.zeros((P, S)), progress=np.zeros((P, S)),
                   policy=np.zeros((P, S), np.int32), iter=np.zeros(P, np.int64),
                   delta=np.zeros(P), status=np.zeros(P, np.int32))
        r = L.MdpViResultC(*(out[k].ctypes.data for k in
                             ("value", "progress", "policy", "iter", "delta", "status")))
        L.check(L.lib().cpr_mdp_value_iteration(self.handle, ctypes.byref(m), ctypes.byref(o),
                                                ctypes.byref(r)))
        out["path_used"] = "resident" if r.path_used == L.MDP_VI_RESIDENT else "global"
        out["kernel_ms"] = r.kernel_ms
        return out

    @staticmethod
    def _mdp_c(dst, used, valid, rew, prg, prb):
        """The cpr_mdp of the dense padded arrays and the arrays it points into."""
        dst = np.asarray(dst)
        if dst.dtype.kind not in "iu":
            raise ValueError("dst: expected an integer array")
        if dst.size and (dst.min() < -2 ** 31 or dst.max() >= 2 ** 31):
            # a cast would wrap it, perhaps into [0, S); clamp it to a value the library refuses
            # in a used slot and ignores in a padding slot
            dst = np.where((dst < 0) | (dst >= 2 ** 31), -1, dst)
        dst = np.ascontiguousarray(dst, dtype=np.int32)
        if dst.ndim != 3:
            raise ValueError("dst: expected [S][A][T]")
        S, A, T = dst.shape
        used = np.ascontiguousarray(used, dtype=np.uint8)
        valid = np.ascontiguousarray(valid, dtype=np.uint8)
        rew = np.ascontiguousarray(rew, dtype=np.float64)
        prg = np.ascontiguousarray(prg, dtype=np.float64)
        prb = np.ascontiguousarray(prb, dtype=np.float64)
        if prb.ndim == 3:
            prb = prb[None]
        if used.shape != dst.shape or rew.shape != dst.shape or prg.shape != dst.shape \
                or valid.shape != (S, A) or prb.ndim != 4 or prb.shape[1:] != dst.shape:
            raise ValueError("the arrays' shapes do not agree with dst [S][A][T]")
        keep = (dst, used, valid, rew, prg, prb)
        return L.MdpC(S, A, T, prb.shape[0], *(x.ctypes.data for x in keep)), keep

    MDP_PE_STATES = {"reachable": L.MDP_PE_REACHABLE, "all": L.MDP_PE_ALL}

    def mdp_policy_evaluation(self, dst, used, valid, rew, prg, prb, point, policy, *, theta,
                              discount=1.0, max_iter=0, states="reachable", start_state=None,
                              start_prob=None, path="auto"):
        """Policy evaluation on the device (cpr_mdp_policy_evaluation) for E evaluations over P
        points of one topology (the arrays of ``mdp_value_iteration``): ``point`` [E] indexes
        the points, ``policy`` [E][S] holds the action slot a state plays or -1.
        ``states="reachable"`` evaluates the states reached from ``start_state`` [E][n] with
        ``start_prob`` [E][n] > 0 (one row [n] serves every evaluation), ``"all"`` every state.
        ``max_iter`` 0: until delta < theta. Returns a dict of reward, progress [E][S], iter,
        delta, status [E], path_used ("resident" / "global") and kernel_ms. Invalid input
        raises ``CprError`` before anything is launched."""
        m, keep = self._mdp_c(dst, used, valid, rew, prg, prb)
        S = m.S
        point = np.ascontiguousarray(point, dtype=np.int32)
        policy = np.asarray(policy)
        if policy.dtype.kind not in "iu":
            raise ValueError("policy: expected an integer array")
        # an entry beyond int32 names no slot either way: keep it refused after the cast
        policy = np.ascontiguousarray(np.clip(policy, -1, 2 ** 31 - 1), dtype=np.int32)
        if policy.ndim == 1:
            policy = policy[None]
        E = policy.shape[0]
        if point.ndim != 1 or policy.ndim != 2 or policy.shape[1] != S or point.shape[0] != E:
            raise ValueError("expected point [E] and policy [E][S]")
        if path not in self.MDP_VI_PATHS:
            raise ValueError(f"path: expected one of {sorted(self.MDP_VI_PATHS)}")
        if states not in self.MDP_PE_STATES:
            raise ValueError(f"states: expected one of {sorted(self.MDP_PE_STATES)}")
        n_start, ss, sp = 0, None, None
        if states == "reachable":
            if start_state is None or start_prob is None:
                raise ValueError('states="reachable" needs start_state and start_prob')
            ss = np.asarray(start_state)
            if ss.dtype.kind not in "iu":
                raise ValueError("start_state: expected an integer array")
            ss = np.clip(ss, -1, 2 ** 31 - 1).astype(np.int32)
            sp = np.asarray(start_prob, dtype=np.float64)
            if ss.ndim == 1:
                ss, sp = np.tile(ss, (E, 1)), np.tile(sp, (E, 1))
            ss, sp = np.ascontiguousarray(ss), np.ascontiguousarray(sp)
            if ss.ndim != 2 or ss.shape[0] != E or sp.shape != ss.shape:
                raise ValueError("expected start_state and start_prob [E][n] or [n]")
            n_start = ss.shape[1]
        job = L.MdpPeC(E, point.ctypes.data, policy.ctypes.data, self.MDP_PE_STATES[states],
                       n_start, ss.ctypes.data if ss is not None else None,
                       sp.ctypes.data if sp is not None else None)
        o = L.MdpPeOptsC(float(theta), float(discount), int(max_iter), self.MDP_VI_PATHS[path])
        out = dict(reward=np.zeros((E, S)), progress=np.zeros((E, S)),
                   iter=np.zeros(E, np.int64), delta=np.zeros(E), status=np.zeros(E, np.int32))
        r = L.MdpPeResultC(*(out[k].ctypes.data for k in
                             ("reward", "progress", "iter", "delta", "status")))
        L.check(L.lib().cpr_mdp_policy_evaluation(self.handle, ctypes.byref(m), ctypes.byref(job),
                                                  ctypes.byref(o), ctypes.byref(r)))
        del keep
        out["path_used"] = "resident" if r.path_used == L.MDP_VI_RESIDENT else "global"
        out["kernel_ms"] = r.kernel_ms
        return out


def default_context():
    dev = int(os.environ.get("LOCAL_RANK", "0"))
    if dev not in _default_ctx:
        n = ctypes.c_int()
        L.check(L.lib().cpr_device_count(ctypes.byref(n)))
        if n.value == 0:
            raise RuntimeError("cpr_amd: no HIP device visible")
        _default_ctx[dev] = Context(dev % n.value)
    return _default_ctx[dev]


def make_config(
    alpha,
    gamma=0.5,
    defenders=None,
    policy=L.POLICY_SAPIRSHTEIN_2016_SM1,
    network=L.NET_SELFISH_MINING,
    mode=L.MODE_GYM,
    activation_delay=1.0,
    propagation_delay=1e-9,
    max_steps=None,
    max_progress=None,
    max_time=None,
    activations=0,
    seed=0,
    unit_observation=True,
    n_lanes=0,
    table=None,
    protocol=L.PROTO_NAKAMOTO,
    reward_scheme=L.REWARD_CONSTANT,
    k=8,
    table_dim=None,
    subblock_selection=1,
    delay_lo=math.nan,
    delay_hi=math.nan,
    horizon=100.0,
):
    """Build a cpr_config. ``defenders=None`` applies the gym's rule
    d = max(2, ceil(1 / (1 - gamma))) (gym/ocaml/cpr_gym/envs.py:70-76).
    B_k tables (protocol=PROTO_BK) hold dim*dim*(k+1)*(k+1)*3 actions
    (include/cpr_hip.h CPR_BK_POLICY_TABLE)."""
    if defenders is None and network == L.NET_SELFISH_MINING:
        if gamma >= 1:
            raise ValueError("gamma must be smaller than 1")
        defenders = max(2, int(math.ceil(1 / (1 - gamma))))
    c = L.Config()
    c.protocol = protocol
    c.reward_scheme = reward_scheme
    c.network = network
    c.mode = mode
    c.policy = policy
    c.unit_observation = 1 if unit_observation else 0
    c.alpha = alpha
    c.gamma = gamma
    c.defenders = defenders or 1
    c.activation_delay = activation_delay
    c.propagation_delay = propagation_delay
    c.max_steps = 0 if max_steps is None else int(max_steps)
    c.max_progress = 0.0 if max_progress is None else float(max_progress)
    c.max_time = 0.0 if max_time is None else float(max_time)
    c.activations = int(activations)
    c.seed = int(seed) & ((1 << 64) - 1)
    c.n_lanes = int(n_lanes)
    c.k = int(k)
    c.subblock_selection = int(subblock_selection)
    c.delay_lo = float(delay_lo)
    c.delay_hi = float(delay_hi)
    c.horizon = float(horizon)
    keep = None
    if table is not None and protocol in (L.PROTO_BK, L.PROTO_TAILSTORM):
        keep = np.ascontiguousarray(table, dtype=np.uint8).ravel()
        per = (k + 1) * (k + 1) * 3
        dim = int(round((keep.size // per) ** 0.5)) if table_dim is None else int(table_dim)
        if dim * dim * per != keep.size:
            raise ValueError("B_k / Tailstorm policy table must have dim*dim*(k+1)*(k+1)*3 "
                             "entries")
        c.policy = L.BK_POLICY_TABLE if protocol == L.PROTO_BK else L.TS_POLICY_TABLE
        c.policy_table = keep.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        c.policy_table_dim = dim
    elif table is not None and protocol in (L.PROTO_FC16, L.PROTO_FC16_ENV):
        keep = np.ascontiguousarray(table, dtype=np.uint8).ravel()
        dim = int(round((keep.size // 3) ** 0.5))
        if dim * dim * 3 != keep.size:
            raise ValueError("FC16 policy table must have dim*dim*3 entries")
        c.policy = L.FC16_POLICY_TABLE
        c.policy_table = keep.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        c.policy_table_dim = dim
    elif table is not None and protocol == L.PROTO_ETHEREUM:
        keep = np.ascontiguousarray(table, dtype=np.uint8).ravel()
        dim = int(round((keep.size // 2) ** 0.5))
        if dim * dim * 2 != keep.size:
            raise ValueError("Ethereum policy table must have dim*dim*2 entries")
        c.policy = L.ETH_POLICY_TABLE
        c.policy_table = keep.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        c.policy_table_dim = dim
    elif table is not None:
        keep = np.ascontiguousarray(table, dtype=np.uint8)
        dim = int(round((keep.size // 2) ** 0.5))
        if dim * dim * 2 != keep.size:
            raise ValueError("policy table must have dim*dim*2 entries")
        c.policy = L.POLICY_TABLE
        c.policy_table = keep.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        c.policy_table_dim = dim
    return c, keep


def _f32(name, a):
    """A C-contiguous float32 numpy copy of a numpy array or torch tensor."""
    if hasattr(a, "detach"):  # torch tensor (torch is not imported here)
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype.kind not in "fiu":
        raise TypeError(f"{name}: expected a numeric array, got dtype {a.dtype}")
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name}: non-finite value")
    return a


class PolicyNet:
    """An actor-critic MLP for ``Batch.set_policy_net``: SB3's MlpPolicy shape (separate pi
    and vf trunks, ReLU, linear heads; experiments/train/ppo.py:400-416).

    ``pi`` / ``vf``: lists of (W, b) per hidden layer, W [out, in] as torch.nn.Linear (numpy
    arrays or torch tensors); ``pi_head`` = (W [n_actions, width_pi], b), ``vf_head`` =
    (W [1, width_vf], b); ``extra``: constants appended to every observation (the alpha,
    gamma features of AssumptionScheduleWrapper). Both trunks have the same depth (1..4);
    every width is a multiple of 16 in [16, 512]."""

    def __init__(self, pi, pi_head, vf, vf_head, extra=()):
        self.extra = tuple(float(x) for x in extra)
        if len(self.extra) > L.POLICY_NET_MAX_EXTRA:
            raise ValueError(f"extra: at most {L.POLICY_NET_MAX_EXTRA} values")
        if not all(math.isfinite(x) for x in self.extra):
            raise ValueError("extra: non-finite value")
        if len(pi) != len(vf):
            raise ValueError(f"pi / vf: depths differ ({len(pi)} and {len(vf)} hidden layers)")
        if not 1 <= len(pi) <= L.POLICY_NET_MAX_DEPTH:
            raise ValueError(f"pi: depth {len(pi)}, expected 1..{L.POLICY_NET_MAX_DEPTH}")
        self.depth = len(pi)
        self.pi = self._trunk("pi", pi)
        self.vf = self._trunk("vf", vf)
        if self.pi[0][0].shape[1] != self.vf[0][0].shape[1]:
            raise ValueError("vf[0]: input width differs from pi[0]")
        self.n_in = self.pi[0][0].shape[1]
        self.width_pi = self.pi[0][0].shape[0]
        self.width_vf = self.vf[0][0].shape[0]
        self.pi_head = self._layer("pi_head", pi_head, self.width_pi, None)
        self.vf_head = self._layer("vf_head", vf_head, self.width_vf, 1)
        self.n_actions = self.pi_head[0].shape[0]

    @staticmethod
    def _layer(name, wb, n_in, n_out):
        w, b = wb
        w, b = _f32(name + " weight", w), _f32(name + " bias", b)
        if w.ndim != 2 or b.ndim != 1 or b.shape[0] != w.shape[0]:
            raise ValueError(f"{name}: expected W [out, in] and b [out], got "
                             f"{list(w.shape)} and {list(b.shape)}")
        if n_in is not None and w.shape[1] != n_in:
            raise ValueError(f"{name}: input width {w.shape[1]}, expected {n_in}")
        if n_out is not None and w.shape[0] != n_out:
            raise ValueError(f"{name}: {w.shape[0]} outputs, expected {n_out}")
        return w, b

    @classmethod
    def _trunk(cls, name, layers):
        out = []
        for i, wb in enumerate(layers):
            w, b = cls._layer(f"{name}[{i}]", wb, out[-1][0].shape[0] if out else None, None)
            width = w.shape[0]
            if width % 16 != 0 or not 16 <= width <= 512:
                raise ValueError(f"{name}[{i}]: width {width} is not a multiple of 16 in "
                                 f"[16, 512]")
            if out and width != out[0][0].shape[0]:
                raise ValueError(f"{name}[{i}]: width {width} differs from {name}[0]'s "
                                 f"{out[0][0].shape[0]}")
            out.append((w, b))
        return out

    @classmethod
    def from_state_dict(cls, sd, extra=()):
        """From an SB3 ActorCriticPolicy state dict (or any torch module with its names):
        mlp_extractor.policy_net.{0,2,4,...}.{weight,bias}, mlp_extractor.value_net.*,
        action_net.*, value_net.*. stable_baselines3 is not imported."""
        def trunk(prefix):
            idx = sorted({int(k[len(prefix):].split(".")[0]) for k in sd if k.startswith(prefix)})
            if not idx:
                raise KeyError(f"state dict has no {prefix}*")
            return [(sd[f"{prefix}{i}.weight"], sd[f"{prefix}{i}.bias"]) for i in idx]

        return cls(pi=trunk("mlp_extractor.policy_net."),
                   pi_head=(sd["action_net.weight"], sd["action_net.bias"]),
                   vf=trunk("mlp_extractor.value_net."),
                   vf_head=(sd["value_net.weight"], sd["value_net.bias"]), extra=extra)

    def state_dict(self):
        """{name: f32 array} in SB3's ActorCriticPolicy naming: the inverse of
        ``from_state_dict`` (wrap the arrays in ``torch.from_numpy`` for ``load_state_dict``)."""
        sd = {}
        for prefix, trunk in (("mlp_extractor.policy_net.", self.pi),
                              ("mlp_extractor.value_net.", self.vf)):
            for i, (w, b) in enumerate(trunk):
                sd[f"{prefix}{2 * i}.weight"] = w
                sd[f"{prefix}{2 * i}.bias"] = b
        sd["action_net.weight"], sd["action_net.bias"] = self.pi_head
        sd["value_net.weight"], sd["value_net.bias"] = self.vf_head
        return sd

    def zeros_like(self):
        """A network of the same shape and extras with zeroed parameters."""
        def z(wb):
            return np.zeros_like(wb[0]), np.zeros_like(wb[1])

        return PolicyNet([z(x) for x in self.pi], z(self.pi_head), [z(x) for x in self.vf],
                         z(self.vf_head), extra=self.extra)

    def cstruct(self):
        """The cpr_policy_net over this object's arrays (which must outlive the call)."""
        c = L.PolicyNetC()
        c.n_extra = len(self.extra)
        for i, x in enumerate(self.extra):
            c.extra[i] = x
        c.depth = self.depth
        c.width_pi = self.width_pi
        c.width_vf = self.width_vf
        for i in range(self.depth):
            c.pi_w[i], c.pi_b[i] = self.pi[i][0].ctypes.data, self.pi[i][1].ctypes.data
            c.vf_w[i], c.vf_b[i] = self.vf[i][0].ctypes.data, self.vf[i][1].ctypes.data
        c.pi_head_w, c.pi_head_b = self.pi_head[0].ctypes.data, self.pi_head[1].ctypes.data
        c.vf_head_w, c.vf_head_b = self.vf_head[0].ctypes.data, self.vf_head[1].ctypes.data
        return c

    def forward_f64(self, obs):
        """Reference forward in numpy float64 on the f32-rounded inputs: (logits, value)."""
        x = np.asarray(obs, dtype=np.float64).astype(np.float32).astype(np.float64)
        x = np.concatenate([x, np.tile(np.float32(self.extra).astype(np.float64),
                                       (x.shape[0], 1))], axis=1)
        outs = []
        for trunk, head in ((self.pi, self.pi_head), (self.vf, self.vf_head)):
            h = x
            for w, b in trunk:
                h = np.maximum(h @ w.astype(np.float64).T + b.astype(np.float64), 0.0)
            outs.append(h @ head[0].astype(np.float64).T + head[1].astype(np.float64))
        return outs[0], outs[1][:, 0]


class EvalResult:
    """What ``Batch.evaluate_net`` returns. ``per_alpha``: one dict per table entry with
    ``alpha``, ``n`` (valid episodes), ``mean_<column>`` / ``std_<column>`` for the columns of
    ``_lib.EVAL_COLUMNS`` and that alpha's ``summary`` (a ``Summary``); ``stats``: the same
    numbers as a structured array (``_lib.EVAL_ALPHA_DTYPE``); ``records``: a structured array
    (``_lib.EVAL_RECORD_DTYPE``), record i is episode first_episode + i, or None; ``total``:
    the sum of the per-alpha summaries."""

    def __init__(self, stats, summaries, records, total):
        self.stats, self.summaries, self.records, self.total = stats, summaries, records, total
        self.per_alpha = []
        for st, sm in zip(stats, summaries):
            d = {"alpha": float(st["alpha"]), "n": int(st["n"]), "summary": sm}
            for c, name in enumerate(L.EVAL_COLUMNS):
                d["mean_" + name] = float(st["mean"][c])
                d["std_" + name] = float(st["std"][c])
            self.per_alpha.append(d)


class Batch:
    def __init__(self, config, ctx=None, keep=None):
        self.ctx = ctx or default_context()
        self.config = config
        self._keep = keep
        h = ctypes.c_void_p()
        L.check(L.lib().cpr_batch_create(self.ctx.handle, ctypes.byref(config), ctypes.byref(h)))
        self.handle = h
        self.n_lanes = int(config.n_lanes)
        self.obs_len = self.observation_spec()[0]
        # int32 per lane of observe_fields: the observation's fields, except for the generic env
        self.n_fields = 7 if config.protocol == L.PROTO_GENERIC_NAKAMOTO else self.obs_len
        self._coverage_warned = False
        self._lane_env = False
        self._n_alpha = 1  # table entries of the lane env: evaluate_net's result count

    def close(self):
        if self.handle:
            # cpr_batch_destroy reads the batch's context (it launches what is pending there and
            # waits for its stream): a batch that outlived its context, e.g. one a failed test
            # left to the garbage collector after its fixture closed the context, is dropped
            # without the call, since the context's memory is gone
            if self.ctx.handle:
                L.lib().cpr_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- fused episodes
    def run(self, n_episodes, first_episode=0, records=False, summary=None):
        s = summary if summary is not None else L.Summary()
        rec = np.zeros(n_episodes, dtype=L.RECORD_DTYPE) if records else None
        L.check(
            L.lib().cpr_run_episodes(
                self.handle, n_episodes, first_episode, ctypes.byref(s), L.ptr(rec), 0
            )
        )
        return (s, rec) if records else s

    def replay(self, trace, records=True, summary=None):
        """Replay an exported activation/delay trace (cpr_replay): record e is trace
        episode e, run with this batch's protocol, mode and policy."""
        s = summary if summary is not None else L.Summary()
        rec = np.zeros(trace.n_episodes, dtype=L.RECORD_DTYPE) if records else None
        ct = trace.ctrace()
        L.check(L.lib().cpr_replay(self.handle, ctypes.byref(ct), ctypes.byref(s), L.ptr(rec), 0))
        return (s, rec) if records else s

    @property
    def n_nodes(self):
        """Nodes of the batch's network: 2, defenders + 1 (attacker first) or the clique."""
        c = self.config
        if c.network == L.NET_TWO_AGENTS:
            return 2
        return int(c.defenders) if c.network == L.NET_HONEST_CLIQUE else int(c.defenders) + 1

    def node_outputs(self, n_episodes=0, first_episode=0, trace=None):
        """Per-node outputs (cpr_node_outputs): (records, activations [n, n_nodes] int64,
        rewards [n, n_nodes] f64) of keyed episodes [first, first + n) or of a trace; the
        `activations` / `reward` columns of a csv_runner.ml row."""
        if trace is not None:
            n_episodes = trace.n_episodes
        nn = self.n_nodes
        rec = np.zeros(n_episodes, dtype=L.RECORD_DTYPE)
        acts = np.zeros((n_episodes, nn), dtype=np.int64)
        rews = np.zeros((n_episodes, nn), dtype=np.float64)
        ct = trace.ctrace() if trace is not None else None
        L.check(L.lib().cpr_node_outputs(
            self.handle, n_episodes, first_episode, ctypes.byref(ct) if ct is not None else None,
            nn, L.ptr(rec), L.ptr(acts), L.ptr(rews)))
        return rec, acts, rews

    def last_launch(self):
        """(kernel_ms, activations) of the last fused-episode launch (HIP events). After
        ``run_async`` it waits for that launch; a point that ran in a group of m sweep points
        reports the group's kernel time / m."""
        ms = ctypes.c_double()
        acts = ctypes.c_int64()
        L.check(L.lib().cpr_last_launch(self.handle, ctypes.byref(ms), ctypes.byref(acts)))
        return ms.value, acts.value

    def launch_shape(self):
        """(lanes, resident lanes) of the last episode-kernel launch (cpr_launch_shape)."""
        lanes = ctypes.c_int64()
        res = ctypes.c_int64()
        L.check(L.lib().cpr_launch_shape(self.handle, ctypes.byref(lanes), ctypes.byref(res)))
        return lanes.value, res.value

    def run_async(self, n_episodes, first_episode, summary_dev_ptr, records_dev_ptr=None):
        """cpr_run_episodes_async: the summary (a zeroed device cpr_summary) is complete after
        ``ctx.synchronize()``. The launch may be deferred until then: summary-only calls of
        one context on the gym's two-defender networks (gamma <= .5) that share seed, first
        episode and episode count (an alpha sweep with common random numbers) run as one
        kernel per group, with the same results: up to five points (gamma = 0) or two in one
        lane, and two (gamma = 0) or four adjacent lanes that run further points of the same
        episode and share its draws, so ten or eight calls make one launch; fewer pending
        calls run in groups of one lane's points. Any other call on the context or its
        batches launches what is pending first. ``CPR_NAK_FUSE`` (read at every call) is the
        most points per lane; 0 launches every call at once. ``CPR_NAK_FUSE_LANES`` (read at
        every call) caps the lanes per episode; 1 keeps the groups of one lane."""
        L.check(
            L.lib().cpr_run_episodes_async(
                self.handle, n_episodes, first_episode, summary_dev_ptr, records_dev_ptr
            )
        )

    # ---- lockstep gym lanes
    def reset(self, mask=None, episode_ids=None):
        obs = np.zeros((self.n_lanes, self.obs_len), dtype=np.float64)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        e = None if episode_ids is None else np.ascontiguousarray(episode_ids, dtype=np.uint64)
        L.check(L.lib().cpr_reset(self.handle, L.ptr(m), L.ptr(e), L.ptr(obs)))
        log_steps, _ = self.lockstep_coverage()
        ms = int(self.config.max_steps)
        if log_steps and 0 < ms < 2**30 and log_steps < ms and not self._coverage_warned:
            self._coverage_warned = True
            warnings.warn(f"{self.n_lanes} lockstep lanes x {ms}-step episodes exceed the "
                          f"action-log budget: lanes leaving the closed form after step "
                          f"{log_steps} keep its flags instead of an exact re-run",
                          RuntimeWarning, stacklevel=2)
        return obs

    def lockstep_coverage(self):
        """(action-log steps, exact-engine slots) of the lockstep lanes
        (cpr_lockstep_coverage); (0, 0) before the first reset or without exact lanes."""
        s, k = ctypes.c_int64(), ctypes.c_int64()
        L.check(L.lib().cpr_lockstep_coverage(self.handle, ctypes.byref(s), ctypes.byref(k)))
        return s.value, k.value

    def step(self, actions, with_info=True):
        n = self.n_lanes
        a = np.ascontiguousarray(actions, dtype=np.int32)
        obs = np.zeros((n, self.obs_len), dtype=np.float64)
        rew = np.zeros(n, dtype=np.float64)
        done = np.zeros(n, dtype=np.uint8)
        info = None
        si = None
        if with_info:
            info = {
                "episode_reward_attacker": np.zeros(n),
                "episode_reward_defender": np.zeros(n),
                "episode_progress": np.zeros(n),
                "episode_chain_time": np.zeros(n),
                "episode_sim_time": np.zeros(n),
                "episode_n_steps": np.zeros(n, dtype=np.int64),
                "episode_n_activations": np.zeros(n, dtype=np.int64),
                "head_height": np.zeros(n, dtype=np.int32),
                "head_miner": np.zeros(n, dtype=np.int32),
                "status": np.zeros(n, dtype=np.uint32),
            }
            si = L.StepInfo()
            for k, v in info.items():
                ct = np.ctypeslib.as_ctypes_type(v.dtype)
                setattr(si, k, v.ctypes.data_as(ctypes.POINTER(ct)))
        L.check(
            L.lib().cpr_step(
                self.handle, L.ptr(a), L.ptr(obs), L.ptr(rew), L.ptr(done),
                ctypes.byref(si) if si is not None else None,
            )
        )
        return obs, rew, done.astype(bool), info

    def observe_fields(self):
        f = np.zeros((self.n_lanes, self.n_fields), dtype=np.int32)
        L.check(L.lib().cpr_observe_fields(self.handle, L.ptr(f)))
        return f

    def policy_actions(self, policy, obs):
        o = np.ascontiguousarray(np.atleast_2d(obs), dtype=np.float64)
        if o.shape[1] != self.obs_len:
            raise ValueError("invalid dimensions")
        out = np.zeros(o.shape[0], dtype=np.int32)
        L.check(L.lib().cpr_policy_actions(self.handle, policy, L.ptr(o), o.shape[0], L.ptr(out)))
        return out

    def rollout(self, n_steps, outputs=False, summary=None, device_outputs=None):
        """Device rollout (cpr_rollout; Nakamoto, Ethereum, B_k and Tailstorm batches with
        n_lanes > 0): every lane takes n_steps steps with the batch policy, auto-resetting
        finished episodes at episode id + n_lanes. A first call without reset() starts lane
        i at episode i; later calls, step() and reset() continue from the lanes' state.
        ``outputs=True`` returns host arrays
        obs [n_steps, n_lanes, obs_len], reward [n_steps, n_lanes], done [n_steps, n_lanes];
        ``device_outputs=(obs_ptr, reward_ptr, done_ptr)`` writes to caller-owned device
        memory instead. Returns the summary (and the arrays if requested)."""
        s = summary if summary is not None else L.Summary()
        n = self.n_lanes
        if device_outputs is not None:
            o, r, d = (None if x is None else ctypes.c_void_p(int(x)) for x in device_outputs)
            L.check(L.lib().cpr_rollout(self.handle, int(n_steps), o, r, d, 1, ctypes.byref(s)))
            return s
        if not outputs:
            L.check(L.lib().cpr_rollout(self.handle, int(n_steps), None, None, None, 0,
                                        ctypes.byref(s)))
            return s
        obs = np.zeros((n_steps, n, self.obs_len))
        rew = np.zeros((n_steps, n))
        done = np.zeros((n_steps, n), dtype=np.uint8)
        L.check(L.lib().cpr_rollout(self.handle, int(n_steps), L.ptr(obs), L.ptr(rew),
                                    L.ptr(done), 0, ctypes.byref(s)))
        return s, obs, rew, done.astype(bool)

    # ---- neural-network policies (cpr_policy_net_set / _forward, cpr_rollout_net)
    def set_policy_net(self, net):
        """Upload a ``PolicyNet`` (replacing any earlier one). Its input width must be
        obs_len + len(extra) and its action head n_actions of this batch."""
        if not isinstance(net, PolicyNet):
            raise TypeError("net: expected a PolicyNet")
        n_act = self.observation_spec()[1]
        if net.n_in != self.obs_len + len(net.extra):
            raise ValueError(f"pi[0]/vf[0]: input width {net.n_in}, this batch needs obs_len "
                             f"{self.obs_len} + {len(net.extra)} extra")
        if net.n_actions != n_act:
            raise ValueError(f"pi_head: {net.n_actions} actions, this batch has {n_act}")
        L.check(L.lib().cpr_policy_net_set(self.handle, ctypes.byref(net.cstruct())))
        self._net = net

    def policy_net_forward(self, obs, deterministic=True, episode0=0, logits=False):
        """The network on observation rows [n, obs_len]: (actions int32, logp f64, value
        f64[, logits f32 [n, n_actions]]). Sampled mode draws row r at (episode
        episode0 + r, step 0)."""
        o = np.ascontiguousarray(np.atleast_2d(obs), dtype=np.float64)
        if o.ndim != 2 or o.shape[1] != self.obs_len:
            raise ValueError(f"obs: expected [n, {self.obs_len}], got {list(o.shape)}")
        n = o.shape[0]
        if n < 1:
            raise ValueError("obs: at least one row")
        act = np.zeros(n, dtype=np.int32)
        logp = np.zeros(n)
        val = np.zeros(n)
        lg = np.zeros((n, self.observation_spec()[1]), dtype=np.float32) if logits else None
        L.check(L.lib().cpr_policy_net_forward(
            self.handle, L.ptr(o), n, 1 if deterministic else 0, int(episode0), L.ptr(act),
            L.ptr(logp), L.ptr(val), L.ptr(lg)))
        return (act, logp, val, lg) if logits else (act, logp, val)

    # ---- the gym layers of cpr-v0 over the lanes (cpr_lane_env_set)
    GYM_REWARDS = {"engine": L.GYM_REWARD_ENGINE, "sparse_relative": L.GYM_REWARD_SPARSE_RELATIVE,
                   "sparse_per_progress": L.GYM_REWARD_SPARSE_PER_PROGRESS,
                   "dense_per_progress": L.GYM_REWARD_DENSE_PER_PROGRESS}
    REWARD_SHAPES = {"none": L.SHAPE_NONE, "per_alpha": L.SHAPE_PER_ALPHA, "cut": L.SHAPE_CUT}

    SCHEDULES = {"choice": L.SCHEDULE_CHOICE, "cycle": L.SCHEDULE_CYCLE}

    def set_lane_env(self, alphas=None, alpha_column=None, reward="engine", shape="none",
                     dense_target=None, schedule="choice"):
        """The assumption schedule and reward wrappers of cpr-v0 on the lanes, before the
        first reset or rollout. ``alphas``: the table an episode's alpha is chosen from by
        (seed, episode) (None: the config's alpha); ``alpha_column``: the column of the
        network's extras that a rollout feeds with the lane's alpha (None: constants only);
        ``reward`` in GYM_REWARDS, ``shape`` in REWARD_SHAPES ("per_alpha" is r / alpha, "cut"
        is ppo.py's); ``dense_target``: episode_len of "dense_per_progress". They apply to
        ``rollout_net``'s reward; ``step`` keeps the engine's. ``schedule``: "choice" (an entry
        per episode by (seed, episode), ppo.py's random.choice) or "cycle" (episode e runs at
        entry e mod len(alphas), the reference wrapper's itertools.cycle)."""
        if schedule not in self.SCHEDULES:
            raise ValueError(f"schedule: expected one of {sorted(self.SCHEDULES)}")
        if reward not in self.GYM_REWARDS:
            raise ValueError(f"reward: expected one of {sorted(self.GYM_REWARDS)}")
        if shape not in self.REWARD_SHAPES:
            raise ValueError(f"shape: expected one of {sorted(self.REWARD_SHAPES)}")
        e = L.LaneEnvC()
        tab = None
        if alphas is not None:
            tab = np.ascontiguousarray(np.atleast_1d(alphas), dtype=np.float64)
            if tab.ndim != 1:
                raise ValueError("alphas: expected a sequence of floats")
            e.n_alpha = tab.size
            e.alpha = tab.ctypes.data
        e.alpha_column = -1 if alpha_column is None else int(alpha_column)
        e.gym_reward = self.GYM_REWARDS[reward]
        e.reward_shape = self.REWARD_SHAPES[shape]
        e.dense_target = 0.0 if dense_target is None else float(dense_target)
        L.check(L.lib().cpr_lane_env_set(self.handle, ctypes.byref(e)))
        self._lane_env = True
        L.check(L.lib().cpr_lane_env_schedule(self.handle, self.SCHEDULES[schedule]))
        self._n_alpha = 1 if tab is None else int(tab.size)

    # ---- evaluation (cpr_eval_net, cpr_policy_net_copy; DESIGN.md §4.14 "Evaluation")
    def evaluate_net(self, episodes_per_alpha, first_episode=0, deterministic=True,
                     check_every=None, records=True):
        """Whole episodes of the batch's network, one result per alpha (cpr_eval_net): the
        episode set [first_episode, first_episode + n_alpha * episodes_per_alpha), every lane
        reset first, the reward of the lane env summed per episode. The results depend on the
        seed, the set and the network only, not on the lane count or on ``check_every`` (the
        steps between two looks at the finished-episode counter; None: max_steps). Returns an
        ``EvalResult``. Afterwards ``step`` and the rollouts need a ``reset``."""
        a = self._n_alpha
        o = L.EvalOptsC()
        o.episodes_per_alpha = int(episodes_per_alpha)
        o.first_episode = int(first_episode)
        o.deterministic = 1 if deterministic else 0
        o.check_every = 0 if check_every is None else int(check_every)
        n_set = a * max(0, o.episodes_per_alpha)
        rec = np.zeros(n_set, dtype=L.EVAL_RECORD_DTYPE) if records else None
        stats = np.zeros(a, dtype=L.EVAL_ALPHA_DTYPE)
        sums = (L.Summary * a)()
        total = L.Summary()
        L.check(L.lib().cpr_eval_net(self.handle, ctypes.byref(o), L.ptr(rec), L.ptr(stats),
                                     ctypes.cast(sums, ctypes.c_void_p), ctypes.byref(total)))
        return EvalResult(stats, list(sums), rec, total)

    def copy_policy_net_from(self, other):
        """Take ``other``'s current weights (cpr_policy_net_copy): device to device on the
        context's stream, for an eval batch beside the batch being trained. Shapes and
        extras must match a network this batch already has; its Adam state is zeroed."""
        L.check(L.lib().cpr_policy_net_copy(self.handle, other.handle))
        self._net = getattr(other, "_net", None)

    def lane_alpha(self):
        """alpha of every lane's current episode (cpr_lane_alpha)."""
        a = np.zeros(self.n_lanes)
        L.check(L.lib().cpr_lane_alpha(self.handle, L.ptr(a)))
        return a

    ROLLOUT_NET_OUTPUTS = ("obs0", "obs", "action", "reward", "done", "logp", "value")
    ROLLOUT_ENV_OUTPUTS = ("alpha0", "alpha", "engine_reward")

    def _rollout_arrays(self, n_steps):
        n = self.n_lanes
        return {
            "obs0": np.zeros((n, self.obs_len)),
            "obs": np.zeros((n_steps, n, self.obs_len)),
            "action": np.zeros((n_steps, n), dtype=np.int32),
            "reward": np.zeros((n_steps, n)),
            "done": np.zeros((n_steps, n), dtype=np.uint8),
            "logp": np.zeros((n_steps, n)),
            "value": np.zeros((n_steps + 1, n)),
        }

    def rollout_net(self, n_steps, deterministic=False, outputs=True, summary=None,
                    device_outputs=None):
        """Rollout driven by the batch's network (cpr_rollout_net): per step the network
        forward, the lockstep step, bookkeeping and auto-reset run on the device with no host
        synchronisation. Returns (summary, arrays): ``outputs=True`` gives host arrays
        obs0 [n_lanes, obs_len], obs [n_steps, n_lanes, obs_len], action, reward, done, logp
        [n_steps, n_lanes] and value [n_steps + 1, n_lanes] (row n_steps: the bootstrap value);
        ``device_outputs={name: device pointer}`` (e.g. torch tensors' ``data_ptr()``) writes
        those buffers on the device instead and returns the same dict.

        With a lane env (``set_lane_env``) the call goes through cpr_rollout_net_env:
        ``reward`` is the wrapped and shaped reward, and the arrays gain alpha0 [n_lanes],
        alpha [n_steps, n_lanes] (the alpha of the episode obs0 / obs[t] belongs to) and
        engine_reward [n_steps, n_lanes] (the unwrapped reward); ``device_outputs`` accepts
        those names too (with or without a lane env)."""
        n_steps = int(n_steps)
        if n_steps < 1:
            raise ValueError("n_steps: at least 1")
        s = summary if summary is not None else L.Summary()
        n = self.n_lanes
        o = L.RolloutNetOut()
        eo = L.RolloutEnvOut()
        det = 1 if deterministic else 0
        if device_outputs is not None:
            use_env = getattr(self, "_lane_env", False)
            for k, v in device_outputs.items():
                if k in self.ROLLOUT_ENV_OUTPUTS:
                    setattr(eo, k, None if v is None else int(v))
                    use_env = True
                elif k in self.ROLLOUT_NET_OUTPUTS:
                    setattr(o, k, None if v is None else int(v))
                else:
                    raise ValueError(f"device_outputs: unknown output {k!r}")
            if use_env:
                L.check(L.lib().cpr_rollout_net_env(self.handle, n_steps, det, ctypes.byref(o),
                                                    ctypes.byref(eo), 1, ctypes.byref(s)))
            else:
                L.check(L.lib().cpr_rollout_net(self.handle, n_steps, det, ctypes.byref(o), 1,
                                                ctypes.byref(s)))
            return s, device_outputs
        if getattr(self, "_lane_env", False):
            arrays = {}
            if outputs:
                arrays = self._rollout_arrays(n_steps)
                arrays.update(alpha0=np.zeros(n), alpha=np.zeros((n_steps, n)),
                              engine_reward=np.zeros((n_steps, n)))
                for k, v in arrays.items():
                    setattr(eo if k in self.ROLLOUT_ENV_OUTPUTS else o, k, v.ctypes.data)
            L.check(L.lib().cpr_rollout_net_env(self.handle, n_steps, det, ctypes.byref(o),
                                                ctypes.byref(eo), 0, ctypes.byref(s)))
            if outputs:
                arrays["done"] = arrays["done"].astype(bool)
            return s, arrays
        arrays = {}
        if outputs:
            arrays = self._rollout_arrays(n_steps)
            for k, v in arrays.items():
                setattr(o, k, v.ctypes.data)
        L.check(L.lib().cpr_rollout_net(self.handle, n_steps, 1 if deterministic else 0,
                                        ctypes.byref(o), 0, ctypes.byref(s)))
        if outputs:
            arrays["done"] = arrays["done"].astype(bool)
        return s, arrays

    def rollout_net_fused(self):
        """Whether the batch's last ``rollout_net`` / ``ppo_iterate`` ran as one kernel
        (cpr_rollout_net_fused; FC16 env batches) instead of the launch
        sequence. Off by default; ``CPR_FC16_ROLLOUT_FUSED=1`` (read at every call) turns it
        on, with the same outputs bit for bit."""
        v = ctypes.c_int32()
        L.check(L.lib().cpr_rollout_net_fused(self.handle, ctypes.byref(v)))
        return bool(v.value)

    # ---- the learner (cpr_gae, cpr_ppo_*; DESIGN.md §4.14 "Learner")
    def gae(self, reward, done, value, gamma=0.99, lam=0.95, device=False, n_steps=None,
            out=None):
        """SB3's compute_returns_and_advantage over step-major buffers (cpr_gae): reward, done
        [n_steps, n_lanes], value [n_steps + 1, n_lanes] -> (advantage, return) arrays. With
        ``device=True`` the three are device pointers (ints, e.g. torch tensors'
        ``data_ptr()``), ``n_steps`` is given and the result goes to the device pointers
        ``out=(advantage, return)``."""
        if device:
            if n_steps is None or out is None:
                raise ValueError("gae: device=True needs n_steps and out=(adv_ptr, ret_ptr)")
            ptrs = [ctypes.c_void_p(int(x)) for x in (reward, done, value, out[0], out[1])]
            L.check(L.lib().cpr_gae(self.handle, int(n_steps), ptrs[0], ptrs[1], ptrs[2],
                                    float(gamma), float(lam), ptrs[3], ptrs[4], 1))
            return out
        r = np.ascontiguousarray(reward, dtype=np.float64)
        d = np.ascontiguousarray(done, dtype=np.uint8)
        v = np.ascontiguousarray(value, dtype=np.float64)
        if r.ndim != 2 or r.shape[1] != self.n_lanes or d.shape != r.shape or \
                v.shape != (r.shape[0] + 1, r.shape[1]):
            raise ValueError(f"gae: expected reward, done [n_steps, {self.n_lanes}] and value "
                             f"[n_steps + 1, {self.n_lanes}]")
        adv, ret = np.zeros_like(r), np.zeros_like(r)
        L.check(L.lib().cpr_gae(self.handle, r.shape[0], L.ptr(r), L.ptr(d), L.ptr(v), float(gamma),
                                float(lam), L.ptr(adv), L.ptr(ret), 0))
        return adv, ret

    PPO_DATA = ("obs", "alpha", "action", "old_logp", "advantage", "ret")

    def _ppo_data(self, data, device):
        """(cpr_ppo_data, the arrays it points to) of a dict with the keys of PPO_DATA
        (``alpha`` optional): host arrays, or with ``device=True`` device pointers and ``n``."""
        c = L.PpoDataC()
        if device:
            c.n = int(data["n"])
            for k in self.PPO_DATA:
                v = data.get(k)
                setattr(c, k, None if v is None else int(v))
            c.on_device = 1
            return c, None
        dt = {"obs": np.float64, "alpha": np.float64, "action": np.int32, "old_logp": np.float64,
              "advantage": np.float64, "ret": np.float64}
        keep = {}
        for k in self.PPO_DATA:
            v = data.get(k)
            if v is None:
                if k != "alpha":
                    raise ValueError(f"data: {k!r} is missing")
                continue
            keep[k] = np.ascontiguousarray(v, dtype=dt[k])
        n = keep["action"].size
        keep["obs"] = keep["obs"].reshape(-1, self.obs_len)
        for k, v in keep.items():
            if v.shape[0] != n or (k != "obs" and v.ndim != 1):
                raise ValueError(f"data: {k!r} has shape {list(v.shape)}, expected {n} rows")
            setattr(c, k, v.ctypes.data)
        c.n = n
        c.on_device = 0
        return c, keep

    @staticmethod
    def _ppo_opts(options):
        from .ppo import PPOOptions

        o = options if options is not None else PPOOptions()
        for name in ("minibatch", "n_epochs"):
            if int(getattr(o, name)) < 1:
                raise ValueError(f"{name}: at least 1")
        for name in ("lr", "clip_range"):
            if not math.isfinite(float(getattr(o, name))):
                raise ValueError(f"{name}: non-finite value")
        return o.cstruct()

    def ppo_param_count(self):
        n = ctypes.c_int64()
        L.check(L.lib().cpr_ppo_param_count(self.handle, ctypes.byref(n)))
        return n.value

    def ppo_gradients(self, data, rows, options=None, device=False):
        """The PPO gradient of the minibatch ``rows`` (int32 indices into ``data``; a device
        pointer and ``data["n_rows"]`` with ``device=True``) without touching the weights:
        (flat f32 gradient in ``cpr_amd.ppo.param_arrays`` order, statistics dict)."""
        o = self._ppo_opts(options)
        c, keep = self._ppo_data(data, device)
        if device:
            idx, n_rows = ctypes.c_void_p(int(rows)), int(data["n_rows"])
        else:
            ia = np.ascontiguousarray(rows, dtype=np.int32).ravel()
            idx, n_rows = L.ptr(ia), ia.size
        grad = np.zeros(self.ppo_param_count(), dtype=np.float32)
        st = L.PpoStats()
        L.check(L.lib().cpr_ppo_gradients(self.handle, ctypes.byref(c), idx, n_rows,
                                          ctypes.byref(o), L.ptr(grad), ctypes.byref(st)))
        del keep
        return grad, st.as_dict()

    def ppo_update(self, data, options=None, perm=None, device=False):
        """n_epochs x ceil(n / minibatch) steps of gradient, clip and Adam on the batch's device
        weights (cpr_ppo_update). ``perm``: int32 [n_epochs, n] (a device pointer with
        ``device=True``), or None for the library's keyed permutations. Returns the update's
        statistics dict (means over the minibatches)."""
        o = self._ppo_opts(options)
        c, keep = self._ppo_data(data, device)
        pa = None
        if perm is None:
            pp = None
        elif device:
            pp = ctypes.c_void_p(int(perm))
        else:
            pa = np.ascontiguousarray(perm, dtype=np.int32)
            if pa.shape != (o.n_epochs, c.n):
                raise ValueError(f"perm: expected [{o.n_epochs}, {c.n}], got {list(pa.shape)}")
            pp = L.ptr(pa)
        st = L.PpoStats()
        L.check(L.lib().cpr_ppo_update(self.handle, ctypes.byref(c), ctypes.byref(o), pp,
                                       ctypes.byref(st)))
        del keep, pa
        return st.as_dict()

    def ppo_iterate(self, n_steps, options=None, summary=None):
        """One PPO iteration on the device (cpr_ppo_iterate): a sampled network rollout of
        ``n_steps`` into buffers the batch owns, GAE, the update. Returns (summary of the
        rollout, statistics dict of the update)."""
        o = self._ppo_opts(options)
        s = summary if summary is not None else L.Summary()
        st = L.PpoStats()
        L.check(L.lib().cpr_ppo_iterate(self.handle, int(n_steps), ctypes.byref(o), ctypes.byref(s),
                                        ctypes.byref(st)))
        return s, st.as_dict()

    # ---- Q-learning (cpr_dqn_*; DESIGN.md §4.14 "Q-learning")
    DQN_DATA = ("obs", "alpha", "action", "reward", "done", "next_obs")

    @staticmethod
    def _dqn_opts(options):
        from .dqn import DQNOptions

        o = options if options is not None else DQNOptions()
        return o.cstruct()

    def dqn_init(self, capacity_steps):
        """The replay ring of ``capacity_steps`` slots of ``n_lanes`` transitions and the target
        network, a copy of the current weights (cpr_dqn_init)."""
        L.check(L.lib().cpr_dqn_init(self.handle, int(capacity_steps)))

    def dqn_collect(self, n_steps, epsilon, summary=None):
        """``n_steps`` epsilon-greedy steps of every lane into the ring (cpr_dqn_collect).
        Returns the rollout's summary."""
        s = summary if summary is not None else L.Summary()
        L.check(L.lib().cpr_dqn_collect(self.handle, int(n_steps), float(epsilon), ctypes.byref(s)))
        return s

    def dqn_replay_state(self):
        """(size, cursor, capacity) of the ring, in slots."""
        v = [ctypes.c_int64() for _ in range(3)]
        L.check(L.lib().cpr_dqn_replay_state(self.handle, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def dqn_replay(self, first_slot=0, n_slots=None):
        """Slots [first_slot, first_slot + n_slots) of the ring (cpr_dqn_replay_get; default:
        the written ones) as a dict of arrays shaped [n_slots, n_lanes, ...] with the keys of
        ``DQN_DATA``. Slot ``capacity`` is the guard slot behind the ring."""
        if n_slots is None:
            n_slots = self.dqn_replay_state()[0] - first_slot
        n_slots, n = int(n_slots), self.n_lanes
        out = {"obs": np.zeros((n_slots, n, self.obs_len)), "alpha": np.zeros((n_slots, n)),
               "action": np.zeros((n_slots, n), dtype=np.int32), "reward": np.zeros((n_slots, n)),
               "done": np.zeros((n_slots, n), dtype=np.uint8),
               "next_obs": np.zeros((n_slots, n, self.obs_len))}
        c = L.DqnDataC()
        for k, v in out.items():
            setattr(c, k, v.ctypes.data)
        L.check(L.lib().cpr_dqn_replay_get(self.handle, int(first_slot), n_slots, ctypes.byref(c)))
        return out

    def _dqn_data(self, data):
        c = L.DqnDataC()
        dt = {"obs": np.float64, "alpha": np.float64, "action": np.int32, "reward": np.float64,
              "done": np.uint8, "next_obs": np.float64}
        keep = {}
        for k in self.DQN_DATA:
            v = data.get(k)
            if v is None:
                if k != "alpha":
                    raise ValueError(f"data: {k!r} is missing")
                continue
            keep[k] = np.ascontiguousarray(v, dtype=dt[k])
        n = keep["action"].size
        for k in ("obs", "next_obs"):
            keep[k] = keep[k].reshape(-1, self.obs_len)
        for k in ("alpha", "action", "reward", "done"):
            if k in keep:
                keep[k] = keep[k].reshape(-1)
        for k, v in keep.items():
            if v.shape[0] != n:
                raise ValueError(f"data: {k!r} has shape {list(v.shape)}, expected {n} rows")
            setattr(c, k, v.ctypes.data)
        c.n = n
        c.on_device = 0
        return c, keep

    def dqn_gradients(self, data, rows, options=None):
        """The Q-learning gradient of the transitions ``rows`` (indices into ``data``, a dict of
        host arrays with the keys of ``DQN_DATA``, ``alpha`` optional) without touching the
        weights: (flat f32 gradient in ``cpr_amd.ppo.param_arrays`` order, statistics dict)."""
        o = self._dqn_opts(options)
        c, keep = self._dqn_data(data)
        ia = np.ascontiguousarray(rows, dtype=np.int64).ravel()
        grad = np.zeros(self.ppo_param_count(), dtype=np.float32)
        st = L.DqnStats()
        L.check(L.lib().cpr_dqn_gradients(self.handle, ctypes.byref(c), L.ptr(ia), ia.size,
                                          ctypes.byref(o), L.ptr(grad), ctypes.byref(st)))
        del keep
        return grad, st.as_dict()

    def dqn_update(self, gradient_steps=None, options=None, idx=None):
        """``gradient_steps`` (default: the options') steps of gradient, clip and Adam on the
        ring (cpr_dqn_update). ``idx``: integers [gradient_steps, batch] of flat transition
        indices slot * n_lanes + lane, or None for the library's keyed draws. Returns the
        update's statistics dict."""
        o = self._dqn_opts(options)
        g = int(o.gradient_steps if gradient_steps is None else gradient_steps)
        ia = None
        if idx is not None:
            ia = np.ascontiguousarray(idx, dtype=np.int64)
            if ia.shape != (g, o.batch):
                raise ValueError(f"idx: expected [{g}, {o.batch}], got {list(ia.shape)}")
        st = L.DqnStats()
        L.check(L.lib().cpr_dqn_update(self.handle, g, ctypes.byref(o), L.ptr(ia),
                                       ctypes.byref(st)))
        return st.as_dict()

    def dqn_last_indices(self, gradient_steps, batch):
        """The indices the last ``dqn_update`` read, [gradient_steps, batch], from the device."""
        out = np.zeros((int(gradient_steps), int(batch)), dtype=np.int64)
        L.check(L.lib().cpr_dqn_last_indices(self.handle, L.ptr(out), out.size))
        return out

    def dqn_target_sync(self, tau=1.0):
        """target = (1 - tau) target + tau weights, SB3's polyak_update (cpr_dqn_target_sync)."""
        L.check(L.lib().cpr_dqn_target_sync(self.handle, float(tau)))

    def dqn_iterate(self, n_steps, epsilon, options=None, summary=None):
        """One DQN iteration on the device (cpr_dqn_iterate): collect, the target update when
        its interval was crossed, the gradient steps once learning has started. Returns
        (summary of the rollout, statistics dict; ``n_steps`` 0 if no update ran)."""
        o = self._dqn_opts(options)
        s = summary if summary is not None else L.Summary()
        st = L.DqnStats()
        L.check(L.lib().cpr_dqn_iterate(self.handle, int(n_steps), float(epsilon), ctypes.byref(o),
                                        ctypes.byref(s), ctypes.byref(st)))
        return s, st.as_dict()

    def get_target_net(self):
        """The target network as a ``PolicyNet`` (cpr_dqn_target_get)."""
        net = getattr(self, "_net", None)
        if net is None:
            raise L.CprError(L.CPR_E_STATE, "no policy network set (set_policy_net)")
        out = net.zeros_like()
        c = out.cstruct()
        L.check(L.lib().cpr_dqn_target_get(self.handle, ctypes.byref(c)))
        return out

    def get_policy_net(self):
        """The batch's current weights as a ``PolicyNet`` (cpr_policy_net_get)."""
        net = getattr(self, "_net", None)
        if net is None:
            raise L.CprError(L.CPR_E_STATE, "no policy network set (set_policy_net)")
        out = net.zeros_like()
        c = out.cstruct()
        L.check(L.lib().cpr_policy_net_get(self.handle, ctypes.byref(c)))
        return out

    def observation_spec(self):
        ol = ctypes.c_int32()
        na = ctypes.c_int32()
        low = np.zeros(16)
        high = np.zeros(16)
        L.check(
            L.lib().cpr_observation_spec(
                self.handle, ctypes.byref(ol), ctypes.byref(na), L.ptr(low), L.ptr(high)
            )
        )
        return ol.value, na.value, low[: ol.value], high[: ol.value]


def policy_registry(protocol=L.PROTO_NAKAMOTO):
    """[(name, id)] in the reference's registry order (nakamoto_ssz.ml:342-350)."""
    out = []
    for i in range(L.lib().cpr_policy_count(protocol)):
        pid = ctypes.c_int32()
        name = L.lib().cpr_policy_name(protocol, i, ctypes.byref(pid))
        out.append((name.decode(), pid.value))
    return out
