"""ctypes binding of libcpr_hip (include/cpr_hip.h).

The shared object is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950). There
is no fallback: if the library is missing or no HIP device is present, the product path
raises instead of silently computing anything on the CPU.
"""

import ctypes
import os
import pathlib

import numpy as np

LIB_PATH = pathlib.Path(__file__).resolve().parent / "libcpr_hip.so"

# enums (include/cpr_hip.h)
CPR_OK = 0
CPR_E_INVALID_ARG = -1
CPR_E_UNSUPPORTED = -2
CPR_E_HIP = -3
CPR_E_CAPACITY = -4
CPR_E_STATE = -5
CPR_E_INTERNAL = -6

PROTO_NAKAMOTO = 0
PROTO_ETHEREUM = 1
PROTO_BK = 2
PROTO_TAILSTORM = 3
REWARD_PUNISH = 3
REWARD_HYBRID = 4
SELECT_ALTRUISTIC = 0
SELECT_HEURISTIC = 1
SELECT_OPTIMAL = 2
TS_POLICY_HONEST = 0
TS_POLICY_TABLE = 7  # include/cpr_hip.h, the B_k table layout
TS_POLICY_GET_AHEAD = 1
TS_POLICY_MINOR_DELAY = 2
TS_POLICY_AVOID_LOSS = 3
TS_POLICY_AVOID_LOSS_A = 4
TS_POLICY_AVOID_LOSS_B = 5
TS_POLICY_LONG_DELAY = 6
TS_POLICY_RANDOM = 8  # loop tasks: keyed random Action8 (cpr_protocols.ml:658-782)
REWARD_CONSTANT = 0
REWARD_DISCOUNT = 1
REWARD_BLOCK = 2
BK_POLICY_HONEST = 0
BK_POLICY_GET_AHEAD = 1
BK_POLICY_MINOR_DELAY = 2
BK_POLICY_AVOID_LOSS = 3
BK_POLICY_TABLE = 4
BK_POLICY_RANDOM = 5
ETH_POLICY_HONEST = 0
ETH_POLICY_TABLE = 5  # include/cpr_hip.h: [(pub_h, priv_h) clamped to D][event]
ETH_POLICY_SELFISH_RELEASE = 1
ETH_POLICY_SELFISH_DISCARD = 2
ETH_POLICY_FN19 = 3
ETH_POLICY_FN19PKEL = 4
ETH_POLICY_RANDOM = 6
NET_SELFISH_MINING = 0
NET_TWO_AGENTS = 1
NET_HONEST_CLIQUE = 2
NET_EXP_CLIQUE = 3  # include/cpr_hip.h: attacker + `defenders`, exponential link delays
NET_ABSTRACT_GAMMA = 4  # FLAGGED abstract-gamma mode (include/cpr_hip.h), gamma in [0, 1]
MODE_GYM = 0
MODE_LOOP = 1

POLICY_HONEST = 0
POLICY_SIMPLE = 1
POLICY_EYAL_SIRER_2014 = 2
POLICY_SAPIRSHTEIN_2016_SM1 = 3
POLICY_TABLE = 4
POLICY_RANDOM = 5  # loop tasks on the event engine (cpr_protocols.ml:658-782)

PROTO_FC16 = 4  # gym/rust/src/fc16.rs abstract model (fused episodes)
PROTO_FC16_ENV = 5  # the same model with lockstep lanes: reset / step, networks, the learner
# gym/rust/src/generic/mod.rs over proto/nakamoto.rs (Nakamoto-v0): release / consider per block
PROTO_GENERIC_NAKAMOTO = 6
GENERIC_MAX_STEPS = 4096  # csrc/generic_lane.h kGenericMaxSteps
GENERIC_MAX_K = 11
FC16_POLICY_HONEST = 0
FC16_POLICY_SM1 = 1
FC16_POLICY_TABLE = 2
FC16_WAIT, FC16_ADOPT, FC16_OVERRIDE, FC16_MATCH = 0, 1, 2, 3
ST_TIE = 1
ST_OVERLAP = 2
ST_DEEP_FORK = 4
ST_TIE_UNRESOLVED = 8
ST_STALE_TIME = 16
ST_CAPACITY = 32
ST_REFERENCE_RAISES = 64
ST_TRACE_MISS = 128
ST_EXACT_RERUN = 256
ST_INVALID = ST_CAPACITY | ST_REFERENCE_RAISES | ST_TRACE_MISS  # include/cpr_hip.h
ST_LOCKSTEP_INEXACT = ST_OVERLAP | ST_DEEP_FORK | ST_TIE_UNRESOLVED | ST_STALE_TIME
ABI_VERSION = 11  # include/cpr_hip.h CPR_ABI_VERSION this module's structures follow

HIST_BINS = 64
# largest group of sweep points one fused lane runs at gamma = 0 and with deferred races
# (csrc/nak_fused.h CPR_NAK_FUSE_MAX, CPR_NAK_FUSE_MAX_ARR; only the tests read them, and
# tests/test_gpu_fused_points.py test_group_sizes* fail if the library groups otherwise)
NAK_FUSE_MAX = 5
NAK_FUSE_MAX_ARR = 2
# lanes per episode of a full lane-group launch (csrc/nak_fused.h CPR_NAK_FUSE_LANES,
# CPR_NAK_FUSE_LANES_ARR; tests/test_gpu_lane_groups.py fails if the library cuts otherwise)
NAK_FUSE_LANES = 2
NAK_FUSE_LANES_ARR = 4


class Config(ctypes.Structure):
    _fields_ = [
        ("protocol", ctypes.c_int32),
        ("network", ctypes.c_int32),
        ("mode", ctypes.c_int32),
        ("policy", ctypes.c_int32),
        ("policy_table", ctypes.POINTER(ctypes.c_uint8)),
        ("policy_table_dim", ctypes.c_int32),
        ("unit_observation", ctypes.c_int32),
        ("alpha", ctypes.c_double),
        ("gamma", ctypes.c_double),
        ("defenders", ctypes.c_int32),
        ("reward_scheme", ctypes.c_int32),
        ("activation_delay", ctypes.c_double),
        ("propagation_delay", ctypes.c_double),
        ("max_steps", ctypes.c_int64),
        ("max_progress", ctypes.c_double),
        ("max_time", ctypes.c_double),
        ("activations", ctypes.c_int64),
        ("seed", ctypes.c_uint64),
        ("n_lanes", ctypes.c_int64),
        ("k", ctypes.c_int32),
        ("subblock_selection", ctypes.c_int32),
        ("delay_lo", ctypes.c_double),
        ("delay_hi", ctypes.c_double),
        ("horizon", ctypes.c_double),
    ]


class EpisodeRecord(ctypes.Structure):
    _fields_ = [
        ("reward_attacker", ctypes.c_double),
        ("reward_defender", ctypes.c_double),
        ("progress", ctypes.c_double),
        ("chain_time", ctypes.c_double),
        ("sim_time", ctypes.c_double),
        ("n_steps", ctypes.c_int64),
        ("n_activations", ctypes.c_int64),
        ("head_height", ctypes.c_int32),
        ("head_miner", ctypes.c_int32),
        ("status", ctypes.c_uint32),
        ("head_work", ctypes.c_int32),
    ]


RECORD_DTYPE = np.dtype(
    [
        ("reward_attacker", "<f8"),
        ("reward_defender", "<f8"),
        ("progress", "<f8"),
        ("chain_time", "<f8"),
        ("sim_time", "<f8"),
        ("n_steps", "<i8"),
        ("n_activations", "<i8"),
        ("head_height", "<i4"),
        ("head_miner", "<i4"),
        ("status", "<u4"),
        ("head_work", "<i4"),
    ]
)
assert RECORD_DTYPE.itemsize == ctypes.sizeof(EpisodeRecord)


class Summary(ctypes.Structure):
    _fields_ = [
        ("episodes", ctypes.c_int64),
        ("steps", ctypes.c_int64),
        ("activations", ctypes.c_int64),
        ("reward_attacker_fx", ctypes.c_int64),
        ("reward_defender_fx", ctypes.c_int64),
        ("progress_fx", ctypes.c_int64),
        ("rel_revenue_fx", ctypes.c_uint64),
        ("rel_revenue_sq_fx", ctypes.c_uint64),
        ("orphans", ctypes.c_int64),
        ("status_tie", ctypes.c_int64),
        ("status_overlap", ctypes.c_int64),
        ("status_other", ctypes.c_int64),
        ("hist", ctypes.c_int64 * HIST_BINS),
        ("invalid", ctypes.c_int64),
    ]

    FIELDS = [f for f, _ in _fields_ if f != "hist"]

    def to_array(self):
        """int64 vector (fields then histogram) — the RCCL all-reduce payload."""
        head = [getattr(self, f) for f in self.FIELDS]
        head = [x - (1 << 64) if x >= (1 << 63) else x for x in head]
        return np.array(head + list(self.hist), dtype=np.int64)

    @classmethod
    def from_array(cls, a):
        s = cls()
        for i, f in enumerate(cls.FIELDS):
            v = int(a[i])
            if f.startswith("rel_") and v < 0:
                v += 1 << 64
            setattr(s, f, v)
        for i in range(HIST_BINS):
            s.hist[i] = int(a[len(cls.FIELDS) + i])
        return s

    def as_dict(self):
        d = {f: int(getattr(self, f)) for f in self.FIELDS}
        d["hist"] = [int(x) for x in self.hist]
        n = max(1, d["episodes"])
        d["mean_rel_revenue"] = d["rel_revenue_fx"] / 2**32 / n
        d["mean_reward_attacker"] = d["reward_attacker_fx"] / 2**20 / n
        d["mean_progress"] = d["progress_fx"] / 2**20 / n
        return d


class StepInfo(ctypes.Structure):
    _fields_ = [
        ("episode_reward_attacker", ctypes.POINTER(ctypes.c_double)),
        ("episode_reward_defender", ctypes.POINTER(ctypes.c_double)),
        ("episode_progress", ctypes.POINTER(ctypes.c_double)),
        ("episode_chain_time", ctypes.POINTER(ctypes.c_double)),
        ("episode_sim_time", ctypes.POINTER(ctypes.c_double)),
        ("episode_n_steps", ctypes.POINTER(ctypes.c_int64)),
        ("episode_n_activations", ctypes.POINTER(ctypes.c_int64)),
        ("head_height", ctypes.POINTER(ctypes.c_int32)),
        ("head_miner", ctypes.POINTER(ctypes.c_int32)),
        ("status", ctypes.POINTER(ctypes.c_uint32)),
    ]


POLICY_NET_MAX_DEPTH = 4
POLICY_NET_MAX_EXTRA = 8
TAG_POLICY = 0x60000000  # keyed-stream tag of sampled network actions (cpr_stream.h)


class PolicyNetC(ctypes.Structure):
    """cpr_policy_net (include/cpr_hip.h): host pointers to f32 arrays."""

    _fields_ = [
        ("n_extra", ctypes.c_int32),
        ("extra", ctypes.c_float * POLICY_NET_MAX_EXTRA),
        ("depth", ctypes.c_int32),
        ("width_pi", ctypes.c_int32),
        ("width_vf", ctypes.c_int32),
        ("pi_w", ctypes.c_void_p * POLICY_NET_MAX_DEPTH),
        ("pi_b", ctypes.c_void_p * POLICY_NET_MAX_DEPTH),
        ("pi_head_w", ctypes.c_void_p),
        ("pi_head_b", ctypes.c_void_p),
        ("vf_w", ctypes.c_void_p * POLICY_NET_MAX_DEPTH),
        ("vf_b", ctypes.c_void_p * POLICY_NET_MAX_DEPTH),
        ("vf_head_w", ctypes.c_void_p),
        ("vf_head_b", ctypes.c_void_p),
    ]


class RolloutNetOut(ctypes.Structure):
    """cpr_rollout_net_out: optional step-major output buffers."""

    _fields_ = [
        ("obs0", ctypes.c_void_p),
        ("obs", ctypes.c_void_p),
        ("action", ctypes.c_void_p),
        ("reward", ctypes.c_void_p),
        ("done", ctypes.c_void_p),
        ("logp", ctypes.c_void_p),
        ("value", ctypes.c_void_p),
    ]


# lane env (cpr_lane_env_set): enum cpr_gym_reward, enum cpr_reward_shape
GYM_REWARD_ENGINE = 0
GYM_REWARD_SPARSE_RELATIVE = 1
GYM_REWARD_SPARSE_PER_PROGRESS = 2
GYM_REWARD_DENSE_PER_PROGRESS = 3
SHAPE_NONE = 0
SHAPE_PER_ALPHA = 1
SHAPE_CUT = 2
LANE_ENV_MAX_ALPHA = 4096
TAG_ASSUME = 0x70000000  # keyed-stream tag of an episode's alpha draw (lane_env.h)


class LaneEnvC(ctypes.Structure):
    """cpr_lane_env (include/cpr_hip.h)."""

    _fields_ = [
        ("n_alpha", ctypes.c_int32),
        ("alpha", ctypes.c_void_p),
        ("alpha_column", ctypes.c_int32),
        ("gym_reward", ctypes.c_int32),
        ("reward_shape", ctypes.c_int32),
        ("dense_target", ctypes.c_double),
    ]


class RolloutEnvOut(ctypes.Structure):
    """cpr_rollout_env_out: optional output buffers."""

    _fields_ = [
        ("alpha0", ctypes.c_void_p),
        ("alpha", ctypes.c_void_p),
        ("engine_reward", ctypes.c_void_p),
    ]


# the assumption schedule (cpr_lane_env_schedule): enum cpr_alpha_schedule
SCHEDULE_CHOICE = 0
SCHEDULE_CYCLE = 1


class EvalOptsC(ctypes.Structure):
    """cpr_eval_opts (include/cpr_hip.h)."""

    _fields_ = [
        ("episodes_per_alpha", ctypes.c_int64),
        ("first_episode", ctypes.c_uint64),
        ("deterministic", ctypes.c_int32),
        ("check_every", ctypes.c_int64),
    ]


class EvalRecord(ctypes.Structure):
    """cpr_eval_record: one finished episode of an evaluation."""

    _fields_ = [
        ("episode", ctypes.c_uint64),
        ("alpha", ctypes.c_double),
        ("episode_reward", ctypes.c_double),
        ("episode_sim_time", ctypes.c_double),
        ("episode_chain_time", ctypes.c_double),
        ("episode_progress", ctypes.c_double),
        ("reward_attacker", ctypes.c_double),
        ("reward_defender", ctypes.c_double),
        ("episode_n_activations", ctypes.c_int64),
        ("episode_n_steps", ctypes.c_int64),
        ("height", ctypes.c_int64),
        ("alpha_index", ctypes.c_int32),
        ("status", ctypes.c_uint32),
    ]


_NP = {ctypes.c_uint64: "<u8", ctypes.c_double: "<f8", ctypes.c_int64: "<i8",
       ctypes.c_int32: "<i4", ctypes.c_uint32: "<u4"}
EVAL_RECORD_DTYPE = np.dtype([(n, _NP[t]) for n, t in EvalRecord._fields_])
assert EVAL_RECORD_DTYPE.itemsize == ctypes.sizeof(EvalRecord)

# enum cpr_eval_column: the columns EvalCallback logs, in cpr_eval_alpha's order
EVAL_COLUMNS = ("episode_reward", "episode_sim_time", "episode_chain_time", "episode_progress",
                "episode_n_activations")


class EvalAlpha(ctypes.Structure):
    """cpr_eval_alpha: one alpha's statistics over its valid episodes."""

    _fields_ = [
        ("alpha", ctypes.c_double),
        ("n", ctypes.c_int64),
        ("mean", ctypes.c_double * len(EVAL_COLUMNS)),
        ("std", ctypes.c_double * len(EVAL_COLUMNS)),
    ]


EVAL_ALPHA_DTYPE = np.dtype([("alpha", "<f8"), ("n", "<i8"), ("mean", "<f8", (len(EVAL_COLUMNS),)),
                             ("std", "<f8", (len(EVAL_COLUMNS),))])
assert EVAL_ALPHA_DTYPE.itemsize == ctypes.sizeof(EvalAlpha)


class PpoOptsC(ctypes.Structure):
    """cpr_ppo_opts (include/cpr_hip.h)."""

    _fields_ = [
        ("n_epochs", ctypes.c_int32),
        ("minibatch", ctypes.c_int64),
        ("clip_range", ctypes.c_double),
        ("ent_coef", ctypes.c_double),
        ("vf_coef", ctypes.c_double),
        ("max_grad_norm", ctypes.c_double),
        ("lr", ctypes.c_double),
        ("beta1", ctypes.c_double),
        ("beta2", ctypes.c_double),
        ("adam_eps", ctypes.c_double),
        ("normalize_advantage", ctypes.c_int32),
        ("gae_gamma", ctypes.c_double),
        ("gae_lambda", ctypes.c_double),
        ("perm_seed", ctypes.c_uint64),
    ]


class PpoDataC(ctypes.Structure):
    """cpr_ppo_data: n rows of training data, host or device pointers."""

    _fields_ = [
        ("n", ctypes.c_int64),
        ("obs", ctypes.c_void_p),
        ("alpha", ctypes.c_void_p),
        ("action", ctypes.c_void_p),
        ("old_logp", ctypes.c_void_p),
        ("advantage", ctypes.c_void_p),
        ("ret", ctypes.c_void_p),
        ("on_device", ctypes.c_int32),
    ]


class PpoStats(ctypes.Structure):
    """cpr_ppo_stats: SB3's logged statistics of a minibatch or an update."""

    _fields_ = [
        ("policy_loss", ctypes.c_double),
        ("value_loss", ctypes.c_double),
        ("entropy_loss", ctypes.c_double),
        ("approx_kl", ctypes.c_double),
        ("clip_fraction", ctypes.c_double),
        ("loss", ctypes.c_double),
        ("grad_norm", ctypes.c_double),
        ("n_minibatches", ctypes.c_int64),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


TAG_PERM = 0x80000000  # keyed-stream tag of cpr_ppo_update's permutations
TAG_EXPLORE = 0x90000000  # ... of cpr_dqn_collect's exploration coins (dqn.h)
TAG_REPLAY = 0xA0000000  # ... of cpr_dqn_update's sampled transitions


class DqnOptsC(ctypes.Structure):
    """cpr_dqn_opts (include/cpr_hip.h)."""

    _fields_ = [
        ("batch", ctypes.c_int64),
        ("gradient_steps", ctypes.c_int32),
        ("gamma", ctypes.c_double),
        ("lr", ctypes.c_double),
        ("beta1", ctypes.c_double),
        ("beta2", ctypes.c_double),
        ("adam_eps", ctypes.c_double),
        ("max_grad_norm", ctypes.c_double),
        ("tau", ctypes.c_double),
        ("target_update_interval", ctypes.c_int64),
        ("learning_starts", ctypes.c_int64),
        ("sample_seed", ctypes.c_uint64),
    ]


class DqnDataC(ctypes.Structure):
    """cpr_dqn_data: n transitions, host or device pointers."""

    _fields_ = [
        ("n", ctypes.c_int64),
        ("obs", ctypes.c_void_p),
        ("alpha", ctypes.c_void_p),
        ("action", ctypes.c_void_p),
        ("reward", ctypes.c_void_p),
        ("done", ctypes.c_void_p),
        ("next_obs", ctypes.c_void_p),
        ("on_device", ctypes.c_int32),
    ]


class DqnStats(ctypes.Structure):
    """cpr_dqn_stats: the statistics of a gradient step or an update."""

    _fields_ = [
        ("loss", ctypes.c_double),
        ("abs_td", ctypes.c_double),
        ("q", ctypes.c_double),
        ("target", ctypes.c_double),
        ("grad_norm", ctypes.c_double),
        ("n_steps", ctypes.c_int64),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


MDP_VI_AUTO, MDP_VI_RESIDENT, MDP_VI_GLOBAL = 0, 1, 2  # enum cpr_mdp_vi_path
MDP_VI_CONVERGED, MDP_VI_MAX_ITER, MDP_VI_NOT_CONVERGED = 0, 1, 2  # enum cpr_mdp_vi_status


class MdpC(ctypes.Structure):
    """cpr_mdp: P points of one topology in the dense padded form, host pointers."""

    _fields_ = [
        ("S", ctypes.c_int32),
        ("A", ctypes.c_int32),
        ("T", ctypes.c_int32),
        ("P", ctypes.c_int32),
        ("dst", ctypes.c_void_p),
        ("used", ctypes.c_void_p),
        ("valid", ctypes.c_void_p),
        ("rew", ctypes.c_void_p),
        ("prg", ctypes.c_void_p),
        ("prb", ctypes.c_void_p),
    ]


class MdpViOptsC(ctypes.Structure):
    """cpr_mdp_vi_opts."""

    _fields_ = [
        ("stop_delta", ctypes.c_double),
        ("discount", ctypes.c_double),
        ("max_iter", ctypes.c_int64),
        ("path", ctypes.c_int32),
    ]


class MdpViResultC(ctypes.Structure):
    """cpr_mdp_vi_result: the caller's arrays and the two scalars the call fills in."""

    _fields_ = [
        ("value", ctypes.c_void_p),
        ("progress", ctypes.c_void_p),
        ("policy", ctypes.c_void_p),
        ("iter", ctypes.c_void_p),
        ("delta", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
        ("path_used", ctypes.c_int32),
        ("kernel_ms", ctypes.c_double),
    ]


MDP_PE_REACHABLE, MDP_PE_ALL = 0, 1  # enum cpr_mdp_pe_states
MDP_PE_CONVERGED, MDP_PE_MAX_ITER, MDP_PE_NOT_CONVERGED = 0, 1, 2  # enum cpr_mdp_pe_status


class MdpPeC(ctypes.Structure):
    """cpr_mdp_pe: E evaluations (point, policy, start states) over one cpr_mdp."""

    _fields_ = [
        ("E", ctypes.c_int64),
        ("point", ctypes.c_void_p),
        ("policy", ctypes.c_void_p),
        ("states", ctypes.c_int32),
        ("n_start", ctypes.c_int32),
        ("start_state", ctypes.c_void_p),
        ("start_prob", ctypes.c_void_p),
    ]


class MdpPeOptsC(ctypes.Structure):
    """cpr_mdp_pe_opts."""

    _fields_ = [
        ("theta", ctypes.c_double),
        ("discount", ctypes.c_double),
        ("max_iter", ctypes.c_int64),
        ("path", ctypes.c_int32),
    ]


class MdpPeResultC(ctypes.Structure):
    """cpr_mdp_pe_result: the caller's arrays and the two scalars the call fills in."""

    _fields_ = [
        ("reward", ctypes.c_void_p),
        ("progress", ctypes.c_void_p),
        ("iter", ctypes.c_void_p),
        ("delta", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
        ("path_used", ctypes.c_int32),
        ("kernel_ms", ctypes.c_double),
    ]


class CTrace(ctypes.Structure):
    _fields_ = [
        ("n_episodes", ctypes.c_int64),
        ("act_offset", ctypes.c_void_p),
        ("act_miner", ctypes.c_void_p),
        ("act_delay", ctypes.c_void_p),
        ("pow_offset", ctypes.c_void_p),
        ("pow_hash", ctypes.c_void_p),
        ("link_offset", ctypes.c_void_p),
        ("link_key", ctypes.c_void_p),
        ("link_delay", ctypes.c_void_p),
    ]


class Trace:
    """An exported activation/delay trace (cpr_trace, include/cpr_hip.h): CSR numpy arrays
    over episodes. ``ctrace()`` gives the C struct (the arrays must outlive it)."""

    ARRAYS = [
        ("act_offset", np.int64), ("act_miner", np.int32), ("act_delay", np.float64),
        ("pow_offset", np.int64), ("pow_hash", np.int32),
        ("link_offset", np.int64), ("link_key", np.uint64), ("link_delay", np.float64),
    ]

    def __init__(self, **arrays):
        for name, dt in self.ARRAYS:
            setattr(self, name, np.ascontiguousarray(arrays[name], dtype=dt))
        self.n_episodes = len(self.act_offset) - 1

    def episode(self, e):
        """Trace of episode e alone."""
        a0, a1 = self.act_offset[e], self.act_offset[e + 1]
        p0, p1 = self.pow_offset[e], self.pow_offset[e + 1]
        l0, l1 = self.link_offset[e], self.link_offset[e + 1]
        return Trace(act_offset=[0, a1 - a0], act_miner=self.act_miner[a0:a1],
                     act_delay=self.act_delay[a0:a1], pow_offset=[0, p1 - p0],
                     pow_hash=self.pow_hash[p0:p1], link_offset=[0, l1 - l0],
                     link_key=self.link_key[l0:l1], link_delay=self.link_delay[l0:l1])

    def save(self, path):
        np.savez_compressed(path, **{n: getattr(self, n) for n, _ in self.ARRAYS})

    # binary layout written by the OCaml recorder (integration/ocaml/trace_hooks.ml
    # `write`): magic, u32 version, u32 n_episodes, then per array of ARRAYS: u64 count and
    # that many little-endian elements (act_miner / pow_hash as 32-bit ints)
    MAGIC = b"CPRTRACE"
    _WIRE = {"act_offset": "<i8", "act_miner": "<i4", "act_delay": "<f8", "pow_offset": "<i8",
             "pow_hash": "<i4", "link_offset": "<i8", "link_key": "<u8", "link_delay": "<f8"}

    def save_binary(self, path):
        """The OCaml recorder's format (a Python mirror of trace_hooks.ml `write`)."""
        with open(path, "wb") as f:
            f.write(self.MAGIC)
            f.write(np.array([1, self.n_episodes], dtype="<u4").tobytes())
            for name, _ in self.ARRAYS:
                a = np.ascontiguousarray(getattr(self, name), dtype=self._WIRE[name])
                f.write(np.array([len(a)], dtype="<u8").tobytes())
                f.write(a.tobytes())

    @classmethod
    def load(cls, path):
        """An .npz (Trace.save, the oracle's exporter) or the OCaml recorder's binary file."""
        with open(path, "rb") as f:
            head = f.read(len(cls.MAGIC))
        if head != cls.MAGIC:
            with np.load(path, allow_pickle=False) as z:
                return cls(**{n: z[n] for n, _ in cls.ARRAYS})
        raw = open(path, "rb").read()
        ver, n_ep = np.frombuffer(raw, dtype="<u4", count=2, offset=8)
        if ver != 1:
            raise ValueError(f"{path}: trace format version {ver}, expected 1")
        o, arrays = 16, {}
        for name, _ in cls.ARRAYS:
            (cnt,) = np.frombuffer(raw, dtype="<u8", count=1, offset=o)
            o += 8
            dt = np.dtype(cls._WIRE[name])
            arrays[name] = np.frombuffer(raw, dtype=dt, count=int(cnt), offset=o).copy()
            o += int(cnt) * dt.itemsize
        if o != len(raw) or len(arrays["act_offset"]) != n_ep + 1:
            raise ValueError(f"{path}: malformed trace file")
        return cls(**arrays)

    def ctrace(self):
        t = CTrace()
        t.n_episodes = self.n_episodes
        for name, _ in self.ARRAYS:
            setattr(t, name, self.__dict__[name].ctypes.data)
        return t


# every symbol include/cpr_hip.h declares
EXPORTS = [
    "cpr_version",
    "cpr_abi_version",
    "cpr_last_error",
    "cpr_ctx_create",
    "cpr_ctx_destroy",
    "cpr_device_count",
    "cpr_batch_create",
    "cpr_batch_destroy",
    "cpr_run_episodes",
    "cpr_run_episodes_async",
    "cpr_synchronize",
    "cpr_replay",
    "cpr_node_outputs",
    "cpr_last_launch",
    "cpr_launch_shape",
    "cpr_rerun_hbm_retries",
    "cpr_rerun_stats",
    "cpr_lockstep_coverage",
    "cpr_reset",
    "cpr_step",
    "cpr_observe_fields",
    "cpr_rollout",
    "cpr_policy_net_set",
    "cpr_policy_net_forward",
    "cpr_rollout_net",
    "cpr_lane_env_set",
    "cpr_lane_alpha",
    "cpr_lane_env_schedule",
    "cpr_eval_net",
    "cpr_policy_net_copy",
    "cpr_rollout_net_env",
    "cpr_rollout_net_fused",
    "cpr_gae",
    "cpr_ppo_opts_default",
    "cpr_ppo_gradients",
    "cpr_ppo_param_count",
    "cpr_ppo_update",
    "cpr_ppo_iterate",
    "cpr_dqn_opts_default",
    "cpr_dqn_init",
    "cpr_dqn_collect",
    "cpr_dqn_gradients",
    "cpr_dqn_update",
    "cpr_dqn_last_indices",
    "cpr_dqn_target_sync",
    "cpr_dqn_iterate",
    "cpr_dqn_replay_get",
    "cpr_dqn_replay_state",
    "cpr_dqn_target_get",
    "cpr_policy_net_get",
    "cpr_policy_actions",
    "cpr_observation_spec",
    "cpr_policy_count",
    "cpr_policy_name",
    "cpr_stream_fill",
    "cpr_mdp_vi_opts_default",
    "cpr_mdp_value_iteration",
    "cpr_mdp_pe_opts_default",
    "cpr_mdp_policy_evaluation",
]


class CprError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


_lib = None


def _declare(L):
    P = ctypes.POINTER
    vp = ctypes.c_void_p
    L.cpr_version.restype = ctypes.c_char_p
    L.cpr_abi_version.restype = ctypes.c_int
    L.cpr_last_error.restype = ctypes.c_char_p
    L.cpr_ctx_create.argtypes = [ctypes.c_int, P(vp)]
    L.cpr_ctx_destroy.argtypes = [vp]
    L.cpr_device_count.argtypes = [P(ctypes.c_int)]
    L.cpr_batch_create.argtypes = [vp, P(Config), P(vp)]
    L.cpr_batch_destroy.argtypes = [vp]
    L.cpr_run_episodes.argtypes = [vp, ctypes.c_int64, ctypes.c_uint64, P(Summary), vp, ctypes.c_int]
    L.cpr_run_episodes_async.argtypes = [vp, ctypes.c_int64, ctypes.c_uint64, vp, vp]
    L.cpr_synchronize.argtypes = [vp]
    L.cpr_replay.argtypes = [vp, P(CTrace), P(Summary), vp, ctypes.c_int]
    L.cpr_node_outputs.argtypes = [vp, ctypes.c_int64, ctypes.c_uint64, vp, ctypes.c_int32, vp,
                                   vp, vp]
    L.cpr_last_launch.argtypes = [vp, P(ctypes.c_double), P(ctypes.c_int64)]
    L.cpr_launch_shape.argtypes = [vp, P(ctypes.c_int64), P(ctypes.c_int64)]
    L.cpr_rerun_hbm_retries.argtypes = [vp, P(ctypes.c_int64)]
    L.cpr_rerun_stats.argtypes = [vp, P(ctypes.c_int64), P(ctypes.c_int64), P(ctypes.c_double)]
    L.cpr_lockstep_coverage.argtypes = [vp, P(ctypes.c_int64), P(ctypes.c_int64)]
    L.cpr_reset.argtypes = [vp, vp, vp, vp]
    L.cpr_step.argtypes = [vp, vp, vp, vp, vp, P(StepInfo)]
    L.cpr_observe_fields.argtypes = [vp, vp]
    L.cpr_rollout.argtypes = [vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int, P(Summary)]
    L.cpr_policy_net_set.argtypes = [vp, P(PolicyNetC)]
    L.cpr_policy_net_forward.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64, vp,
                                         vp, vp, vp]
    L.cpr_rollout_net.argtypes = [vp, ctypes.c_int64, ctypes.c_int, P(RolloutNetOut), ctypes.c_int,
                                  P(Summary)]
    L.cpr_lane_env_set.argtypes = [vp, P(LaneEnvC)]
    L.cpr_lane_alpha.argtypes = [vp, vp]
    L.cpr_lane_env_schedule.argtypes = [vp, ctypes.c_int]
    L.cpr_eval_net.argtypes = [vp, P(EvalOptsC), vp, vp, vp, P(Summary)]
    L.cpr_policy_net_copy.argtypes = [vp, vp]
    L.cpr_rollout_net_env.argtypes = [vp, ctypes.c_int64, ctypes.c_int, P(RolloutNetOut),
                                      P(RolloutEnvOut), ctypes.c_int, P(Summary)]
    L.cpr_rollout_net_fused.argtypes = [vp, P(ctypes.c_int32)]
    L.cpr_gae.argtypes = [vp, ctypes.c_int64, vp, vp, vp, ctypes.c_double, ctypes.c_double, vp, vp,
                          ctypes.c_int]
    L.cpr_ppo_opts_default.argtypes = [P(PpoOptsC)]
    L.cpr_ppo_gradients.argtypes = [vp, P(PpoDataC), vp, ctypes.c_int64, P(PpoOptsC), vp,
                                    P(PpoStats)]
    L.cpr_ppo_param_count.argtypes = [vp, P(ctypes.c_int64)]
    L.cpr_ppo_update.argtypes = [vp, P(PpoDataC), P(PpoOptsC), vp, P(PpoStats)]
    L.cpr_ppo_iterate.argtypes = [vp, ctypes.c_int64, P(PpoOptsC), P(Summary), P(PpoStats)]
    L.cpr_dqn_opts_default.argtypes = [P(DqnOptsC)]
    L.cpr_dqn_init.argtypes = [vp, ctypes.c_int64]
    L.cpr_dqn_collect.argtypes = [vp, ctypes.c_int64, ctypes.c_double, P(Summary)]
    L.cpr_dqn_gradients.argtypes = [vp, P(DqnDataC), vp, ctypes.c_int64, P(DqnOptsC), vp,
                                    P(DqnStats)]
    L.cpr_dqn_update.argtypes = [vp, ctypes.c_int32, P(DqnOptsC), vp, P(DqnStats)]
    L.cpr_dqn_last_indices.argtypes = [vp, vp, ctypes.c_int64]
    L.cpr_dqn_target_sync.argtypes = [vp, ctypes.c_double]
    L.cpr_dqn_iterate.argtypes = [vp, ctypes.c_int64, ctypes.c_double, P(DqnOptsC), P(Summary),
                                  P(DqnStats)]
    L.cpr_dqn_replay_get.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, P(DqnDataC)]
    L.cpr_dqn_replay_state.argtypes = [vp, P(ctypes.c_int64), P(ctypes.c_int64),
                                       P(ctypes.c_int64)]
    L.cpr_dqn_target_get.argtypes = [vp, P(PolicyNetC)]
    L.cpr_policy_net_get.argtypes = [vp, P(PolicyNetC)]
    L.cpr_policy_actions.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_int64, vp]
    L.cpr_observation_spec.argtypes = [vp, P(ctypes.c_int32), P(ctypes.c_int32), vp, vp]
    L.cpr_policy_count.argtypes = [ctypes.c_int32]
    L.cpr_policy_name.restype = ctypes.c_char_p
    L.cpr_policy_name.argtypes = [ctypes.c_int32, ctypes.c_int32, P(ctypes.c_int32)]
    L.cpr_stream_fill.argtypes = [
        vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int64, vp, vp
    ]
    L.cpr_mdp_vi_opts_default.argtypes = [P(MdpViOptsC)]
    L.cpr_mdp_value_iteration.argtypes = [vp, P(MdpC), P(MdpViOptsC), P(MdpViResultC)]
    L.cpr_mdp_pe_opts_default.argtypes = [P(MdpPeOptsC)]
    L.cpr_mdp_policy_evaluation.argtypes = [vp, P(MdpC), P(MdpPeC), P(MdpPeOptsC),
                                            P(MdpPeResultC)]


def lib():
    """Load libcpr_hip.so (no fallback: raises if it is missing)."""
    global _lib
    if _lib is None:
        path = os.environ.get("CPR_HIP_LIB", str(LIB_PATH))
        if not os.path.exists(path):
            raise ImportError(
                f"libcpr_hip.so not found at {path}; run __graft_entry__.build() (hipcc, gfx950)"
            )
        L = ctypes.CDLL(path)
        _declare(L)
        if L.cpr_abi_version() != ABI_VERSION:
            raise ImportError(f"{path} has ABI {L.cpr_abi_version()}, this module expects "
                              f"{ABI_VERSION}; rebuild with __graft_entry__.build()")
        _lib = L
    return _lib


def check(rc):
    if rc != CPR_OK:
        raise CprError(rc, lib().cpr_last_error().decode())
    return rc


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None
