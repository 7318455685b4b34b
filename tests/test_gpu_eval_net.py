"""Evaluation of the policy network per alpha on the device (cpr_eval_net, the cyclic
assumption schedule, cpr_policy_net_copy) — needs an MI355X.

Shared shape: 32 lanes, the table {0.125, 0.25, 0.375, 0.5} cycled (episode e runs at entry
e % 4), gamma 0.5, max_steps 32, 24 episodes per alpha: 96 episodes, three per lane. The
integer network is test_gpu_lane_env.py's, so the oracle side's forward_f64 decisions are exact.

1. records against the oracle: one oracle gym env per episode, made with alpha TABLE[e % 4],
   wrapped by cpr_amd/wrappers.py (sparse_relative, r / alpha, EpisodeRecorderWrapper) and
   driven by forward_f64; every record field bit for bit (the status word is the device
   route's diagnostic: checked for validity). One variant ends episodes by max_progress, at
   different steps, so that lanes park and check_every matters;
2. invariance under n_lanes, check_every, first_episode, also in sampled mode;
3. per-alpha summaries against eval_ref's restatement from the records, their sum, and the
   summary of a rollout that finishes exactly the same episodes;
4. the statistics against eval_ref's restatement of the documented order, bit for bit;
5. the cyclic schedule on reset / step / masked reset; a one-entry table under either schedule;
6. copy_policy_net_from and ppo.train(eval_batch=...);
7. refusals.
"""

import ctypes
import functools

import numpy as np
import pytest

import eval_ref as E
import oracle_py as O
from cpr_amd import _lib as L
from cpr_amd import device, envs, wrappers
from cpr_amd import ppo as P
from test_gpu_lane_env import float_net, int_net, magnitude_bound

pytestmark = pytest.mark.gpu

N = 32
TABLE = (0.125, 0.25, 0.375, 0.5)
A = len(TABLE)
GAMMA = 0.5
CFG_ALPHA = 0.33  # the batch's own alpha: no episode may run at it
MAX_STEPS = 32
EPA = 24
N_SET = A * EPA
PROTO = {"nakamoto": dict(protocol=L.PROTO_NAKAMOTO), "bk": dict(protocol=L.PROTO_BK, k=2)}
SHAPE = {"nakamoto": (4, 4), "bk": (8, 8)}
ENV = {"nakamoto": O.GymEnv, "bk": O.BkGymEnv}
BASE = {"nakamoto": dict(max_steps=MAX_STEPS, propagation_delay=0.05, seed=2024,
                         unit_observation=False),
        "bk": dict(max_steps=MAX_STEPS, seed=2024, unit_observation=False)}
# the variant whose episodes end by progress, at different steps
PROGRESS = {"nakamoto": 6, "bk": 8}
WSEED = 3
INFO_KEYS = ["alpha", "episode_sim_time", "episode_chain_time", "episode_progress",
             "episode_n_activations", "episode_n_steps", "episode_reward_attacker",
             "episode_reward_defender", "head_height"]
ENV_ARGS = dict(alphas=TABLE, alpha_column=0, reward="sparse_relative", shape="per_alpha",
                schedule="cycle")


@pytest.fixture(scope="module")
def ctx():
    return device.default_context()


def conf(proto, variant):
    kw = dict(BASE[proto])
    if variant == "progress":
        kw["max_progress"] = PROGRESS[proto]
    return kw


def make_cfg(proto, variant, n_lanes=N, alpha=CFG_ALPHA, **over):
    kw = dict(conf(proto, variant), **over)
    return device.make_config(**dict(PROTO[proto], alpha=alpha, gamma=GAMMA, n_lanes=n_lanes, **kw))


def the_net(proto, extra=(TABLE[0], GAMMA)):
    ol, na = SHAPE[proto]
    return int_net(WSEED, ol + 2, na, extra)


def eval_batch(ctx, proto, variant, n_lanes=N, net=None, **over):
    cfg, keep = make_cfg(proto, variant, n_lanes=n_lanes, **over)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    b.set_lane_env(**ENV_ARGS)
    b.set_policy_net(net if net is not None else the_net(proto))
    return b


class OracleEnv:
    """An oracle gym env under cpr_amd/wrappers.py: the wrappers' env protocol, and the alpha
    the assumption schedule reports in info."""

    action_space = observation_space = None

    def __init__(self, core, alpha):
        self.core, self.alpha = core, alpha

    @property
    def unwrapped(self):
        return self

    def reset(self):
        return self.core.reset()

    def step(self, action):
        obs, r, d, info = self.core.step(action)
        return obs, r, d, dict(info, alpha=self.alpha)


@functools.lru_cache(maxsize=None)
def oracle_records(proto, variant):
    """The 96 records the reference's eval env would log, and what the preconditions need:
    (records, Nakamoto diag, every network input row)."""
    ol, na = SHAPE[proto]
    cfgs = {a: make_cfg(proto, variant, alpha=a)[0] for a in TABLE}
    nets = {a: the_net(proto, (a, GAMMA)) for a in TABLE}
    rec = np.zeros(N_SET, dtype=L.EVAL_RECORD_DTYPE)
    diag, rows, actions = 0, [], set()
    for e in range(N_SET):
        a = TABLE[e % A]
        core = ENV[proto](cfgs[a], episode=e)
        env = wrappers.SparseRelativeRewardWrapper(OracleEnv(core, a))
        env = wrappers.MapRewardWrapper(env, lambda r, i: r / i["alpha"])
        env = wrappers.EpisodeRecorderWrapper(env, n=1, info_keys=INFO_KEYS)
        o, done = env.reset(), False
        while not done:
            rows.append(np.concatenate([o, [a, GAMMA]]))
            act = int(np.argmax(nets[a].forward_f64(np.asarray(o)[None])[0][0]))
            actions.add(act)
            o, _, done, _ = env.step(act)
        h = env.erw_history[-1]
        r = rec[e]
        r["episode"], r["alpha_index"], r["alpha"] = e, e % A, h["alpha"]
        r["episode_reward"] = h["episode_reward"]
        for k in ("episode_sim_time", "episode_chain_time", "episode_progress",
                  "episode_n_activations", "episode_n_steps"):
            r[k] = h[k]
        r["reward_attacker"] = h["episode_reward_attacker"]
        r["reward_defender"] = h["episode_reward_defender"]
        r["height"] = int(h["episode_progress"]) if proto == "bk" else h["head_height"]
        if proto == "nakamoto":
            diag |= core.diag()
    return rec, diag, np.array(rows), actions


RECORD_FIELDS = [f for f in L.EVAL_RECORD_DTYPE.names if f != "status"]


def assert_records_equal(got, want, fields=L.EVAL_RECORD_DTYPE.names):
    for f in fields:
        x, y = got[f], want[f]
        if x.dtype.kind == "f":
            x, y = x.view(np.uint64), y.view(np.uint64)
        bad = np.flatnonzero(x != y)
        assert len(bad) == 0, (f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])


def assert_same_result(x, y):
    assert_records_equal(x.records, y.records)
    assert x.stats.tobytes() == y.stats.tobytes()
    for sx, sy in zip(x.summaries, y.summaries):
        assert bytes(sx) == bytes(sy)
    assert bytes(x.total) == bytes(y.total)


# ------------------------------------------------------------- 1. records against the oracle

@pytest.mark.parametrize("variant", ["steps", "progress"])
@pytest.mark.parametrize("proto", ["nakamoto", "bk"])
def test_records_equal_the_oracle_under_the_python_wrappers(ctx, proto, variant):
    want, diag, rows, actions = oracle_records(proto, variant)
    # preconditions, on the oracle's run: exact integer arithmetic (inputs are multiples of
    # 1/8 and every partial sum is below 2^21), a non-trivial policy, rewards paid
    assert np.array_equal(rows * 8, np.rint(rows * 8))
    assert magnitude_bound(the_net(proto), rows) < 2 ** 21
    assert len(actions) >= 3 and np.any(want["episode_reward"] != 0.0)
    if proto == "nakamoto":
        assert diag & 2  # DIAG_OVERLAP: the exact hand-over ran
    steps = want["episode_n_steps"]
    if variant == "steps":
        assert np.all(steps == MAX_STEPS)
    else:
        assert len(np.unique(steps)) >= 2
        quota = [int(steps[i::N].sum()) for i in range(N)]  # lane i runs episodes i, i + 32, i + 64
        assert len(set(quota)) >= 2  # a lane finishes its three episodes before another
    res = eval_batch(ctx, proto, variant).evaluate_net(EPA, check_every=5)
    assert_records_equal(res.records, want, RECORD_FIELDS)
    st = res.records["status"]
    assert not (st & L.ST_INVALID).any()
    assert not ((st & L.ST_LOCKSTEP_INEXACT != 0) & (st & L.ST_EXACT_RERUN == 0)).any()
    assert [d["alpha"] for d in res.per_alpha] == list(TABLE)


# ------------------------------------------------------------------------- 2. invariance

@functools.lru_cache(maxsize=None)
def base_result(proto, variant="progress"):
    return eval_batch(device.default_context(), proto, variant).evaluate_net(EPA)


@pytest.mark.parametrize("n_lanes,check_every", [(32, 5), (20, None), (20, 5), (96, None), (96, 5)])
@pytest.mark.parametrize("proto", ["nakamoto", "bk"])
def test_results_do_not_depend_on_lanes_or_check_every(ctx, proto, n_lanes, check_every):
    got = eval_batch(ctx, proto, "progress", n_lanes=n_lanes).evaluate_net(
        EPA, check_every=check_every)
    assert_same_result(got, base_result(proto))


@pytest.mark.parametrize("proto", ["nakamoto", "bk"])
def test_a_later_first_episode_is_a_slice_of_the_larger_set(ctx, proto):
    base = base_result(proto)
    first, epa = 6, 6  # episodes 6 .. 29: entry j's first slot is (j - 6) % 4
    got = eval_batch(ctx, proto, "progress").evaluate_net(epa, first_episode=first)
    assert_records_equal(got.records, base.records[first:first + A * epa])
    assert np.array_equal(got.records["episode"], np.arange(first, first + A * epa))
    check_reduction(got, first)


def sampled_net(proto):
    ol, na = SHAPE[proto]
    return float_net(7, ol + 2, 2, 48, 32, na, extra=(0.4, GAMMA))


@pytest.mark.parametrize("proto", ["nakamoto", "bk"])
def test_sampled_mode_does_not_depend_on_lanes(ctx, proto):
    net = sampled_net(proto)
    x = eval_batch(ctx, proto, "progress", n_lanes=32, net=net).evaluate_net(
        EPA, deterministic=False)
    y = eval_batch(ctx, proto, "progress", n_lanes=20, net=net).evaluate_net(
        EPA, deterministic=False, check_every=5)
    assert_same_result(x, y)
    d = eval_batch(ctx, proto, "progress", net=net).evaluate_net(EPA, deterministic=True)
    assert d.records.tobytes() != x.records.tobytes()  # the draws are in use


# ------------------------------------------------------------- 3., 4. summaries, statistics

def check_reduction(res, first=0):
    """Per-alpha summaries and statistics against eval_ref's restatement from the records."""
    per = len(res.records) // A
    total = {f: 0 for f in E.SUM_FIELDS}
    hist = np.zeros(L.HIST_BINS, dtype=np.int64)
    for j, slots in enumerate(E.alpha_slots(A, first, len(res.records))):
        mine = res.records[slots]
        assert len(mine) == per and np.all(mine["alpha_index"] == j)
        assert np.all(mine["alpha"] == TABLE[j])
        want = E.summary(mine)
        assert E.summary_of(res.summaries[j]) == want, j
        assert want["episodes"] == per and want["invalid"] == 0
        n, mean, std = E.stats(mine)
        assert (res.stats["n"][j], res.stats["alpha"][j]) == (n, TABLE[j])
        assert E.same_bits(res.stats["mean"][j], mean), (j, res.stats["mean"][j], mean)
        assert E.same_bits(res.stats["std"][j], std), (j, res.stats["std"][j], std)
        d = res.per_alpha[j]
        assert d["n"] == n and d["summary"] is res.summaries[j]
        assert E.same_bits([d["mean_" + c] for c in L.EVAL_COLUMNS], mean)
        assert E.same_bits([d["std_" + c] for c in L.EVAL_COLUMNS], std)
        for f in E.SUM_FIELDS:
            total[f] += want[f]
        hist += np.array(want["hist"])
    got = E.summary_of(res.total)
    assert got == dict(total, hist=hist.tolist())  # the field-wise sum


@pytest.mark.parametrize("variant", ["steps", "progress"])
@pytest.mark.parametrize("proto", ["nakamoto", "bk"])
def test_per_alpha_summaries_and_statistics_follow_the_records(ctx, proto, variant):
    res = base_result(proto, variant)
    assert len(res.records) == N_SET
    check_reduction(res)
    assert res.total.episodes == N_SET
    # the statistics are not degenerate: alphas differ, and so do episodes within an alpha
    assert len(np.unique(res.stats["mean"][:, 0])) >= 2
    assert np.all(res.stats["std"][:, 1] > 0)  # sim time


@pytest.mark.parametrize("proto", ["nakamoto", "bk"])
def test_total_equals_a_rollout_that_finishes_the_same_episodes(ctx, proto):
    """96 lanes, episodes of exactly max_steps steps: a rollout of max_steps steps finishes
    episodes 0 .. 95 and nothing else. Every summary field that is over finished episodes is
    equal. `activations` is, by the rollout's contract, that of the whole rollout: it also
    counts what the 96 auto-reset episodes 96 .. 191 simulated up to their first observation,
    which no evaluation of the set [0, 96) can contain; so the evaluation's is compared with
    its records, and the rollout's must exceed it."""
    total = base_result(proto, "steps").total
    b = eval_batch(ctx, proto, "steps", n_lanes=N_SET)
    s, out = b.rollout_net(MAX_STEPS, deterministic=True)
    assert out["done"][-1].all() and not out["done"][:-1].any()
    for f in E.SUM_FIELDS:
        if f != "activations":
            assert getattr(s, f) == getattr(total, f), f
    assert list(s.hist) == list(total.hist)
    assert total.activations == int(base_result(proto, "steps").records["episode_n_activations"].sum())
    assert s.activations > total.activations


# ---------------------------------------------- 5. the cyclic schedule on the existing paths

@pytest.mark.parametrize("proto", ["nakamoto", "bk"])
def test_cycle_schedule_on_reset_step_and_masked_reset(ctx, proto):
    cfg, keep = make_cfg(proto, "progress")
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    b.set_lane_env(alphas=TABLE, schedule="cycle")
    policy = {"nakamoto": L.POLICY_SAPIRSHTEIN_2016_SM1, "bk": L.BK_POLICY_GET_AHEAD}[proto]
    ids = np.arange(100, 100 + N, dtype=np.uint64)  # a reset at caller-chosen ids

    def want():
        return np.array([TABLE[int(e) % A] for e in ids])

    obs = b.reset(episode_ids=ids)
    assert np.array_equal(b.lane_alpha(), want())
    dones = 0
    for t in range(48):
        obs, _, done, _ = b.step(b.policy_actions(policy, obs))
        if done.any():
            dones += int(done.sum())
            ids[done] += N
            obs = b.reset(mask=done, episode_ids=ids)
        assert np.array_equal(b.lane_alpha(), want()), t
    assert dones > N  # lanes went through more than one masked reset


@pytest.mark.parametrize("proto", ["nakamoto", "bk"])
def test_one_entry_table_is_the_same_under_either_schedule(ctx, proto):
    out = []
    for schedule in ("choice", "cycle"):
        cfg, keep = make_cfg(proto, "progress", alpha=0.4)
        b = device.Batch(cfg, ctx=ctx, keep=keep)
        b.set_lane_env(alphas=[0.4], alpha_column=0, reward="sparse_relative", shape="per_alpha",
                       schedule=schedule)
        b.set_policy_net(sampled_net(proto))
        s, arrays = b.rollout_net(48, deterministic=False)
        out.append((bytes(s), {k: v.tobytes() for k, v in arrays.items()}))
        assert arrays["done"].any()
    assert out[0] == out[1]


def test_device_env_fn_builds_the_eval_env(ctx):
    b, extras = envs.device_env_fn(N, ctx=ctx, seed=7, protocol="nakamoto", episode_len=16,
                                   alpha=list(TABLE), gamma=GAMMA, shape="cut", eval=True)
    b.set_policy_net(int_net(WSEED, 4 + 2, 4, extras))
    res = b.evaluate_net(2)
    assert np.array_equal(res.records["alpha"], [TABLE[e % A] for e in range(2 * A)])
    ra, rd = res.records["reward_attacker"], res.records["reward_defender"]
    rel = np.divide(ra, ra + rd, out=np.zeros_like(ra), where=(ra + rd) != 0)
    assert np.array_equal(res.records["episode_reward"], rel / res.records["alpha"])  # per_alpha


# ------------------------------------------------------- 6. copy_policy_net_from and train

def train_batch(ctx, seed=41):
    cfg, keep = device.make_config(**dict(PROTO["nakamoto"], alpha=0.35, gamma=GAMMA, max_steps=6,
                                          seed=seed, n_lanes=70))
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    b.set_lane_env(alphas=[0.2, 0.3, 0.45], alpha_column=0, reward="sparse_relative",
                   shape="per_alpha")
    b.set_policy_net(float_net(33, 4 + 2, 2, 32, 32, 4, extra=(0.375, 0.7)))
    return b


def small_eval_batch(ctx, net=None):
    cfg, keep = device.make_config(**dict(PROTO["nakamoto"], alpha=0.35, gamma=GAMMA, max_steps=6,
                                          seed=977, n_lanes=N))
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    b.set_lane_env(alphas=[0.2, 0.3, 0.45], alpha_column=0, reward="sparse_relative",
                   shape="per_alpha", schedule="cycle")
    if net is not None:
        b.set_policy_net(net)
    return b


OPTS = P.PPOOptions(n_epochs=2, minibatch=100, ent_coef=0.01, lr=1e-3)


def test_copy_policy_net_equals_a_host_round_trip(ctx):
    tr = train_batch(ctx)
    before = P.flatten_params(tr.get_policy_net())
    tr.ppo_iterate(8, OPTS)
    trained = tr.get_policy_net()
    assert np.any(P.flatten_params(trained) != before)
    ev = small_eval_batch(ctx)  # no network yet: it acquires the shapes
    ev.copy_policy_net_from(tr)
    twin = small_eval_batch(ctx, net=trained)
    x, y = ev.evaluate_net(8), twin.evaluate_net(8)
    assert_same_result(x, y)
    assert P.flatten_params(ev.get_policy_net()).tobytes() == P.flatten_params(trained).tobytes()
    assert P.flatten_params(tr.get_policy_net()).tobytes() == P.flatten_params(trained).tobytes()
    # a second copy into the now-shaped batch, after another update
    tr.ppo_iterate(8, OPTS)
    ev.copy_policy_net_from(tr)
    twin.set_policy_net(tr.get_policy_net())
    assert_same_result(ev.evaluate_net(8), twin.evaluate_net(8))


def test_train_with_an_eval_batch(ctx):
    plain = train_batch(ctx)
    ref = [(bytes(s), st) for s, st in P.train(plain, 3, 8, OPTS)]
    tr, ev = train_batch(ctx), small_eval_batch(ctx)
    got = list(P.train(tr, 3, 8, OPTS, eval_batch=ev, eval_freq=2, eval_start=0,
                       eval_episodes_per_alpha=8))
    for it, ((s, st), (rs, rst)) in enumerate(zip(got, ref)):
        evaluated = it % 2 == 0
        assert ("eval/mean_episode_reward" in st) == evaluated, it
        assert bytes(s) == rs and {k: v for k, v in st.items() if not k.startswith("eval/")} == rst
        if not evaluated:
            continue
        table = st["eval/per_alpha"]
        assert [d["alpha"] for d in table] == [0.2, 0.3, 0.45]
        assert all(d["n"] == 8 and d["summary"].episodes == 8 for d in table)
        for c in L.EVAL_COLUMNS:
            assert np.isfinite(st["eval/mean_" + c]) and np.isfinite(st["eval/std_" + c])
    assert P.flatten_params(tr.get_policy_net()).tobytes() == \
        P.flatten_params(plain.get_policy_net()).tobytes()
    # the first evaluation saw the initial weights: the host's numbers from its records
    first = small_eval_batch(ctx, net=train_batch(ctx)._net).evaluate_net(8)
    want = P.eval_statistics(first)
    x = first.records["episode_reward"]
    assert want["eval/mean_episode_reward"] == float(np.mean(x))
    assert want["eval/std_episode_reward"] == float(np.std(x, ddof=1))
    assert got[0][1]["eval/mean_episode_reward"] == want["eval/mean_episode_reward"]
    assert got[0][1]["eval/std_episode_sim_time"] == want["eval/std_episode_sim_time"]


# --------------------------------------------------------------------------- 7. refusals

def _code(fn):
    with pytest.raises(L.CprError) as e:
        fn()
    return e.value.code


def test_refusals(ctx):
    cfg, keep = make_cfg("nakamoto", "steps")
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    b.set_lane_env(**ENV_ARGS)
    assert _code(lambda: b.evaluate_net(2)) == L.CPR_E_STATE  # no network
    assert L.lib().cpr_lane_env_schedule(b.handle, 2) == L.CPR_E_INVALID_ARG
    assert L.lib().cpr_lane_env_schedule(b.handle, -1) == L.CPR_E_INVALID_ARG
    with pytest.raises(ValueError):
        b.set_lane_env(alphas=TABLE, schedule="shuffle")
    b.set_policy_net(the_net("nakamoto"))
    assert _code(lambda: b.evaluate_net(0)) == L.CPR_E_INVALID_ARG
    assert _code(lambda: b.evaluate_net(-3)) == L.CPR_E_INVALID_ARG
    assert _code(lambda: b.evaluate_net(2, check_every=-1)) == L.CPR_E_INVALID_ARG
    # none of the refused calls started an evaluation: the schedule can still be set
    assert L.lib().cpr_lane_env_schedule(b.handle, L.SCHEDULE_CYCLE) == L.CPR_OK
    b.evaluate_net(2)
    # the lanes stand in later episodes: stepping needs a reset of every lane
    acts = np.zeros(N, dtype=np.int32)
    assert _code(lambda: b.step(acts)) == L.CPR_E_STATE
    assert _code(lambda: b.rollout_net(2)) == L.CPR_E_STATE
    mask = np.ones(N, dtype=np.uint8)
    mask[3] = 0
    assert _code(lambda: b.reset(mask=mask)) == L.CPR_E_STATE
    assert L.lib().cpr_lane_env_schedule(b.handle, L.SCHEDULE_CYCLE) == L.CPR_E_STATE
    b.evaluate_net(2)  # another evaluation needs none
    b.reset()
    b.step(acts)
    b.rollout_net(2)
    # the schedule entry after a reset
    cfg, keep = make_cfg("bk", "steps")
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    b.set_lane_env(alphas=TABLE)
    b.reset()
    assert L.lib().cpr_lane_env_schedule(b.handle, L.SCHEDULE_CYCLE) == L.CPR_E_STATE
    # max_steps = 0: nothing bounds an episode
    cfg, keep = make_cfg("nakamoto", "progress", max_steps=0)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    b.set_lane_env(**ENV_ARGS)
    b.set_policy_net(the_net("nakamoto"))
    assert _code(lambda: b.evaluate_net(2)) == L.CPR_E_UNSUPPORTED
    # several alphas under the keyed choice
    cfg, keep = make_cfg("nakamoto", "steps")
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    b.set_lane_env(alphas=TABLE, alpha_column=0)
    b.set_policy_net(the_net("nakamoto"))
    assert _code(lambda: b.evaluate_net(2)) == L.CPR_E_UNSUPPORTED
    # FC16
    cfg, keep = device.make_config(alpha=0.3, gamma=0.5, protocol=L.PROTO_FC16, max_steps=100,
                                   policy=L.FC16_POLICY_HONEST, n_lanes=4)
    fc = device.Batch(cfg, ctx=ctx, keep=keep)
    assert _code(lambda: fc.evaluate_net(2)) == L.CPR_E_UNSUPPORTED
    assert L.lib().cpr_lane_env_schedule(fc.handle, L.SCHEDULE_CYCLE) == L.CPR_E_UNSUPPORTED
    # NULL arguments
    o = L.EvalOptsC()
    o.episodes_per_alpha = 1
    assert L.lib().cpr_eval_net(b.handle, ctypes.byref(o), None, None, None, None) == \
        L.CPR_E_INVALID_ARG


def test_copy_refusals(ctx):
    src = eval_batch(ctx, "nakamoto", "steps")
    cfg, keep = make_cfg("nakamoto", "steps")
    empty = device.Batch(cfg, ctx=ctx, keep=keep)
    assert _code(lambda: src.copy_policy_net_from(empty)) == L.CPR_E_STATE  # nothing to copy
    # different shapes: width, depth, extras
    for net in (float_net(1, 4 + 2, 3, 48, 32, 4, extra=(TABLE[0], GAMMA)),
                float_net(1, 4 + 2, 2, 32, 32, 4, extra=(TABLE[0], GAMMA)),
                float_net(1, 4 + 2, 3, 32, 32, 4, extra=(0.3, GAMMA)),
                float_net(1, 4 + 1, 3, 32, 32, 4, extra=(TABLE[0],))):
        dst = device.Batch(cfg, ctx=ctx, keep=keep)
        dst.set_policy_net(net)
        assert _code(lambda: dst.copy_policy_net_from(src)) == L.CPR_E_INVALID_ARG
    # another protocol: observation and action widths differ
    other = eval_batch(ctx, "bk", "steps")
    assert _code(lambda: other.copy_policy_net_from(src)) == L.CPR_E_INVALID_ARG
    cfgb, keepb = make_cfg("bk", "steps")
    assert _code(lambda: device.Batch(cfgb, ctx=ctx, keep=keepb).copy_policy_net_from(src)) == \
        L.CPR_E_INVALID_ARG
    # a lane env whose alpha column the source's extras do not reach
    dst = device.Batch(cfg, ctx=ctx, keep=keep)
    dst.set_lane_env(alphas=TABLE, alpha_column=0)
    one = device.Batch(cfg, ctx=ctx, keep=keep)
    one.set_policy_net(float_net(1, 4, 1, 16, 16, 4))
    assert _code(lambda: dst.copy_policy_net_from(one)) == L.CPR_E_INVALID_ARG
    # the same shapes: accepted, and the copy is the source's network
    dst = device.Batch(cfg, ctx=ctx, keep=keep)
    dst.set_policy_net(the_net("nakamoto").zeros_like())
    dst.copy_policy_net_from(src)
    assert P.flatten_params(dst.get_policy_net()).tobytes() == \
        P.flatten_params(the_net("nakamoto")).tobytes()
