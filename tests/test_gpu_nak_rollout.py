"""cpr_rollout over the Nakamoto closed-form lanes against the CPU oracle — needs an MI355X.

Every lane of a rollout must equal sequential oracle gym episodes with the auto-reset ids
i, i + n, i + 2n, ... and the oracle's own policy, bit for bit: observation floats (after a
done, the new episode's reset observation), rewards and dones. Lanes that leave the closed
form (propagation delay 0.05) must stay exact through the hand-over to the exact engine and
back. Summaries are compared with the oracle's records and with the fused episode kernel.
"""

import functools

import numpy as np
import pytest

import oracle_py as O
from cpr_amd import _lib as L
from cpr_amd import device

pytestmark = pytest.mark.gpu

SM1 = L.POLICY_SAPIRSHTEIN_2016_SM1


@pytest.fixture(scope="module")
def ctx():
    return device.default_context()


class Ref:
    """n oracle gym envs stepped with `policy`, auto-reset at episode id + n."""

    def __init__(self, cfg, n, policy, table=None):
        self.cfg, self.n, self.policy, self.table = cfg, n, policy, table
        self.ep = list(range(n))
        self.envs = [O.GymEnv(cfg, episode=i) for i in range(n)]
        self.obs0 = np.array([e.reset() for e in self.envs])
        self.finished = []  # info of every finished episode
        self.info = [None] * n  # info of each lane's last step
        self.last_done = [False] * n

    def actions(self):
        return np.array([O.nak_policy(self.policy, e.fields(), self.table) for e in self.envs],
                        dtype=np.int32)

    def run(self, T, reset=True):
        n = self.n
        obs = np.zeros((T, n, 4))
        rew = np.zeros((T, n))
        done = np.zeros((T, n), dtype=bool)
        for i in range(n):
            for t in range(T):
                e = self.envs[i]
                a = O.nak_policy(self.policy, e.fields(), self.table)
                o, r, d, info = e.step(a)
                self.info[i], self.last_done[i] = info, d
                if d and reset:
                    self.finished.append(info)
                    self.ep[i] += n
                    e = self.envs[i] = O.GymEnv(self.cfg, episode=self.ep[i])
                    o = e.reset()
                obs[t, i], rew[t, i], done[t, i] = o, r, d
        return obs, rew, done


def _check(got, ref):
    s, obs, rew, done = got
    robs, rrew, rdone = ref
    bad = np.argwhere(done != rdone)
    assert len(bad) == 0, ("done", bad[0])
    bad = np.argwhere(rew != rrew)
    assert len(bad) == 0, ("reward", bad[0], rew[tuple(bad[0])], rrew[tuple(bad[0])])
    bad = np.argwhere(obs != robs)
    assert len(bad) == 0, ("obs", bad[0], obs[tuple(bad[0][:2])], robs[tuple(bad[0][:2])])
    return s


def _batch(ctx, **kw):
    cfg, keep = device.make_config(**kw)
    return cfg, keep, device.Batch(cfg, ctx=ctx, keep=keep)


SUM_FIELDS = ["episodes", "reward_attacker_fx", "reward_defender_fx", "progress_fx",
              "rel_revenue_fx", "rel_revenue_sq_fx", "orphans", "status_tie", "status_overlap",
              "status_other", "invalid"]

BASE = dict(alpha=0.33, gamma=0.5, policy=SM1, max_steps=70, seed=123, n_lanes=32)
N1, T1 = 32, 300


@functools.lru_cache(maxsize=None)
def _base_ref():
    cfg, _ = device.make_config(**BASE)
    ref = Ref(cfg, N1, SM1)
    return ref, ref.run(T1)


@pytest.fixture(scope="module")
def base_rollout(ctx):
    cfg, keep, b = _batch(ctx, **BASE)
    return b, b.rollout(T1, outputs=True)


def test_nak_rollout_matches_sequential_oracle_episodes(ctx, base_rollout):
    ref, arrays = _base_ref()
    b, got = base_rollout
    s = _check(got, arrays)
    assert s.steps == N1 * T1
    assert len(ref.finished) == 4 * N1 and s.episodes == len(ref.finished)
    assert not any(ref.last_done)  # T is no multiple of max_steps: lanes end mid-episode
    acts = sum(int(i["episode_n_activations"]) for i in ref.finished) + \
        sum(int(i["episode_n_activations"]) for i in ref.info)
    assert s.activations == acts, (s.activations, acts)


def test_nak_rollout_split_and_resume(ctx, base_rollout):
    _, (s, obs, rew, done) = base_rollout
    _, _, b2 = _batch(ctx, **BASE)
    sa, obs_a, rew_a, done_a = b2.rollout(123, outputs=True)
    sb, obs_b, rew_b, done_b = b2.rollout(T1 - 123, outputs=True)
    assert np.array_equal(np.concatenate([obs_a, obs_b]), obs)
    assert np.array_equal(np.concatenate([rew_a, rew_b]), rew)
    assert np.array_equal(np.concatenate([done_a, done_b]), done)
    for f in ["steps", "activations"] + SUM_FIELDS:
        assert getattr(sa, f) + getattr(sb, f) == getattr(s, f), f
    assert [a + c for a, c in zip(sa.hist, sb.hist)] == list(s.hist)
    s2 = b2.rollout(10)
    assert s2.steps == N1 * 10


def test_nak_rollout_interleaved_with_step(ctx):
    cfg, keep, b = _batch(ctx, **BASE)
    ref = Ref(cfg, N1, SM1)
    _check(b.rollout(50, outputs=True), ref.run(50))
    for _ in range(5):
        acts = ref.actions()
        obs, rew, done, _ = b.step(acts)
        robs, rrew, rdone = ref.run(1, reset=False)
        assert np.array_equal(obs, robs[0]) and np.array_equal(rew, rrew[0])
        assert np.array_equal(done, rdone[0]) and not done.any()
    _check(b.rollout(50, outputs=True), ref.run(50))
    assert len(ref.finished) == N1  # every lane passed max_steps = 70 in the second rollout


def test_nak_rollout_table_policy_unit_observation(ctx):
    n, T = 16, 150
    table = np.random.default_rng(3).integers(0, 4, size=12 * 12 * 2).astype(np.uint8)
    cfg, keep, b = _batch(ctx, alpha=0.45, gamma=0.5, table=table, unit_observation=True,
                          max_steps=40, seed=77, n_lanes=n)
    assert cfg.policy == L.POLICY_TABLE
    ref = Ref(cfg, n, L.POLICY_TABLE, table)
    s = _check(b.rollout(T, outputs=True), ref.run(T))
    assert s.episodes == len(ref.finished) == n * (T // 40)


@pytest.mark.parametrize("policy", [L.POLICY_HONEST, L.POLICY_SIMPLE, L.POLICY_EYAL_SIRER_2014])
def test_nak_rollout_builtin_policies(ctx, policy):
    n, T = 16, 150
    cfg, keep, b = _batch(ctx, alpha=0.45, gamma=0.5, policy=policy, unit_observation=False,
                          max_steps=40, seed=77, n_lanes=n)
    ref = Ref(cfg, n, policy)
    s = _check(b.rollout(T, outputs=True), ref.run(T))
    assert s.episodes == len(ref.finished)


def test_nak_rollout_abstract_gamma_network(ctx):
    # the flagged abstract-gamma mode has no exact engine: one closed-form pass per call
    n, T = 16, 150
    cfg, keep, b = _batch(ctx, alpha=0.4, gamma=1.0, defenders=3, network=L.NET_ABSTRACT_GAMMA,
                          policy=SM1, unit_observation=False, max_steps=40, seed=11, n_lanes=n)
    ref = Ref(cfg, n, SM1)
    s = _check(b.rollout(T, outputs=True), ref.run(T))
    assert s.episodes == len(ref.finished) == n * (T // 40)


def test_nak_rollout_fc16_stays_unsupported(ctx):
    cfg, keep = device.make_config(alpha=0.3, gamma=0.5, protocol=L.PROTO_FC16, max_steps=100,
                                   policy=L.FC16_POLICY_HONEST, n_lanes=4)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    with pytest.raises(L.CprError) as e:
        b.rollout(4)
    assert e.value.code == L.CPR_E_UNSUPPORTED


@pytest.mark.parametrize("clause", ["max_progress", "max_time"])
def test_nak_rollout_termination_clauses(ctx, clause):
    n, T = 16, 400
    kw = dict(max_progress=24) if clause == "max_progress" else dict(max_time=24.5)
    cfg, keep, b = _batch(ctx, alpha=0.33, gamma=0.5, policy=SM1, max_steps=5000, seed=5,
                          n_lanes=n, **kw)
    ref = Ref(cfg, n, SM1)
    s = _check(b.rollout(T, outputs=True), ref.run(T))
    assert len(ref.finished) >= n
    assert s.episodes == len(ref.finished)
    assert all(i["episode_n_steps"] < 5000 for i in ref.finished)


HAND = dict(alpha=0.42, gamma=0.5, propagation_delay=0.05, policy=SM1, seed=901, max_steps=60,
            n_lanes=64)


def test_nak_rollout_hand_over_to_exact_engine(ctx):
    n, T = 64, 150
    cfg, keep, b = _batch(ctx, **HAND)
    rec = O.run_episodes(cfg, 0, 128, threads=8)
    overlap = (rec["status"] & L.ST_OVERLAP) != 0
    # lanes go closed form -> exact -> closed form inside one call
    assert overlap.sum() > 64 and (~overlap).sum() >= 8
    ref = Ref(cfg, n, SM1)
    s = _check(b.rollout(T, outputs=True), ref.run(T))
    assert len(ref.finished) == 128 and s.episodes == 128
    assert s.reward_attacker_fx == sum(int(x) << 20 for x in rec["reward_attacker"])
    assert s.reward_defender_fx == sum(int(x) << 20 for x in rec["reward_defender"])
    assert s.progress_fx == sum(int(x) << 20 for x in rec["progress"])
    assert s.orphans == int((rec["n_activations"] - rec["head_height"]).sum())
    assert s.status_overlap == int(overlap.sum())
    assert s.invalid == 0
    # cpr_step continues from the lanes' state, exact lanes included
    acts = ref.actions()
    obs, rew, done, info = b.step(acts)
    robs, rrew, rdone = ref.run(1, reset=False)
    assert np.array_equal(obs, robs[0]) and np.array_equal(rew, rrew[0])
    assert np.array_equal(done, rdone[0])
    st = info["status"]
    assert not ((st & L.ST_LOCKSTEP_INEXACT != 0) & (st & L.ST_EXACT_RERUN == 0)).any()


def test_nak_rollout_hand_over_gamma0_eyal_sirer(ctx):
    n, T = 64, 150
    kw = dict(HAND, gamma=0.0, policy=L.POLICY_EYAL_SIRER_2014)
    cfg, keep, b = _batch(ctx, **kw)
    ref = Ref(cfg, n, L.POLICY_EYAL_SIRER_2014)
    _check(b.rollout(T, outputs=True), ref.run(T))


@pytest.mark.parametrize("n,T", [(70, 1), (1, 130)])
def test_nak_rollout_ragged_shapes_and_null_outputs(ctx, n, T):
    kw = dict(alpha=0.33, gamma=0.5, policy=SM1, max_steps=50, seed=31, n_lanes=n)
    cfg, keep, b = _batch(ctx, **kw)
    ref = Ref(cfg, n, SM1)
    s = _check(b.rollout(T, outputs=True), ref.run(T))
    assert s.steps == n * T and s.episodes == len(ref.finished)
    _, _, b2 = _batch(ctx, **kw)
    s2 = b2.rollout(T)
    for f in ["steps", "activations"] + SUM_FIELDS:
        assert getattr(s2, f) == getattr(s, f), f
    assert list(s2.hist) == list(s.hist)


def test_nak_rollout_summary_equals_fused_episodes(ctx, base_rollout):
    b, (s, _, _, _) = base_rollout
    cfg, keep = device.make_config(**BASE)
    fused = device.Batch(cfg, ctx=ctx, keep=keep).run(N1 * (T1 // BASE["max_steps"]),
                                                      first_episode=0)
    for f in SUM_FIELDS:
        assert getattr(s, f) == getattr(fused, f), f
    assert list(s.hist) == list(fused.hist)
