"""The timed sweep path against the CPU oracle, summary word by summary word.

cpr_run_episodes_async groups the bench's calls into k_run_episodes_fused launches (five
gamma = 0 or two gamma = .5 points per lane, lane groups of 2 or 4 lanes per episode, packed
tips, the wave work queue, the gamma = .5 eager second passes on the side stream through the
context's two list buffers). Every case here issues such calls as bench.py's one_step does
(run_async per point into zeroed device summaries, one synchronize at the end), runs the same
episodes in the oracle (oracle/src, pinned by the reference's own vectors in
test_oracle_kat.py), reduces the oracle's records with oracle_py.reduce_records (written from
include/cpr_hip.h, checked by test_reduce_records_host.py) and compares with integer
equality: episodes, steps, activations, the three *_fx sums, rel_revenue_fx,
rel_revenue_sq_fx, orphans, all 64 histogram bins and invalid. Nothing takes a tolerance.

status_tie and status_overlap are diagnostics of the route that ran (include/cpr_hip.h), so
they are bounded, not compared: the device's tie count is at most the oracle's, and positive
where a case exists to provoke ties or overlaps. status_other must be 0.

Every case also asserts that the intended kernel ran: the members of one launch report
equal shares of one kernel's time (last_launch), cut as L.NAK_FUSE_MAX* / L.NAK_FUSE_LANES*
say, and a member that runs alone reports the one-point kernel's resident lanes. No case
compares one device path with another; test_gpu_fused_points.py, test_gpu_lane_groups.py
and test_gpu_packed_tips.py do that.
"""

import ctypes
import os

import pytest

import oracle_py as O
from cpr_amd import _lib as L
from cpr_amd import device

pytestmark = pytest.mark.gpu

NAMAX = L.NAK_FUSE_MAX
NAMAX_ARR = L.NAK_FUSE_MAX_ARR  # gamma = .5
G0 = L.NAK_FUSE_LANES           # lanes per episode, gamma = 0
G5 = L.NAK_FUSE_LANES_ARR       # gamma = .5
FULL0 = NAMAX * G0              # a full lane-group launch: 10 members
FULL5 = NAMAX_ARR * G5          # 8 members
SHAPE = {0.0: (FULL0, NAMAX, G0), 0.5: (FULL5, NAMAX_ARR, G5)}
WORDS = ctypes.sizeof(L.Summary) // 8

BENCH_ALPHAS = (0.05, 0.10, 0.15, 0.20, 0.25, 0.30, 0.35, 0.40, 0.45, 0.50)  # bench.py
BENCH_SEED = 0x5EED0000
BENCH_STEPS = 2016
ALPHAS = (.05, .25, .35, .45, .5, .10, .15, .20, .30, .40, .33)  # test_gpu_lane_groups.py
SEED = 0x0AC1E
# one full and one partial wave for every lane-group width: 64 / G episodes per wave
N = 64 * 5 + 37
EXACT = ["episodes", "steps", "activations", "reward_attacker_fx", "reward_defender_fx",
         "progress_fx", "rel_revenue_fx", "rel_revenue_sq_fx", "orphans", "invalid"]
POLICIES = {"honest": L.POLICY_HONEST, "simple": L.POLICY_SIMPLE,
            "es2014": L.POLICY_EYAL_SIRER_2014, "sm1": L.POLICY_SAPIRSHTEIN_2016_SM1}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def ctx(torch):
    c = device.Context(0)
    yield c
    c.close()


class Env:
    """Environment variables for the calls inside (the library reads them at every call);
    None unsets."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


GROUPED = dict(CPR_NAK_FUSE=None, CPR_NAK_FUSE_LANES=None)

_oracle_cache = {}


def _oracle(cfg, first, n):
    """reduce_records of the oracle's episodes [first, first + n) of cfg, with the greatest
    head height beside it; computed once per (config, first, n) in this module."""
    key = (bytes(cfg), int(first), int(n))
    if key not in _oracle_cache:
        rec = O.run_episodes(cfg, first, n, threads=8)
        red = O.reduce_records(rec)
        red["max_height"] = int(rec["head_height"].max())
        _oracle_cache[key] = red
    return _oracle_cache[key]


def _cycle(alphas, m):
    return [alphas[i % len(alphas)] for i in range(m)]


def _points(alphas, **kw):
    return [dict(alpha=a, **kw) for a in alphas]


def _sweep(torch, ctx, points, rounds, env=None):
    """One batch per point (device.make_config keywords); per round (first, n) one run_async
    per batch, all into the same zeroed device summaries; one synchronize; then the oracle
    over the rounds' (contiguous) episodes. Returns (device Summary, oracle reduction) per
    point, each batch's last_launch ms and launch_shape, and the one-point kernel's resident
    lanes of each batch (its launch_shape before any launch)."""
    assert all(rounds[i][0] + rounds[i][1] == rounds[i + 1][0] for i in range(len(rounds) - 1))
    cfgs, batches = [], []
    for p in points:
        cfg, keep = device.make_config(**p)
        cfgs.append(cfg)
        batches.append(device.Batch(cfg, ctx=ctx, keep=keep))
    try:
        resident1 = [b.launch_shape()[1] for b in batches]
        sums = [torch.zeros(WORDS, dtype=torch.int64, device="cuda") for _ in batches]
        with Env(**dict(GROUPED, **(env or {}))):
            try:
                for first, n in rounds:
                    for b, s in zip(batches, sums):
                        b.run_async(n, first, s.data_ptr())
            finally:
                ctx.synchronize()
            ms = [b.last_launch()[0] for b in batches]
            shapes = [b.launch_shape() for b in batches]
        got = [L.Summary.from_buffer_copy(s.cpu().numpy().tobytes()) for s in sums]
    finally:
        for b in batches:
            b.close()
    first, total = rounds[0][0], sum(n for _, n in rounds)
    ref = [_oracle(cfg, first, total) for cfg in cfgs]
    return got, ref, ms, shapes, resident1


def _describe(p):
    return ", ".join(f"{k}={v}" for k, v in p.items())


def _assert_pinned(points, got, ref):
    """Every route-independent word equal to the oracle's; the route diagnostics bounded."""
    for p, s, r in zip(points, got, ref):
        for f in EXACT:
            assert int(getattr(s, f)) == r[f], \
                f"{_describe(p)}: {f}: device {int(getattr(s, f))}, oracle {r[f]}"
        hist = [int(x) for x in s.hist]
        for i in range(L.HIST_BINS):
            assert hist[i] == r["hist"][i], \
                f"{_describe(p)}: hist[{i}]: device {hist[i]}, oracle {r['hist'][i]}"
        assert s.status_other == 0, f"{_describe(p)}: status_other: device {s.status_other}"
        assert 0 <= s.status_tie <= r["status_tie"], \
            f"{_describe(p)}: status_tie: device {s.status_tie}, oracle {r['status_tie']}"
        assert 0 <= s.status_overlap <= s.episodes, _describe(p)


def _assert_cut(ms, shapes, resident1, full, namax):
    """Members launched one after the other ran as full lane-group launches first, the rest in
    groups of namax: the members of one launch report equal shares of one kernel's time, and
    a member left alone ran the one-point kernel (its resident lanes)."""
    m = len(ms)
    nfull = m // full * full
    for i in range(m):
        g0 = i - i % full if i < nfull else nfull + (i - nfull) // namax * namax
        size = full if i < nfull else min(namax, m - g0)
        assert ms[i] > 0
        assert ms[i] == ms[g0], (i, g0, ms)
        if size == 1:
            assert shapes[i][1] == resident1[i], (i, shapes[i], resident1[i])


def _assert_one_launch(ms, shapes, resident1):
    assert len(ms) >= 2 and len(set(ms)) == 1 and ms[0] > 0, ms
    assert len(set(shapes)) == 1, shapes


# ---- a. the bench's 20 points in its order, two rounds, one synchronize

def test_bench_order(torch, ctx):
    points = [dict(alpha=a, gamma=g, max_steps=BENCH_STEPS, seed=BENCH_SEED)
              for g in (0.0, 0.5) for a in BENCH_ALPHAS]
    n = 165  # gamma = 0: 32 episodes a wave, 5 waves and 5 lanes; gamma = .5: 16 a wave
    got, ref, ms, shapes, res1 = _sweep(torch, ctx, points, [(0, n), (n, n)])
    _assert_pinned(points, got, ref)
    assert all(s.episodes == 2 * n and s.steps == 2 * n * BENCH_STEPS for s in got)
    k = len(BENCH_ALPHAS)
    # gamma = 0: one launch of ten; gamma = .5: a launch of eight, then a launch of two
    _assert_cut(ms[:k], shapes[:k], res1[:k], FULL0, NAMAX)
    _assert_cut(ms[k:], shapes[k:], res1[k:], FULL5, NAMAX_ARR)
    assert k == FULL0 and k == FULL5 + NAMAX_ARR  # else this case no longer is what it says
    _assert_one_launch(ms[:k], shapes[:k], res1[:k])
    _assert_one_launch(ms[k:k + FULL5], shapes[k:k + FULL5], res1[k:k + FULL5])
    _assert_one_launch(ms[k + FULL5:], shapes[k + FULL5:], res1[k + FULL5:])


# ---- b. cuts: one member more and one fewer than a full lane-group launch

@pytest.mark.parametrize("gamma, extra", [(0.0, 1), (0.0, -1), (0.5, 1), (0.5, -1)])
def test_cuts(torch, ctx, gamma, extra):
    full, namax, _ = SHAPE[gamma]
    m = full + extra
    points = _points(_cycle(ALPHAS, m), gamma=gamma, max_steps=300, seed=SEED)
    got, ref, ms, shapes, res1 = _sweep(torch, ctx, points, [(0, N)])
    _assert_pinned(points, got, ref)
    assert all(s.episodes == N for s in got)
    _assert_cut(ms, shapes, res1, full, namax)
    if extra > 0:
        # a full launch, and the member past it alone in the one-point kernel
        _assert_one_launch(ms[:full], shapes[:full], res1[:full])
        assert shapes[full][1] == res1[full] and shapes[full] != shapes[0]
    else:
        assert len(set(ms[:namax])) == 1  # one lane's points a launch


# ---- c. the built-in policies

@pytest.mark.parametrize("policy", list(POLICIES))
def test_policies(torch, ctx, policy):
    for gamma in (0.0, 0.5):
        full, namax, _ = SHAPE[gamma]
        points = _points(_cycle(ALPHAS, 10), gamma=gamma, policy=POLICIES[policy], max_steps=300,
                         seed=SEED)
        got, ref, ms, shapes, res1 = _sweep(torch, ctx, points, [(0, N)])
        _assert_pinned(points, got, ref)
        _assert_cut(ms, shapes, res1, full, namax)
        _assert_one_launch(ms[:full], shapes[:full], res1[:full])


# ---- d. the longest episodes either kind of group takes

TO_95 = (.05, .15, .25, .33, .40, .45, .50, .60, .80, .95)
TO_45 = (.05, .10, .15, .20, .25, .30, .33, .35, .40, .45)
# (gamma = 0 SM1 at alpha >= .5 over 16384 steps is left out: the oracle needs 23 to 35 s for
# 32 to 64 such episodes. Honest play at alpha .95 reaches the packed tip word's greatest
# heights and attacker counts all the same.)
LONGEST = [("honest", 0.0, 16384, TO_95), ("sm1", 0.0, 16384, TO_45),
           ("honest", 0.5, 4094, TO_95), ("sm1", 0.5, 4094, TO_95)]


@pytest.mark.parametrize("policy, gamma, max_steps, alphas", LONGEST,
                         ids=[f"{p}-g{g}-{s}" for p, g, s, _ in LONGEST])
def test_longest_episodes(torch, ctx, policy, gamma, max_steps, alphas):
    full, namax, _ = SHAPE[gamma]
    points = _points(alphas, gamma=gamma, policy=POLICIES[policy], max_steps=max_steps, seed=SEED)
    n = 48  # gamma = 0: a full wave of 32 and 16 lanes; gamma = .5: three waves of 16
    got, ref, ms, shapes, res1 = _sweep(torch, ctx, points, [(0, n)])
    _assert_pinned(points, got, ref)
    assert all(s.episodes == n and s.steps == n * max_steps for s in got)
    _assert_cut(ms, shapes, res1, full, namax)
    _assert_one_launch(ms[:full], shapes[:full], res1[:full])
    if policy == "honest" and gamma == 0.0:
        # heights beyond 13 bits of the packed word
        assert max(r["max_height"] for r in ref) > 1 << 13


# ---- e. exact re-runs of flagged episodes, under each member's own launch

@pytest.mark.parametrize("gamma, members, cap",
                         [(0.0, FULL0, None), (0.5, FULL5, None), (0.0, 2, 4), (0.5, 2, 4)])
def test_exact_reruns(torch, ctx, gamma, members, cap):
    # a 1e-3 delay: overlaps, each re-run exactly; with a re-run queue of four entries the
    # rest waits in each point's own overflow flags
    points = _points(_cycle(ALPHAS[1:], members), gamma=gamma, propagation_delay=1e-3,
                     max_steps=300, seed=SEED)
    n = 2048
    r0 = ctx.rerun_stats()[0]
    got, ref, ms, shapes, res1 = _sweep(torch, ctx, points, [(0, n)],
                                        env=dict(CPR_RERUN_QUEUE_CAP=cap))
    r1 = ctx.rerun_stats()[0]
    _assert_pinned(points, got, ref)
    assert r1 > r0
    assert all(s.status_overlap > (cap or 0) and s.episodes == n for s in got)
    _assert_one_launch(ms, shapes, res1)


# ---- f. ties, and three groups' second passes through the context's two list buffers

def test_ties_and_list_buffer_rotation(torch, ctx):
    points = _points(_cycle((.25, .30, .35, .40, .45), FULL5), gamma=0.5, propagation_delay=1e-10,
                     max_steps=BENCH_STEPS, seed=SEED)
    n = 229  # 16 episodes a wave: 14 waves and 5 lanes
    got, ref, ms, shapes, res1 = _sweep(torch, ctx, points, [(0, n), (n, n), (2 * n, n)])
    _assert_pinned(points, got, ref)
    assert all(s.episodes == 3 * n for s in got)
    assert sum(r["status_tie"] for r in ref) > 0
    assert sum(s.status_tie for s in got) > 0
    _assert_one_launch(ms, shapes, res1)


# ---- g. the work queue hands every episode out exactly once

@pytest.mark.parametrize("gamma", [0.0, 0.5])
def test_work_queue(torch, ctx, gamma):
    full, namax, g = SHAPE[gamma]
    alphas = _cycle(ALPHAS, full)
    # the lane-group kernel's resident lanes, from a launch of the same shape
    probe = _sweep(torch, ctx, _points(alphas, gamma=gamma, max_steps=16, seed=SEED), [(0, N)])
    resident = probe[3][0][1]
    _assert_pinned(_points(alphas, gamma=gamma, max_steps=16, seed=SEED), probe[0], probe[1])
    # twice what the launch starts with, three further waves and a partial one
    n = 2 * resident // g + 64 * 3 + 37
    points = _points(alphas, gamma=gamma, max_steps=16, seed=SEED)
    got, ref, ms, shapes, res1 = _sweep(torch, ctx, points, [(0, n)])
    _assert_pinned(points, got, ref)
    assert all(s.episodes == n and s.activations == 17 * n for s in got)
    _assert_one_launch(ms, shapes, res1)
    assert shapes[0][0] // g < n  # more episodes than the launch has lanes for


# ---- h. the high words of seed and episode number

@pytest.mark.parametrize("gamma", [0.0, 0.5])
def test_high_words_of_seed_and_episode(torch, ctx, gamma):
    full, namax, _ = SHAPE[gamma]
    points = _points(_cycle(ALPHAS, full), gamma=gamma, max_steps=300, seed=2**63 + 7)
    got, ref, ms, shapes, res1 = _sweep(torch, ctx, points, [(2**40 + 3, N)])
    _assert_pinned(points, got, ref)
    assert all(s.episodes == N for s in got)
    _assert_one_launch(ms, shapes, res1)
    # other episodes than those of the low words alone
    low = _sweep(torch, ctx, [dict(points[0], seed=7)], [(3, N)])
    _assert_pinned([dict(points[0], seed=7)], low[0], low[1])
    assert low[1][0]["rel_revenue_fx"] != ref[0]["rel_revenue_fx"]


# ---- i. the bench's --full column: abstract gamma = 1 through run_async, never fused

def test_abstract_gamma_1(torch, ctx):
    points = _points(BENCH_ALPHAS, gamma=1.0, network=L.NET_ABSTRACT_GAMMA, defenders=2,
                     max_steps=BENCH_STEPS, seed=BENCH_SEED)
    n = 165
    got, ref, ms, shapes, res1 = _sweep(torch, ctx, points, [(0, n)])
    _assert_pinned(points, got, ref)
    assert all(s.episodes == n and s.steps == n * BENCH_STEPS for s in got)
    # every call a launch of its own, in the one-point kernel
    assert all(x > 0 for x in ms) and len(set(ms)) > 1, ms
    assert all(sh[1] == r for sh, r in zip(shapes, res1)), (shapes, res1)
