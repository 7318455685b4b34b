"""Lane groups of k_run_episodes_fused: a sweep group spread over adjacent lanes.

A pending group of cpr_run_episodes_async grows to (points per lane) x (lanes per episode)
members and is cut into full lane-group launches first, then into the one-lane groups of
test_gpu_fused_points.py (capi.hip fuse_launch_pending; nak_fused.h "lane groups"). The
pattern is that file's: every case runs the same calls grouped (the default) and with
CPR_NAK_FUSE=0 (every call launches at once, the one-point kernel), and compares every
Summary.FIELDS word and the histogram of every point.
"""

import ctypes
import os

import pytest

from cpr_amd import _lib as L
from cpr_amd import device

pytestmark = pytest.mark.gpu

NAMAX = L.NAK_FUSE_MAX
NAMAX_ARR = L.NAK_FUSE_MAX_ARR  # gamma = .5
G0 = L.NAK_FUSE_LANES           # lanes per episode, gamma = 0
G5 = L.NAK_FUSE_LANES_ARR       # gamma = .5
FULL0 = NAMAX * G0              # a full lane-group launch: 10 members
FULL5 = NAMAX_ARR * G5          # 8 members
ALPHAS = (.05, .25, .35, .45, .5, .10, .15, .20, .30, .40, .33)
SEED = 0x1A9E5
N = 64 * 5 + 37  # no multiple of 16 or 32
WORDS = ctypes.sizeof(L.Summary) // 8


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


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
UNFUSED = dict(CPR_NAK_FUSE=0, CPR_NAK_FUSE_LANES=None)


def _batch(ctx, alpha, gamma=0.0, max_steps=300, seed=SEED, **kw):
    cfg, keep = device.make_config(alpha=alpha, gamma=gamma, max_steps=max_steps, seed=seed, **kw)
    return device.Batch(cfg, ctx=ctx, keep=keep)


def _batches(ctx, m, **kw):
    return [_batch(ctx, ALPHAS[i % len(ALPHAS)], **kw) for i in range(m)]


def _close(batches):
    for b in batches:
        b.close()


def _zeros(torch, k):
    return [torch.zeros(WORDS, dtype=torch.int64, device="cuda") for _ in range(k)]


def _read(sums):
    return [L.Summary.from_buffer_copy(s.cpu().numpy().tobytes()) for s in sums]


def _assert_equal(got, ref, what=""):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        for f in L.Summary.FIELDS:
            assert getattr(a, f) == getattr(b, f), (what, i, f, getattr(a, f), getattr(b, f))
        assert list(a.hist) == list(b.hist), (what, i, "hist")


def _sweep(torch, ctx, batches, n, first=0):
    """One asynchronous call per batch, then the synchronize that completes the summaries."""
    sums = _zeros(torch, len(batches))
    for b, s in zip(batches, sums):
        b.run_async(n, first, s.data_ptr())
    ctx.synchronize()
    return _read(sums)


def _both(torch, ctx, batches, n, first=0):
    with Env(**GROUPED):
        got = _sweep(torch, ctx, batches, n, first)
    with Env(**UNFUSED):
        ref = _sweep(torch, ctx, batches, n, first)
    _assert_equal(got, ref)
    return got


@pytest.fixture(scope="module")
def ctx(torch):
    c = device.Context(0)
    yield c
    c.close()


def _assert_cut(batches, ms, full, namax):
    """Members launched one after the other ran as full lane-group launches first, the rest in
    groups of namax: the members of one launch report equal shares of one kernel's time."""
    m = len(batches)
    nfull = m // full * full
    for i in range(m):
        g0 = i - i % full if i < nfull else nfull + (i - nfull) // namax * namax
        assert ms[i] == ms[g0], (i, g0, ms)
        assert ms[i] > 0


@pytest.mark.parametrize("max_steps", [299, 300])
@pytest.mark.parametrize("m", [FULL0, FULL0 + 1, FULL0 - 1])
def test_gamma0_members(torch, ctx, m, max_steps):
    batches = _batches(ctx, m, max_steps=max_steps)
    with Env(**GROUPED):
        got = _sweep(torch, ctx, batches, N)
        ms = [b.last_launch()[0] for b in batches]
    _assert_cut(batches, ms, FULL0, NAMAX)
    if m >= FULL0:
        assert len(set(ms[:FULL0])) == 1  # one launch for the full shape
    with Env(**UNFUSED):
        ref = _sweep(torch, ctx, batches, N)
    _assert_equal(got, ref)
    assert all(s.episodes == N and s.steps == N * max_steps for s in got)
    _close(batches)


@pytest.mark.parametrize("max_steps", [299, 300])
@pytest.mark.parametrize("m", [FULL5, FULL5 + 2, FULL5 // 2, FULL5 + 1])
def test_gamma05_members(torch, ctx, m, max_steps):
    batches = _batches(ctx, m, gamma=0.5, max_steps=max_steps)
    with Env(**GROUPED):
        got = _sweep(torch, ctx, batches, N)
        ms = [b.last_launch()[0] for b in batches]
    _assert_cut(batches, ms, FULL5, NAMAX_ARR)
    if m >= FULL5:
        assert len(set(ms[:FULL5])) == 1
    with Env(**UNFUSED):
        ref = _sweep(torch, ctx, batches, N)
    _assert_equal(got, ref)
    assert all(s.episodes == N and s.steps == N * max_steps for s in got)
    _close(batches)


@pytest.mark.parametrize("gamma, m", [(0.0, FULL0), (0.5, FULL5)])
@pytest.mark.parametrize("max_steps", [299, 300])
def test_fewer_episodes_than_a_wave(torch, ctx, gamma, m, max_steps):
    batches = _batches(ctx, m, gamma=gamma, max_steps=max_steps)
    got = _both(torch, ctx, batches, 5)
    assert all(s.episodes == 5 for s in got)
    _close(batches)


@pytest.mark.parametrize("max_steps", [299, 300])
@pytest.mark.parametrize("pol", [L.POLICY_HONEST, L.POLICY_SIMPLE, L.POLICY_EYAL_SIRER_2014,
                                 L.POLICY_SAPIRSHTEIN_2016_SM1])
def test_policies(torch, ctx, pol, max_steps):
    for gamma in (0.0, 0.5):
        batches = _batches(ctx, 10, gamma=gamma, policy=pol, max_steps=max_steps)
        got = _both(torch, ctx, batches, N)
        assert all(s.episodes == N for s in got)
        _close(batches)


@pytest.mark.parametrize("gamma, m, g", [(0.0, FULL0, G0), (0.5, FULL5, G5)])
def test_work_queue(torch, ctx, gamma, m, g):
    # waves take further episodes from the queue, 64 / G at a time; the last is partly filled
    batches = _batches(ctx, m, gamma=gamma, max_steps=16)
    with Env(**GROUPED):
        _sweep(torch, ctx, batches, N)  # the lane-group kernel's resident lanes
        resident = batches[0].launch_shape()[1]
    n = 2 * resident // g + 64 * 3 + 37
    got = _both(torch, ctx, batches, n)
    assert all(s.episodes == n and s.activations == 17 * n for s in got)
    _close(batches)


@pytest.mark.parametrize("max_steps", [299, 300])
@pytest.mark.parametrize("cap", [None, 4])
@pytest.mark.parametrize("gamma, m", [(0.0, 10), (0.5, 8)])
def test_reruns(torch, ctx, gamma, m, cap, max_steps):
    # flagged episodes go to the exact re-run under their own point's launch; with a re-run
    # queue of four entries the rest waits in each point's own overflow flags
    batches = _batches(ctx, m, gamma=gamma, propagation_delay=1e-3, max_steps=max_steps)
    n = 1024
    try:
        with Env(CPR_RERUN_QUEUE_CAP=cap, **GROUPED):
            r0 = ctx.rerun_stats()[0]
            got = _sweep(torch, ctx, batches, n)
            r1 = ctx.rerun_stats()[0]
        with Env(CPR_RERUN_QUEUE_CAP=cap, **UNFUSED):
            ref = _sweep(torch, ctx, batches, n)
            r2 = ctx.rerun_stats()[0]
    finally:
        ctx.synchronize()
    _assert_equal(got, ref)
    assert all(s.status_overlap > 0 and s.episodes == n for s in got)
    assert r1 - r0 == r2 - r1 > 0
    _close(batches)


def test_tie_heavy_group(torch, ctx):
    # the configuration of test_deferred_races_tie_heavy (test_gpu_parity.py) as an
    # eight-point lane group: a 1e-10 delay over 2016-step episodes makes same-instant ties
    # common, so every member lists many episodes for its eager second pass
    n = 4096 + 37
    batches = _batches(ctx, 8, gamma=0.5, max_steps=2016, propagation_delay=1e-10, seed=0x7E5)
    got = _both(torch, ctx, batches, n)
    assert all(s.episodes == n for s in got)
    assert got[0].status_tie > n // 50
    _assert_equal(got[:1], [batches[0].run(n, records=True)[0]], "records")
    _close(batches)


@pytest.mark.parametrize("max_steps", [299, 300])
def test_bench_order(torch, ctx, max_steps):
    # the bench's order: ten gamma = 0 calls, then ten gamma = .5 calls, twice, one synchronize
    batches = _batches(ctx, 10, max_steps=max_steps) + \
        _batches(ctx, 10, gamma=0.5, max_steps=max_steps)

    def script():
        sums = _zeros(torch, len(batches))
        for first in (0, 5000):
            for b, s in zip(batches, sums):
                b.run_async(N, first, s.data_ptr())
        ctx.synchronize()
        return _read(sums)
    with Env(**GROUPED):
        got = script()
        ms = [b.last_launch()[0] for b in batches]
    with Env(**UNFUSED):
        ref = script()
    _assert_equal(got, ref)
    assert all(s.episodes == 2 * N and s.steps == 2 * N * max_steps for s in got)
    # one launch per full shape
    assert len(set(ms[:10])) == 1
    assert len(set(ms[10:18])) == 1 and ms[18] == ms[19]
    _close(batches)


@pytest.mark.parametrize("max_steps", [299, 300])
@pytest.mark.parametrize("kind", ["seed", "second_context"])
def test_group_break_in_the_middle(torch, ctx, kind, max_steps):
    # six members of a ten-point group pending, then a call that must launch them first
    ctx2 = device.Context(0)

    def script():
        head = _batches(ctx, 6, max_steps=max_steps)
        extra = dict(seed=SEED + 1) if kind == "seed" else {}
        tail = [_batch(ctx2 if kind == "second_context" else ctx, a, max_steps=max_steps, **extra)
                for a in ALPHAS[6:10]]
        sums = _zeros(torch, 10)
        for b, s in zip(head + tail, sums):
            b.run_async(N, 0, s.data_ptr())
        ctx.synchronize()
        ctx2.synchronize()
        out = _read(sums)
        _close(head + tail)
        return out
    with Env(**GROUPED):
        got = script()
    with Env(**UNFUSED):
        ref = script()
    ctx2.close()
    _assert_equal(got, ref, kind)
    assert all(s.episodes == N and s.steps == N * max_steps for s in got)


@pytest.mark.parametrize("max_steps", [299, 300])
def test_lanes_1_is_the_one_lane_grouping(torch, ctx, max_steps):
    # CPR_NAK_FUSE_LANES=1: groups of NAMAX, launched when full, in the five-point kernel
    five = _batches(ctx, NAMAX, max_steps=max_steps)
    with Env(**GROUPED):
        _sweep(torch, ctx, five, N)
        shape5 = five[0].launch_shape()
    batches = _batches(ctx, 10, max_steps=max_steps)
    with Env(CPR_NAK_FUSE=None, CPR_NAK_FUSE_LANES=1):
        got = _sweep(torch, ctx, batches, N)
        ms = [b.last_launch()[0] for b in batches]
        shapes = [b.launch_shape() for b in batches]
    assert len(set(ms[:NAMAX])) == 1 and len(set(ms[NAMAX:])) == 1
    assert all(s == shape5 for s in shapes)
    with Env(**GROUPED):
        _sweep(torch, ctx, batches, N)
        assert batches[0].launch_shape() != shape5  # the lane-group kernel's
    with Env(**UNFUSED):
        ref = _sweep(torch, ctx, batches, N)
    _assert_equal(got, ref)
    _close(five + batches)
