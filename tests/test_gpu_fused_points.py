"""Sweep points that share their draws, run in one k_run_episodes_fused lane.

cpr_run_episodes_async defers the d = 2, built-in-policy summary launches of the two timed
kernels (gamma = 0; gamma = .5 with deferred races) and runs those that share seed, first
episode and episode count as one group (capi.hip fuse_launch_pending,
kernels_nak_fused.hip). Every case runs the same calls twice, grouped (the default) and with
CPR_NAK_FUSE=0 (every call launches at once, the one-point kernel), and compares every
Summary.FIELDS word and the histogram of every point.
"""

import ctypes
import os

import numpy as np
import pytest

from cpr_amd import _lib as L
from cpr_amd import device

pytestmark = pytest.mark.gpu

NAMAX = L.NAK_FUSE_MAX
NAMAX_ARR = L.NAK_FUSE_MAX_ARR  # gamma = .5
ALPHAS = (.05, .25, .35, .45, .5, .10)
SEED = 0xF05ED
N = 64 * 5 + 37
WORDS = ctypes.sizeof(L.Summary) // 8


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


class Env:
    """CPR_NAK_FUSE for the calls inside (the library reads it at every call)."""

    def __init__(self, fuse):
        self.fuse = fuse

    def __enter__(self):
        self.old = os.environ.get("CPR_NAK_FUSE")
        if self.fuse is None:
            os.environ.pop("CPR_NAK_FUSE", None)
        else:
            os.environ["CPR_NAK_FUSE"] = str(self.fuse)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("CPR_NAK_FUSE", None)
        else:
            os.environ["CPR_NAK_FUSE"] = self.old


def _batch(ctx, alpha, gamma=0.0, max_steps=300, seed=SEED, **kw):
    cfg, keep = device.make_config(alpha=alpha, gamma=gamma, max_steps=max_steps, seed=seed, **kw)
    return device.Batch(cfg, ctx=ctx, keep=keep)


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
    with Env(None):
        got = _sweep(torch, ctx, batches, n, first)
    with Env(0):
        ref = _sweep(torch, ctx, batches, n, first)
    _assert_equal(got, ref)
    return got


@pytest.fixture(scope="module")
def ctx(torch):
    c = device.Context(0)
    yield c
    c.close()


def _assert_grouping(batches, resident1, namax, ms):
    """Batches launched one after the other ran in groups of namax, the rest in one more:
    a group of two or more runs the fused kernel, whose resident lanes (launch_shape) differ
    from the one-point kernel's, and its members report equal shares of one kernel's time.
    This also holds the library's largest group to the bindings' constant."""
    m = len(batches)
    for i, b in enumerate(batches):
        g0 = i - i % namax
        size = min(namax, m - g0)
        assert (b.launch_shape()[1] != resident1) == (size >= 2), (i, size, b.launch_shape())
        assert ms[i] == ms[g0]


@pytest.mark.parametrize("m", range(1, NAMAX + 2))
def test_group_sizes(torch, ctx, m):
    # partial groups, a full group, and the split after a full group
    batches = [_batch(ctx, ALPHAS[i % len(ALPHAS)]) for i in range(m)]
    resident1 = batches[0].launch_shape()[1]  # before any launch: the one-point kernel's
    with Env(None):
        got = _sweep(torch, ctx, batches, N)
        ms = [b.last_launch()[0] for b in batches]
    assert all(x > 0 for x in ms)
    _assert_grouping(batches, resident1, NAMAX, ms)
    with Env(0):
        ref = _sweep(torch, ctx, batches, N)
        assert all(b.last_launch()[0] > 0 for b in batches)
    _assert_equal(got, ref)
    for s in got:
        assert s.episodes == N
    if m == NAMAX + 1:
        # the record kernel's summary: one more device-to-device link (its records are what
        # the parity tests compare with the oracle, its summary is reduced on the device).
        # The fused path's own pin to the oracle is tests/test_gpu_sweep_oracle.py
        _assert_equal(got, [b.run(N, records=True)[0] for b in batches], "records")
    for b in batches:
        b.close()


def test_policies(torch, ctx):
    k = min(3, NAMAX)
    for pol in (L.POLICY_HONEST, L.POLICY_SIMPLE, L.POLICY_EYAL_SIRER_2014,
                L.POLICY_SAPIRSHTEIN_2016_SM1):
        batches = [_batch(ctx, a, policy=pol) for a in ALPHAS[1:1 + k]]
        got = _both(torch, ctx, batches, N)
        assert all(s.episodes == N for s in got)
        for b in batches:
            b.close()


@pytest.mark.parametrize("max_steps", [16384, 16385])
def test_lazy_clock_limit(torch, ctx, max_steps):
    # 16384: the longest episode the lazy clock takes (the fused path); 16385: not fusable
    batches = [_batch(ctx, a, max_steps=max_steps) for a in (.25, .45)]
    n = 96
    resident1 = batches[0].launch_shape()[1]  # the one-point kernel's
    with Env(None):
        got = _sweep(torch, ctx, batches, n)
    # the fused kernel holds fewer lanes than the one-point kernel
    for b in batches:
        assert (b.launch_shape()[1] != resident1) == (max_steps == 16384)
    with Env(0):
        ref = _sweep(torch, ctx, batches, n)
    _assert_equal(got, ref)
    assert all(s.episodes == n and s.steps == n * max_steps for s in got)
    for b in batches:
        b.close()


def test_work_queue(torch, ctx):
    # waves take further episodes from the queue; the last wave is partly filled
    batches = [_batch(ctx, a, max_steps=16) for a in (.10, .35, .5)[:min(3, NAMAX)]]
    n = 2 * batches[0].launch_shape()[1] + 64 * 3 + 37
    got = _both(torch, ctx, batches, n)
    assert all(s.episodes == n and s.activations == n * 17 for s in got)
    for b in batches:
        b.close()


def test_reruns(torch, ctx):
    # flagged episodes go to the exact re-run under their own point's launch
    batches = [_batch(ctx, a, propagation_delay=1e-3) for a in ALPHAS[1:1 + NAMAX]]
    n = 2048
    with Env(None):
        r0 = ctx.rerun_stats()[0]
        got = _sweep(torch, ctx, batches, n)
        r1 = ctx.rerun_stats()[0]
    with Env(0):
        ref = _sweep(torch, ctx, batches, n)
        r2 = ctx.rerun_stats()[0]
    _assert_equal(got, ref)
    assert all(s.status_overlap > 0 and s.episodes == n for s in got)
    assert r1 - r0 == r2 - r1 > 0
    for b in batches:
        b.close()


def test_reruns_through_overflow_flags(torch, ctx):
    # a re-run queue of four entries: the rest waits in each point's own overflow flags
    batches = [_batch(ctx, a, propagation_delay=1e-3) for a in (.25, .45)]
    old = os.environ.get("CPR_RERUN_QUEUE_CAP")
    os.environ["CPR_RERUN_QUEUE_CAP"] = "4"
    try:
        got = _both(torch, ctx, batches, 1024)
    finally:
        if old is None:
            os.environ.pop("CPR_RERUN_QUEUE_CAP")
        else:
            os.environ["CPR_RERUN_QUEUE_CAP"] = old
        ctx.synchronize()
    assert all(s.status_overlap > 4 and s.episodes == 1024 for s in got)
    for b in batches:
        b.close()


BREAKS = ["first", "n", "seed", "gamma", "records", "policy", "defenders", "last_launch",
          "sync_run", "close_sibling", "second_context"]


def _break_script(torch, ctx, ctx2, kind):
    """A pending group of two, then a call that must launch it first. Every summary."""
    a, b = _batch(ctx, .25), _batch(ctx, .35)
    extra = {"seed": dict(seed=SEED + 1), "gamma": dict(gamma=0.5),
             "policy": dict(policy=L.POLICY_EYAL_SIRER_2014),
             "defenders": dict(defenders=3)}.get(kind, {})
    c = _batch(ctx2 if kind == "second_context" else ctx, .45, **extra)
    sib = _batch(ctx, .10)
    sums = _zeros(torch, 3)
    host = []
    rec = None
    a.run_async(N, 0, sums[0].data_ptr())
    b.run_async(N, 0, sums[1].data_ptr())
    n3, first3 = N, 0
    if kind == "first":
        first3 = 1000
    elif kind == "n":
        n3 = N + 64
    elif kind == "records":
        rec = torch.zeros(N * L.RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    elif kind == "last_launch":
        assert a.last_launch()[0] > 0
    elif kind == "sync_run":
        host.append(sib.run(N))
    elif kind == "close_sibling":
        sib.close()
    c.run_async(n3, first3, sums[2].data_ptr(), rec.data_ptr() if rec is not None else None)
    ctx.synchronize()
    ctx2.synchronize()
    out = _read(sums) + host
    assert [s.episodes for s in out[:3]] == [N, N, n3]  # nothing lost, nothing counted twice
    for x in (a, b, c, sib):
        x.close()
    return out


@pytest.mark.parametrize("kind", BREAKS)
def test_group_breaks(torch, ctx, kind):
    ctx2 = device.Context(0)
    with Env(None):
        got = _break_script(torch, ctx, ctx2, kind)
    with Env(0):
        ref = _break_script(torch, ctx, ctx2, kind)
    ctx2.close()
    _assert_equal(got, ref, kind)


def test_same_point_twice(torch, ctx):
    b = _batch(ctx, .35)
    got = _both(torch, ctx, [b, b], N)
    _assert_equal(got[:1], got[1:])
    assert got[0].episodes == N
    b.close()


# ---- gamma = .5: the deferred-race kernel's groups (second-pass lists per member)

@pytest.mark.parametrize("m", range(1, NAMAX_ARR + 2))
def test_group_sizes_gamma05(torch, ctx, m):
    batches = [_batch(ctx, ALPHAS[i % len(ALPHAS)], gamma=0.5) for i in range(m)]
    resident1 = batches[0].launch_shape()[1]
    with Env(None):
        got = _sweep(torch, ctx, batches, N)
        ms = [b.last_launch()[0] for b in batches]
    assert all(x > 0 for x in ms)
    _assert_grouping(batches, resident1, NAMAX_ARR, ms)
    with Env(0):
        ref = _sweep(torch, ctx, batches, N)
    _assert_equal(got, ref)
    assert all(s.episodes == N for s in got)
    if m == NAMAX_ARR + 1:
        _assert_equal(got, [b.run(N, records=True)[0] for b in batches], "records")
    for b in batches:
        b.close()


def test_reruns_gamma05(torch, ctx):
    # overlaps (hybrid exact re-runs under each point's own launch) beside listed races
    batches = [_batch(ctx, a, gamma=0.5, propagation_delay=1e-3)
               for a in ALPHAS[1:1 + NAMAX_ARR]]
    n = 2048
    with Env(None):
        r0 = ctx.rerun_stats()[0]
        got = _sweep(torch, ctx, batches, n)
        r1 = ctx.rerun_stats()[0]
    with Env(0):
        ref = _sweep(torch, ctx, batches, n)
        r2 = ctx.rerun_stats()[0]
    _assert_equal(got, ref)
    assert all(s.status_overlap > 0 and s.episodes == n for s in got)
    assert r1 - r0 == r2 - r1 > 0
    for b in batches:
        b.close()


@pytest.mark.parametrize("n", [16384 + 37])
def test_tie_heavy_group(torch, ctx, n):
    # the configuration of test_deferred_races_tie_heavy (test_gpu_parity.py), as a group: a
    # 1e-10 delay over 2016-step episodes makes same-instant ties common, so every member
    # lists many episodes for its eager second pass; n is no multiple of 64
    batches = [_batch(ctx, a, gamma=0.5, max_steps=2016, propagation_delay=1e-10, seed=0x7E5)
               for a in (.4, .25, .45)[:min(3, NAMAX_ARR)]]
    got = _both(torch, ctx, batches, n)
    assert all(s.episodes == n for s in got)
    assert got[0].status_tie > n // 50
    _assert_equal(got[:1], [batches[0].run(n, records=True)[0]], "records")
    for b in batches:
        b.close()


def test_gamma0_and_gamma05_groups_alternate(torch, ctx):
    # the bench's order: a gamma = 0 sweep, then a gamma = .5 sweep, twice, one synchronize
    k0, k5 = min(3, NAMAX), min(3, NAMAX_ARR)
    batches = [_batch(ctx, a) for a in ALPHAS[:k0]] + \
              [_batch(ctx, a, gamma=0.5) for a in ALPHAS[:k5]]

    def script():
        sums = _zeros(torch, len(batches))
        for first in (0, 5000):
            for b, s in zip(batches, sums):
                b.run_async(N, first, s.data_ptr())
        ctx.synchronize()
        return _read(sums)
    with Env(None):
        got = script()
    with Env(0):
        ref = script()
    _assert_equal(got, ref)
    assert all(s.episodes == 2 * N for s in got)
    for b in batches:
        b.close()
