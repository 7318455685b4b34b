"""k_run_episodes_fused over packed tips (nakamoto_lane.h PTip: a tip's height and attacker
count in one word) against the one-point kernels, which keep whole BRef tips.

Every case runs the same calls grouped (the default: the fused kernels) and with
CPR_NAK_FUSE=0 (every call launches at once, the one-point kernel; read at every call), and
compares every Summary.FIELDS word and the histogram of every point, among them the tie and
overlap counts, and the exact re-runs each side made.
"""

import ctypes
import os

import pytest

from cpr_amd import _lib as L
from cpr_amd import device

pytestmark = pytest.mark.gpu

SEED = 0x9AC7ED
WORDS = ctypes.sizeof(L.Summary) // 8
TEN = (.05, .10, .15, .20, .25, .30, .35, .40, .45, .50)
LONG = (.05, .15, .25, .33, .40, .45, .50, .60, .80, .95)
POLICIES = [L.POLICY_HONEST, L.POLICY_SIMPLE, L.POLICY_EYAL_SIRER_2014,
            L.POLICY_SAPIRSHTEIN_2016_SM1]


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
    """Environment variables for the calls inside; None unsets."""

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


def _sweep(torch, ctx, batches, n):
    sums = [torch.zeros(WORDS, dtype=torch.int64, device="cuda") for _ in batches]
    for b, s in zip(batches, sums):
        b.run_async(n, 0, s.data_ptr())
    ctx.synchronize()
    return [L.Summary.from_buffer_copy(s.cpu().numpy().tobytes()) for s in sums]


def _both(torch, ctx, alphas, n, **kw):
    """The points of one sweep group fused and one by one: equal summaries and re-runs."""
    batches = []
    for a in alphas:
        cfg, keep = device.make_config(alpha=a, seed=SEED, **kw)
        batches.append(device.Batch(cfg, ctx=ctx, keep=keep))
    try:
        with Env(CPR_NAK_FUSE=None, CPR_NAK_FUSE_LANES=None):
            r0 = ctx.rerun_stats()[0]
            got = _sweep(torch, ctx, batches, n)
            ms = [b.last_launch()[0] for b in batches]
            r1 = ctx.rerun_stats()[0]
        with Env(CPR_NAK_FUSE=0, CPR_NAK_FUSE_LANES=None):
            ref = _sweep(torch, ctx, batches, n)
            r2 = ctx.rerun_stats()[0]
    finally:
        ctx.synchronize()
        for b in batches:
            b.close()
    for i, (a, b) in enumerate(zip(got, ref)):
        for f in L.Summary.FIELDS:
            assert getattr(a, f) == getattr(b, f), (i, f, getattr(a, f), getattr(b, f))
        assert list(a.hist) == list(b.hist), (i, "hist")
    assert r1 - r0 == r2 - r1
    assert all(s.episodes == n for s in got)
    return got, ms


def _assert_launches(ms, gamma):
    # gamma = 0: one launch of five points x two lanes; gamma = .5: two points x four lanes,
    # then the two left over (members of one launch report equal shares of its time)
    full = L.NAK_FUSE_MAX * L.NAK_FUSE_LANES if gamma == 0.0 else \
        L.NAK_FUSE_MAX_ARR * L.NAK_FUSE_LANES_ARR
    assert all(m > 0 for m in ms)
    assert len(set(ms[:full])) == 1
    if full < len(ms):
        assert len(set(ms[full:])) == 1 and ms[full] != ms[0]


@pytest.mark.parametrize("gamma", [0.0, 0.5])
def test_ten_alphas(torch, ctx, gamma):
    # 1,000 episodes: no multiple of 64 / G, the last wave partly empty
    got, ms = _both(torch, ctx, TEN, 1000, gamma=gamma, max_steps=300)
    _assert_launches(ms, gamma)
    assert all(s.steps == 1000 * 300 for s in got)
    if gamma == 0.5:
        assert sum(s.status_tie for s in got) > 0


@pytest.mark.parametrize("gamma", [0.0, 0.5])
def test_longest_episodes(torch, ctx, gamma):
    # max_steps = 2^14, the largest the lazy clock admits: heights pass 2^8 and approach 2^14
    # in both halves of a tip's word (alpha = .95: nearly every block the attacker's)
    got, ms = _both(torch, ctx, LONG, 256, gamma=gamma, max_steps=16384)
    # gamma = .5: the deferred races keep release indices in 12 bits of a list entry, so the
    # library fuses such points only up to a private-chain capacity of 4096 (max_steps <=
    # 4094, run_episodes_fusable); at 16384 steps every point launches alone and only the
    # summaries are compared. test_longest_fused_episodes_gamma05 is the fused kernel's limit
    if gamma == 0.0:
        _assert_launches(ms, gamma)
    assert all(s.steps == 256 * 16384 and s.activations == 256 * 16385 for s in got)


def test_longest_fused_episodes_gamma05(torch, ctx):
    # max_steps = 4094, the largest at which gamma = .5 points run in the fused kernel
    got, ms = _both(torch, ctx, LONG, 256, gamma=0.5, max_steps=4094)
    _assert_launches(ms, 0.5)
    assert all(s.steps == 256 * 4094 and s.activations == 256 * 4095 for s in got)


@pytest.mark.parametrize("pol", POLICIES)
def test_policies(torch, ctx, pol):
    for gamma in (0.0, 0.5):
        _both(torch, ctx, TEN, 1000, gamma=gamma, max_steps=300, policy=pol)
