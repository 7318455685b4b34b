"""k_run_episodes_fused with the trimmed step (the policy as flags, one released tip per step,
no capacity test: nakamoto_lane.h policy_flags, apply_flags, LaneMem::cap_test) against the
one-point kernels, which keep the action code, form every chain block where it is used and
test the private chain's capacity at every activation.

Every case runs the same calls grouped (the default: the fused kernels) and with
CPR_NAK_FUSE=0 (every call launches at once, the one-point kernel; read at every call), and
compares every Summary.FIELDS word and the 64 histogram bins of every point, and the exact
re-runs each side made. max_steps = 62 gives a private-chain capacity of exactly
max_steps + 2 = 64 (no rounding slack); alpha = .95 grows the private chain nearly every
activation. Every case asserts from the library's group sizes that the three shipped shapes
ran: five points x two lanes (gamma = 0), two points x four lanes and the two points left
over (gamma = .5).
"""

import ctypes
import os

import pytest

from cpr_amd import _lib as L
from cpr_amd import device

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000
N = 512
WORDS = ctypes.sizeof(L.Summary) // 8
TEN = (.05, .10, .15, .20, .25, .30, .35, .40, .45, .50)
WITH_95 = (.05, .15, .25, .33, .40, .45, .50, .60, .80, .95)
POLICIES = [L.POLICY_HONEST, L.POLICY_SIMPLE, L.POLICY_EYAL_SIRER_2014,
            L.POLICY_SAPIRSHTEIN_2016_SM1]
FULL = {0.0: L.NAK_FUSE_MAX * L.NAK_FUSE_LANES, 0.5: L.NAK_FUSE_MAX_ARR * L.NAK_FUSE_LANES_ARR}


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


def _both(torch, ctx, alphas, gamma, **kw):
    """The points of one sweep group fused and one by one: equal summaries and re-runs, and
    the fused side cut into the shipped shapes."""
    batches = []
    for a in alphas:
        cfg, keep = device.make_config(alpha=a, gamma=gamma, seed=SEED, **kw)
        batches.append(device.Batch(cfg, ctx=ctx, keep=keep))
    try:
        resident1 = [b.launch_shape()[1] for b in batches]  # the one-point kernel's
        with Env(CPR_NAK_FUSE=None, CPR_NAK_FUSE_LANES=None):
            r0 = ctx.rerun_stats()[0]
            got = _sweep(torch, ctx, batches, N)
            ms = [b.last_launch()[0] for b in batches]
            shapes = [b.launch_shape() for b in batches]
            r1 = ctx.rerun_stats()[0]
        with Env(CPR_NAK_FUSE=0, CPR_NAK_FUSE_LANES=None):
            ref = _sweep(torch, ctx, batches, N)
            shapes1 = [b.launch_shape() for b in batches]
            r2 = ctx.rerun_stats()[0]
    finally:
        ctx.synchronize()
        for b in batches:
            b.close()
    for i, (a, b) in enumerate(zip(got, ref)):
        for f in L.Summary.FIELDS:
            assert getattr(a, f) == getattr(b, f), (i, f, getattr(a, f), getattr(b, f))
        assert len(a.hist) == 64 and list(a.hist) == list(b.hist), (i, "hist")
    assert r1 - r0 == r2 - r1
    assert all(s.episodes == N for s in got)
    # the shapes: the members of one launch report equal shares of one kernel's time and one
    # launch shape. gamma = 0: ten points in one launch (5 x 2); gamma = .5: eight (2 x 4),
    # then the two left over in a launch of their own (2 x 1)
    full = FULL[gamma]
    assert len(alphas) == 10 and full == (10 if gamma == 0.0 else 8)
    assert (L.NAK_FUSE_MAX, L.NAK_FUSE_LANES) == (5, 2)
    assert (L.NAK_FUSE_MAX_ARR, L.NAK_FUSE_LANES_ARR) == (2, 4)
    assert all(m > 0 for m in ms)
    assert len(set(ms[:full])) == 1 and len(set(shapes[:full])) == 1, (ms, shapes)
    if full < len(ms):
        assert len(set(ms[full:])) == 1 and ms[full] != ms[0], ms
        assert len(set(shapes[full:])) == 1 and shapes[full] != shapes[0], shapes
    # and the other side ran the one-point kernel (its resident lanes), every call alone
    assert all(sh[1] == r for sh, r in zip(shapes1, resident1)), (shapes1, resident1)
    return got


@pytest.mark.parametrize("max_steps", [62, 300])
@pytest.mark.parametrize("gamma", [0.0, 0.5])
def test_ten_alphas(torch, ctx, gamma, max_steps):
    got = _both(torch, ctx, TEN, gamma, max_steps=max_steps)
    assert all(s.steps == N * max_steps and s.activations == N * (max_steps + 1) for s in got)
    assert all(s.status_other == 0 for s in got)


@pytest.mark.parametrize("max_steps", [62, 300])
@pytest.mark.parametrize("gamma", [0.0, 0.5])
def test_group_with_alpha_95(torch, ctx, gamma, max_steps):
    got = _both(torch, ctx, WITH_95, gamma, max_steps=max_steps)
    assert all(s.steps == N * max_steps for s in got)
    assert all(s.status_other == 0 for s in got)


@pytest.mark.parametrize("pol", POLICIES)
def test_policies(torch, ctx, pol):
    for gamma in (0.0, 0.5):
        for max_steps in (62, 300):
            _both(torch, ctx, TEN, gamma, max_steps=max_steps, policy=pol)
