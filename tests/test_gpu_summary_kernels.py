"""The summary-only Nakamoto kernels (the bench's two launches) beside the record kernel and
the oracle.

b.run(n) without records takes the timed path: k_run_episodes with the lazy clock, at
gamma = 0 the d = 2 specialisation (32-bit miner draw, defender index by a shift, 32-bit
masks, the high-word skip test) or its general-d fallback, at gamma = .5 the deferred races
with the eager second pass. b.run(n, records=True) runs the general record kernel, whose
records must equal the oracle's episode for episode; every summary field and the histogram
of the two device runs must be equal. So a summary-only kernel that decides a miner, a skip
or a mask differently shows up against the oracle's episodes, summed.
"""

import numpy as np
import pytest

import oracle_py as O
from cpr_amd import _lib as L
from cpr_amd import device

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000
FIELDS = [f for f in L.RECORD_DTYPE.names if f not in ("status",)]


@pytest.fixture(scope="module")
def ctx():
    return device.default_context()


def _records_equal(a, b):
    bad = {}
    for f in FIELDS:
        neq = np.nonzero(a[f] != b[f])[0]
        if len(neq):
            bad[f] = (int(neq[0]), a[f][neq[0]], b[f][neq[0]], len(neq))
    return bad


def _check(ctx, n, first=0, **kw):
    cfg, keep = device.make_config(seed=SEED, **kw)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    s0 = b.run(n, first_episode=first)
    s1, rec = b.run(n, first_episode=first, records=True)
    ref = O.run_episodes(cfg, first, n, threads=8)
    assert _records_equal(rec, ref) == {}
    for f in L.Summary.FIELDS:
        assert getattr(s0, f) == getattr(s1, f), f
    assert list(s0.hist) == list(s1.hist)
    assert s0.episodes == n
    return s0


@pytest.mark.parametrize("gamma", [0.0, 0.5])
@pytest.mark.parametrize("alpha", [0.05, 0.45])
def test_bench_shape_partial_last_wave(ctx, gamma, alpha):
    # the bench's episode length; five waves and 37 lanes of a sixth
    _check(ctx, 64 * 5 + 37, alpha=alpha, gamma=gamma, max_steps=2016)


LONG = [
    dict(alpha=0.45, gamma=0.0),
    dict(alpha=0.45, gamma=0.5),
    dict(alpha=0.05, gamma=0.0, policy=L.POLICY_HONEST),
    dict(alpha=0.05, gamma=0.5, policy=L.POLICY_HONEST),
]


@pytest.mark.parametrize("steps", [16384, 16385])
@pytest.mark.parametrize("kw", LONG, ids=lambda k: f"a{k['alpha']}-g{k['gamma']}-p{k.get('policy', 3)}")
def test_longest_lazy_episode_and_one_past_it(ctx, kw, steps):
    # 2^14 steps is the longest episode the lazy clock takes (lazy_clock_ok); at 2^14 + 1
    # the eager kernels run. Both sides of the limit must agree with the oracle. (Honest
    # play at alpha = .05 reaches the greatest heights, SM1 at .45 the greatest forks.)
    _check(ctx, 128, max_steps=steps, **kw)


@pytest.mark.parametrize("defenders", [2, 3, 5])
def test_gamma0_defender_counts(ctx, defenders):
    # d = 2: the specialised kernel (defender index w1 >> 31); d = 3, 5: its fallback (one
    # 32-bit multiply-high); the head's tie-break reads the miner's index
    _check(ctx, 512, alpha=0.33, gamma=0.0, defenders=defenders, max_steps=300)


@pytest.mark.parametrize("gamma", [0.0, 0.5])
def test_long_delay_overlaps(ctx, gamma):
    # a 1e-3 delay sends ~2.5e-3 of the activations down the skip test's exact branch, which
    # must find the real overlaps (each re-run exactly)
    s = _check(ctx, 2048, alpha=0.33, gamma=gamma, max_steps=300, propagation_delay=1e-3)
    assert s.status_overlap > 0
