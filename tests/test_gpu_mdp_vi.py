"""Value iteration on the device (cpr_mdp_value_iteration, kernels_mdp.hip) —
needs an MI355X. Every result is compared with cpr_amd.mdp.value_iteration on the same packed
MDP and must equal it in all five fields, value and progress bit for bit, on the resident path
(one workgroup per point, vectors in LDS) and on the global path (one launch per sweep)."""

import ctypes
import json
import pathlib

import numpy as np
import pytest

from cpr_amd import _lib as L
from cpr_amd import device, mdp

pytestmark = pytest.mark.gpu

PATHS = ["resident", "global"]
GRID_ALPHAS, GRID_GAMMAS = (0.1, 0.33, 0.45), (0.0, 0.5, 1.0)
GOLDEN = json.loads((pathlib.Path(__file__).parent / "golden" / "mdp_fc16_vi.json")
                    .read_text())["cases"]


@pytest.fixture(scope="module")
def ctx():
    return device.default_context()


def ssz(alpha, gamma, mfl, horizon):
    _states, tab = mdp.compile_mdp(mdp.BitcoinSM(alpha, gamma, mfl))
    return mdp.pack(mdp.ptmdp(tab, horizon))


def same(dev, host, path=None):
    """All five fields, value and progress by their bytes."""
    assert dev["vi_iter"] == host["vi_iter"]
    assert dev["vi_delta"] == host["vi_delta"]
    assert dev["vi_policy"].tolist() == host["vi_policy"].tolist()
    assert dev["vi_value"].tobytes() == host["vi_value"].tobytes()
    assert dev["vi_progress"].tobytes() == host["vi_progress"].tobytes()
    if path is not None:
        assert dev["vi_path"] == path


_host = {}


def host_solve(key, m, **kw):
    """The host solve of a case, computed once and shared by the paths."""
    if key not in _host:
        _host[key] = mdp.value_iteration(m, **kw)
    return _host[key]


@pytest.mark.parametrize("path", PATHS)
def test_single_point(ctx, path):
    m = ssz(0.33, 0.5, 4, 10)
    assert m["dst"].shape[0] == 40  # 39 states and the terminal one
    host = host_solve("single", m, stop_delta=1e-6)
    assert host["vi_iter"] == 147
    dev = mdp.value_iteration_device(m, stop_delta=1e-6, path=path, ctx=ctx)
    same(dev, host, path)
    assert dev["vi_status"] == L.MDP_VI_CONVERGED


@pytest.fixture(scope="module")
def grid():
    ms = [ssz(a, g, 8, 20) for a in GRID_ALPHAS for g in GRID_GAMMAS]
    hosts = [mdp.value_iteration(m, stop_delta=1e-6) for m in ms]
    return ms, hosts


@pytest.mark.parametrize("path", PATHS)
def test_grid_points_stop_independently(ctx, grid, path):
    ms, hosts = grid
    assert len(ms) == 9 and ms[0]["dst"].shape[0] == 158
    iters = [h["vi_iter"] for h in hosts]
    assert min(iters) == 225 and max(iters) == 437 and len(set(iters)) > 4
    devs = mdp.value_iteration_device(ms, stop_delta=1e-6, path=path, ctx=ctx)
    assert len(devs) == 9
    for dev, host in zip(devs, hosts):
        same(dev, host, path)
        assert dev["vi_status"] == L.MDP_VI_CONVERGED


@pytest.mark.parametrize("path", PATHS)
def test_more_sweeps_than_one_bounded_launch(ctx, path):
    # 992 states: not a multiple of 64, the last wave partly idle, one state per thread (1,024
    # threads); ~1,750 sweeps: two bounded launches of the resident kernel (1,024 sweeps each),
    # the vectors carried through global memory between them
    m = ssz(0.33, 0.5, 20, 100)
    assert m["dst"].shape[0] == 992
    host = host_solve("mfl20", m, stop_delta=1e-6)
    assert host["vi_iter"] > 1024
    same(mdp.value_iteration_device(m, stop_delta=1e-6, path=path, ctx=ctx), host, path)


# More states than threads: the resident workgroup has at most 1,024 threads, thread tid owns
# the states tid, tid + 1,024, ... and the kernel is instantiated for 1, 2, 4 and 10 states per
# thread. One case per instantiation above 1, each with a last round that only some threads
# take part in (S no multiple of 1,024, the larger two no multiple of 64 either).
def _many_states(name):
    if name == "ssz-cutoff-40":  # 3,982 states: 4 per thread
        return ssz(0.33, 0.5, 40, 100), dict(stop_delta=1e-6, max_iter=12)
    S = {"random-1500": 1500, "random-9999": 9999}[name]  # 2 and 10 per thread
    return random_mdp(S, 3, 4, seed=S), dict(stop_delta=1e-6, max_iter=6, discount=0.95)


@pytest.mark.parametrize("name,per_thread", [("random-1500", 2), ("ssz-cutoff-40", 4),
                                             ("random-9999", 10)])
def test_more_states_than_threads(ctx, name, per_thread):
    m, kw = _many_states(name)
    S = m["dst"].shape[0]
    assert -(-S // 1024) > 1 and S % 1024 != 0
    assert min(p for p in (1, 2, 4, 10) if p * 1024 >= S) == per_thread
    host = mdp.value_iteration(m, **kw)
    assert host["vi_iter"] == kw["max_iter"] and host["vi_delta"] > 0
    for path in PATHS:
        same(mdp.value_iteration_device(m, path=path, ctx=ctx, **kw), host, path)
    # two points in one launch: the second workgroup reads its own probabilities
    other = dict(m, prb=np.where(m["used"], m["prb"] * 0.75, m["prb"]))
    host2 = mdp.value_iteration(other, **kw)
    devs = mdp.value_iteration_device([m, other], path="resident", ctx=ctx, **kw)
    same(devs[0], host, "resident")
    same(devs[1], host2, "resident")


@pytest.mark.parametrize("path", PATHS)
def test_options(ctx, path):
    m = ssz(0.33, 0.5, 4, 10)
    host = host_solve("max_iter", m, stop_delta=0.0, max_iter=7)
    assert host["vi_iter"] == 7
    dev = mdp.value_iteration_device(m, stop_delta=0.0, max_iter=7, path=path, ctx=ctx)
    same(dev, host, path)
    assert dev["vi_status"] == L.MDP_VI_MAX_ITER
    host = host_solve("discount", m, stop_delta=1e-9, discount=0.9)
    assert host["vi_iter"] == 94
    same(mdp.value_iteration_device(m, stop_delta=1e-9, discount=0.9, path=path, ctx=ctx), host,
         path)


def hand_made():
    """Four states, A = 3, T = 2. State 0: two actions of bit-equal value (the first is kept;
    the third is worse). State 1: one action of negative value (taken: none was taken yet).
    State 2: no action. State 3: one action back to state 0; its padding slot and the invalid
    actions' slots carry garbage with used = 0."""
    S, A, T = 4, 3, 2
    dst = np.zeros((S, A, T), np.int64)
    prb = np.zeros((S, A, T))
    rew = np.zeros((S, A, T))
    prg = np.zeros((S, A, T))
    used = np.zeros((S, A, T), bool)
    valid = np.zeros((S, A), bool)

    def put(s, a, t, d, p, r, g):
        dst[s, a, t], prb[s, a, t], rew[s, a, t], prg[s, a, t], used[s, a, t] = d, p, r, g, True
        valid[s, a] = True

    put(0, 0, 0, 1, 0.5, 1.0, 1.0)
    put(0, 0, 1, 2, 0.5, 3.0, 0.0)
    put(0, 1, 0, 1, 0.5, 1.0, 2.0)  # the same value as action 0, another progress
    put(0, 1, 1, 2, 0.5, 3.0, 0.0)
    put(0, 2, 0, 2, 1.0, 0.25, 0.0)
    put(1, 0, 0, 2, 1.0, -2.0, 1.0)
    put(3, 0, 0, 0, 0.75, 0.5, 1.0)
    for s, a, t in [(3, 0, 1), (1, 1, 0), (2, 0, 0), (2, 2, 1)]:
        dst[s, a, t], prb[s, a, t], rew[s, a, t], prg[s, a, t] = 10 ** 6, 1e300, np.inf, np.nan
    dst[1, 2, 1] = -7
    return dict(dst=dst, prb=prb, rew=rew, prg=prg, used=used, valid=valid)


@pytest.mark.parametrize("path", PATHS)
def test_hand_made_mdps(ctx, path):
    m = hand_made()
    with np.errstate(all="ignore"):
        host = mdp.value_iteration(m, stop_delta=1e-12, discount=0.5)
    assert host["vi_policy"].tolist() == [0, 0, -1, 0]
    assert host["vi_value"][1] == -2.0 and host["vi_value"][2] == 0.0
    same(mdp.value_iteration_device(m, stop_delta=1e-12, discount=0.5, path=path, ctx=ctx), host,
         path)
    # T = A = 1: a two-state chain into a state without action
    one = dict(dst=np.array([[[1]], [[0]]]), prb=np.array([[[0.5]], [[0.0]]]),
               rew=np.array([[[2.0]], [[0.0]]]), prg=np.array([[[1.0]], [[0.0]]]),
               used=np.array([[[True]], [[False]]]), valid=np.array([[True], [False]]))
    host = mdp.value_iteration(one, stop_delta=1e-9)
    assert host["vi_policy"].tolist() == [0, -1] and host["vi_value"].tolist() == [1.0, 0.0]
    same(mdp.value_iteration_device(one, stop_delta=1e-9, path=path, ctx=ctx), host, path)


def random_mdp(S, A, T, seed):
    rng = np.random.default_rng(seed)
    used = rng.random((S, A, T)) < 0.8
    valid = rng.random((S, A)) < 0.9
    prb = rng.random((S, A, T))
    prb /= np.maximum((prb * used).sum(axis=2, keepdims=True), 1e-9)
    return dict(dst=rng.integers(0, S, (S, A, T)), prb=prb, rew=rng.random((S, A, T)) * 4 - 1,
                prg=rng.random((S, A, T)), used=used, valid=valid)


def test_auto_path_and_the_guard(ctx):
    small = ssz(0.33, 0.5, 4, 10)
    assert mdp.value_iteration_device(small, stop_delta=1e-6, ctx=ctx)["vi_path"] == "resident"
    # 20,000 states need 320,000 bytes for value and progress: more than a CU's LDS
    m = random_mdp(20_000, 3, 4, seed=0x4D4450)
    host = mdp.value_iteration(m, stop_delta=1e-6, max_iter=5)
    dev = mdp.value_iteration_device(m, stop_delta=1e-6, max_iter=5, ctx=ctx)
    same(dev, host, "global")
    with pytest.raises(L.CprError) as e:
        mdp.value_iteration_device(m, stop_delta=1e-6, max_iter=5, path="resident", ctx=ctx)
    assert e.value.code == L.CPR_E_CAPACITY


@pytest.mark.parametrize("path", PATHS)
def test_the_cap_ends_a_solve_that_cannot_converge(ctx, path, monkeypatch):
    # a two-state cycle with reward 1 and discount 1 grows for ever. The library's cap of 2^20
    # sweeps takes more than a second to reach, so the launcher's cap is lowered for this call
    # (CPR_MDP_VI_SWEEP_CAP): 2,500 sweeps are three launches of the resident kernel
    monkeypatch.setenv("CPR_MDP_VI_SWEEP_CAP", "2500")
    cycle = dict(dst=np.array([[[1]], [[0]]]), prb=np.ones((2, 1, 1)), rew=np.ones((2, 1, 1)),
                 prg=np.ones((2, 1, 1)), used=np.ones((2, 1, 1), bool),
                 valid=np.ones((2, 1), bool))
    # a second point that converges at once keeps its own status
    still = dict(cycle, prb=np.zeros((2, 1, 1)))
    devs = mdp.value_iteration_device([cycle, still], stop_delta=1e-6, path=path, ctx=ctx)
    assert devs[0]["vi_status"] == L.MDP_VI_NOT_CONVERGED
    assert devs[0]["vi_iter"] == 2500 and devs[0]["vi_delta"] == 1.0
    assert devs[0]["vi_value"].tolist() == [2500.0, 2500.0]
    assert devs[1]["vi_status"] == L.MDP_VI_CONVERGED and devs[1]["vi_iter"] == 1
    host = mdp.value_iteration(cycle, stop_delta=1e-6, max_iter=2500)
    same(devs[0], host)


@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: f"a{c['alpha']:.3f}-g{c['gamma']}")
def test_goldens(ctx, case):
    m = ssz(case["alpha"], case["gamma"], case["maximum_fork_length"], case["horizon"])
    for path in PATHS:
        vi = mdp.value_iteration_device(m, stop_delta=case["stop_delta"], path=path, ctx=ctx)
        assert vi["vi_iter"] == case["vi_iter"]
        assert vi["vi_policy"].tolist() == case["vi_policy"]
        assert vi["vi_value"].tolist() == case["vi_value"]  # bit for bit


def test_grid_tables_and_solve_grid(ctx, grid):
    _ms, hosts = grid
    kw = dict(maximum_fork_length=8, horizon=20)
    solved = mdp.solve_grid(GRID_ALPHAS, GRID_GAMMAS, ctx=ctx, **kw)
    pts = [(a, g) for a in GRID_ALPHAS for g in GRID_GAMMAS]
    for (model, states, vi), (a, g), host in zip(solved, pts, hosts):
        assert (model.alpha, model.gamma) == (a, g)
        assert states == mdp.compile_mdp(mdp.BitcoinSM(a, g, 8))[0]
        same(vi, host)
    tables = mdp.policy_table_grid(GRID_ALPHAS, GRID_GAMMAS, ctx=ctx, **kw)
    fc16 = mdp.fc16_table_grid(GRID_ALPHAS, GRID_GAMMAS, ctx=ctx, **kw)
    for (a, g), t, f in zip(pts, tables, fc16):
        assert t.tolist() == mdp.policy_table(a, g, **kw).tolist()
        assert f.tolist() == mdp.fc16_table(a, g, **kw).tolist()
    assert mdp.policy_table(0.33, 0.5, device=True, **kw).tolist() == tables[4].tolist()
    _model, _states, vi = mdp.solve(0.33, 0.5, device=True, **kw)
    same(vi, hosts[4])


def _call(ctx, m, prb=None, **opts):
    o = dict(stop_delta=1e-6, discount=1.0, max_iter=0, path="auto")
    o.update(opts)
    return ctx.mdp_value_iteration(m["dst"], m["used"], m["valid"], m["rew"], m["prg"],
                                   m["prb"] if prb is None else prb, **o)


def test_validation(ctx):
    m = ssz(0.33, 0.5, 4, 10)
    slot = tuple(np.argwhere(m["used"])[3])
    pad = tuple(np.argwhere(~m["used"])[0])

    def bad(code=L.CPR_E_INVALID_ARG, **kw):
        with pytest.raises(L.CprError) as e:
            _call(ctx, kw.pop("m", m), **kw)
        assert e.value.code == code and str(e.value)

    bad(discount=0.0)
    bad(discount=1.5)
    bad(discount=float("nan"))
    bad(stop_delta=-1e-9)
    bad(stop_delta=0.0, max_iter=0)
    bad(max_iter=-1)
    for key, value in [("dst", 40), ("dst", -1), ("rew", np.inf), ("prg", np.nan),
                       ("prb", -np.inf)]:
        arr = m[key].copy()
        arr[slot] = value
        bad(m=dict(m, **{key: arr}))
        # the same garbage in a padding slot is ignored
        arr = m[key].copy()
        arr[pad] = value
        _call(ctx, dict(m, **{key: arr}))
    # a dst that a cast to int32 would wrap into [0, S) is refused like any other
    arr = m["dst"].copy()
    arr[slot] = 2 ** 32 + 3
    bad(m=dict(m, dst=arr))
    # a non-finite probability in the second point only
    prb = np.stack([m["prb"], m["prb"]])
    prb[1][slot] = np.nan
    bad(prb=prb)
    # sizes < 1 and an unknown path, through the C ABI
    lib = L.lib()
    opts = L.MdpViOptsC()
    L.check(lib.cpr_mdp_vi_opts_default(ctypes.byref(opts)))
    assert (opts.stop_delta, opts.discount, opts.max_iter, opts.path) == (1e-6, 1.0, 0, 0)
    a = {k: np.ascontiguousarray(m[k], dt) for k, dt in
         [("dst", np.int32), ("used", np.uint8), ("valid", np.uint8), ("rew", np.float64),
          ("prg", np.float64), ("prb", np.float64)]}
    S, A, T = a["dst"].shape
    out = [np.zeros(S), np.zeros(S), np.zeros(S, np.int32), np.zeros(1, np.int64), np.zeros(1),
           np.zeros(1, np.int32)]
    res = L.MdpViResultC(*(x.ctypes.data for x in out))

    def rc(sizes, path=0, mdp_ok=True):
        c = L.MdpC(*sizes, *(a[k].ctypes.data for k in ("dst", "used", "valid", "rew", "prg", "prb")))
        opts.path = path
        return lib.cpr_mdp_value_iteration(ctx.handle, ctypes.byref(c) if mdp_ok else None,
                                           ctypes.byref(opts), ctypes.byref(res))

    assert rc((S, A, T, 1)) == L.CPR_OK and out[3][0] == 147
    for sizes in [(0, A, T, 1), (S, 0, T, 1), (S, A, 0, 1), (S, A, T, 0), (-1, A, T, 1)]:
        assert rc(sizes) == L.CPR_E_INVALID_ARG
        assert lib.cpr_last_error()
    assert rc((S, A, T, 1), path=3) == L.CPR_E_INVALID_ARG
    assert rc((S, A, T, 1), mdp_ok=False) == L.CPR_E_INVALID_ARG
