"""The learner on the device (cpr_gae, cpr_ppo_*; DESIGN.md §4.14 "Learner") — needs an MI355X.

1. GAE bit for bit against ppo_ref.gae_ref, host and device pointers;
2. the minibatch gradient against torch's float64 autograd: per parameter tensor the device's
   relative L2 error may be at most 8x the error of torch's own float32 CPU autograd on the
   same inputs (the device sums rows in MFMA k-chains and block partials, not in torch's
   order, and rounds dlogits and the saved activations to f32 once more);
3. two calls return identical bytes;
4. the norm clip and Adam against torch, given the device's gradient;
5. minibatching: an update equals hand-driven single-minibatch updates; keyed permutations;
6. ppo_iterate equals rollout_net -> gae -> ppo_update composed by hand;
7. refusals.

Measured gradient errors (worst device / torch-f32 ratio per network) are in
profiles/ppo_grad_error.json: 3.9x at the worst of 780 tensors.

The loss statistics are compared with rtol 1e-5 against float64. That proved too tight for
approx_kl alone (3x256, B = 1: (rho - 1) - log rho = 1.9e-4 at |log rho| = 0.02 loses four
digits of the f32 logits; device 2.3e-9 off, torch-f32 2.8e-8 off), so a statistic may
instead be within 8x the error of the torch-f32 statistic, the gradient's measure.
"""

import ctypes
import json
import os

import numpy as np
import pytest
import torch

import ppo_ref
from cpr_amd import _lib as L
from cpr_amd import device
from cpr_amd import ppo as P

pytestmark = pytest.mark.gpu

PROTO = {
    "nakamoto": dict(protocol=L.PROTO_NAKAMOTO),
    "bk": dict(protocol=L.PROTO_BK, k=2),
    "bk4": dict(protocol=L.PROTO_BK, k=4),
    "ethereum": dict(protocol=L.PROTO_ETHEREUM, reward_scheme=L.REWARD_DISCOUNT),
}


@pytest.fixture(scope="module")
def ctx():
    return device.default_context()


def _batch(ctx, proto, **kw):
    cfg, keep = device.make_config(**dict(PROTO[proto], **kw))
    return device.Batch(cfg, ctx=ctx, keep=keep)


def float_net(seed, n_in, depth, wpi, wvf, n_act, extra=()):
    """Gaussian weights scaled 1/sqrt(fan_in): asymmetric, so an operand or C-write swap shows."""
    rng = np.random.default_rng(seed)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    def trunk(w):
        return [lin(w, n_in if i == 0 else w) for i in range(depth)]

    return device.PolicyNet(pi=trunk(wpi), pi_head=lin(n_act, wpi), vf=trunk(wvf),
                            vf_head=lin(1, wvf), extra=extra)


def net_for(b, seed, depth, wpi, wvf, extra=()):
    ol, na = b.observation_spec()[:2]
    return float_net(seed, ol + len(extra), depth, wpi, wvf, na, extra)


def forward_with_bound(net, obs):
    """(logits, value, logits bound, value bound) in float64: the reference forward on the
    f32-rounded inputs and, per output, the standard f32 dot-product bound propagated through
    the layers: err_out <= |W| err_in + gamma_{K+1} (|W| (|x| + err_in) + |b|), gamma_k =
    k 2^-24 / (1 - k 2^-24); ReLU is 1-Lipschitz."""
    u = 2.0 ** -24
    x = np.asarray(obs, dtype=np.float64).astype(np.float32).astype(np.float64)
    x = np.concatenate([x, np.tile(np.float32(net.extra).astype(np.float64), (len(x), 1))], axis=1)
    outs = []
    for trunk, head in ((net.pi, net.pi_head), (net.vf, net.vf_head)):
        h, e = x, np.zeros_like(x)
        layers = [(w, b, True) for w, b in trunk] + [(head[0], head[1], False)]
        for w, b, relu in layers:
            W, B = w.astype(np.float64), b.astype(np.float64)
            k = W.shape[1] + 1
            gam = k * u / (1 - k * u)
            y = h @ W.T + B
            e = e @ np.abs(W).T + gam * ((np.abs(h) + e) @ np.abs(W).T + np.abs(B))
            h = np.maximum(y, 0.0) if relu else y
        outs.append((h, e))
    return outs[0][0], outs[1][0][:, 0], outs[0][1], outs[1][1][:, 0]


def flat_rollout(b, n_steps):
    """A sampled network rollout as flat training rows: the policy input of row (t, lane) is
    obs0 for t = 0 and obs[t - 1] after; the same for the alphas."""
    s, a = b.rollout_net(n_steps, deterministic=False)
    n = b.n_lanes
    obs = np.concatenate([a["obs0"][None], a["obs"][:-1]]).reshape(n_steps * n, -1)
    out = dict(obs=obs, action=a["action"].ravel(), logp=a["logp"].ravel(), arrays=a, summary=s)
    if "alpha" in a:
        out["alpha"] = np.concatenate([a["alpha0"][None], a["alpha"][:-1]]).ravel()
    return out


def training_rows(b, n_steps, seed):
    """Rows of a short sampled rollout with random advantages of both signs, its returns, and
    old_logp perturbed so that rho stays inside the clip range for a third of the rows, leaves
    it above for a third and below for a third."""
    r = flat_rollout(b, n_steps)
    rng = np.random.default_rng(seed)
    n = r["action"].size
    grp = np.arange(n) % 3
    delta = np.where(grp == 0, rng.uniform(-0.02, 0.02, n),
                     np.where(grp == 1, 1.0, -1.0) * rng.uniform(0.15, 0.4, n))
    # the returns are the rollout's own (GAE of its rewards, dones and values): returns centred
    # on the values would make the value head's bias gradient, mean(v - R), a cancelling sum
    # whose relative error no f32 forward bounds
    a = r["arrays"]
    _, ret = b.gae(a["reward"], a["done"], a["value"], 0.99, 0.95)
    data = dict(obs=r["obs"], action=r["action"], old_logp=r["logp"] - delta,
                advantage=rng.standard_normal(n), ret=ret.ravel())
    if "alpha" in r:
        data["alpha"] = r["alpha"]
    return data


def take(data, rows):
    return {k: v[rows] for k, v in data.items()}


def identity(n, epochs=1):
    return np.tile(np.arange(n, dtype=np.int32), (epochs, 1))


def weights(b):
    return P.flatten_params(b.get_policy_net())


# ------------------------------------------------------------------ 1. GAE

@pytest.mark.parametrize("gl", [(0.99, 0.95), (1.0, 1.0)])
@pytest.mark.parametrize("n_lanes", [1, 70])
@pytest.mark.parametrize("n_steps", [1, 5])
def test_gae_bit_for_bit(ctx, n_steps, n_lanes, gl):
    b = _batch(ctx, "nakamoto", alpha=0.3, gamma=0.5, max_steps=16, seed=1, n_lanes=n_lanes)
    rng = np.random.default_rng(100 * n_steps + n_lanes)
    reward = rng.standard_normal((n_steps, n_lanes))
    value = rng.standard_normal((n_steps + 1, n_lanes))
    done = np.zeros((n_steps, n_lanes), dtype=np.uint8)
    done[0, 0::3] = 1            # the first step of some lanes
    done[-1, 1::3] = 1           # the last step of others
    if n_lanes > 2 and n_steps >= 3:
        done[1:3, 2] = 1         # two consecutive steps of one
    ref_adv, ref_ret = ppo_ref.gae_ref(reward, done, value, *gl)
    adv, ret = b.gae(reward, done, value, *gl)
    assert np.array_equal(adv, ref_adv) and np.array_equal(ret, ref_ret)
    dev = [torch.tensor(x, device="cuda") for x in (reward, done, value)]
    out = [torch.zeros((n_steps, n_lanes), dtype=torch.float64, device="cuda") for _ in range(2)]
    b.gae(*(t.data_ptr() for t in dev), *gl, device=True, n_steps=n_steps,
          out=(out[0].data_ptr(), out[1].data_ptr()))
    assert np.array_equal(out[0].cpu().numpy(), ref_adv)
    assert np.array_equal(out[1].cpu().numpy(), ref_ret)


# ------------------------------------------------------------------ 2. gradient

NETS = {"1x16": (1, 16, 16), "2x32-48": (2, 32, 48), "3x64": (3, 64, 64), "3x256": (3, 256, 256)}
# observation shapes: Ethereum has the 24-wide head and, with one extra, K = 11 (no multiple
# of 4); B_k runs with a lane env, so that the alpha column comes from the rows' alphas
SHAPES = {"nakamoto": dict(extra=(0.375, 0.7)), "bk": dict(extra=(0.375, 0.7), lane_env=True),
          "ethereum": dict(extra=(0.7,))}
ROWS = (1, 63, 65, 130, 257)
OPTS = P.PPOOptions(ent_coef=0.01)
GRAD_ERRORS = {}
GRAD_OVER = []


def rel_err(a, ref):
    """relative L2 error, absolute where the reference tensor vanishes"""
    n = np.linalg.norm(ref)
    return np.linalg.norm(a - ref) / (n if n >= 1e-30 else 1.0)


@pytest.mark.parametrize("proto", list(SHAPES))
@pytest.mark.parametrize("netname", list(NETS))
def test_gradient_against_float64_autograd(ctx, netname, proto):
    depth, wpi, wvf = NETS[netname]
    shape = SHAPES[proto]
    b = _batch(ctx, proto, alpha=0.35, gamma=0.5, max_steps=12, seed=23, n_lanes=70)
    col = None
    if shape.get("lane_env"):
        col = 0
        b.set_lane_env(alphas=[0.2, 0.3, 0.45], alpha_column=0)
    net = net_for(b, 7 + depth + wpi, depth, wpi, wvf, shape["extra"])
    b.set_policy_net(net)
    data = training_rows(b, 4, seed=31)
    N = data["action"].size
    assert N == 280
    perm = np.random.default_rng(5).permutation(N).astype(np.int32)
    sizes = [a.size for _, a in P.param_arrays(net)]
    names = [n for n, _ in P.param_arrays(net)]
    worst, over = 0.0, []
    for B in ROWS:
        rows = perm[:B]
        assert B == 1 or not np.array_equal(rows, np.sort(rows))  # a real gather
        d = take(data, rows)
        x = ppo_ref.net_input(net, d["obs"], d.get("alpha"), col)
        s64, g64, info = ppo_ref.ppo_loss(net, x, d["action"], d["old_logp"], d["advantage"],
                                          d["ret"], OPTS, torch.float64)
        s32, g32, _ = ppo_ref.ppo_loss(net, x, d["action"], d["old_logp"], d["advantage"],
                                       d["ret"], OPTS, torch.float32)
        # the inputs reach every branch (asserted on the reference, before the device)
        rho, A, c = info["rho"], info["adv"], OPTS.clip_range
        if B >= 63:
            for sa in (1, -1):
                assert np.any((sa * A > 0) & (rho > 1 + c)), (B, sa, "above")
                assert np.any((sa * A > 0) & (rho < 1 - c)), (B, sa, "below")
            assert np.any((rho > 1 - c) & (rho < 1 + c))
        for hs in info["hidden"]:
            for h in hs:
                assert np.any(h == 0.0) and np.any(h > 0.0)
        grad, st = b.ppo_gradients(data, rows, OPTS)
        assert grad.dtype == np.float32 and grad.size == g64.size == sum(sizes)
        o = 0
        for name, k in zip(names, sizes):
            ed = rel_err(grad[o:o + k].astype(np.float64), g64[o:o + k])
            et = rel_err(g32[o:o + k], g64[o:o + k])
            print(f"{proto} {netname} B {B} {name}: device {ed:.3e} torch-f32 {et:.3e} "
                  f"ratio {ed / et if et else float('inf') if ed else 0.0:.2f}")
            if et > 0:
                worst = max(worst, ed / et)
            if not ed <= 8 * et:  # every figure first; the assertion is at the end
                over.append(dict(case=f"{proto}/{netname}", rows=B, tensor=name, device=ed,
                                 torch_f32=et))
            o += k
        for key in ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction",
                    "loss", "grad_norm"):
            print(f"{proto} {netname} B {B} {key}: device {st[key]!r} f64 {s64[key]!r} "
                  f"torch-f32 {s32[key]!r}")
            # rtol 1e-5 against float64; where a statistic is too ill-conditioned in the f32
            # logits for that (approx_kl = (rho - 1) - log rho at |log rho| ~ 0.02 loses four
            # digits), the gradient's measure: at most 8x torch-f32's own error
            tol = max(1e-5 * abs(s64[key]), 8 * abs(s32[key] - s64[key]))
            assert abs(st[key] - s64[key]) <= tol, (B, key, st[key], s64[key], s32[key])
        assert st["n_minibatches"] == 1
    GRAD_ERRORS[f"{proto}/{netname}"] = worst
    GRAD_OVER.extend(over)
    out = os.environ.get("CPR_PPO_GRAD_ERROR_OUT")
    if out:  # the measurement behind profiles/ppo_grad_error.json
        with open(out, "w") as f:
            json.dump({"bound": 8.0, "rows": list(ROWS),
                       "worst_device_over_torch_f32": GRAD_ERRORS,
                       "above_bound": GRAD_OVER}, f, indent=1)
    assert not over, over


# ------------------------------------------------------------------ 3. reproducibility

def test_gradients_repeat_bit_for_bit(ctx):
    b = _batch(ctx, "ethereum", alpha=0.35, gamma=0.5, max_steps=12, seed=3, n_lanes=70)
    b.set_policy_net(net_for(b, 2, 3, 256, 256, (0.7,)))
    data = training_rows(b, 4, seed=9)
    rows = np.random.default_rng(1).permutation(280).astype(np.int32)[:257]
    g1, s1 = b.ppo_gradients(data, rows, OPTS)
    g2, s2 = b.ppo_gradients(data, rows, OPTS)
    assert g1.tobytes() == g2.tobytes() and np.any(g1 != 0)
    assert s1 == s2
    # a fresh batch as well: nothing depends on what the scratch held before
    b2 = _batch(ctx, "ethereum", alpha=0.35, gamma=0.5, max_steps=12, seed=3, n_lanes=70)
    b2.set_policy_net(net_for(b2, 2, 3, 256, 256, (0.7,)))
    g3, s3 = b2.ppo_gradients(data, rows, OPTS)
    assert g1.tobytes() == g3.tobytes() and s1 == s3


# ------------------------------------------------------------------ 4. clip and Adam

@pytest.mark.parametrize("max_norm", [0.01, 1e3])
def test_clip_and_adam_given_the_gradient(ctx, max_norm):
    b = _batch(ctx, "bk", alpha=0.35, gamma=0.5, max_steps=12, seed=4, n_lanes=70)
    net = net_for(b, 12, 2, 32, 48, (0.375, 0.7))
    b.set_policy_net(net)
    data = take(training_rows(b, 2, seed=13), np.arange(3, 67))
    opts = P.PPOOptions(n_epochs=1, minibatch=64, max_grad_norm=max_norm, ent_coef=0.01)
    shapes = [a.shape for _, a in P.param_arrays(net)]
    ref = ppo_ref.TorchAdam([a for _, a in P.param_arrays(net)], opts)
    assert np.array_equal(weights(b), P.flatten_params(net))  # get before any update
    for t in (1, 2):  # t = 2: non-zero m and v
        grad, st = b.ppo_gradients(data, np.arange(64), opts)
        assert (st["grad_norm"] > max_norm) == (max_norm < 1)
        ust = b.ppo_update(data, opts, perm=identity(64))
        assert ust["n_minibatches"] == 1
        assert ust["grad_norm"] == st["grad_norm"] and ust["loss"] == st["loss"]
        new, step = ref.step(list(P.unflatten_grads(net, grad).values()))
        got = P.unflatten_grads(net, weights(b))
        worst = 0.0
        for (name, w), want, s, shp in zip(got.items(), new, step, shapes):
            assert w.shape == shp
            tol = np.spacing(np.abs(want)).astype(np.float64) + 1e-6 * np.abs(s)
            diff = np.abs(w.astype(np.float64) - want.astype(np.float64))
            worst = max(worst, float(np.max(diff / tol)))
            assert np.all(diff <= tol), (t, name, float(np.max(diff / tol)))
            assert np.any(s != 0.0)
        print(f"max_norm {max_norm} t {t}: worst difference / tolerance {worst:.3f}")
        # torch continues from the device's weights (its m and v are its own)
        with torch.no_grad():
            for p, w in zip(ref.ps, got.values()):
                p.copy_(torch.tensor(w))


# ------------------------------------------------------------------ 5. minibatching

def _mb_batch(ctx, seed=6):
    b = _batch(ctx, "nakamoto", alpha=0.35, gamma=0.5, max_steps=12, seed=seed, n_lanes=70)
    b.set_policy_net(net_for(b, 21, 2, 32, 48, (0.375, 0.7)))
    return b


def test_update_equals_hand_driven_minibatches(ctx):
    b = _mb_batch(ctx)
    data = take(training_rows(b, 2, seed=17), np.arange(130))
    opts = P.PPOOptions(n_epochs=2, minibatch=64, ent_coef=0.01, lr=1e-3)
    rng = np.random.default_rng(8)
    perm = np.stack([rng.permutation(130), rng.permutation(130)]).astype(np.int32)
    st = b.ppo_update(data, opts, perm=perm)
    assert st["n_minibatches"] == 6
    twin = _mb_batch(ctx)
    assert np.array_equal(weights(twin), P.flatten_params(twin._net))
    sums = dict.fromkeys(st, 0.0)
    sizes = []
    for e in range(2):
        for s0 in range(0, 130, 64):
            rows = perm[e, s0:s0 + 64]
            sizes.append(len(rows))
            one = P.PPOOptions(n_epochs=1, minibatch=len(rows), ent_coef=0.01, lr=1e-3)
            s1 = twin.ppo_update(take(data, rows), one, perm=identity(len(rows)))
            for k in sums:
                sums[k] += s1[k]
    assert sizes == [64, 64, 2, 64, 64, 2]
    assert weights(b).tobytes() == weights(twin).tobytes()
    assert np.any(weights(b) != P.flatten_params(b._net))
    for k in ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "loss",
              "grad_norm"):
        assert st[k] == pytest.approx(sums[k] / 6, rel=1e-14, abs=1e-300)


def test_keyed_permutations(ctx):
    data = take(training_rows(_mb_batch(ctx), 2, seed=17), np.arange(130))
    got = []
    for perm_seed in (0, 0, 1):
        b = _mb_batch(ctx)  # fresh: the update count of its draws starts at 0
        opts = P.PPOOptions(n_epochs=2, minibatch=64, ent_coef=0.01, lr=1e-3, perm_seed=perm_seed)
        assert b.ppo_update(data, opts)["n_minibatches"] == 6
        got.append(weights(b))
    assert got[0].tobytes() == got[1].tobytes()
    assert got[0].tobytes() != got[2].tobytes()


# ------------------------------------------------------------------ 6. composition

@pytest.mark.parametrize("proto", ["nakamoto", "bk4"])
def test_iterate_equals_the_three_calls(ctx, proto):
    def make():
        b = _batch(ctx, proto, alpha=0.35, gamma=0.5, max_steps=6, seed=41, n_lanes=70)
        b.set_lane_env(alphas=[0.2, 0.3, 0.45], alpha_column=0, reward="sparse_relative",
                       shape="per_alpha")
        b.set_policy_net(net_for(b, 33, 2, 32, 32, (0.375, 0.7)))
        return b

    opts = P.PPOOptions(n_epochs=2, minibatch=100, ent_coef=0.01, lr=1e-3)
    b, twin = make(), make()
    for it in range(2):  # the second iteration continues from the lanes' state
        s, st = b.ppo_iterate(8, opts)
        r = flat_rollout(twin, 8)
        a = r["arrays"]
        adv, ret = twin.gae(a["reward"], a["done"], a["value"], opts.gae_gamma, opts.gae_lambda)
        st2 = twin.ppo_update(dict(obs=r["obs"], alpha=r["alpha"], action=r["action"],
                                   old_logp=r["logp"], advantage=adv.ravel(), ret=ret.ravel()),
                              opts)
        s2 = r["summary"]
        assert bytes(s) == bytes(s2), it
        assert s.steps == 8 * 70 and (it == 0 or s.episodes > 0)
        assert st == st2, it
        assert st["n_minibatches"] == 2 * 6
        assert weights(b).tobytes() == weights(twin).tobytes(), it
        assert np.any(a["done"]) and np.any(a["reward"] != 0)
    trained = b.get_policy_net()
    assert np.any(P.flatten_params(trained) != P.flatten_params(b._net))
    # the lanes act with the updated network: the forward entry on the downloaded weights
    obs = flat_rollout(twin, 1)["obs"][:64]
    act, logp, val, lg = b.policy_net_forward(obs, deterministic=True, logits=True)
    rl, rv, el, ev = forward_with_bound(trained, obs)
    assert np.all(np.abs(lg.astype(np.float64) - rl) <= el)
    assert np.all(np.abs(val - rv) <= ev)
    # ... and not with the initial one
    rl0 = forward_with_bound(b._net, obs)[0]
    assert np.any(np.abs(lg.astype(np.float64) - rl0) > el)


def test_train_loop_and_lr_schedule(ctx):
    b = _batch(ctx, "nakamoto", alpha=0.35, gamma=0.5, max_steps=6, seed=2, n_lanes=70)
    b.set_policy_net(net_for(b, 3, 1, 16, 16))
    lrs = [st["lr"] for _, st in P.train(b, 3, 4, P.PPOOptions(n_epochs=1, minibatch=140),
                                         lr_schedule=lambda x: 1e-3 * x)]
    assert lrs == pytest.approx([1e-3, 1e-3 * 2 / 3, 1e-3 / 3])


# ------------------------------------------------------------------ 7. refusals

def test_refusals(ctx):
    b = _batch(ctx, "nakamoto", alpha=0.35, gamma=0.5, max_steps=6, seed=2, n_lanes=70)
    data = dict(obs=np.zeros((4, b.obs_len)), action=np.zeros(4, dtype=np.int32),
                old_logp=np.zeros(4), advantage=np.ones(4), ret=np.zeros(4))
    # before set_policy_net: a state error from every entry
    for call in (lambda: b.ppo_update(data), lambda: b.ppo_iterate(4),
                 lambda: b.get_policy_net(), lambda: b.ppo_param_count()):
        with pytest.raises(L.CprError) as e:
            call()
        assert e.value.code == L.CPR_E_STATE
    st = L.PpoStats()
    o = P.PPOOptions().cstruct()
    c, keep = b._ppo_data(data, False)
    idx = np.zeros(1, dtype=np.int32)
    g = np.zeros(1, dtype=np.float32)
    assert L.lib().cpr_ppo_gradients(b.handle, ctypes.byref(c), L.ptr(idx), 1, ctypes.byref(o),
                                     L.ptr(g), ctypes.byref(st)) == L.CPR_E_STATE
    # the training kernels' LDS budget: the training forward needs what the rollout's forward
    # needs (ppo.h ppo_lds_bytes), so a network cpr_policy_net_set accepts trains; the widest
    # depth-1 network does
    wide = net_for(b, 1, 1, 512, 512)
    b.set_policy_net(wide)
    grad, _ = b.ppo_gradients(data, np.arange(4), P.PPOOptions())
    assert grad.size == b.ppo_param_count() and np.any(grad != 0)
    # option values: Python names the field before the call, the library after it
    for field, bad in (("minibatch", 0), ("n_epochs", 0), ("lr", float("nan")),
                       ("lr", float("inf")), ("clip_range", float("nan"))):
        with pytest.raises(ValueError, match=field):
            b.ppo_update(data, P.PPOOptions(**{field: bad}))
        o = P.PPOOptions(**{field: bad}).cstruct()
        rc = L.lib().cpr_ppo_update(b.handle, ctypes.byref(c), ctypes.byref(o), None,
                                    ctypes.byref(st))
        assert rc == L.CPR_E_INVALID_ARG and field in L.lib().cpr_last_error().decode()
    assert np.array_equal(weights(b), P.flatten_params(wide))  # nothing was launched
    # rows outside the data
    with pytest.raises(L.CprError) as e:
        b.ppo_gradients(data, np.array([4]), P.PPOOptions())
    assert e.value.code == L.CPR_E_INVALID_ARG
    del keep


def test_fc16_is_unsupported(ctx):
    cfg, keep = device.make_config(alpha=0.3, gamma=0.5, protocol=L.PROTO_FC16, max_steps=100,
                                   policy=L.FC16_POLICY_HONEST, n_lanes=4)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    o = P.PPOOptions().cstruct()
    st, s = L.PpoStats(), L.Summary()
    assert L.lib().cpr_ppo_iterate(b.handle, 4, ctypes.byref(o), ctypes.byref(s),
                                   ctypes.byref(st)) == L.CPR_E_UNSUPPORTED
    c = L.PpoDataC()
    assert L.lib().cpr_ppo_update(b.handle, ctypes.byref(c), ctypes.byref(o), None,
                                  ctypes.byref(st)) == L.CPR_E_UNSUPPORTED
