"""device.PolicyNet without a GPU: shape validation, SB3 state-dict names, the f64 reference
forward and the C struct handed to cpr_policy_net_set."""

import ctypes

import numpy as np
import pytest

from cpr_amd import _lib as L
from cpr_amd import device


def _layers(rng, n_in, widths):
    out = []
    for w in widths:
        out.append((rng.standard_normal((w, n_in)).astype(np.float32),
                    rng.standard_normal(w).astype(np.float32)))
        n_in = w
    return out


def _net(n_in=6, pi=(32, 32), vf=(48, 48), n_actions=4, extra=(0.25, 0.5), seed=0):
    rng = np.random.default_rng(seed)
    return dict(pi=_layers(rng, n_in, pi), pi_head=_layers(rng, pi[-1], (n_actions,))[0],
                vf=_layers(rng, n_in, vf), vf_head=_layers(rng, vf[-1], (1,))[0], extra=extra)


def test_policy_net_shapes():
    net = device.PolicyNet(**_net())
    assert (net.depth, net.n_in, net.width_pi, net.width_vf, net.n_actions) == (2, 6, 32, 48, 4)
    c = net.cstruct()
    assert (c.n_extra, c.depth, c.width_pi, c.width_vf) == (2, 2, 32, 48)
    assert [c.extra[i] for i in range(2)] == [0.25, 0.5]
    assert c.pi_w[1] == net.pi[1][0].ctypes.data and c.vf_head_b == net.vf_head[1].ctypes.data
    assert c.pi_w[2] is None and c.vf_b[3] is None


def test_policy_net_rejects_width_not_multiple_of_16():
    with pytest.raises(ValueError, match=r"pi\[0\].*multiple of 16"):
        device.PolicyNet(**_net(pi=(24, 24)))
    with pytest.raises(ValueError, match=r"vf\[0\].*multiple of 16"):
        device.PolicyNet(**_net(vf=(528, 528)))


def test_policy_net_rejects_depth_mismatch_and_ragged_trunk():
    with pytest.raises(ValueError, match="depths differ"):
        device.PolicyNet(**_net(pi=(32, 32), vf=(32,)))
    with pytest.raises(ValueError, match=r"pi\[1\].*differs"):
        device.PolicyNet(**_net(pi=(32, 64)))
    with pytest.raises(ValueError, match="depth 5"):
        device.PolicyNet(**_net(pi=(16,) * 5, vf=(16,) * 5))


def test_policy_net_rejects_wrong_head_size():
    kw = _net()
    kw["vf_head"] = _layers(np.random.default_rng(1), 48, (2,))[0]
    with pytest.raises(ValueError, match="vf_head: 2 outputs"):
        device.PolicyNet(**kw)
    kw = _net()
    kw["pi_head"] = _layers(np.random.default_rng(1), 16, (4,))[0]
    with pytest.raises(ValueError, match="pi_head: input width 16"):
        device.PolicyNet(**kw)
    kw = _net()
    kw["pi_head"] = (kw["pi_head"][0], kw["pi_head"][1][:3])
    with pytest.raises(ValueError, match="pi_head"):
        device.PolicyNet(**kw)


def test_policy_net_rejects_non_finite_weight_and_extra():
    kw = _net()
    kw["vf"][1][0][3, 5] = np.nan
    with pytest.raises(ValueError, match=r"vf\[1\] weight: non-finite"):
        device.PolicyNet(**kw)
    kw = _net()
    kw["pi_head"][1][0] = np.inf
    with pytest.raises(ValueError, match="pi_head bias: non-finite"):
        device.PolicyNet(**kw)
    with pytest.raises(ValueError, match="extra"):
        device.PolicyNet(**_net(extra=(0.1, float("nan"))))
    with pytest.raises(ValueError, match="extra: at most 8"):
        device.PolicyNet(**_net(extra=(0.0,) * 9))
    with pytest.raises(TypeError, match=r"pi\[0\] weight"):
        kw = _net()
        kw["pi"][0] = (np.array([["a"]]), kw["pi"][0][1])
        device.PolicyNet(**kw)


def test_from_state_dict_round_trips_a_torch_module_with_sb3_names():
    import torch
    nn = torch.nn

    class Extractor(nn.Module):
        def __init__(self, n_in, w):
            super().__init__()
            self.policy_net = nn.Sequential(nn.Linear(n_in, w), nn.ReLU(), nn.Linear(w, w),
                                            nn.ReLU(), nn.Linear(w, w), nn.ReLU())
            self.value_net = nn.Sequential(nn.Linear(n_in, w), nn.ReLU(), nn.Linear(w, w),
                                           nn.ReLU(), nn.Linear(w, w), nn.ReLU())

    class Policy(nn.Module):  # the parameter names of SB3's ActorCriticPolicy
        def __init__(self, n_in=6, w=64, n_actions=4):
            super().__init__()
            self.mlp_extractor = Extractor(n_in, w)
            self.action_net = nn.Linear(w, n_actions)
            self.value_net = nn.Linear(w, 1)

        def forward(self, x):
            return (self.action_net(self.mlp_extractor.policy_net(x)),
                    self.value_net(self.mlp_extractor.value_net(x))[:, 0])

    torch.manual_seed(5)
    pol = Policy().double()
    net = device.PolicyNet.from_state_dict(pol.state_dict(), extra=(0.25, 0.5))
    assert (net.depth, net.n_in, net.width_pi, net.width_vf, net.n_actions) == (3, 6, 64, 64, 4)
    sd = {k: v.float() for k, v in pol.state_dict().items()}
    for i, key in enumerate(["0", "2", "4"]):
        assert np.array_equal(net.pi[i][0], sd[f"mlp_extractor.policy_net.{key}.weight"].numpy())
        assert np.array_equal(net.vf[i][1], sd[f"mlp_extractor.value_net.{key}.bias"].numpy())
    assert np.array_equal(net.pi_head[0], sd["action_net.weight"].numpy())
    assert np.array_equal(net.vf_head[1], sd["value_net.bias"].numpy())
    # the f64 reference forward is the module's forward on f32-rounded weights and inputs
    pol32 = Policy().double()
    pol32.load_state_dict({k: v.double() for k, v in sd.items()})
    obs = np.random.default_rng(2).random((9, 4))
    x = np.concatenate([obs.astype(np.float32).astype(np.float64),
                        np.tile([0.25, 0.5], (9, 1))], axis=1)
    lg, val = pol32(torch.from_numpy(x))
    rl, rv = net.forward_f64(obs)
    assert np.allclose(rl, lg.detach().numpy(), rtol=1e-12, atol=1e-14)
    assert np.allclose(rv, val.detach().numpy(), rtol=1e-12, atol=1e-14)


def test_from_state_dict_names_the_missing_key():
    with pytest.raises(KeyError, match="mlp_extractor.policy_net"):
        device.PolicyNet.from_state_dict({})


def test_c_struct_matches_header(tmp_path):
    import pathlib
    import subprocess

    root = pathlib.Path(__file__).resolve().parent.parent
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cpr_hip.h"\n'
        'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(cpr_policy_net),'
        ' offsetof(cpr_policy_net, depth), offsetof(cpr_policy_net, pi_w),'
        ' offsetof(cpr_policy_net, vf_head_b), sizeof(cpr_rollout_net_out));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", f"-I{root / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    P = L.PolicyNetC
    assert got == [ctypes.sizeof(P), P.depth.offset, P.pi_w.offset, P.vf_head_b.offset,
                   ctypes.sizeof(L.RolloutNetOut)]
    assert L.TAG_POLICY == 0x60000000
