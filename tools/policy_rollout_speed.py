"""Network-driven rollout throughput probe: cpr_rollout_net against the host loop it
replaces, at the reference's training shapes.

  bk8       65,536 B_k lanes, k = 8, 3x64 network  (experiments/train/configs/bk-8.yaml)
  nakamoto  65,536 Nakamoto lanes, 3x256 network   (experiments/train/configs/nakamoto.yaml)

Per shape:
  (a) Batch.rollout_net, sampled actions, every output written to device memory (torch
      tensors): what a PPO learner consumes
  (b) the only path without it: a host loop of Batch.step with the same network evaluated by
      torch (f32, Categorical sampling) on the same GPU
  (c) k_policy_forward alone (Batch.policy_net_forward over the lanes' observations; the
      kernel's own time from HIP events), with its f32 TFLOP/s against the 157 TF f32 matrix
      peak

Warm-up calls first, then timed ones; medians. Prints one JSON line and writes it to --out
(default profiles/policy_rollout_speed.json)."""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpr_amd import _lib as L, device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lanes", type=int, default=65536)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--host-steps", type=int, default=8)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--shapes", default="bk8,nakamoto")
ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_rollout_speed.json"))
args = ap.parse_args()
N, T, R = args.lanes, args.steps, args.repeats
F32_MATRIX_PEAK_TF = 157.0

SHAPES = {
    "bk8": dict(cfg=dict(protocol=L.PROTO_BK, k=8, alpha=0.33, gamma=0.5, max_steps=2016, seed=7),
                width=64),
    "nakamoto": dict(cfg=dict(protocol=L.PROTO_NAKAMOTO, alpha=0.33, gamma=0.5, max_steps=2016,
                              propagation_delay=1e-9, seed=7), width=256),
}
DEPTH, EXTRA = 3, (0.33, 0.5)

ctx = device.default_context()
dev = torch.device("cuda", ctx.device)
med = statistics.median


def timed(fn):
    for _ in range(args.warmup):
        fn()
    rows = []
    for _ in range(R):
        ctx.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        extra = fn()
        rows.append((time.perf_counter() - t0, extra))
    return med(r[0] for r in rows), med(r[1] for r in rows)


class TorchNet(torch.nn.Module):
    """The same network in torch, from the PolicyNet's arrays."""

    def __init__(self, net):
        super().__init__()

        def seq(trunk, head):
            mods = []
            for w, b in list(trunk) + [head]:
                lin = torch.nn.Linear(w.shape[1], w.shape[0])
                lin.weight.data = torch.from_numpy(w.copy())
                lin.bias.data = torch.from_numpy(b.copy())
                mods += [lin, torch.nn.ReLU()]
            return torch.nn.Sequential(*mods[:-1])

        self.pi, self.vf = seq(net.pi, net.pi_head), seq(net.vf, net.vf_head)
        self.extra = torch.tensor(net.extra, dtype=torch.float32)

    @torch.no_grad()
    def act(self, obs):
        x = torch.from_numpy(obs).to(dev).float()
        x = torch.cat([x, self.extra.to(dev).expand(x.shape[0], -1)], dim=1)
        dist = torch.distributions.Categorical(logits=self.pi(x))
        a = dist.sample()
        return a.int().cpu().numpy(), dist.log_prob(a).cpu().numpy(), self.vf(x)[:, 0].cpu().numpy()


def random_net(n_in, width, n_act):
    rng = np.random.default_rng(1)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    def trunk():
        return [lin(width, n_in if i == 0 else width) for i in range(DEPTH)]

    return device.PolicyNet(pi=trunk(), pi_head=lin(n_act, width), vf=trunk(),
                            vf_head=lin(1, width), extra=EXTRA)


def shape_case(name):
    sh = SHAPES[name]
    cfg, keep = device.make_config(n_lanes=N, **sh["cfg"])
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    ol, na = b.observation_spec()[:2]
    net = random_net(ol + len(EXTRA), sh["width"], na)
    b.set_policy_net(net)
    out = dict(lanes=N, depth=DEPTH, width=sh["width"], obs_len=ol, n_actions=na)

    # (a) the device rollout, every output in device memory
    bufs = dict(obs0=torch.empty((N, ol), dtype=torch.float64, device=dev),
                obs=torch.empty((T, N, ol), dtype=torch.float64, device=dev),
                action=torch.empty((T, N), dtype=torch.int32, device=dev),
                reward=torch.empty((T, N), dtype=torch.float64, device=dev),
                done=torch.empty((T, N), dtype=torch.uint8, device=dev),
                logp=torch.empty((T, N), dtype=torch.float64, device=dev),
                value=torch.empty((T + 1, N), dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}

    def roll():
        b.rollout_net(T, deterministic=False, device_outputs=ptrs)
        return b.last_launch()[0]

    wall, ms = timed(roll)
    out["a_rollout_net"] = dict(steps_per_call=T, wall_s=wall, device_ms=ms,
                                env_steps_per_s=N * T / wall)
    assert torch.isfinite(bufs["logp"]).all() and int(bufs["action"].max()) < na

    # (b) the host loop: torch forward on the same GPU, Batch.step
    b2 = device.Batch(cfg, ctx=ctx, keep=keep)
    tnet = TorchNet(net).to(dev)
    state = {"obs": b2.reset()}
    H = args.host_steps

    def host():
        obs = state["obs"]
        for _ in range(H):
            a, _, _ = tnet.act(obs)
            obs, _, _, _ = b2.step(a, with_info=False)
        state["obs"] = obs
        return 0.0

    wall_h, _ = timed(host)
    out["b_host_loop_torch"] = dict(steps_per_call=H, wall_s=wall_h,
                                    env_steps_per_s=N * H / wall_h)
    out["a_over_b_env_steps"] = out["a_rollout_net"]["env_steps_per_s"] / (N * H / wall_h)

    # (c) the forward kernel alone
    obs = bufs["obs"][T - 1].cpu().numpy()

    def fwd():
        b.policy_net_forward(obs, deterministic=False)
        return b.last_launch()[0]

    _, kms = timed(fwd)
    flop = 2.0 * N * sum(w.size for trunk, head in ((net.pi, net.pi_head), (net.vf, net.vf_head))
                         for w, _ in list(trunk) + [head])
    tf = flop / (kms * 1e-3) / 1e12
    out["c_forward_kernel"] = dict(kernel_ms=kms, flop=flop, f32_tflops=tf,
                                   fraction_of_f32_matrix_peak=tf / F32_MATRIX_PEAK_TF)
    return out


res = dict(shape=dict(lanes=N, steps_per_call=T, host_loop_steps=args.host_steps, repeats=R,
                      warmup=args.warmup, f32_matrix_peak_tf=F32_MATRIX_PEAK_TF))
for name in args.shapes.split(","):
    res[name] = shape_case(name)
line = json.dumps(res)
print(line, flush=True)
out = pathlib.Path(args.out)
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(line + "\n")
