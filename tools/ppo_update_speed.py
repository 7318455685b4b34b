"""Throughput of the device learner (cpr_ppo_update) against the same update written in torch
on the same GPU: 65,536 lanes x 64 steps of a Nakamoto network rollout (4.19 M samples), the
3x64 and 3x256 networks, minibatch 4,096 and 65,536.

One variant per process (a comparison alternates processes of this tool):
  device  Batch.ppo_update on device pointers with an explicit permutation
  torch   torch.nn modules in f32 with the same initial weights, the same minibatches (the same
          permutation), SB3's loss, clip_grad_norm_ and torch.optim.Adam(eps=1e-5); the
          observations are converted to f32 once, outside the timing

Both train --epochs epochs per call (default 1: a call is one pass over the samples; SB3's 10
scale both sides alike). Warm-up calls first, then --repeats timed ones (host clock around the
synchronous call); one JSON line per (network, minibatch) is printed and appended to --out.
Reported: samples/s (samples x epochs / wall) and f32 TFLOP/s counting 3x the forward's FLOPs
per sample over the whole call, Adam and the reductions included.

--summarize FILE --json OUT folds the lines of alternating runs into one document: per
(variant, network, minibatch) the median of every timed call."""
import argparse
import json
import pathlib
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--variant", choices=["device", "torch"])
ap.add_argument("--tree", default=str(pathlib.Path(__file__).resolve().parent.parent))
ap.add_argument("--lanes", type=int, default=65536)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--epochs", type=int, default=1)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--widths", default="64,256")
ap.add_argument("--minibatches", default="4096,65536")
ap.add_argument("--out", default=None)
ap.add_argument("--summarize", default=None)
ap.add_argument("--json", default=None)
args = ap.parse_args()

if args.summarize:
    groups = {}
    for line in pathlib.Path(args.summarize).read_text().splitlines():
        r = json.loads(line)
        g = groups.setdefault((r["variant"], r["network"], r["minibatch"]), dict(r, walls_s=[]))
        g["walls_s"] += r["walls_s"]
    rows = []
    for g in groups.values():
        w = statistics.median(g["walls_s"])
        work = g["samples"] * g["epochs"]
        rows.append(dict(variant=g["variant"], network=g["network"], minibatch=g["minibatch"],
                         samples=g["samples"], epochs=g["epochs"], timed_calls=len(g["walls_s"]),
                         wall_s=w, samples_per_s=work / w,
                         tflops_f32=3 * g["forward_flops_per_sample"] * work / w / 1e12))
    by = {(r["variant"], r["network"], r["minibatch"]): r for r in rows}
    ratio = {f"{n}/mb{m}": by[("device", n, m)]["samples_per_s"] / by[("torch", n, m)]["samples_per_s"]
             for (v, n, m) in by if v == "device" and ("torch", n, m) in by}
    doc = dict(tool="tools/ppo_update_speed.py", rows=rows, device_over_torch_samples_per_s=ratio)
    pathlib.Path(args.json).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(ratio))
    sys.exit(0)

sys.path.insert(0, args.tree)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpr_amd import _lib as L, device  # noqa: E402
from cpr_amd import ppo as P  # noqa: E402

N, T, DEPTH = args.lanes, args.steps, 3
ctx = device.default_context()
dev = torch.device("cuda", ctx.device)


def random_net(n_in, width, n_act, extra):
    rng = np.random.default_rng(1)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    def trunk():
        return [lin(width, n_in if i == 0 else width) for i in range(DEPTH)]

    return device.PolicyNet(pi=trunk(), pi_head=lin(n_act, width), vf=trunk(),
                            vf_head=lin(1, width), extra=extra)


def rollout_data(b, ol):
    """A sampled rollout and its GAE in device memory, as flat training rows."""
    f64 = torch.float64
    obs = torch.empty((T + 1, N, ol), dtype=f64, device=dev)  # obs0, then obs[t]
    bufs = dict(action=torch.empty((T, N), dtype=torch.int32, device=dev),
                reward=torch.empty((T, N), dtype=f64, device=dev),
                done=torch.empty((T, N), dtype=torch.uint8, device=dev),
                logp=torch.empty((T, N), dtype=f64, device=dev),
                value=torch.empty((T + 1, N), dtype=f64, device=dev))
    adv = torch.empty((T, N), dtype=f64, device=dev)
    ret = torch.empty((T, N), dtype=f64, device=dev)
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    ptrs["obs0"] = obs.data_ptr()
    ptrs["obs"] = obs[1:].data_ptr()
    b.rollout_net(T, deterministic=False, device_outputs=ptrs)
    b.gae(ptrs["reward"], ptrs["done"], ptrs["value"], 0.99, 0.95, device=True, n_steps=T,
          out=(adv.data_ptr(), ret.data_ptr()))
    return dict(obs=obs[:T].reshape(T * N, ol), action=bufs["action"].reshape(-1),
                old_logp=bufs["logp"].reshape(-1), advantage=adv.reshape(-1), ret=ret.reshape(-1),
                keep=(obs, bufs))


class TorchNet(torch.nn.Module):
    def __init__(self, net):
        super().__init__()

        def seq(layers, head):
            mods = []
            for w, bias in list(layers) + [head]:
                lin = torch.nn.Linear(w.shape[1], w.shape[0])
                with torch.no_grad():
                    lin.weight.copy_(torch.from_numpy(w))
                    lin.bias.copy_(torch.from_numpy(bias))
                mods += [lin, torch.nn.ReLU()]
            return torch.nn.Sequential(*mods[:-1])

        self.pi = seq(net.pi, net.pi_head)
        self.vf = seq(net.vf, net.vf_head)
        self.extra = torch.tensor(net.extra, dtype=torch.float32)


def case(width, mb):
    cfg, keep = device.make_config(protocol=L.PROTO_NAKAMOTO, gamma=0.5, max_steps=2016,
                                   propagation_delay=1e-9, seed=7, n_lanes=N, alpha=0.33)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    ol, na = b.observation_spec()[:2]
    net = random_net(ol + 2, width, na, (0.33, 0.5))
    b.set_policy_net(net)
    d = rollout_data(b, ol)
    n = T * N
    opts = P.PPOOptions(n_epochs=args.epochs, minibatch=mb)
    g = torch.Generator(device="cpu").manual_seed(3)
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(args.epochs)]).to(
        torch.int32).to(dev)
    torch.cuda.synchronize()
    flops = 2 * sum(w.size for trunk, head in ((net.pi, net.pi_head), (net.vf, net.vf_head))
                    for w, _ in list(trunk) + [head])
    if args.variant == "device":
        data = dict(n=n, obs=d["obs"].data_ptr(), action=d["action"].data_ptr(),
                    old_logp=d["old_logp"].data_ptr(), advantage=d["advantage"].data_ptr(),
                    ret=d["ret"].data_ptr())

        def call():
            return b.ppo_update(data, opts, perm=perm.data_ptr(), device=True)
    else:
        model = TorchNet(net).to(dev)
        extra = model.extra.to(dev)
        x = torch.cat([d["obs"].float(), extra.expand(n, 2)], dim=1)
        act = d["action"].long()
        olp, adv_all, ret_all = d["old_logp"].float(), d["advantage"].float(), d["ret"].float()
        opt = torch.optim.Adam(model.parameters(), lr=opts.lr, eps=opts.adam_eps)
        c = opts.clip_range
        torch.cuda.synchronize()

        def call():
            last = None
            for e in range(args.epochs):
                for s0 in range(0, n, mb):
                    idx = perm[e, s0:s0 + mb].long()
                    xb, adv = x[idx], adv_all[idx]
                    if len(adv) > 1:
                        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
                    logp_all = torch.log_softmax(model.pi(xb), dim=1)
                    logp = logp_all.gather(1, act[idx][:, None])[:, 0]
                    ratio = torch.exp(logp - olp[idx])
                    pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - c, 1 + c)).mean()
                    vl = torch.nn.functional.mse_loss(ret_all[idx], model.vf(xb)[:, 0])
                    el = (torch.exp(logp_all) * logp_all).sum(dim=1).mean()
                    loss = pl + opts.ent_coef * el + opts.vf_coef * vl
                    opt.zero_grad(set_to_none=True)
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_(model.parameters(), opts.max_grad_norm)
                    opt.step()
                    last = loss
            torch.cuda.synchronize()
            return dict(loss=float(last))

    for _ in range(args.warmup):
        st = call()
    walls = []
    for _ in range(args.repeats):
        ctx.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = call()
        walls.append(time.perf_counter() - t0)
    assert np.isfinite(st["loss"])
    w = statistics.median(walls)
    return dict(variant=args.variant, network=f"{DEPTH}x{width}", minibatch=mb, samples=n,
                epochs=args.epochs, forward_flops_per_sample=flops, wall_s=w,
                samples_per_s=n * args.epochs / w, walls_s=walls, last_loss=st["loss"])


for width in (int(x) for x in args.widths.split(",")):
    for mb in (int(x) for x in args.minibatches.split(",")):
        line = json.dumps(case(width, mb))
        print(line, flush=True)
        if args.out:
            out = pathlib.Path(args.out)
            out.parent.mkdir(parents=True, exist_ok=True)
            with out.open("a") as f:
                f.write(line + "\n")
