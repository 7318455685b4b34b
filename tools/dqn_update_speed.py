"""Throughput of device Q-learning (cpr_dqn_update) against the same update written in torch on
the same GPU, on a replay ring filled by an FC16 env batch (4,096 lanes x 64 slots = 262,144
transitions): dqn.yml's shape (batch 500, 100 gradient steps per call, 2 x 64) and one large
batch (65,536 rows, 10 steps).

One variant per process (a comparison alternates processes of this tool):
  device  Batch.dqn_update with explicit indices (the upload of the indices is inside the call)
  torch   torch.nn modules in f32 with the same initial weights and target, the ring's rows as
          f32 tensors on the GPU, the same indices, smooth_l1_loss, clip_grad_norm_ and
          torch.optim.Adam(eps=1e-8)

Warm-up calls first, then --repeats timed ones (host clock around the synchronous call); one
JSON line per shape is printed and appended to --out. Reported: gradient steps/s and rows/s.

--summarize FILE --json OUT folds the lines of alternating runs into one document: per
(variant, shape) the median of every timed call, and device over torch in steps/s."""
import argparse
import json
import pathlib
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--variant", choices=["device", "torch"])
ap.add_argument("--tree", default=str(pathlib.Path(__file__).resolve().parent.parent))
ap.add_argument("--lanes", type=int, default=4096)
ap.add_argument("--slots", type=int, default=64)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--shapes", default="500x100,65536x10", help="batch x gradient steps, ...")
ap.add_argument("--out", default=None)
ap.add_argument("--summarize", default=None)
ap.add_argument("--json", default=None)
args = ap.parse_args()

if args.summarize:
    groups = {}
    for line in pathlib.Path(args.summarize).read_text().splitlines():
        r = json.loads(line)
        g = groups.setdefault((r["variant"], r["batch"], r["gradient_steps"]), dict(r, walls_s=[]))
        g["walls_s"] += r["walls_s"]
    rows = []
    for g in groups.values():
        w = statistics.median(g["walls_s"])
        rows.append(dict(variant=g["variant"], network=g["network"], batch=g["batch"],
                         gradient_steps=g["gradient_steps"], transitions=g["transitions"],
                         timed_calls=len(g["walls_s"]), wall_s=w,
                         steps_per_s=g["gradient_steps"] / w,
                         rows_per_s=g["gradient_steps"] * g["batch"] / w))
    by = {(r["variant"], r["batch"], r["gradient_steps"]): r for r in rows}
    ratio = {f"batch{b}x{s}": by[("device", b, s)]["steps_per_s"] / by[("torch", b, s)]["steps_per_s"]
             for (v, b, s) in by if v == "device" and ("torch", b, s) in by}
    doc = dict(tool="tools/dqn_update_speed.py", rows=rows, device_over_torch_steps_per_s=ratio)
    pathlib.Path(args.json).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(ratio))
    sys.exit(0)

sys.path.insert(0, args.tree)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpr_amd import _lib as L, device  # noqa: E402
from cpr_amd import dqn as Q  # noqa: E402

N, SLOTS, DEPTH, WIDTH = args.lanes, args.slots, 2, 64
ctx = device.default_context()
dev = torch.device("cuda", ctx.device)


def random_net(n_in, n_act):
    rng = np.random.default_rng(1)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    def trunk():
        return [lin(WIDTH, n_in if i == 0 else WIDTH) for i in range(DEPTH)]

    return device.PolicyNet(pi=trunk(), pi_head=lin(n_act, WIDTH), vf=trunk(),
                            vf_head=lin(1, WIDTH))


def q_module(net):
    mods = []
    for w, bias in list(net.pi) + [net.pi_head]:
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(bias))
        mods += [lin, torch.nn.ReLU()]
    return torch.nn.Sequential(*mods[:-1])


def case(batch, steps):
    cfg, keep = device.make_config(protocol=L.PROTO_FC16_ENV, alpha=0.4, gamma=0.5, horizon=25,
                                   max_steps=254, seed=7, n_lanes=N, policy=L.FC16_POLICY_HONEST)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    ol, na = b.observation_spec()[:2]
    net = random_net(ol, na)
    b.set_policy_net(net)
    b.dqn_init(SLOTS)
    b.dqn_collect(SLOTS, 0.5)
    n = SLOTS * N
    opts = Q.DQNOptions(batch=batch, gradient_steps=steps, gamma=1.0, lr=1e-3, max_grad_norm=10.0)
    idx = np.random.default_rng(3).integers(0, n, (steps, batch))
    if args.variant == "device":
        def call():
            return b.dqn_update(options=opts, idx=idx)
    else:
        rep = b.dqn_replay()
        f32 = lambda k: torch.tensor(rep[k].reshape(n, -1), dtype=torch.float32, device=dev)  # noqa: E731
        x, xn = f32("obs"), f32("next_obs")
        rew, nnt = f32("reward")[:, 0], 1.0 - f32("done")[:, 0]
        act = torch.tensor(rep["action"].reshape(n), dtype=torch.int64, device=dev)
        model, target = q_module(net).to(dev), q_module(net).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=opts.lr, eps=opts.adam_eps)
        tidx = torch.tensor(idx, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def call():
            last = None
            for g in range(steps):
                i = tidx[g]
                with torch.no_grad():
                    y = rew[i] + nnt[i] * opts.gamma * target(xn[i]).max(dim=1).values
                q = model(x[i]).gather(1, act[i][:, None])[:, 0]
                loss = torch.nn.functional.smooth_l1_loss(q, y)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(model.parameters(), opts.max_grad_norm)
                opt.step()
                last = loss
            torch.cuda.synchronize()
            return dict(loss=float(last.detach()))

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
    b.close()
    return dict(variant=args.variant, network=f"{DEPTH}x{WIDTH}", batch=batch, gradient_steps=steps,
                transitions=n, wall_s=w, steps_per_s=steps / w, walls_s=walls,
                last_loss=st["loss"])


for shape in args.shapes.split(","):
    bsz, steps = (int(v) for v in shape.split("x"))
    line = json.dumps(case(bsz, steps))
    print(line, flush=True)
    if args.out:
        out = pathlib.Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        with out.open("a") as f:
            f.write(line + "\n")
