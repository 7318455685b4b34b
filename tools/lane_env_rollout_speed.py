"""Network rollout throughput with and without a lane env (cpr_lane_env_set), at the shapes of
tools/policy_rollout_speed.py: 65,536 lanes, 64 steps per call, every output in device memory.

  bk8       B_k lanes, k = 8, 3x64 network
  nakamoto  Nakamoto lanes, 3x256 network

One variant per process (a comparison alternates processes of this tool):
  plain  Batch.rollout_net on a batch without a lane env. With --tree PATH the package and its
         library are imported from another checkout (the commit before the lane env), which
         makes it the baseline of an A/B
  table  the same batch with a 20-entry alpha table fed to the network's alpha column,
         sparse_relative rewards and r / alpha
  split  what mixing 20 alphas takes without a table: 20 batches of lanes / 20 lanes, one alpha
         each, rolled out in turn (one round = every batch once)

Warm-up calls first, then --repeats timed ones (host clock around the synchronous call);
prints one JSON line per shape (median and every sample) and appends it to --out."""
import argparse
import json
import pathlib
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--variant", choices=["plain", "table", "split"], required=True)
ap.add_argument("--tree", default=str(pathlib.Path(__file__).resolve().parent.parent))
ap.add_argument("--label", default=None)
ap.add_argument("--lanes", type=int, default=65536)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--shapes", default="bk8,nakamoto")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.tree)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpr_amd import _lib as L, device  # noqa: E402

N, T = args.lanes, args.steps
N_ALPHA = 20
ALPHAS = [0.05 + 0.02 * i for i in range(N_ALPHA)]  # 0.05 .. 0.43
SHAPES = {
    "bk8": dict(cfg=dict(protocol=L.PROTO_BK, k=8, gamma=0.5, max_steps=2016, seed=7), width=64),
    "nakamoto": dict(cfg=dict(protocol=L.PROTO_NAKAMOTO, gamma=0.5, max_steps=2016,
                              propagation_delay=1e-9, seed=7), width=256),
}
DEPTH = 3
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


def make_batch(sh, lanes, alpha, seed_offset=0):
    c = dict(sh["cfg"])
    c["seed"] += seed_offset
    cfg, keep = device.make_config(n_lanes=lanes, alpha=alpha, **c)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    ol, na = b.observation_spec()[:2]
    return b, ol, na


def buffers(lanes, ol):
    f64 = torch.float64
    bufs = dict(obs0=torch.empty((lanes, ol), dtype=f64, device=dev),
                obs=torch.empty((T, lanes, ol), dtype=f64, device=dev),
                action=torch.empty((T, lanes), dtype=torch.int32, device=dev),
                reward=torch.empty((T, lanes), dtype=f64, device=dev),
                done=torch.empty((T, lanes), dtype=torch.uint8, device=dev),
                logp=torch.empty((T, lanes), dtype=f64, device=dev),
                value=torch.empty((T + 1, lanes), dtype=f64, device=dev))
    torch.cuda.synchronize()
    return bufs


def shape_case(name):
    sh = SHAPES[name]
    if args.variant == "split":
        per = -(-N // N_ALPHA)  # 3,277 lanes at 65,536
        batches = []
        for j, a in enumerate(ALPHAS):
            b, ol, na = make_batch(sh, per, a, seed_offset=j)
            b.set_policy_net(random_net(ol + 2, sh["width"], na, (a, 0.5)))
            batches.append(b)
        bufs = buffers(per, ol)
        ptrs = {k: v.data_ptr() for k, v in bufs.items()}
        steps = per * N_ALPHA * T

        def call():
            for b in batches:
                b.rollout_net(T, deterministic=False, device_outputs=ptrs)
    else:
        b, ol, na = make_batch(sh, N, 0.33)
        if args.variant == "table":
            b.set_lane_env(alphas=ALPHAS, alpha_column=0, reward="sparse_relative",
                           shape="per_alpha")
        b.set_policy_net(random_net(ol + 2, sh["width"], na, (0.33, 0.5)))
        bufs = buffers(N, ol)
        if args.variant == "table":
            bufs["alpha0"] = torch.empty(N, dtype=torch.float64, device=dev)
            bufs["alpha"] = torch.empty((T, N), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
        ptrs = {k: v.data_ptr() for k, v in bufs.items()}
        steps = N * T

        def call():
            b.rollout_net(T, deterministic=False, device_outputs=ptrs)

    for _ in range(args.warmup):
        call()
    walls = []
    for _ in range(args.repeats):
        ctx.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    assert torch.isfinite(bufs["logp"]).all() and int(bufs["action"].max()) < na
    if args.variant == "table":
        assert len(torch.unique(bufs["alpha"])) == N_ALPHA
    w = statistics.median(walls)
    return dict(label=args.label or args.variant, variant=args.variant, shape=name, lanes=N,
                steps_per_call=T, env_steps_per_call=steps, wall_s=w, env_steps_per_s=steps / w,
                samples_env_steps_per_s=[steps / x for x in walls])


for name in args.shapes.split(","):
    line = json.dumps(shape_case(name))
    print(line, flush=True)
    if args.out:
        out = pathlib.Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        with out.open("a") as f:
            f.write(line + "\n")
