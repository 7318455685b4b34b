"""FC16 env network rollout: the one-kernel path (k_fc16_rollout_net) against the launch
sequence (CPR_FC16_ROLLOUT_FUSED=0: forward, step, collect and reset kernels per step, the
architecture of the other four protocols' cpr_rollout_net).

Shapes: 4,096 and 65,536 lanes x 3x64 and 3x256 networks, 64 steps per call, sampled actions,
every output written to device memory (torch tensors): what cpr_ppo_iterate consumes.

Method: per shape, `--pairs` alternating pairs of fresh processes (fused, sequence, fused,
...), so that neither path always runs on a warmer device; each process warms up, then times
`--repeats` calls (wall clock around the synchronous call) and reports their median and
range. The parent never opens the GPU. Prints one JSON line and writes it to --out (default
profiles/fc16_rollout_speed.json); `fused_wins_every_pair` per shape is the criterion of
DESIGN.md §4.10 for the default."""
import argparse
import json
import os
import pathlib
import statistics
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--lanes", default="4096,65536")
ap.add_argument("--widths", default="64,256")
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--pairs", type=int, default=3)
ap.add_argument("--out", default=str(ROOT / "profiles" / "fc16_rollout_speed.json"))
ap.add_argument("--child", nargs=2, metavar=("LANES", "WIDTH"), help=argparse.SUPPRESS)
args = ap.parse_args()
T, DEPTH, EXTRA = args.steps, 3, (0.33, 0.5)


def child(n, width):
    import numpy as np
    import torch

    from cpr_amd import _lib as L, device

    ctx = device.default_context()
    dev = torch.device("cuda", ctx.device)
    cfg, keep = device.make_config(protocol=L.PROTO_FC16_ENV, alpha=0.33, gamma=0.5, horizon=100,
                                   max_steps=2016, seed=7, n_lanes=n,
                                   policy=L.FC16_POLICY_HONEST)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    rng = np.random.default_rng(1)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    def trunk():
        return [lin(width, 3 + len(EXTRA) if i == 0 else width) for i in range(DEPTH)]

    b.set_policy_net(device.PolicyNet(pi=trunk(), pi_head=lin(4, width), vf=trunk(),
                                      vf_head=lin(1, width), extra=EXTRA))
    bufs = dict(obs0=torch.empty((n, 3), dtype=torch.float64, device=dev),
                obs=torch.empty((T, n, 3), dtype=torch.float64, device=dev),
                action=torch.empty((T, n), dtype=torch.int32, device=dev),
                reward=torch.empty((T, n), dtype=torch.float64, device=dev),
                done=torch.empty((T, n), dtype=torch.uint8, device=dev),
                logp=torch.empty((T, n), dtype=torch.float64, device=dev),
                value=torch.empty((T + 1, n), dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    walls, kernel_ms = [], []
    for k in range(args.warmup + args.repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        b.rollout_net(T, deterministic=False, device_outputs=ptrs)
        dt = time.perf_counter() - t0
        if k >= args.warmup:
            walls.append(dt)
            kernel_ms.append(b.last_launch()[0])
    assert torch.isfinite(bufs["logp"]).all() and int(bufs["action"].max()) < 4
    print(json.dumps(dict(fused=b.rollout_net_fused(), wall_s_median=statistics.median(walls),
                          wall_s_min=min(walls), wall_s_max=max(walls),
                          device_ms_median=statistics.median(kernel_ms),
                          env_steps_per_s=n * T / statistics.median(walls))))


def run_child(n, width, fused):
    env = dict(os.environ)
    env["CPR_FC16_ROLLOUT_FUSED"] = "1" if fused else "0"
    p = subprocess.run([sys.executable, __file__, "--child", str(n), str(width), "--steps", str(T),
                        "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                       env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"child ({n}, {width}, fused={fused}) failed: {p.stderr[-2000:]}")
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["fused"] == fused, r
    return r


if args.child:
    child(int(args.child[0]), int(args.child[1]))
    sys.exit(0)

res = dict(method=dict(steps_per_call=T, depth=DEPTH, repeats=args.repeats, warmup=args.warmup,
                       pairs=args.pairs, outputs="device", actions="sampled",
                       timing="wall clock around the synchronous call, median of repeats; "
                              "alternating fresh processes"), shapes=[])
for n in (int(x) for x in args.lanes.split(",")):
    for width in (int(x) for x in args.widths.split(",")):
        pairs = []
        for _ in range(args.pairs):
            f = run_child(n, width, True)
            q = run_child(n, width, False)
            pairs.append(dict(fused=f, sequence=q,
                              speedup=f["env_steps_per_s"] / q["env_steps_per_s"]))
        sp = [p["speedup"] for p in pairs]
        res["shapes"].append(dict(
            lanes=n, width=width, pairs=pairs,
            fused_env_steps_per_s_median=statistics.median(p["fused"]["env_steps_per_s"]
                                                           for p in pairs),
            sequence_env_steps_per_s_median=statistics.median(p["sequence"]["env_steps_per_s"]
                                                              for p in pairs),
            speedup_median=statistics.median(sp), speedup_min=min(sp), speedup_max=max(sp),
            fused_wins_every_pair=all(s > 1.0 for s in sp)))
        print(f"# {n} lanes, 3x{width}: speedup {min(sp):.2f} .. {max(sp):.2f}", file=sys.stderr,
              flush=True)
line = json.dumps(res)
print(line, flush=True)
out = pathlib.Path(args.out)
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(line + "\n")
