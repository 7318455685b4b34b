"""Generic release/consider env (CPR_PROTO_GENERIC_NAKAMOTO): what a per-lane block DAG costs.

Per lane count (4,096 and 65,536), in one process:
  rollout    cpr_rollout_net env-steps/s with a 3 x 64 network, sampled actions, K = 2, H = 25,
             max_steps 1000, outputs in device memory; beside it the same network shape and
             lane count on CPR_PROTO_FC16_ENV's launch sequence (the same kernels per step
             around an O(1) env), the two alternating call by call
  probe      an always-Continue batch (a network whose head always picks action 0, H = 10^9,
             max_steps 1000): the device time (events around the call) of a 20-step rollout
             when the lanes hold about 30 blocks and about 890 blocks, and of the same calls on
             the FC16 env; their difference per step is what the generic step and reset kernels
             cost beyond FC16's
             (the step kernel's own duration under a profiler is not measured here)
and once: the pure-Python reference env's single-env steps/s (tests/generic_env_ref.py), for
scale. Each process warms up first; medians of --repeats calls. Prints one JSON line and writes
it to --out (default profiles/generic_env_speed.json)."""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--lanes", default="4096,65536")
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--repeats", type=int, default=8)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=str(ROOT / "profiles" / "generic_env_speed.json"))
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
args = ap.parse_args()
T, DEPTH, WIDTH, PROBE_T = args.steps, 3, 64, 20
WINDOWS = {"blocks_30": 1, "blocks_890": 44}  # index of the 20-step call: steps 20.., 880..


def nets(rng_seed, n_in, n_act, always_zero=False):
    import numpy as np

    from cpr_amd import device

    rng = np.random.default_rng(rng_seed)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    def trunk():
        return [lin(WIDTH, n_in if i == 0 else WIDTH) for i in range(DEPTH)]

    head = lin(n_act, WIDTH)
    if always_zero:  # the head's logits are its bias: action 0 whatever the observation
        head = (np.zeros_like(head[0]), np.array([8.0] + [0.0] * (n_act - 1), dtype=np.float32))
    return device.PolicyNet(pi=trunk(), pi_head=head, vf=trunk(), vf_head=lin(1, WIDTH))


def make(proto, n, horizon, always_zero=False):
    from cpr_amd import _lib as L, device

    ctx = device.default_context()
    if proto == "generic":
        cfg, keep = device.make_config(protocol=L.PROTO_GENERIC_NAKAMOTO, alpha=0.33, gamma=0.5,
                                       horizon=horizon, max_steps=1000, seed=7, n_lanes=n, k=2,
                                       policy=0)
    else:
        cfg, keep = device.make_config(protocol=L.PROTO_FC16_ENV, alpha=0.33, gamma=0.5,
                                       horizon=horizon, max_steps=1000, seed=7, n_lanes=n,
                                       policy=L.FC16_POLICY_HONEST)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    ol, na = b.observation_spec()[:2]
    b.set_policy_net(nets(1, ol, na, always_zero))
    return b


def buffers(b, steps):
    """torch tensors for every output of a call, or (None, None) where torch sees no GPU: the
    rollout then runs without output buffers (the result's `outputs` says which)"""
    import torch

    if not torch.cuda.is_available():
        return None, None
    n, ol = b.n_lanes, b.obs_len
    dev = torch.device("cuda", b.ctx.device)
    bufs = dict(obs0=torch.empty((n, ol), dtype=torch.float64, device=dev),
                obs=torch.empty((steps, n, ol), dtype=torch.float64, device=dev),
                action=torch.empty((steps, n), dtype=torch.int32, device=dev),
                reward=torch.empty((steps, n), dtype=torch.float64, device=dev),
                done=torch.empty((steps, n), dtype=torch.uint8, device=dev),
                logp=torch.empty((steps, n), dtype=torch.float64, device=dev),
                value=torch.empty((steps + 1, n), dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    return bufs, {k: v.data_ptr() for k, v in bufs.items()}


def roll(b, steps, deterministic, ptrs):
    if ptrs is None:
        b.rollout_net(steps, deterministic=deterministic, outputs=False)
    else:
        b.rollout_net(steps, deterministic=deterministic, device_outputs=ptrs)


def probe(n, protos=("generic", "fc16")):
    """device ms of each 20-step always-action-0 call, per proto and window"""
    out = {}
    for proto in protos:
        b = make(proto, n, 1e9, always_zero=True)
        bufs, ptrs = buffers(b, PROBE_T)
        ms = []
        for _ in range(max(WINDOWS.values()) + 1):
            roll(b, PROBE_T, True, ptrs)
            ms.append(b.last_launch()[0])
        assert bufs is None or int(bufs["action"].max()) == 0
        out[proto] = {w: ms[i] / PROBE_T for w, i in WINDOWS.items()}
        if proto == "generic":
            # 900 Continue steps: a lane holds 901 blocks (unless one of its ~600 termination
            # words, each firing with probability 1e-9, ended an episode on the way)
            f = b.observe_fields()[:, 5]
            assert int(f.max()) == PROBE_T * (max(WINDOWS.values()) + 1) + 1, int(f.max())
            assert float(f.mean()) > int(f.max()) - 1
            out["generic_blocks_at_end"] = float(f.mean())
    return out


def child(n):
    b = {p: make(p, n, 25 if p == "generic" else 100) for p in ("generic", "fc16")}
    io = {p: buffers(b[p], T) for p in b}
    walls = {p: [] for p in b}
    dev_ms = {p: [] for p in b}
    for k in range(args.warmup + args.repeats):
        for p in b:  # alternating, call by call
            b[p].ctx.synchronize()
            t0 = time.perf_counter()
            roll(b[p], T, False, io[p][1])
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                walls[p].append(dt)
                dev_ms[p].append(b[p].last_launch()[0])
    res = dict(lanes=n, outputs="device" if io["generic"][1] is not None else "none")
    for p in b:
        res[p] = dict(env_steps_per_s=n * T / statistics.median(walls[p]),
                      wall_s_median=statistics.median(walls[p]), wall_s_min=min(walls[p]),
                      wall_s_max=max(walls[p]), device_ms_median=statistics.median(dev_ms[p]))
    res["generic_over_fc16"] = res["generic"]["env_steps_per_s"] / res["fc16"]["env_steps_per_s"]
    res["probe_device_ms_per_step"] = probe(n)
    print(json.dumps(res))


def reference_steps_per_s():
    sys.path.insert(0, str(ROOT / "tests"))
    import generic_env_ref as R

    env = R.GenericNakamotoRef(7, 0.33, 0.5, 25, 1000)
    steps, ep = 0, 0
    t0 = time.perf_counter()
    while steps < 3000:
        env.reset(ep)
        ep += 1
        while True:
            f = env.fields()
            _, _, term, trunc = env.step(R.honest_action(f[3], f[4]))
            steps += 1
            if term or trunc:
                break
    return steps / (time.perf_counter() - t0)


if args.child:
    child(int(args.child))
    sys.exit(0)
res = dict(method=dict(steps_per_call=T, network=f"{DEPTH}x{WIDTH}", k=2, horizon=25,
                       max_steps=1000, repeats=args.repeats, warmup=args.warmup,
                       actions="sampled",
                       timing="wall clock around the synchronous call, median of repeats; generic "
                              "and FC16 env alternate call by call in one process per lane "
                              "count; probe: device events around a 20-step call"),
           lanes=[])
for n in (int(x) for x in args.lanes.split(",")):
    p = subprocess.run([sys.executable, __file__, "--child", str(n), "--steps", str(T),
                        "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                       capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"child {n} failed: {p.stderr[-2000:]}")
    res["lanes"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    print(f"# {n} lanes done", file=sys.stderr, flush=True)
res["python_reference_steps_per_s"] = reference_steps_per_s()
line = json.dumps(res)
print(line, flush=True)
out = pathlib.Path(args.out)
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(line + "\n")
