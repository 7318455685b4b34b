"""Nakamoto device-rollout throughput probe: 65,536 closed-form lanes, SM1, alpha .33,
gamma .5, the gym's 1e-9 delay, max_steps 2016, 512 steps per lane and call.

  (a) cpr_rollout without outputs
  (b) cpr_rollout writing obs / reward / done to device memory (torch tensors)
  (c) the host loop it replaces: policy_actions + step(with_info=False), 32 steps
  (d) cpr_run_episodes, summary only, over the same number of activations as (a), and over
      one 2016-step episode per lane (the fused kernel at the rollout's lane count)

Warm-up calls first, then REPEATS timed ones; medians. Prints one JSON line and writes it to
--out (default profiles/nak_rollout_speed.json)."""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from cpr_amd import _lib as L, device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lanes", type=int, default=65536)
ap.add_argument("--steps", type=int, default=512)
ap.add_argument("--host-steps", type=int, default=32)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=str(ROOT / "profiles" / "nak_rollout_speed.json"))
args = ap.parse_args()
N, T, R = args.lanes, args.steps, max(5, args.repeats)
KW = dict(alpha=0.33, gamma=0.5, policy=L.POLICY_SAPIRSHTEIN_2016_SM1, max_steps=2016,
          propagation_delay=1e-9, seed=7)

ctx = device.default_context()
med = statistics.median


def timed(fn):
    """medians over R timed calls of fn() -> (steps, activations, kernel_ms)"""
    for _ in range(args.warmup):
        fn()
    rows = []
    for _ in range(R):
        ctx.synchronize()
        t0 = time.perf_counter()
        steps, acts, ms = fn()
        rows.append((time.perf_counter() - t0, steps, acts, ms))
    wall = med(r[0] for r in rows)
    steps, acts = med(r[1] for r in rows), med(r[2] for r in rows)
    ms = med(r[3] for r in rows)
    out = dict(wall_s=wall, steps=steps, activations=acts, kernel_ms=ms,
               env_steps_per_s=steps / wall, activations_per_s=acts / wall)
    if ms:
        out["kernel_env_steps_per_s"] = steps / ms * 1e3
        out["kernel_activations_per_s"] = acts / ms * 1e3
    return out


def rollout_case(dev_out):
    cfg, keep = device.make_config(n_lanes=N, **KW)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    ptrs = None
    if dev_out:
        dev = torch.device("cuda", ctx.device)
        o_t = torch.empty((T, N, 4), dtype=torch.float64, device=dev)
        r_t = torch.empty((T, N), dtype=torch.float64, device=dev)
        d_t = torch.empty((T, N), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ptrs = (o_t.data_ptr(), r_t.data_ptr(), d_t.data_ptr())

    def call():
        s = b.rollout(T, device_outputs=ptrs) if dev_out else b.rollout(T)
        return s.steps, s.activations, b.last_launch()[0]

    out = timed(call)
    if dev_out:
        out["output_bytes"] = o_t.numel() * 8 + r_t.numel() * 8 + d_t.numel()
    out["lanes"], out["resident_lanes"] = b.launch_shape()
    return out


def host_loop_case():
    cfg, keep = device.make_config(n_lanes=N, **KW)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    state = {"obs": b.reset()}
    H = args.host_steps

    def call():
        obs = state["obs"]
        for _ in range(H):
            acts = b.policy_actions(KW["policy"], obs)
            obs, _, _, _ = b.step(acts, with_info=False)
        state["obs"] = obs
        return N * H, N * H, 0.0  # closed form at 1e-9: one activation per step

    return timed(call)


def fused_case(n_eps):
    cfg, keep = device.make_config(**KW)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    first = {"e": 0}

    def call():
        s = b.run(n_eps, first_episode=first["e"])
        first["e"] += n_eps
        return s.steps, s.activations, b.last_launch()[0]

    out = timed(call)
    out["episodes"] = n_eps
    return out


res = dict(shape=dict(lanes=N, steps_per_call=T, host_loop_steps=args.host_steps, repeats=R,
                      warmup=args.warmup, **{k: v for k, v in KW.items()}))
res["a_rollout_no_outputs"] = a = rollout_case(False)
res["b_rollout_device_outputs"] = bb = rollout_case(True)
res["c_host_loop"] = c = host_loop_case()
res["d_fused_same_activations"] = d = fused_case(max(1, round(a["activations"] / 2017)))
res["d_fused_episode_per_lane"] = d2 = fused_case(N)
res["ratios"] = dict(
    a_over_c_env_steps=a["env_steps_per_s"] / c["env_steps_per_s"],
    b_over_c_env_steps=bb["env_steps_per_s"] / c["env_steps_per_s"],
    a_over_d_activations=a["activations_per_s"] / d["activations_per_s"],
    a_over_d_episode_per_lane_activations=a["activations_per_s"] / d2["activations_per_s"],
)
line = json.dumps(res)
print(line, flush=True)
out = pathlib.Path(args.out)
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(line + "\n")
