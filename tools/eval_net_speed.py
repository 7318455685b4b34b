"""Time of one evaluation of the policy network (Batch.evaluate_net, cpr_eval_net) against the
same evaluation done without it: a deterministic network rollout whose step arrays are copied
to the host and binned by alpha there.

Shape (experiments/train/ppo.py's eval env at the lane count of tools/policy_rollout_speed.py):
65,536 lanes, a 20-entry alpha grid, episodes of exactly --episode-len steps (max_steps alone
ends them), sparse_relative reward / alpha, 3,276 episodes per alpha: 65,520 episodes, one
round of the lanes.

  bk8       B_k lanes, k = 8, 3x64 network
  nakamoto  Nakamoto lanes, 3x256 network

  eval     evaluate_net(3276, records=False) on a batch with the cyclic schedule: per-alpha
           summaries and mean / std of five columns, nothing per step leaves the device
  rollout  rollout_net(episode_len, deterministic=True, outputs=True) on a batch with the
           same table under the keyed choice, then on the host: the reward of every finished
           episode and its alpha from the step arrays, mean and std per alpha (of the reward
           alone: the rollout has no per-episode sim time, chain time or activations to bin)

The two variants alternate call by call in one process (a fresh batch per variant, kept for all
calls; the rollout batch is reset before each call so that every call runs whole episodes):
--warmup calls of each first, then --repeats timed pairs, host clock around the synchronous
call. Prints one JSON line per shape (medians and every sample) and appends it to --out.
With --only eval|rollout one variant runs alone (for a kernel trace of its own)."""
import argparse
import json
import pathlib
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--lanes", type=int, default=65536)
ap.add_argument("--episode-len", type=int, default=128)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--shapes", default="bk8,nakamoto")
ap.add_argument("--only", choices=["eval", "rollout"], default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402

from cpr_amd import _lib as L, device  # noqa: E402

N, T = args.lanes, args.episode_len
N_ALPHA = 20
ALPHAS = [0.05 + 0.02 * i for i in range(N_ALPHA)]  # 0.05 .. 0.43
EPA = N // N_ALPHA  # 3,276 at 65,536 lanes: one round of the lanes
SHAPES = {
    "bk8": dict(cfg=dict(protocol=L.PROTO_BK, k=8, gamma=0.5, seed=7), width=64),
    "nakamoto": dict(cfg=dict(protocol=L.PROTO_NAKAMOTO, gamma=0.5, propagation_delay=1e-9, seed=7),
                     width=256),
}
DEPTH = 3
ctx = device.default_context()


def random_net(n_in, width, n_act, extra):
    rng = np.random.default_rng(1)

    def lin(n_out, fan_in):
        return ((rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                (0.1 * rng.standard_normal(n_out)).astype(np.float32))

    def trunk():
        return [lin(width, n_in if i == 0 else width) for i in range(DEPTH)]

    return device.PolicyNet(pi=trunk(), pi_head=lin(n_act, width), vf=trunk(),
                            vf_head=lin(1, width), extra=extra)


def make_batch(sh, schedule):
    cfg, keep = device.make_config(n_lanes=N, alpha=0.33, max_steps=T, **sh["cfg"])
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    ol, na = b.observation_spec()[:2]
    b.set_lane_env(alphas=ALPHAS, alpha_column=0, reward="sparse_relative", shape="per_alpha",
                   schedule=schedule)
    b.set_policy_net(random_net(ol + 2, sh["width"], na, (0.33, 0.5)))
    return b


def host_binned(b):
    """The parent commit's route: step arrays to the host, episodes binned by alpha there."""
    b.reset()
    _, a = b.rollout_net(T, deterministic=True, outputs=True)
    done = a["done"]
    alpha = np.concatenate([a["alpha0"][None], a["alpha"][:-1]])  # of the step's own episode
    # episode reward: the sum of a lane's rewards since its previous done
    csum = np.cumsum(a["reward"], axis=0)
    t_idx, lane = np.nonzero(done)
    order = np.lexsort((t_idx, lane))
    t_idx, lane = t_idx[order], lane[order]
    end = csum[t_idx, lane]
    prev = np.concatenate([[0.0], end[:-1]])
    prev[np.concatenate([[True], lane[1:] != lane[:-1]])] = 0.0
    ep_reward, ep_alpha = end - prev, alpha[t_idx, lane]
    out = {}
    for x in ALPHAS:
        r = ep_reward[ep_alpha == x]
        out[x] = (r.size, float(r.mean()) if r.size else float("nan"),
                  float(r.std(ddof=1)) if r.size > 1 else float("nan"))
    return out


def timed(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def shape_case(name):
    sh = SHAPES[name]
    calls = {}
    if args.only != "rollout":
        be = make_batch(sh, "cycle")
        calls["eval"] = lambda: be.evaluate_net(EPA, records=False)
    if args.only != "eval":
        br = make_batch(sh, "choice")
        calls["rollout"] = lambda: host_binned(br)
    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    walls = {k: [] for k in calls}
    last = {}
    for _ in range(args.repeats):
        for k, fn in calls.items():  # alternating
            w, last[k] = timed(fn)
            walls[k].append(w)
    out = dict(shape=name, lanes=N, episode_len=T, n_alpha=N_ALPHA, episodes_per_alpha=EPA,
               episodes=EPA * N_ALPHA, repeats=args.repeats)
    if "eval" in calls:
        res = last["eval"]
        assert res.total.episodes == EPA * N_ALPHA and res.total.steps == EPA * N_ALPHA * T
        assert all(d["n"] == EPA for d in res.per_alpha)
        out.update(eval_wall_s=statistics.median(walls["eval"]), eval_samples_s=walls["eval"],
                   eval_kernel_ms=be.last_launch()[0],
                   eval_env_steps_per_s=EPA * N_ALPHA * T / statistics.median(walls["eval"]),
                   eval_mean_reward=[d["mean_episode_reward"] for d in res.per_alpha])
    if "rollout" in calls:
        assert sum(v[0] for v in last["rollout"].values()) == N
        out.update(rollout_wall_s=statistics.median(walls["rollout"]),
                   rollout_samples_s=walls["rollout"],
                   rollout_mean_reward=[last["rollout"][x][1] for x in ALPHAS])
    if len(calls) == 2:
        out["rollout_over_eval"] = out["rollout_wall_s"] / out["eval_wall_s"]
    return out


for name in args.shapes.split(","):
    row = shape_case(name)
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
