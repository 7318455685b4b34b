"""The device learner against ground truth: PPO on the FC16 env (CPR_PROTO_FC16_ENV), the
network tabulated after every iteration (mdp.fc16_table_from_net) and the table's exact
expected episode reward (mdp.fc16_policy_value: no Monte Carlo noise) recorded beside the exact
values of honest play, SM1 and the value-iteration table. Every row also has `pto_revenue`: the
same table as a policy of the PTO-mapped MDP (mdp.mdp_policy_from_table), reward over progress
from the start states by mdp.policy_evaluation_device; DESIGN.md 4.8 tells the two apart.

alpha .4, gamma .5, horizon 25. The network is tabulated for a, h < --dim; on the table's
border (a or h = dim - 1) honest play replaces the network's action, as the MDP's
maximum_fork_length cuts the state space, so that the policy's chain is finite whatever the
network does. Reports the curve; gates on nothing. Prints one JSON line and writes it to
--out (default profiles/fc16_ppo_vs_optimum.json)."""
import argparse
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402

from cpr_amd import _lib as L, device, mdp, ppo  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lanes", type=int, default=4096)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--iterations", type=int, default=40)
ap.add_argument("--width", type=int, default=64)
ap.add_argument("--depth", type=int, default=2)
ap.add_argument("--dim", type=int, default=24)
ap.add_argument("--lr", type=float, default=1e-3)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--out", default=str(ROOT / "profiles" / "fc16_ppo_vs_optimum.json"))
args = ap.parse_args()
ALPHA, GAMMA, HORIZON, DIM = 0.4, 0.5, 25, args.dim


def honest(a, h):
    return mdp.FC16_OVERRIDE if a > h else (mdp.FC16_ADOPT if h > a else mdp.FC16_WAIT)


def sm1(a, h):
    if h > a:
        return mdp.FC16_ADOPT
    if h == 1 and a == 1:
        return mdp.FC16_MATCH
    if h == a - 1 and h >= 1:
        return mdp.FC16_OVERRIDE
    return mdp.FC16_WAIT


def table_of(fn):
    t = np.zeros((DIM, DIM, 3), np.uint8)
    for a in range(DIM):
        for h in range(DIM):
            t[a, h, :] = fn(a, h)
    return t.ravel()


def with_honest_border(table):
    t = np.array(table, np.uint8).reshape(DIM, DIM, 3)
    for x in range(DIM):
        t[DIM - 1, x, :] = honest(DIM - 1, x)
        t[x, DIM - 1, :] = honest(x, DIM - 1)
    return t.ravel()


def value(table):
    v, g = mdp.fc16_policy_value(ALPHA, GAMMA, HORIZON, table)
    return dict(reward=float(v), progress=float(g), reward_per_progress=float(v / g))


res = dict(setup=dict(alpha=ALPHA, gamma=GAMMA, horizon=HORIZON, lanes=args.lanes,
                      steps_per_iteration=args.steps, iterations=args.iterations,
                      network=f"{args.depth}x{args.width}", lr=args.lr, table_dim=DIM,
                      border="honest play where a or h = dim - 1"))
vi = mdp.fc16_table(ALPHA, GAMMA, dim=DIM, maximum_fork_length=DIM - 1, horizon=HORIZON)
FIXED = dict(honest=table_of(honest), sm1=with_honest_border(table_of(sm1)),
             value_iteration=with_honest_border(vi))
for name, fixed in FIXED.items():
    res[name] = value(fixed)

# the other measure: the table mapped onto the PTO-mapped MDP of the same cut-off
MODEL = mdp.BitcoinSM(ALPHA, GAMMA, DIM - 1)
STATES, TAB = mdp.compile_mdp(MODEL)
PTO = mdp.pack(mdp.ptmdp(TAB, HORIZON))
START = [(sid, p) for sid, (_s, p) in enumerate(MODEL.start())]


def pto_revenue(table, ctx):
    """Reward over progress of the table's MDP policy from the model's start states. A table
    that earns nothing stops in its first sweep (the stop asks the reward's delta alone), with
    no progress at the start states yet: 0, as mdp.revenue_matrix has it."""
    policy = mdp.mdp_policy_from_table(MODEL, STATES, table, "fc16")
    pe = mdp.policy_evaluation_device(PTO, [policy], theta=1e-6, start=START, ctx=ctx)[0]
    reward = sum(p * pe["pe_reward"][s] for s, p in START)
    progress = sum(p * pe["pe_progress"][s] for s, p in START)
    return float(reward / progress) if progress else 0.0


def main():
    """The GPU part. The batch and the context are closed before the interpreter exits, as
    bench.py closes its own: nothing of the library is left to module teardown."""
    ctx = device.Context(0)
    for name, fixed in FIXED.items():
        res[name]["pto_revenue"] = pto_revenue(fixed, ctx)
    cfg, keep = device.make_config(protocol=L.PROTO_FC16_ENV, alpha=ALPHA, gamma=GAMMA,
                                   horizon=HORIZON, max_steps=254, seed=args.seed,
                                   n_lanes=args.lanes, policy=L.FC16_POLICY_HONEST)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    rng = np.random.default_rng(args.seed)

    def lin(n_out, fan_in, scale=1.0):
        return ((scale * rng.standard_normal((n_out, fan_in)) / np.sqrt(fan_in)).astype(np.float32),
                np.zeros(n_out, np.float32))

    def trunk():
        return [lin(args.width, 3 if i == 0 else args.width) for i in range(args.depth)]

    b.set_policy_net(device.PolicyNet(pi=trunk(), pi_head=lin(4, args.width, 0.01), vf=trunk(),
                                      vf_head=lin(1, args.width)))
    opts = ppo.PPOOptions(n_epochs=4, minibatch=args.lanes * args.steps // 8, lr=args.lr,
                          ent_coef=0.01, gae_gamma=0.999, clip_range=0.2)
    table = with_honest_border(mdp.fc16_table_from_net(b.get_policy_net(), DIM, ctx=ctx))
    curve = [dict(iteration=0, **value(table), pto_revenue=pto_revenue(table, ctx))]
    for it, (summary, stats) in enumerate(ppo.train(b, args.iterations, args.steps, opts), 1):
        table = with_honest_border(mdp.fc16_table_from_net(b.get_policy_net(), DIM, ctx=ctx))
        row = value(table)
        row.update(pto_revenue=pto_revenue(table, ctx), iteration=it,
                   fused=b.rollout_net_fused(), episodes=int(summary.episodes),
                   policy_loss=stats["policy_loss"], value_loss=stats["value_loss"])
        curve.append(row)
        print(f"# {it}: E[reward] {row['reward']:.4f}  (honest {res['honest']['reward']:.4f}, sm1 "
              f"{res['sm1']['reward']:.4f}, vi {res['value_iteration']['reward']:.4f})",
              file=sys.stderr, flush=True)
    res["curve"] = curve
    line = json.dumps(res)
    print(line, flush=True)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")
    b.close()
    ctx.close()


if __name__ == "__main__":
    main()
