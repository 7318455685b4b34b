"""Golden vectors for cpr_amd.mdp.policy_evaluation / reachable_states from the reference's
own MDP toolbox.

Imports the reference's mdp/lib (numpy/scipy only), as make_mdp_fixture.py does, and records,
for the Sapirshtein FC'16 Bitcoin model at cut-offs 4 and 6, horizons 10 and 100 and three
(alpha, gamma) points, what explicit_mdp.policy_evaluation (:328-378) and reachable_states
(:179-208) give on the PTO-mapped MDP for
  vi        the value-iteration policy (stop_delta 1e-6), theta 1e-6
  first     the first-action policy (slot 0 wherever a state has an action), theta 1e-6
  vi_all    the value-iteration policy with around_state given: every state included
  vi_max5   the value-iteration policy stopped by max_iter = 5
as pe_reward and pe_progress in hex floats, pe_iter and the reachable set. Data only.

Run where the reference is, on the CPU:  python tests/golden/make_mdp_pe_fixture.py
"""

import json
import pathlib
import sys

sys.path.insert(0, "/root/reference/mdp")
from lib.compiler import Compiler  # noqa: E402
from lib.models import aft20barzur, fc16sapirshtein  # noqa: E402

OUT = pathlib.Path(__file__).with_name("mdp_policy_eval.json")
CUTOFFS, HORIZONS = (4, 6), (10, 100)
POINTS = [(0.3, 0.5), (0.1, 0.0), (0.45, 0.9)]
THETA = STOP_DELTA = 1e-6
MAX_ITER = 5


def main():
    cases = []
    for mfl in CUTOFFS:
        for horizon in HORIZONS:
            for alpha, gamma in POINTS:
                model = fc16sapirshtein.BitcoinSM(alpha=alpha, gamma=gamma,
                                                  maximum_fork_length=mfl)
                m = aft20barzur.ptmdp(Compiler(model).mdp(), horizon=horizon)
                vi = m.value_iteration(stop_delta=STOP_DELTA, eps=None, discount=1)
                vi_policy = [int(x) for x in vi["vi_policy"]]
                first = [0 if acts else -1 for acts in m.tab]
                evals = {}
                for name, policy, kw in [("vi", vi_policy, {}), ("first", first, {}),
                                         ("vi_all", vi_policy, dict(around_state=0)),
                                         ("vi_max5", vi_policy, dict(max_iter=MAX_ITER))]:
                    pe = m.policy_evaluation(policy, theta=THETA, discount=1, **kw)
                    evals[name] = dict(
                        policy=policy, states="all" if "around_state" in kw else "reachable",
                        max_iter=kw.get("max_iter"),
                        reachable=sorted(int(s) for s in m.reachable_states(policy)),
                        pe_reward=[float(x).hex() for x in pe["pe_reward"]],
                        pe_progress=[float(x).hex() for x in pe["pe_progress"]],
                        pe_iter=int(pe["pe_iter"]))
                cases.append(dict(alpha=alpha, gamma=gamma, maximum_fork_length=mfl,
                                  horizon=horizon, theta=THETA, stop_delta=STOP_DELTA,
                                  n_states=m.n_states,
                                  start=[[int(s), float(p)] for s, p in sorted(m.start.items())],
                                  vi_value=[float(x).hex() for x in vi["vi_value"]],
                                  evals=evals))
                print(mfl, horizon, alpha, gamma, m.n_states,
                      {k: (v["pe_iter"], len(v["reachable"])) for k, v in evals.items()})
    OUT.write_text(json.dumps({"source": "mdp/lib (fc16sapirshtein, compiler, aft20barzur.ptmdp,"
                                         " explicit_mdp.value_iteration, policy_evaluation,"
                                         " reachable_states)", "cases": cases}) + "\n")
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
