"""Time of the device policy evaluation (cpr_mdp_policy_evaluation) against the host
restatement (cpr_amd.mdp.policy_evaluation, numpy, on the same machine's CPU) on the SSZ'16
Bitcoin model: 9 alpha (.05 ... .45) x 3 gamma (0, .5, 1) points x (the 27 optima + honest +
SM1) policies = 783 evaluations per cut-off in one call per path, horizon 100, theta 1e-6, and
one evaluation (the optimum of alpha .35, gamma .5 at its own point) alone.

Per cut-off and path (resident, resident with CPR_MDP_PE_REREAD=1, global, auto): --warmup
calls, then --repeats timed ones; medians are reported. A call's wall time is a host clock
around mdp.policy_evaluation_device over packed MDPs (checks, reachability walks, re-layout,
upload, every launch, download); kernel_ms is the call's HIP events around its launches. The
host figure is ONE evaluation timed (the same single one) and SCALED by the number of
evaluations; it is marked as scaled. Every device result of the single evaluation is compared
with the host's, bit for bit.

Writes one JSON document to --json and prints it."""
import argparse
import json
import os
import pathlib
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=str(pathlib.Path(__file__).resolve().parent.parent))
ap.add_argument("--cutoffs", default="20,40")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--json", default="profiles/mdp_pe_speed.json")
args = ap.parse_args()

sys.path.insert(0, args.tree)
import numpy as np  # noqa: E402

from cpr_amd import device, mdp  # noqa: E402

ALPHAS = [round(0.05 * i, 2) for i in range(1, 10)]
GAMMAS = [0.0, 0.5, 1.0]
HORIZON, THETA = 100, 1e-6
ctx = device.default_context()


def timed(tabs, pols, starts, path, reread=False):
    if reread:
        os.environ["CPR_MDP_PE_REREAD"] = "1"
    try:
        wall, kern, r = [], [], None
        for i in range(args.warmup + args.repeats):
            t = time.perf_counter()
            r = mdp.policy_evaluation_device(tabs, pols, theta=THETA, start=starts, path=path,
                                             ctx=ctx)
            if i >= args.warmup:
                wall.append((time.perf_counter() - t) * 1e3)
                kern.append(r[0]["pe_kernel_ms"])
    finally:
        os.environ.pop("CPR_MDP_PE_REREAD", None)
    return dict(wall_ms=statistics.median(wall), wall_ms_min=min(wall), wall_ms_max=max(wall),
                kernel_ms=statistics.median(kern), runs=len(wall), path_used=r[0]["pe_path"],
                sweeps_max=max(x["pe_iter"] for x in r),
                sweeps_mean=statistics.mean(x["pe_iter"] for x in r)), r


def variants(tabs, pols, starts, host=None):
    out = {}
    for name, path, reread in [("resident", "resident", False),
                               ("resident_reread", "resident", True),
                               ("global", "global", False), ("auto", "auto", False)]:
        out[name], r = timed(tabs, pols, starts, path, reread)
        if host is not None:
            out[name]["equals_host"] = bool(
                r[0]["pe_iter"] == host["pe_iter"]
                and r[0]["pe_reward"].tobytes() == host["pe_reward"].tobytes()
                and r[0]["pe_progress"].tobytes() == host["pe_progress"].tobytes())
    fastest = min(("resident", "global"), key=lambda k: out[k]["wall_ms"])
    out["auto_chose"] = out["auto"]["path_used"]
    out["fastest_path"] = fastest
    out["auto_is_fastest"] = out["auto_chose"] == fastest
    out["auto_loss"] = out[out["auto_chose"]]["wall_ms"] / out[fastest]["wall_ms"] - 1.0
    return out


doc = dict(tool="tools/mdp_pe_speed.py", horizon=HORIZON, theta=THETA, alphas=ALPHAS,
           gammas=GAMMAS, repeats=args.repeats, warmup=args.warmup, cutoffs=[])
for cutoff in (int(c) for c in args.cutoffs.split(",")):
    solved = mdp.solve_grid(ALPHAS, GAMMAS, maximum_fork_length=cutoff, horizon=HORIZON, ctx=ctx)
    model, states, _vi = solved[0]
    tabs = [mdp.pack(mdp.ptmdp(mdp.compile_mdp(m)[1], HORIZON)) for m, _s, _v in solved]
    starts = [[(0, m.alpha), (1, 1 - m.alpha)] for m, _s, _v in solved]
    pols = [np.asarray(vi["vi_policy"], np.int64) for _m, _s, vi in solved]
    for table in (mdp.fc16_honest_table(cutoff + 1), mdp.fc16_sm1_table(cutoff + 1)):
        pols.append(mdp.mdp_policy_from_table(model, states, table, "fc16"))
    one = ALPHAS.index(0.35) * len(GAMMAS) + GAMMAS.index(0.5)
    t = time.perf_counter()
    host = mdp.policy_evaluation(tabs[one], pols[one], theta=THETA, start=starts[one])
    host_ms = (time.perf_counter() - t) * 1e3
    S, A, T = tabs[0]["dst"].shape
    E = len(pols) * len(tabs)
    row = dict(cutoff=cutoff, states=S, action_slots=A, transition_slots=T, evaluations=E,
               host_one_evaluation_ms=host_ms, host_one_evaluation_sweeps=host["pe_iter"],
               host_all_ms_scaled=host_ms * E, host_scaled=True,
               all=variants(tabs, pols, starts),
               single=variants(tabs[one], [pols[one]], starts[one], host))
    for k in ("all", "single"):
        n = E if k == "all" else 1
        for v in ("resident", "resident_reread", "global"):
            row[k][v]["speedup_vs_host"] = host_ms * n / row[k][v]["wall_ms"]
    doc["cutoffs"].append(row)

text = json.dumps(doc, indent=1)
pathlib.Path(args.json).parent.mkdir(parents=True, exist_ok=True)
pathlib.Path(args.json).write_text(text + "\n")
print(text)
