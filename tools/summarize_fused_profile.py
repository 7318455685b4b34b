"""Per-kernel summary of a rocprofv3 kernel trace and PMC pass of bench.py's sweep, for the
two timed k_run_episodes instantiations and k_run_episodes_fused: launches, mean ms per
launch and per sweep point, and VALU / SALU wave instructions per point-activation.

Usage: python tools/summarize_fused_profile.py KERNEL_STATS.csv COUNTER_COLLECTION.csv \
           [--episodes 5242880] [--max-steps 2016] > summary.json
A fused launch's points are read from its template arguments (k_run_episodes_fused<POL, NA>).
"""
import argparse
import csv
import json
import re
import sys
from collections import defaultdict


def short(name):
    m = re.search(r"k_run_episodes(_fused)?<([^>]*)>", name)
    if not m:
        return None, 0
    args = [a.strip() for a in m.group(2).split(",")]
    if m.group(1):
        # <POL, NA, ARR, G>: NA points per lane, G lanes per episode (before lane groups: no G)
        lanes = int(args[3]) if len(args) > 3 else 1
        return f"k_run_episodes_fused<{', '.join(args)}>", int(args[1]) * lanes
    return f"k_run_episodes<{', '.join(args)}>", 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("stats")
    ap.add_argument("counters")
    ap.add_argument("--episodes", type=int, default=5242880)
    ap.add_argument("--max-steps", type=int, default=2016)
    a = ap.parse_args()
    acts = a.episodes * (a.max_steps + 1)  # per point and launch: every gym episode is this long
    out = {"episodes_per_point": a.episodes, "activations_per_point": acts, "kernels": {}}
    for r in csv.DictReader(open(a.stats)):
        k, na = short(r["Name"])
        if k is None or "ListSource" in k:
            continue
        ms = float(r["AverageNs"]) / 1e6
        out["kernels"][k] = {"points_per_launch": na, "launches": int(r["Calls"]),
                             "ms_per_launch": ms, "ms_per_point": ms / na}
    sums = defaultdict(lambda: defaultdict(float))
    disp = defaultdict(set)
    regs = {}
    for r in csv.DictReader(open(a.counters)):
        k, na = short(r["Kernel_Name"])
        if k is None or k not in out["kernels"]:
            continue
        sums[k][r["Counter_Name"]] += float(r["Counter_Value"])
        disp[k].add(r["Dispatch_Id"])
        regs[k] = (int(r["LDS_Block_Size"]), int(r["Scratch_Size"]))
    for k, c in sums.items():
        e = out["kernels"][k]
        n = len(disp[k])
        per = acts * e["points_per_launch"] * n
        e["pmc_dispatches"] = n
        e["lds_bytes"], e["scratch_bytes"] = regs[k]
        # the counters count wave instructions: one per 64 lanes
        e["valu_wave_instr_per_point_activation"] = c["SQ_INSTS_VALU"] * 64 / per
        e["salu_wave_instr_per_point_activation"] = c["SQ_INSTS_SALU"] * 64 / per
        if c.get("SQ_WAVE_CYCLES"):
            e["wave_cycles_per_point_activation"] = c["SQ_WAVE_CYCLES"] * 64 / per
        if c.get("SQ_WAVES"):
            e["waves_per_launch"] = c["SQ_WAVES"] / n
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
