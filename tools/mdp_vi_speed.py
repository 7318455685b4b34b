"""Time of the device value iteration (cpr_mdp_value_iteration) against the host solver
(cpr_amd.mdp.value_iteration, numpy, on the same machine's CPU) on the SSZ'16 Bitcoin model:
every alpha in .05, .10 ... .45 (9 values; .50 is outside the model) x 3 gamma (0, .5, 1)
per cut-off, horizon 100, stop_delta 1e-6, as one
call per path, and one point (alpha .35, gamma .5) alone.

Per cut-off and path: --warmup calls, then --repeats timed ones. A call's wall time is a host
clock around Context.mdp_value_iteration over the packed arrays (validation, re-layout, upload,
every launch, download); kernel_ms is the call's HIP events around its launches. Model
compilation and packing are outside both (the host solver needs them too). The host solver runs
every point once (--host-points N: only the first N, the total scaled up and marked). Every
device result is compared with the host's, bit for bit.

Bytes streamed per sweep (resident path; value and progress stay in LDS): per point 4 bytes per
transition slot (dst), 1 per action slot (valid) and 24 per used transition (prb, rew, prg).
These are the bytes the sweep needs; the kernel also loads the zeros of unused slots (28 bytes
per slot in all).

Writes one JSON document to --json and prints it."""
import argparse
import json
import pathlib
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=str(pathlib.Path(__file__).resolve().parent.parent))
ap.add_argument("--cutoffs", default="20,40")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--host-points", type=int, default=0, help="0: every point")
ap.add_argument("--json", default="profiles/mdp_vi_speed.json")
args = ap.parse_args()

sys.path.insert(0, args.tree)
import numpy as np  # noqa: E402

from cpr_amd import device, mdp  # noqa: E402

ALPHAS = [round(0.05 * i, 2) for i in range(1, 10)]
GAMMAS = [0.0, 0.5, 1.0]
HORIZON, STOP = 100, 1e-6
ctx = device.default_context()


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def device_call(ms, path):
    first = ms[0]
    prb = np.stack([m["prb"] for m in ms])
    return ctx.mdp_value_iteration(first["dst"], first["used"], first["valid"], first["rew"],
                                   first["prg"], prb, stop_delta=STOP, path=path)


def timed(ms, path):
    for _ in range(args.warmup):
        device_call(ms, path)
    walls, kernels, r = [], [], None
    for _ in range(args.repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = device_call(ms, path)
        walls.append(time.perf_counter() - t0)
        kernels.append(r["kernel_ms"] * 1e-3)
    return r, walls, kernels


def equal(r, p, h):
    return (int(r["iter"][p]) == h["vi_iter"] and float(r["delta"][p]) == h["vi_delta"]
            and r["policy"][p].tolist() == h["vi_policy"].tolist()
            and r["value"][p].tobytes() == h["vi_value"].tobytes()
            and r["progress"][p].tobytes() == h["vi_progress"].tobytes())


def measure(ms, hosts, label):
    """Both paths over the MDPs ``ms`` (hosts: the host results of the first len(hosts))."""
    S, A, T = ms[0]["dst"].shape
    used = int((ms[0]["used"] & ms[0]["valid"][:, :, None]).sum())
    bytes_per_sweep = 4 * S * A * T + S * A + 24 * used
    out = dict(case=label, points=len(ms), states=S, action_slots=A, transition_slots=T,
               used_transitions=used, resident_bytes_per_point_sweep=bytes_per_sweep, paths={})
    for path in ("resident", "global"):
        r, walls, kernels = timed(ms, path)
        sweeps = int(r["iter"].sum())
        w, k = statistics.median(walls), statistics.median(kernels)
        row = dict(wall_s=spread(walls), kernel_s=spread(kernels), sweeps_total=sweeps,
                   sweeps_longest_point=int(r["iter"].max()),
                   point_sweeps_per_s_wall=sweeps / w, point_sweeps_per_s_kernel=sweeps / k,
                   equal_to_host=all(equal(r, p, h) for p, h in enumerate(hosts)),
                   compared_points=len(hosts))
        if path == "resident":
            row["streamed_bytes_per_s_kernel"] = bytes_per_sweep * sweeps / k
            # the longest point alone bounds the call: its workgroup's own rate
            row["longest_point_us_per_sweep"] = k / int(r["iter"].max()) * 1e6
            row["longest_point_bytes_per_s"] = bytes_per_sweep * int(r["iter"].max()) / k
        out["paths"][path] = row
    auto = device_call(ms, "auto")["path_used"]
    faster = min(out["paths"], key=lambda p: out["paths"][p]["wall_s"]["median"])
    wall = {p: out["paths"][p]["wall_s"]["median"] for p in out["paths"]}
    out.update(auto_path=auto, faster_path=faster, auto_is_faster=auto == faster,
               auto_over_faster_wall=wall[auto] / wall[faster])
    return out


doc = dict(tool="tools/mdp_vi_speed.py", horizon=HORIZON, stop_delta=STOP, alphas=ALPHAS,
           gammas=GAMMAS, repeats=args.repeats, warmup=args.warmup, grids=[], single=[])
for cutoff in (int(c) for c in args.cutoffs.split(",")):
    pts = [(a, g) for a in ALPHAS for g in GAMMAS]
    t0 = time.perf_counter()
    ms = []
    for a, g in pts:
        _states, tab = mdp.compile_mdp(mdp.BitcoinSM(a, g, cutoff))
        ms.append(mdp.pack(mdp.ptmdp(tab, HORIZON)))
    t_pack = time.perf_counter() - t0
    n_host = args.host_points or len(pts)
    hosts, host_s = [], []
    for m in ms[:n_host]:
        t0 = time.perf_counter()
        hosts.append(mdp.value_iteration(m, stop_delta=STOP))
        host_s.append(time.perf_counter() - t0)
    g = measure(ms, hosts, f"grid cut-off {cutoff}")
    host_total = sum(host_s) * len(pts) / n_host
    g.update(maximum_fork_length=cutoff, compile_and_pack_s=t_pack,
             host_s_per_point=spread(host_s), host_points_timed=n_host,
             host_total_s=host_total, host_total_extrapolated=n_host < len(pts),
             host_sweeps_per_s=sum(h["vi_iter"] for h in hosts) / sum(host_s))
    for path, row in g["paths"].items():
        row["host_over_device_wall"] = host_total / row["wall_s"]["median"]
    doc["grids"].append(g)
    print(json.dumps(g), flush=True)
    i = pts.index((0.35, 0.5))
    if i < n_host:
        s = measure([ms[i]], [hosts[i]], f"single point cut-off {cutoff}, alpha .35, gamma .5")
        s.update(maximum_fork_length=cutoff, host_s=host_s[i])
        for path, row in s["paths"].items():
            row["host_over_device_wall"] = host_s[i] / row["wall_s"]["median"]
        doc["single"].append(s)
        print(json.dumps(s), flush=True)

out = pathlib.Path(args.json)
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(json.dumps(doc, indent=1) + "\n")
