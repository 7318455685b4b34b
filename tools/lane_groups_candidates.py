"""One candidate grouping of bench.py's sweep at one gamma: the ten alphas as one group sweep
(ten cpr_run_episodes_async calls, one synchronize), a warm-up sweep and then --sweeps timed
ones. Prints one JSON line: wall ms per point of every sweep, the kernel ms per point the
library reports (cpr_last_launch) and every member's launch shape.

The grouping comes from the environment the library reads (CPR_NAK_FUSE, CPR_NAK_FUSE_LANES)
and the library from CPR_HIP_LIB (tools/build_variants.py builds variants, e.g. one point
per lane in groups of eight lanes: --def na1g8 kernels_nak_fused.hip
CPR_NAK_FUSE_MAX_ARR=1,CPR_NAK_FUSE_LANES_ARR=8), so one process measures one candidate:

  CPR_NAK_FUSE_LANES=1 python tools/lane_groups_candidates.py --gamma 0.5 \
      --tag "2 x 1, five launches"
  CPR_HIP_LIB=build/var/na1g8.so python tools/lane_groups_candidates.py --gamma 0.5 --tag "1 x 8"
"""
import argparse
import ctypes
import json
import os
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ALPHAS = [0.05, 0.10, 0.15, 0.20, 0.25, 0.30, 0.35, 0.40, 0.45, 0.50]  # bench.py's


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gamma", type=float, required=True)
    ap.add_argument("--episodes", type=int, default=5242880)
    ap.add_argument("--max-steps", type=int, default=2016)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    import torch

    from cpr_amd import _lib as L
    from cpr_amd import device

    ctx = device.Context(0)
    batches = []
    for al in ALPHAS:
        cfg, keep = device.make_config(alpha=al, gamma=a.gamma, max_steps=a.max_steps,
                                       seed=0x5EED0000)
        batches.append(device.Batch(cfg, ctx=ctx, keep=keep))
    words = ctypes.sizeof(L.Summary) // 8

    def sweep(i):
        sums = [torch.zeros(words, dtype=torch.int64, device="cuda") for _ in batches]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b, s in zip(batches, sums):
            b.run_async(a.episodes, i * a.episodes, s.data_ptr())
        ctx.synchronize()
        dt = time.perf_counter() - t0
        return dt, [L.Summary.from_buffer_copy(s.cpu().numpy().tobytes()) for s in sums]

    sweep(1000)
    wall = []
    for i in range(a.sweeps):
        dt, sums = sweep(i)
        wall.append(round(dt * 1e3 / len(batches), 3))
    kms = [round(b.last_launch()[0], 3) for b in batches]
    out = {"tag": a.tag, "gamma": a.gamma, "lib": os.environ.get("CPR_HIP_LIB", "default"),
           "CPR_NAK_FUSE": os.environ.get("CPR_NAK_FUSE"),
           "CPR_NAK_FUSE_LANES": os.environ.get("CPR_NAK_FUSE_LANES"),
           "ms_per_point_wall": wall, "kernel_ms_per_point": kms,
           "launch_shape": [list(b.launch_shape()) for b in batches],
           # the last sweep's words, to compare candidates with one another
           "episodes": [int(s.episodes) for s in sums],
           "rel_revenue_fx": [int(s.rel_revenue_fx) for s in sums],
           "status_tie": [int(s.status_tie) for s in sums]}
    print(json.dumps(out))
    for b in batches:  # before their context: cpr_batch_destroy enters it
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
