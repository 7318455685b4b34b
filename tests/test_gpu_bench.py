"""bench.py on the GPU: a plain run does the timed sweep alone, and --dump-outputs writes
the per-point summaries of its last timed step, which equal the library's own synchronous
run of the same episode range word for word."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cpr_amd import device

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

EPISODES = 4096
STEPS = 2


def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(STEPS), "--warmup", "1", "--episodes", str(EPISODES),
                        "--dump-outputs", str(out)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == STEPS and d["ms_per_step"] > 0 and d["full"] is False
    npts = len(bench.ALPHAS) * len(bench.GAMMAS)
    assert round(d["episodes_per_s"] * d["ms_per_step"] * STEPS / 1e3) == npts * EPISODES * STEPS
    # what takes runs of its own is behind --full
    for k in ("cpu_baseline", "other_configs", "abstract_gamma_1"):
        assert k not in d, k

    arrs = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(arrs) == {"points", "summary", "summary_hi32", "summary_lo32", "mean_rel_revenue"}
    assert all(a.dtype == np.float64 for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) < 64 << 20
    pts = [(a, g) for g in bench.GAMMAS for a in bench.ALPHAS]
    assert arrs["points"].tolist() == [list(p) for p in pts]
    words = (arrs["summary_hi32"].astype(np.uint64) << np.uint64(32)) \
        | arrs["summary_lo32"].astype(np.uint64)
    assert words.shape[0] == npts
    # the last timed step of one rank runs episodes [(STEPS - 1) * E, STEPS * E) of every point
    for i in (0, len(bench.ALPHAS) - 1, len(bench.ALPHAS), npts - 1):
        a, g = pts[i]
        cfg, keep = device.make_config(alpha=a, gamma=g, max_steps=bench.STEPS_PER_EPISODE,
                                       seed=bench.SEED)
        b = device.Batch(cfg, keep=keep)
        try:
            s = b.run(EPISODES, first_episode=(STEPS - 1) * EPISODES)
        finally:
            b.close()
        assert s.episodes == EPISODES
        assert words[i].view(np.int64).tolist() == s.to_array().tolist(), (a, g)
        assert arrs["mean_rel_revenue"][i, 0] == s.rel_revenue_fx / 2**32 / EPISODES
