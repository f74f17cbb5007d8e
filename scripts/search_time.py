"""Timing of dftpav_kino_search: N default-arena queries (the ego start, goals drawn around it) in one call.

Reports the kernel time (HIP events around the launches), searches/s, the mean iteration count, and the CPU restatement
(oracle_search/, order 2, one core) on a subset for comparison.  Usage: python scripts/search_time.py [--n 1024] [--oracle 16]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dftpav_amd import capi, search_scenes as ss  # noqa: E402
from oracle_search import pysearch as ps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--oracle", type=int, default=16, help="queries the CPU restatement runs (one core)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    grid, res, org, start, _ = ss.arena()
    rng = np.random.default_rng(a.seed)
    r = rng.uniform(6.0, 14.0, a.n)
    ang = rng.uniform(-np.pi, np.pi, a.n)
    goals = np.stack([start[0] + r * np.cos(ang), start[1] + r * np.sin(ang), rng.uniform(-np.pi, np.pi, a.n), np.zeros(a.n)], 1)
    starts = np.repeat(start[None], a.n, 0)
    h = capi.Handle()
    h.set_grid_map(grid, res, org)
    out = h.kino_search(starts, goals)  # warm-up (workspace, code object)
    ms = []
    for _ in range(a.reps):
        o2 = h.kino_search(starts, goals)
        ms.append(h.corridor_last_ms())
        assert all(np.array_equal(out[k], o2[k]) for k in out)
    t0 = time.perf_counter()
    ref = ps.kino_search(grid, res, org, starts[:a.oracle], goals[:a.oracle], order=2, nthreads=1)
    cpu_s = time.perf_counter() - t0
    same = all(np.array_equal(out[k][:a.oracle], ref[k]) for k in ref)
    best = min(ms)
    res_ = dict(n=a.n, kernel_ms=best, kernel_ms_all=ms, searches_per_s=a.n / (best * 1e-3),
                mean_iters=float(out["iters"].mean()), max_iters=int(out["iters"].max()),
                reach_end=int((out["status"] == 2).sum()), budget_hit=int(out["budget_hit"].sum()),
                oracle_queries=a.oracle, oracle_s_one_core=cpu_s, oracle_iters=int(ref["iters"].sum()), oracle_bit_equal=bool(same))
    print(json.dumps(res_))
    h.close()


if __name__ == "__main__":
    main()
