"""Device time of joint selection's pair, greedy and row kernels (dftpav_joint_last_ms through dftpav_debug_joint_select) beside the CPU
oracle on one core, for Q = 64, R = 16 and Q = 1024, R = 4 at K = 64: straight plans of conflict_scenes.straight_plans, one per
candidate, their poses from the candidate oracle; costs random, all eligible; margin 0.5, range 2.0; best of 3 after a warm-up.
The pose kernels and a whole dftpav_plan_queries call are not timed here: straight plans do not come out of a search and a solve.

    python scripts/joint_select_time.py [--extent-per-candidate 12]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from dftpav_amd import capi, conflict_scenes as cs  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from oracle_conflict import pycandidate as pcand, pyjoint as pj  # noqa: E402

DT, K, MARGIN, RANGE = 0.15, 64, 0.5, 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--extent-per-candidate", type=float, default=12.0)
    a = ap.parse_args()
    h = capi.Handle()
    for Q, R in ((64, 16), (1024, 4)):
        C = Q * R
        rng = np.random.default_rng(C)
        plans = cs.straight_plans(po.minco_generate, rng, C, a.extent_per_candidate * np.sqrt(C), t_start=0.0)
        co, dts = np.stack([p["coeffs"] for p in plans]), np.stack([p["coeff_dt"] for p in plans])
        poses = pcand.poses(plans[0]["singul"], plans[0]["piece_nums"], dts, co, 0.0, 0.0, DT, K, order=2).reshape(K, Q, R, 4)
        cost, elig = rng.uniform(0.0, 1.0, (Q, R)), np.ones((Q, R), np.int32)
        got = capi.debug_joint_select(h, poses, cost, elig, MARGIN, RANGE)
        runs = []
        for _ in range(3):
            capi.debug_joint_select(h, poses, cost, elig, MARGIN, RANGE)
            runs.append(h.joint_last_ms())
        _, pair_ms, select_ms = min(runs, key=lambda r: r[1] + r[2])
        t = time.perf_counter()
        ref = pj.select(poses, cost, elig, MARGIN, RANGE, order=2)
        oracle_s = time.perf_counter() - t
        same = all(np.array_equal(got[k], ref[k]) for k in ("winner", "blocked") + pj.FIELDS)
        print(json.dumps(dict(Q=Q, R=R, K=K, pair_ms=pair_ms, select_ms=select_ms, oracle_s=oracle_s, blocked=int(ref["blocked"].sum()),
                              without_plan=int((ref["winner"] < 0).sum()), equal_oracle=bool(same))))
    h.close()


if __name__ == "__main__":
    main()
