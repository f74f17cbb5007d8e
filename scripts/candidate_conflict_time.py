"""Device time of the candidate conflict check (dftpav_batch_check_conflicts) beside the table check's own
(dftpav_planner_check_conflicts) and the CPU oracle on one core: 1 024 installed straight plans, 1 024 x 32 candidates of one layout,
K = 200 clocks at dt = 0.05, margin 0.5, range 2.0; best of 3 after a warm-up, from the handle's HIP events.

    python scripts/candidate_conflict_time.py [--slots 1024] [--per-slot 32] [--oracle-candidates 64]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from dftpav_amd import capi, conflict_scenes as cs, replan_scenes as rs  # noqa: E402
from dftpav_amd.pods import LayoutSpec  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from oracle_conflict import pycandidate as pcand, pyconflict as pc  # noqa: E402

T0, DT, K, MARGIN, RANGE = 0.0, 0.05, 200, 0.5, 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--per-slot", type=int, default=32)
    ap.add_argument("--oracle-candidates", type=int, default=64)
    a = ap.parse_args()
    S, B = a.slots, a.slots * a.per_slot
    extent = 40.0 * np.sqrt(S)                                  # the density of tests/test_gpu_conflicts.py's edge scene, roughly
    plans = cs.straight_plans(po.minco_generate, np.random.default_rng(1), S, extent, t_start=T0)
    h = capi.Handle()
    pl = capi.Planner(h, S, 1)
    pad = rs.padded(dict(slots=plans), cs.MAX_SEG, cs.MAX_PIECES)
    pl.install(pad["slots"], pad["n_seg"], pad["singul"], pad["piece_nums"], pad["coeff_dt"], pad["coeffs"], pad["end_states"], t_start=T0)
    rng = np.random.default_rng(2)
    base = cs.straight_plans(po.minco_generate, rng, S, extent, t_start=T0)
    co = np.repeat(np.stack([p["coeffs"] for p in base]), a.per_slot, axis=0)
    co[:, :, 0, :] += rng.normal(0.0, 1.0, (B, 1, 2))          # every candidate a shifted copy
    dts = np.repeat(np.stack([p["coeff_dt"] for p in base]), a.per_slot, axis=0)
    bt = capi.Batch(h, LayoutSpec([4], [1], 4), B)
    bt.set_coeffs(co, dts)
    best = {}
    for name, call, ms in (("candidates", lambda: bt.check_conflicts(pl, T0, T0, DT, K, MARGIN, RANGE), h.batch_conflicts_last_ms),
                           ("table", lambda: pl.check_conflicts(T0, DT, K, MARGIN, RANGE), h.conflicts_last_ms)):
        call()
        runs = []
        for _ in range(3):
            call()
            runs.append(ms())
        best[name] = min(runs, key=lambda r: r[1])
    n = a.oracle_candidates
    t = time.perf_counter()
    ref = pcand.conflicts([1], [4], dts[:n], co[:n], T0, pc.from_executing([pl.executing(s) for s in range(S)]), T0, DT, K, MARGIN, RANGE, order=2)
    oracle_s = time.perf_counter() - t
    got = bt.check_conflicts(pl, T0, T0, DT, K, MARGIN, RANGE)
    same = all(np.array_equal(got[k][:n], ref[k]) for k in pc.FIELDS)
    print(json.dumps(dict(slots=S, candidates=B, K=K, pose_ms=best["candidates"][0], pair_ms=best["candidates"][1],
                          pair_samples_per_s=B * S * K / (best["candidates"][1] * 1e-3),
                          table_pose_ms=best["table"][0], table_pair_ms=best["table"][1],
                          table_pair_samples_per_s=S * (S - 1) * K / (best["table"][1] * 1e-3),
                          oracle_candidates=n, oracle_s=oracle_s, oracle_pair_samples_per_s=n * S * K / oracle_s, rows_equal_oracle=bool(same))))
    bt.close()
    pl.close()
    h.close()


if __name__ == "__main__":
    main()
