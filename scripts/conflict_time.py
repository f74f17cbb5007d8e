"""Device time of the conflict check between executing plans (dftpav_planner_check_conflicts, conflict.hip): 1 024 installed plans,
straight runs of 20 m across one another on open ground, dense enough that some percent of the pair-samples pass the broad phase;
K = 200 clocks at dt = 0.05.  pose_ms and pair_ms (pair and reduce kernels together) are the handle's own HIP events, best of 3 after a
warm-up.  Beside them: the share of pair-samples that reached the narrow phase, and the CPU oracle's time for the same table on one
core, for scale (its rows must equal the device's).

    python scripts/conflict_time.py [--slots 1024] [--samples 200] [--dt 0.05] [--extent 75] [--margin 0.5] [--range 2.0]

Prints one JSON line.  Its figures are quoted in docs/NEXT_ROWS.md 4.23 only."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from dftpav_amd import capi, conflict_scenes as cs, replan_scenes as rs  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from oracle_conflict import pyconflict as pc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--extent", type=float, default=75.0)
    ap.add_argument("--margin", type=float, default=0.5)
    ap.add_argument("--range", type=float, default=2.0)
    a = ap.parse_args()
    po.build()
    plans = cs.straight_plans(po.minco_generate, np.random.default_rng(1024), a.slots, a.extent, t_start=0.0)
    pad = rs.padded(dict(slots=plans), 1, 4)
    h = capi.Handle(capi.default_params())
    pl = capi.Planner(h, a.slots, 1)
    pl.install(pad["slots"], pad["n_seg"], pad["singul"], pad["piece_nums"], pad["coeff_dt"], pad["coeffs"], pad["end_states"], t_start=0.0)
    pose_ms, pair_ms = [], []
    for _ in range(4):                          # the first is the warm-up
        got = pl.check_conflicts(0.0, a.dt, a.samples, a.margin, a.range)
        ms = h.conflicts_last_ms()
        pose_ms.append(ms[0])
        pair_ms.append(ms[1])
    tab = pc.from_executing([pl.executing(s) for s in range(a.slots)])
    pc.lib()
    t = time.perf_counter()
    ref = pc.conflicts(*tab, 0.0, a.dt, a.samples, a.margin, a.range, order=2)
    oracle_s = time.perf_counter() - t
    same = all(np.array_equal(np.asarray(got[k]).view(np.int32 if k != "min_sep" else np.int64),
                              np.asarray(ref[k]).view(np.int32 if k != "min_sep" else np.int64)) for k in pc.FIELDS)
    print(json.dumps(dict(slots=a.slots, samples=a.samples, dt=a.dt, extent=a.extent, margin=a.margin, range=a.range,
                          pair_samples=ref["examined"], narrow_share=ref["inside"] / max(1, ref["examined"]),
                          conflicting_slots=int((got["conflict_sample"] >= 0).sum()), pose_ms=min(pose_ms[1:]), pair_ms=min(pair_ms[1:]),
                          oracle_one_core_s=oracle_s, equal_to_oracle=bool(same))))
    pl.close()
    h.close()
    assert same


if __name__ == "__main__":
    main()
