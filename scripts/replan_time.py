"""Times the replan loop on 1 024 installed plans: dftpav_replan_check alone, and a dftpav_replan_tick in which roughly a tenth of the
slots replan.  The planner's own events (dftpav_replan_last_ms), best of 3 after a warm-up.  Prints the numbers; asserts nothing.

    python scripts/replan_time.py [--slots 1024] [--restarts 4]

The plans are the crafted lanes of dftpav_amd/replan_scenes.py (straight minimum-jerk trajectories on a free stretch of the default
arena) started at staggered times, so that at the clock of the tick about a tenth of them are near their end with the goal moved."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dftpav_amd import capi, replan_scenes as rs      # noqa: E402
from oracle import pyoracle as po                     # noqa: E402  (only its MINCO generator, to build the plans)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--restarts", type=int, default=4)
    a = ap.parse_args()
    capi.build()
    scene = rs.crafted(po.minco_generate)
    h = capi.Handle()
    h.set_grid_map(scene["grid_before"], scene["resolution"], scene["origin"])
    pl = capi.Planner(h, a.slots, a.restarts)
    pp = capi.default_plan_params()
    makers = (lambda lane, off: rs.plan_a(po.minco_generate, lane, off), lambda lane, off: rs.plan_b(po.minco_generate, lane, off))
    t_now, budget = rs.T_NOW, rs.BUDGET
    goals = np.zeros((a.slots, 4))
    plans = []
    for s in range(a.slots):
        replans = s % 10 == 0                           # a tenth: 3 s left of a one-segment plan, the goal 1 m aside
        p = makers[0](s % 3, (0.0, 1.0) if replans else (0.0, 0.0)) if replans else makers[s % 2](s % 3, (0.0, 0.0))
        p["t_start"] = t_now - 9.0 if replans else t_now - 1.0 - 0.001 * s
        plans.append(p)
        goals[s] = p["end_state"]
    pad = rs.padded(dict(slots=plans))

    def install():
        for k in range(a.slots):
            sl = slice(k, k + 1)
            pl.install(pad["slots"][sl], pad["n_seg"][sl], pad["singul"][sl], pad["piece_nums"][sl], pad["coeff_dt"][sl], pad["coeffs"][sl],
                       pad["end_states"][sl], t_start=pad["t_start"][k])

    install()
    check_ms, tick_ms, flagged, planned = [], [], 0, 0
    for rep in range(4):                                # the first one is the warm-up
        out = pl.check(t_now, budget)
        c, _ = pl.replan_last_ms()
        install()                                       # every tick starts from the same table
        tk = pl.tick(t_now, budget, pp=pp)
        _, t = pl.replan_last_ms()
        flagged, planned = int(out["replan"].sum()), int((tk["plan"]["plan_status"] == capi.PLAN_OK).sum())
        if rep:
            check_ms.append(c)
            tick_ms.append(t)
    print("slots %d, restarts %d: flagged %d, planned %d" % (a.slots, a.restarts, flagged, planned))
    print("dftpav_replan_check, kernel: best %.3f ms of %s" % (min(check_ms), ["%.3f" % v for v in check_ms]))
    print("dftpav_replan_tick, check to adoption: best %.1f ms of %s" % (min(tick_ms), ["%.1f" % v for v in tick_ms]))
    print("stages of the tick's dftpav_plan_queries (search, resampling, groups, all) ms:", pl.info()["stage_ms"])
    pl.close()
    h.close()


if __name__ == "__main__":
    main()
