"""Times the 100 Hz publisher on 1 024 installed plans: dftpav_planner_publish of 5 ticks (one planner period at 100 Hz) and of 500
ticks, the kernel from the planner's own events (dftpav_publish_last_ms) and the whole call by the host's clock, best of 3 after a
warm-up.  Beside it the host alternative it replaces: dftpav_planner_executing per slot plus a numpy evaluation of the same ticks
(positions, velocities, accelerations and the derived fields, no filter chain).  Prints the numbers; asserts nothing.

    python scripts/publish_time.py [--slots 1024]

The plans are the crafted lanes of dftpav_amd/replan_scenes.py started at staggered times."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dftpav_amd import capi, replan_scenes as rs      # noqa: E402
from oracle import pyoracle as po                     # noqa: E402  (only its MINCO generator, to build the plans)


def host_publish(pl, slots, clocks, wheel_base=2.85):
    """the table read back slot by slot, every tick evaluated with numpy (the segment from the clock, no state kept)"""
    K = len(clocks)
    states = np.zeros((K, slots, 8))
    for s in range(slots):
        ex = pl.executing(s)
        M = ex["n_seg"]
        if M == 0:
            continue
        seg = np.minimum(np.searchsorted(ex["end_time"][:M], clocks, side="right"), M - 1)
        t = np.minimum(clocks - ex["start_time"][seg], ex["duration"][seg])
        dtp, N = ex["coeff_dt"][seg], ex["piece_nums"][seg]
        idx = np.clip(np.ceil(t / dtp).astype(np.int64) - 1, 0, N - 1)
        tt = t - idx * dtp
        p0 = np.concatenate([[0], np.cumsum(ex["piece_nums"][:M])])[seg]
        c = ex["coeffs"][p0 + idx]                                   # [K][6][2]
        pw = tt[:, None] ** np.arange(6)[None]
        pos = np.einsum("kj,kjd->kd", pw, c)
        vel = np.einsum("kj,kjd->kd", pw[:, :5] * np.arange(1, 6), c[:, 1:])
        acc = np.einsum("kj,kjd->kd", pw[:, :4] * (np.arange(2, 6) * np.arange(1, 5)), c[:, 2:])
        sg = ex["singul"][seg]
        v = sg * np.hypot(vel[:, 0], vel[:, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            curv = np.where(np.abs(v) < 1e-6, 0.0, (vel[:, 0] * acc[:, 1] - vel[:, 1] * acc[:, 0]) / v ** 3)
            ac = np.where(np.abs(v) < 1e-6, 0.0, (vel * acc).sum(1) / v)
        states[:, s] = np.stack([clocks, pos[:, 0], pos[:, 1], np.arctan2(sg * vel[:, 1], sg * vel[:, 0]), curv, v, ac,
                                 np.arctan(wheel_base * curv)], 1)
    return states


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1024)
    a = ap.parse_args()
    capi.build()
    h = capi.Handle()
    pl = capi.Planner(h, a.slots, 1)
    makers = (rs.plan_a, rs.plan_b, rs.plan_c)
    t_now = rs.T_NOW
    plans = []
    for s in range(a.slots):
        p = makers[s % 3](po.minco_generate, s % 3)
        p["t_start"] = t_now - 1.0 - 0.001 * s
        plans.append(p)
    pad = rs.padded(dict(slots=plans))

    def install():
        for k in range(a.slots):
            sl = slice(k, k + 1)
            pl.install(pad["slots"][sl], pad["n_seg"][sl], pad["singul"][sl], pad["piece_nums"][sl], pad["coeff_dt"][sl], pad["coeffs"][sl],
                       pad["end_states"][sl], t_start=pad["t_start"][k])

    for K in (5, 500):
        clocks = t_now + 0.01 * np.arange(K)
        kern, call, host = [], [], []
        for rep in range(4):                            # the first one is the warm-up
            install()                                   # every call starts from the same publisher state
            t0 = time.perf_counter()
            out = pl.publish(clocks)
            t1 = time.perf_counter()
            ms = pl.publish_last_ms()
            t2 = time.perf_counter()
            host_publish(pl, a.slots, clocks)
            t3 = time.perf_counter()
            if rep:
                kern.append(ms)
                call.append(1e3 * (t1 - t0))
                host.append(1e3 * (t3 - t2))
        print("slots %d, %d ticks: published %d of %d rows" % (a.slots, K, int((out["published"] > 0).sum()), K * a.slots))
        print("  publish_kernel (events): best %.3f ms of %s" % (min(kern), ["%.3f" % v for v in kern]))
        print("  dftpav_planner_publish, the call with its read-back (host clock): best %.3f ms of %s" % (min(call), ["%.3f" % v for v in call]))
        print("  host alternative, dftpav_planner_executing per slot + numpy: best %.1f ms of %s" % (min(host), ["%.1f" % v for v in host]))
    pl.close()
    h.close()


if __name__ == "__main__":
    main()
