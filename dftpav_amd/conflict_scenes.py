"""Crafted executing plans for the conflict check (dftpav_planner_check_conflicts): 35 slots on open ground, for the default vehicle
(1.90 x 4.88, d_cr 1.015), in groups 200 m apart -- further than any range the cases use reaches -- so that every group is one case
of the definition on its own.  The plans are straight minimum-jerk trajectories built with replan_scenes' generator helpers;
`generate` is the MINCO generator the caller brings (the tests: the CPU oracle's).

crafted(generate) returns a dict:
  slots      list of None (empty) or the plan dicts of replan_scenes._plan, with t_start set
  t0, dt, K  the clocks of the check: 101 samples over [50 s, 60 s]
  cases      the (margin, range) pairs the tests run
  expect     slot -> the case it is there for (tests/test_conflict_oracle.py holds the oracle to it)
replan_scenes.padded(scene, max_seg, max_pieces) turns it into the arrays dftpav_planner_install takes.

straight_plans(generate, rng, n, extent) are n seeded straight runs across a square of side `extent`, for the tile-edge tests and the
timing script."""
import numpy as np

from .replan_scenes import _plan, _segment

T0, DT, K = 50.0, 0.1, 101
N_SLOTS = 35
MAX_SEG, MAX_PIECES = 2, 8
GROUP = 200.0                   # distance between the groups, along y
LANE_GAP = 3.0 - 1.90           # two lanes 3.0 m apart, side by side: 1.10 m between the flanks
HEAD_ON_K0 = 2 * (30.0 - 1.015) - 4.88    # head-on, rear axles at -30 and +30 facing one another: nose to nose at k = 0
# The broad phase compares CENTRE distances with R = range + 2 rad >= 5.24 m, so no range cuts off the side-by-side pair, whose
# centres are 3.0 m apart.  The pair a small range does cut off is the staggered one: the same lanes, one vehicle 4.6 m ahead of the
# other, the flanks still 1.10 m apart but the centres sqrt(3.0^2 + 4.6^2) = 5.49 m: outside R for range 0.0, inside for range 1.0.
STAGGER = 4.6
# margin = 0 with the range that cuts the staggered 1.10 m pair (and the 1.09 m nose-to-nose pairs) off; the range that sees them;
# one that sees every group whole
CASES = ((0.0, 0.0), (1.0, 1.0), (0.5, 60.0))


def _run(generate, p0, p1, t_start, seconds=10.0, n_pieces=5, singul=1):
    """a straight run from p0 to p1 at constant speed, `seconds` long"""
    d = float(np.hypot(p1[0] - p0[0], p1[1] - p0[1]))
    v = d / seconds              # boundary speeds are along the direction of motion; singul = -1: the vehicle faces the other way
    plan = _plan([_segment(generate, p0, p1, n_pieces, seconds / n_pieces, singul, v, v)])
    plan["t_start"] = float(t_start)
    return plan


def _held(generate, p_end, heading_deg, t_end):
    """a plan that ended at t_end (before the window) at p_end with the given heading: the vehicle is held there"""
    u = np.array([np.cos(np.radians(heading_deg)), np.sin(np.radians(heading_deg))])
    p1 = np.asarray(p_end, dtype=np.float64)
    return _run(generate, p1 - 6.0 * u, p1, t_end - 3.0, seconds=3.0, n_pieces=2)


def crafted(generate):
    slots, expect = [None] * N_SLOTS, {}

    def put(s, plan, case):
        slots[s], expect[s] = plan, case

    y = 0.0          # three lanes about y = 0, mirror images of one another: the middle one's partners tie, bit for bit
    put(0, _run(generate, (-20.0, 3.0), (20.0, 3.0), T0), "tie_upper")
    put(1, _run(generate, (-20.0, 0.0), (20.0, 0.0), T0), "tie_middle")
    put(2, _run(generate, (-20.0, -3.0), (20.0, -3.0), T0), "tie_lower")
    y = 1 * GROUP    # two parallel lanes 3.0 m apart, side by side
    put(4, _run(generate, (-20.0, y), (20.0, y), T0), "lanes")
    put(5, _run(generate, (-20.0, y + 3.0), (20.0, y + 3.0), T0), "lanes")
    y = 2 * GROUP    # head-on in one lane, closing from 53.09 m to 1.09 m
    put(7, _run(generate, (-30.0, y), (-4.0, y), T0), "head_on")
    put(8, _run(generate, (30.0, y), (4.0, y), T0), "head_on")
    y = 3 * GROUP    # crossing at right angles, both rear axles at the crossing at t = 55
    put(10, _run(generate, (-20.0, y), (20.0, y), T0), "crossing_hit")
    put(11, _run(generate, (0.0, y - 20.0), (0.0, y + 20.0), T0), "crossing_hit")
    y = 4 * GROUP    # the same with one plan 6 s later: it is held at its start while the other passes
    put(13, _run(generate, (-20.0, y), (20.0, y), T0), "crossing_miss")
    put(14, _run(generate, (0.0, y - 20.0), (0.0, y + 20.0), T0 + 6.0), "crossing_miss")
    y = 5 * GROUP    # a plan that ended before t0, held at its end, and one that drives into it from behind
    put(16, _held(generate, (0.0, y), 0.0, T0 - 15.0), "ended_before")
    put(17, _run(generate, (-30.0, y), (-2.0, y), T0), "drives_into_ended")
    y = 6 * GROUP    # a plan that starts after the last clock, held at its start; another passes 0.595 m from its nose
    put(19, _run(generate, (0.0, y), (20.0, y), T0 + 30.0), "starts_after")
    put(20, _run(generate, (5.0, y - 20.0), (5.0, y + 20.0), T0), "passes_waiting")
    y = 7 * GROUP    # a reversing vehicle (facing +x, moving -x) followed 8 m behind by one driving forward in -x: 1.09 m nose to nose
    put(22, _run(generate, (0.0, y), (-20.0, y), T0, singul=-1), "reversing")
    put(23, _run(generate, (8.0, y), (-12.0, y), T0), "follows_reversing")
    y = 8 * GROUP    # forward 10 m, then back 8 m: the gear shift at t0 + 5; a held vehicle 6.5 m ahead of the shift point
    shift = _plan([_segment(generate, (-10.0, y), (0.0, y), 4, 1.25, 1, 0.05, 0.05),
                   _segment(generate, (0.0, y), (-8.0, y), 4, 1.25, -1, 0.05, 0.05)])
    shift["t_start"] = T0
    put(25, shift, "gear_shift")
    put(26, _held(generate, (6.5, y), 0.0, T0 - 15.0), "ahead_of_shift")
    y = 9 * GROUP    # a held vehicle at 30 degrees above one at 0 degrees: its rear right corner over the other's left flank
    put(28, _held(generate, (0.0, y), 0.0, T0 - 15.0), "edge")
    put(29, _held(generate, (0.0, y + 3.5), 30.0, T0 - 15.0), "corner")
    y = 25 * GROUP   # alone
    put(31, _run(generate, (-20.0, y), (20.0, y), T0), "beyond_range")
    y = 10 * GROUP   # the two lanes again, one vehicle STAGGER ahead of the other
    put(33, _run(generate, (-20.0, y), (20.0, y), T0), "lanes_staggered")
    put(34, _run(generate, (-20.0 + STAGGER, y + 3.0), (20.0 + STAGGER, y + 3.0), T0), "lanes_staggered")
    return dict(slots=slots, t0=T0, dt=DT, K=K, cases=CASES, expect=expect)


def straight_plans(generate, rng, n, extent, t_start=0.0, seconds=10.0):
    """n straight runs of 20 m at constant speed, `seconds` long, from seeded starts in a square of side `extent` about the origin in
    seeded directions, all starting at t_start"""
    plans = []
    for _ in range(n):
        p0 = (rng.random(2) - 0.5) * extent
        a = rng.random() * 2.0 * np.pi
        plans.append(_run(generate, p0, p0 + 20.0 * np.array([np.cos(a), np.sin(a)]), t_start, seconds=seconds, n_pieces=4))
    return plans
