"""Crafted executing plans and a clock list for the 100 Hz publisher (dftpav_planner_publish): ten slots on the free lanes of the
default arena (replan_scenes.LANES) that put the cases of TrajPlannerServer::PublishData's trajectory feedback
(traj_server_ros.cpp:240-289) side by side.  `generate` is the MINCO generator the plans are built with, as in replan_scenes.

Every clock and every start time is a multiple of 1 / 2048 s near 100 s and every segment lasts a multiple of 1.5 s, so the
chained end times are exact and a clock can be put exactly on one.

The clocks:
  ticks 0 .. 271      T0 + k / 2048: finer than the publisher's 100 Hz, inside the 0.18 s around the gear shift of slot 6 in
                      which its plan is slower than 0.1 m/s.  Tick 128 is exactly that gear shift.  With the slot's seeded history
                      0.3 rad off, the filter fires on every one of these ticks: the run straddles ticks 255 | 256, the boundary
                      between the kernel's first and second chunk of CHUNK = 256 ticks.
  then, coarse        100.25, 100.5 (end of segment 0 of slot 1, exactly), 100.75 (start of slot 5, exactly), 101.0 (end of slot
                      7), 106.0 (a whole segment of slots 1, 2 and 4 later), 106.25, 100.9375 (a clock that goes back, into the plan of slot 7 again), 106.5, 107.0,
                      109.5, 110.0, 110.25 (end of slot 2), 111.0

crafted(generate) returns a dict:
  slots     list of None (empty) or dict(singul [M], piece_nums [M], coeff_dt [M], coeffs [Ntot][6][2], end_state [4], t_start,
            ctrl_hist = None or (stamp, angle))
  clocks    [K] the full list; CHUNK + 1 of them and the first alone are the two other calls of the tests
  split     where the tests cut the list into two consecutive calls (inside the run of filtered ticks, off the chunk boundary)
  expect    slot -> the case it is there for (tests/test_publish_oracle.py holds the oracle to it)
"""
import numpy as np

from . import replan_scenes as rs

N_SLOTS = 10
T0 = 100.0
CHUNK = 256                     # DFTPAV_PUBLISH_CHUNK
FINE = 1.0 / 2048.0
N_FINE = 272
GEAR_SHIFT = T0 + 128 * FINE    # of slot 6: tick 128
COARSE = (100.25, 100.5, 100.75, 101.0, 106.0, 106.25, 100.9375, 106.5, 107.0, 109.5, 110.0, 110.25, 111.0)
SPLIT = 200


def plan_rest(generate, lane):
    """one forward segment of 4 x 1.5 s along a lane towards -x (heading pi), 12 m, from rest to rest: boundary speeds exactly 0"""
    y = rs.LANES[lane]
    return rs._plan([rs._segment(generate, (-40.0, y), (-52.0, y), 4, 1.5, 1, 0.0, 0.0)])


def clocks():
    return np.array([T0 + k * FINE for k in range(N_FINE)] + list(COARSE))


def crafted(generate):
    slots, expect = [None] * N_SLOTS, {}

    def put(s, plan, t_start, case, ctrl_hist=None):
        plan["t_start"], plan["ctrl_hist"] = float(t_start), ctrl_hist
        slots[s], expect[s] = plan, case

    put(0, rs.plan_a(generate, 1), 99.5, "inside_segment", ctrl_hist=(T0 - 0.01, 0.0))          # 0.5 to 11.5 s into its 12 s
    put(1, rs.plan_c(generate, 2), 96.0, "end_time_exact")                                      # segments end at 100.5, 105, 109.5
    put(2, rs.plan_c(generate, 2), 96.75, "one_step_per_tick")                                  # 101.25, 105.75, 110.25: 101.0 -> 106.0
    put(3, rs.plan_a(generate, 0), 101.5, "before_start")                                       # 287 - 9 ticks before its start
    put(4, rs.plan_c(generate, 0), 94.0, "reverse_segment")                                     # segment 1 from 98.5 to 103
    put(5, plan_rest(generate, 1), 100.75, "standstill_on_start")                               # atan2(0, 0) against heading pi
    put(6, rs.plan_b(generate, 2), GEAR_SHIFT - 6.0, "gear_shift_run", ctrl_hist=(T0 - FINE, 0.3))
    put(7, rs.plan_a(generate, 1), 89.0, "completes_mid_call")                                  # ends at 101.0, then silent
    expect[8] = "empty"
    put(9, rs.plan_b(generate, 0), 97.0, "no_history")                                          # the first tick creates it
    return dict(slots=slots, clocks=clocks(), split=SPLIT, expect=expect)


def padded(scene, max_seg=8, max_pieces=64):
    """the occupied slots as the padded arrays dftpav_planner_install takes (replan_scenes.padded)"""
    return rs.padded(scene, max_seg, max_pieces)
