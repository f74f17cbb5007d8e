"""Crafted executing plans for the conflict trigger (dftpav_planner_check_yield): 24 slots on open ground for the default vehicle, in
groups 200 m apart so that every group is one case of the definition on its own.  Built from conflict_scenes' _run and _held;
`generate` is the MINCO generator the caller brings (the tests: the CPU oracle's).

crafted(generate) returns a dict:
  slots      list of None (empty) or the plan dicts of replan_scenes._plan, with t_start set
  t0, dt, K  the clocks: 101 samples over [50 s, 60 s]
  t_nows     two clocks of the completion test: at the first every running plan is under way, at the second slot 21's has ended
  cases      the (margin, range) pairs the tests run
  expect     slot -> the case it is there for (tests/test_conflict_trigger_oracle.py holds the oracle to it)
replan_scenes.padded(scene, MAX_SEG, MAX_PIECES) turns it into the arrays dftpav_planner_install takes."""
from .conflict_scenes import DT, GROUP, K, MAX_PIECES, MAX_SEG, STAGGER, T0, _held, _run

N_SLOTS = 24
T_NOWS = (T0, T0 + 6.0)
# margin 0 with the range that cuts the staggered pair off; a margin with the smallest range it may have; the same with a range that
# sees every group whole
CASES = ((0.0, 0.0), (0.5, 0.5), (0.5, 60.0))
NOSE_GAP = 0.3                  # the head-on pair's gap at the last clock
HEAD_ON_END = 0.5 * (2 * (1.015 + 0.5 * 4.88) + NOSE_GAP)    # |x| of the rear axles then


def crafted(generate):
    slots, expect = [None] * N_SLOTS, {}

    def put(s, plan, case):
        slots[s], expect[s] = plan, case

    y = 0.0          # crossing at right angles, both under way: the higher slot yields, the lower meets only what it precedes
    put(0, _run(generate, (-20.0, y), (20.0, y), T0), "precedes_all")
    put(1, _run(generate, (0.0, y - 20.0), (0.0, y + 20.0), T0), "crossing_yields")
    y = 1 * GROUP    # a completed plan parked on the path of the LOWER slot: the lower slot yields
    put(3, _run(generate, (-30.0, y), (-2.0, y), T0), "drives_into_parked")
    put(4, _held(generate, (0.0, y), 0.0, T0 - 15.0), "parked_on_path")
    y = 2 * GROUP    # two completed plans overlapping: both rows name a partner, neither yields
    put(6, _held(generate, (0.0, y), 0.0, T0 - 15.0), "both_completed")
    put(7, _held(generate, (0.0, y + 1.0), 0.0, T0 - 15.0), "both_completed")
    y = 3 * GROUP    # slot 10 meets slot 11 at x = -8 after 3 s and slot 9 at x = +8 after 7 s: only slot 9 precedes it
    put(9, _run(generate, (8.0, y - 28.0), (8.0, y + 12.0), T0), "late_partner")
    put(10, _run(generate, (-20.0, y), (20.0, y), T0), "two_partners")
    put(11, _run(generate, (-8.0, y - 12.0), (-8.0, y + 28.0), T0), "early_partner")
    y = 4 * GROUP    # two lanes 3.0 m apart, one vehicle STAGGER ahead: 1.10 m between the flanks, outside the broad phase of range 0
    put(13, _run(generate, (-20.0, y), (20.0, y), T0), "range_cut")
    put(14, _run(generate, (-20.0 + STAGGER, y + 3.0), (20.0 + STAGGER, y + 3.0), T0), "range_cut")
    y = 5 * GROUP    # two lanes 1.5 m apart, side by side: the footprints overlap from the first clock on
    put(16, _run(generate, (-20.0, y), (20.0, y), T0), "at_k0")
    put(17, _run(generate, (-20.0, y + 1.5), (20.0, y + 1.5), T0), "at_k0")
    y = 6 * GROUP    # head-on, closing to NOSE_GAP at the last clock
    put(18, _run(generate, (-30.0, y), (-HEAD_ON_END, y), T0), "at_k_last")
    put(19, _run(generate, (30.0, y), (HEAD_ON_END, y), T0), "at_k_last")
    y = 7 * GROUP    # slot 21 ends at t0 + 5 across the lane of slot 20, which arrives there then: who yields flips with t_now
    put(20, _run(generate, (-20.0, y), (20.0, y), T0), "meets_ending")
    put(21, _run(generate, (0.0, y - 20.0), (0.0, y), T0 - 5.0), "ends_early")
    return dict(slots=slots, t0=T0, dt=DT, K=K, t_nows=T_NOWS, cases=CASES, expect=expect)
