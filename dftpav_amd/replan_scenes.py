"""Crafted executing plans for the replan loop (dftpav_replan_check / dftpav_replan_tick): ten slots on the default arena
(search_scenes.arena) that, at one clock, put every branch of TrajPlannerServer's tick side by side (traj_server_ros.cpp:130-192,
359-501).  The plans are straight minimum-jerk trajectories on three lanes of a free stretch of the arena; `generate` is the
MINCO generator to build them with (inner [N - 1][2], piece duration, head [6], tail [6]) -> (coeffs [N][6][2], cost), which the
caller brings (the tests: the CPU oracle's).

crafted(generate) returns a dict:
  grid, resolution, origin     the arena with the obstacle of slot 3 dropped onto its lane (the map of the check)
  grid_before                  the arena as it was when the plans were made
  t_now, budget                the clock of the tick and Replan's Budget
  slots                        list of None (empty) or dict(singul [M], piece_nums [M], coeff_dt [M], coeffs [Ntot][6][2],
                               end_state [4], t_start, hist = None or (stamp, angle))
  ego_states [10][6]           x, y, angle, v, steer, acc (read for the empty slot only)
  expect                       slot -> the case it is there for (tests/test_replan_oracle.py holds the oracle to it)
"""
import numpy as np

from . import search_scenes as ss

T_NOW = 100.0
BUDGET = 0.5
N_SLOTS = 10
LANES = (25.0, 28.0, 31.0)      # y of the three lanes: free for x in [-66, -30] on the default arena


def _segment(generate, p0, p1, n_pieces, dT, singul, v0, v1):
    """a straight segment from p0 to p1: evenly spaced waypoints, boundary speeds v0 / v1 along the direction of motion"""
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    u = (p1 - p0) / np.hypot(*(p1 - p0))
    inner = np.array([p0 + (p1 - p0) * k / n_pieces for k in range(1, n_pieces)])
    head = np.concatenate([p0, v0 * u, [0.0, 0.0]])
    tail = np.concatenate([p1, v1 * u, [0.0, 0.0]])
    c, _ = generate(inner, float(dT), head, tail)
    return dict(coeffs=c, piece_nums=n_pieces, coeff_dt=float(dT), singul=int(singul), end=p1)


def _plan(segments, goal_offset=(0.0, 0.0)):
    end = segments[-1]["end"]
    return dict(singul=np.array([s["singul"] for s in segments], dtype=np.int32),
                piece_nums=np.array([s["piece_nums"] for s in segments], dtype=np.int32),
                coeff_dt=np.array([s["coeff_dt"] for s in segments]),
                coeffs=np.concatenate([s["coeffs"] for s in segments]),
                end_state=np.array([end[0] + goal_offset[0], end[1] + goal_offset[1], 0.0, 0.0]), t_start=0.0, hist=None)


def plan_a(generate, lane, goal_offset=(0.0, 0.0)):
    """one forward segment of 6 x 2 s along a lane, 24 m"""
    y = LANES[lane]
    return _plan([_segment(generate, (-64.0, y), (-40.0, y), 6, 2.0, 1, 0.05, 0.05)], goal_offset)


def plan_b(generate, lane, goal_offset=(0.0, 0.0)):
    """forward 12 m in 4 x 1.5 s to a near-standstill, then 8 m back in 4 x 1.5 s"""
    y = LANES[lane]
    return _plan([_segment(generate, (-60.0, y), (-48.0, y), 4, 1.5, 1, 0.05, 0.05),
                  _segment(generate, (-48.0, y), (-56.0, y), 4, 1.5, -1, 0.05, 0.05)], goal_offset)


def plan_c(generate, lane):
    """forward, back, forward: three segments of 3 x 1.5 s"""
    y = LANES[lane]
    return _plan([_segment(generate, (-62.0, y), (-54.0, y), 3, 1.5, 1, 0.05, 0.05),
                  _segment(generate, (-54.0, y), (-59.0, y), 3, 1.5, -1, 0.05, 0.05),
                  _segment(generate, (-59.0, y), (-50.0, y), 3, 1.5, 1, 0.05, 0.05)])


def crafted(generate):
    grid, res, origin, start, _ = ss.arena()
    before = grid.copy()
    after = grid.copy()
    # the obstacle of slot 3: a 1 m box on lane 0, 19 m down the plan (cells whose centres lie inside)
    xs = origin[0] + np.arange(grid.shape[1]) * res
    ys = origin[1] + np.arange(grid.shape[0]) * res
    after[np.ix_((ys >= LANES[0] - 0.5) & (ys <= LANES[0] + 0.5), (xs >= -46.0) & (xs <= -45.0))] = 80
    slots, expect = [None] * N_SLOTS, {}

    def put(s, plan, t_start, case, hist=None):
        plan["t_start"], plan["hist"] = float(t_start), hist
        slots[s], expect[s] = plan, case

    put(0, plan_a(generate, 1), T_NOW - 13.0, "complete")                                    # ended at 99
    put(1, plan_a(generate, 1, goal_offset=(0.0, 1.0)), T_NOW - 9.0, "near_target")          # 3 s left of 12, the goal 1 m aside
    put(2, plan_b(generate, 2, goal_offset=(0.0, 1.0)), T_NOW - 4.5, "suppressed_by_turnpoint")   # 1.5 s to the gear shift
    put(3, plan_a(generate, 0), T_NOW - 1.0, "collision_only")                               # 11 s left, the box on its lane
    put(4, plan_a(generate, 1), T_NOW - 1.0, "nothing")
    put(5, plan_a(generate, 1), T_NOW - 11.8, "past_the_end")                                # 0.2 s left, the stamp 0.3 s past the end
    put(6, plan_b(generate, 2), T_NOW + BUDGET - 5.98, "filtered_heading", hist=(T_NOW + BUDGET - 0.05, 0.3))   # 0.02 s before the standstill
    expect[7] = "empty_with_ego"
    put(8, plan_b(generate, 2), T_NOW - 5.7, "pidx_walk")                                    # the stamp in the next segment
    put(9, plan_c(generate, 2), T_NOW - 6.0, "reverse_segment")                              # mid-way through the reverse segment
    ego = np.zeros((N_SLOTS, 6))
    ego[7] = (start[0], start[1], start[2], 0.3, 0.05, 0.1)
    return dict(grid=after, grid_before=before, resolution=res, origin=origin, t_now=T_NOW, budget=BUDGET, slots=slots,
                ego_states=ego, expect=expect)


def padded(scene, max_seg=8, max_pieces=64):
    """the occupied slots as the padded arrays dftpav_planner_install takes: dict(slots [n], n_seg, singul, piece_nums, coeff_dt,
    coeffs, end_states, t_start [n]) -- t_start per plan: install them one call per distinct value"""
    idx = [s for s, p in enumerate(scene["slots"]) if p is not None]
    n = len(idx)
    out = dict(slots=np.array(idx, dtype=np.int32), n_seg=np.zeros(n, np.int32), singul=np.zeros((n, max_seg), np.int32),
               piece_nums=np.zeros((n, max_seg), np.int32), coeff_dt=np.zeros((n, max_seg)),
               coeffs=np.zeros((n, max_seg * max_pieces, 6, 2)), end_states=np.zeros((n, 4)), t_start=np.zeros(n))
    for k, s in enumerate(idx):
        p = scene["slots"][s]
        M = len(p["piece_nums"])
        out["n_seg"][k] = M
        out["singul"][k, :M], out["piece_nums"][k, :M], out["coeff_dt"][k, :M] = p["singul"], p["piece_nums"], p["coeff_dt"]
        out["coeffs"][k, :p["coeffs"].shape[0]] = p["coeffs"]
        out["end_states"][k], out["t_start"][k] = p["end_state"], p["t_start"]
    return out
