"""The CPU restatement of the replan loop (oracle_replan/replan_oracle.cpp) against what already exists -- the collision
re-check and the state read-out of oracle/, and a plain-Python restatement of the scalar decisions -- on the crafted scene of
dftpav_amd/replan_scenes.py; and the scene against its own conditions, by the oracle alone.  No GPU."""
import math

import numpy as np
import pytest

from dftpav_amd import replan_scenes as rs
from oracle_replan import pyreplan as pr

DISCRETE = pr.INTS + ("pidx",)


@pytest.fixture(scope="module")
def scene(oracle):
    return rs.crafted(oracle.minco_generate)


def table_of(scene):
    T = pr.Table(rs.N_SLOTS)
    for s, p in enumerate(scene["slots"]):
        if p is None:
            continue
        T.install(s, p["singul"], p["piece_nums"], p["coeff_dt"], p["coeffs"], p["end_state"], p["t_start"])
        if p["hist"] is not None:
            T.set_history(s, *p["hist"])
    return T


def check(scene, order=2, **kw):
    a = dict(end_states=None, ego_states=scene["ego_states"])
    a.update(kw)
    return pr.replan_check(scene["grid"], scene["resolution"], scene["origin"], table_of(scene), scene["t_now"], scene["budget"],
                           order=order, **a)


@pytest.fixture(scope="module")
def out2(scene):
    return check(scene, order=2)


def _times(p):
    """the chain of traj_container.hpp:58-73 in Python floats (IEEE doubles): per segment duration, start, end"""
    rows, world = [], p["t_start"]
    for N, dt in zip(p["piece_nums"], p["coeff_dt"]):
        d = 0.0
        for _ in range(int(N)):
            d += float(dt)
        rows.append((d, world, world + d))
        world = world + d
    return rows


def _locate(N, dt, t):
    idx = 0
    while idx < N and t > dt:
        t -= dt
        idx += 1
    if idx == N:
        idx -= 1
        t += dt
    return idx, t


def _pos(c, t):
    px = py = 0.0
    tn = 1.0
    for k in range(6):
        px += tn * float(c[k, 0])
        py += tn * float(c[k, 1])
        tn *= t
    return px, py


def test_collision_equals_the_validation_oracle(oracle, scene, out2):
    n = 0
    for s, p in enumerate(scene["slots"]):
        if p is None or out2["complete"][s]:
            assert out2["collision"][s] == 0 and out2["first_sample"][s] == -1
            continue
        col, first = oracle.validate_trajectories(scene["grid"], scene["resolution"], scene["origin"], p["coeffs"][None],
                                                  p["coeff_dt"][None], p["piece_nums"], p["singul"], order=2)
        assert out2["collision"][s] == col[0] and out2["first_sample"][s] == first[0], s
        n += 1
    assert n >= 8 and out2["collision"].sum() >= 1


def test_desired_equals_the_state_oracle(oracle, scene, out2):
    """the desired row against oracle.sample_states given the segment pidx as a one-segment trajectory, t0 = the local time, one
    sample, the filter off.  (sample_states stamps the row with t0 and publishes nothing at or past the segment's end: the stamp
    column is compared with t_now + budget, the slot past its end with Python's own getPos at the clamped time, and in every column with
    sample_states on the clamped piece alone.)"""
    n_in, n_past = 0, 0
    stamp = scene["t_now"] + scene["budget"]
    for s, p in enumerate(scene["slots"]):
        if p is None or out2["complete"][s]:
            continue
        i = int(out2["pidx"][s])
        t = float(out2["t_local"][s])
        rows = _times(p)
        assert t == stamp - rows[i][1] and out2["desired"][s, 0] == stamp
        p0 = int(p["piece_nums"][:i].sum())
        N = int(p["piece_nums"][i])
        if t < rows[i][0]:
            st, nv = oracle.sample_states(p["coeffs"][None, p0:p0 + N], p["coeff_dt"][None, i:i + 1], [N], [int(p["singul"][i])], t0=t,
                                          sample_dt=1.0, n_samples=1, filter_singularity=False, order=2)
            assert nv[0] == 1
            cols = [1, 2, 4, 5, 6, 7] if p["hist"] is not None else [1, 2, 3, 4, 5, 6, 7]   # a filtered heading is the history's
            assert np.array_equal(out2["desired"][s, cols], st[0, 0, cols]), s
            n_in += 1
        else:
            idx, tt = _locate(N, float(p["coeff_dt"][i]), rows[i][0])          # GetState clamps to the total duration
            assert (out2["desired"][s, 1], out2["desired"][s, 2]) == _pos(p["coeffs"][p0 + idx], tt), s
            # every column: the state oracle on that piece alone, given twice its duration so that the clamped time lies inside it
            dt2 = np.array([[2.0 * float(p["coeff_dt"][i])]])
            st, nv = oracle.sample_states(p["coeffs"][None, p0 + idx:p0 + idx + 1], dt2, [1], [int(p["singul"][i])], t0=tt, sample_dt=1.0,
                                          n_samples=1, filter_singularity=False, order=2)
            assert nv[0] == 1 and tt < dt2[0, 0]
            cols = [1, 2, 4, 5, 6, 7] if p["hist"] is not None else [1, 2, 3, 4, 5, 6, 7]
            assert np.array_equal(out2["desired"][s, cols], st[0, 0, cols]), s
            n_past += 1
        d = out2["desired"][s]
        assert np.array_equal(out2["start_state"][s], d[[1, 2, 3, 5]]) and np.array_equal(out2["start_ctrl"][s], d[[7, 6]])
    assert n_in >= 6 and n_past >= 1


def test_scalar_flags_equal_a_python_restatement(scene, out2):
    t_now, stamp = scene["t_now"], scene["t_now"] + scene["budget"]
    for s, p in enumerate(scene["slots"]):
        if p is None:
            assert out2["occupied"][s] == 0 and out2["complete"][s] == 0
            continue
        rows = _times(p)
        M = len(rows)
        assert np.array_equal(out2["duration"][s, :M], [r[0] for r in rows]) and np.array_equal(out2["start_time"][s, :M], [r[1] for r in rows])
        assert np.array_equal(out2["end_time"][s, :M], [r[2] for r in rows])
        complete = t_now > rows[-1][2]
        assert out2["occupied"][s] == 1 and out2["complete"][s] == int(complete), s
        if complete:
            for k in ("exe_index", "is_close_turnpoint", "is_near", "target_moved", "replan"):
                assert out2[k][s] == 0
            continue
        exe = 0
        while exe < M - 1 and rows[exe][2] <= t_now:
            exe += 1
        close = exe != M - 1 and (rows[exe][2] - t_now) < 2.5
        total = 0.0
        for r in rows:
            total += r[0]
        near = (rows[-1][2] - t_now) < 2 * total / 3.0
        p0 = int(p["piece_nums"][:-1].sum())
        idx, tt = _locate(int(p["piece_nums"][-1]), float(p["coeff_dt"][-1]), rows[-1][0])
        lx, ly = _pos(p["coeffs"][p0 + idx], tt)
        ex, ey = lx - float(p["end_state"][0]), ly - float(p["end_state"][1])
        moved = math.sqrt(ex * ex + ey * ey) > 0.1
        pidx = exe
        while True:
            if stamp <= rows[pidx][1] + rows[pidx][0]:
                break
            pidx += 1
            if pidx >= M:
                pidx -= 1
                break
        got = [int(out2[k][s]) for k in ("exe_index", "is_close_turnpoint", "is_near", "target_moved", "pidx")]
        assert got == [exe, int(close), int(near), int(moved), pidx], (s, got)
        assert out2["replan"][s] == int((near and not close and moved) or bool(out2["collision"][s])), s


def test_scene_meets_its_conditions(scene, out2):
    """every case the scene is there for occurs, by the oracle alone (order 2)"""
    o, want = out2, scene["expect"]
    slot = {case: s for s, case in want.items()}
    assert len(slot) == rs.N_SLOTS == len(want)
    rule = (o["is_near"] == 1) & (o["is_close_turnpoint"] == 0) & (o["target_moved"] == 1)
    s = slot["complete"]
    assert o["complete"][s] == 1 and o["replan"][s] == 0 and not o["desired"][s].any()
    s = slot["near_target"]
    assert rule[s] and o["collision"][s] == 0 and o["replan"][s] == 1
    s = slot["suppressed_by_turnpoint"]
    assert o["is_near"][s] == 1 and o["target_moved"][s] == 1 and o["is_close_turnpoint"][s] == 1 and o["collision"][s] == 0 and o["replan"][s] == 0
    s = slot["collision_only"]
    assert not rule[s] and o["collision"][s] == 1 and o["first_sample"][s] > 0 and o["replan"][s] == 1
    before = pr.replan_check(scene["grid_before"], scene["resolution"], scene["origin"], table_of(scene), scene["t_now"], scene["budget"])
    assert before["collision"][s] == 0 and before["replan"][s] == 0          # the obstacle was dropped after the plan was made
    assert before["collision"].sum() == 0
    s = slot["nothing"]
    assert o["occupied"][s] == 1 and o["complete"][s] == 0 and o["replan"][s] == 0 and o["collision"][s] == 0
    s = slot["past_the_end"]
    M = len(scene["slots"][s]["piece_nums"])
    assert o["complete"][s] == 0 and o["pidx"][s] == M - 1 and o["t_local"][s] > o["duration"][s, M - 1]   # the step back, then the clamp
    s = slot["filtered_heading"]
    T = table_of(scene)              # the same tick without the stored state: the heading GetState gives
    T.have_hist[s] = 0
    raw = pr.replan_check(scene["grid"], scene["resolution"], scene["origin"], T, scene["t_now"], scene["budget"], ego_states=scene["ego_states"])
    hist_angle = scene["slots"][s]["hist"][1]
    assert abs(o["desired"][s, 5]) < 0.1 and o["desired"][s, 3] == hist_angle and raw["desired"][s, 3] != hist_angle
    assert o["start_state"][s, 2] == hist_angle
    s = slot["empty_with_ego"]
    e = scene["ego_states"][s]
    assert o["occupied"][s] == 0 and o["replan"][s] == 1
    assert np.array_equal(o["desired"][s], [scene["t_now"] + scene["budget"], e[0], e[1], e[2], 0.0, e[3], e[5], e[4]])
    assert np.array_equal(o["start_state"][s], e[:4]) and np.array_equal(o["start_ctrl"][s], e[4:6])
    without = check(scene, ego_states=None)
    assert without["replan"][s] == 0 and not without["desired"][s].any()
    s = slot["pidx_walk"]
    assert o["pidx"][s] == o["exe_index"][s] + 1
    s = slot["reverse_segment"]
    assert o["exe_index"][s] == 1 and scene["slots"][s]["singul"][o["pidx"][s]] == -1 and o["desired"][s, 5] < 0.0
    # a goal given to the check overrides the stored one
    goals = np.array([p["end_state"] if p is not None else np.zeros(4) for p in scene["slots"]])
    moved = goals.copy()
    moved[slot["nothing"], 1] += 1.0
    assert check(scene, end_states=goals)["replan"][slot["nothing"]] == 0
    assert check(scene, end_states=moved)["target_moved"][slot["nothing"]] == 1


def test_orders_agree_on_every_discrete_output(scene, out2):
    out0 = check(scene, order=0)
    for k in DISCRETE:
        assert np.array_equal(out0[k], out2[k]), k
    assert np.allclose(out0["desired"], out2["desired"], rtol=0, atol=1e-12)
    for k in ("duration", "start_time", "end_time", "t_local"):
        assert np.array_equal(out0[k], out2[k]), k
