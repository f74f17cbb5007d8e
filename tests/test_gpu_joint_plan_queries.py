"""Joint selection through dftpav_plan_queries (joint_select.hip behind the layout groups): off, or on with the conflict filter off,
every output is a plain planner's; on, winners, blocked and rows equal oracle_conflict/joint_oracle.cpp (order 2) on the chain of CPU
oracles of tests/limits_cases.py -- fourteen arena queries that start in one state, R = 4 -- and on a scene of two vehicles side by
side (tests/joint_cases.py: plan_scene); no executing table, so the table test rejects nothing."""
import numpy as np
import pytest

import joint_cases as jc
import limits_cases as lc
from oracle_conflict import pyjoint as pj

pytestmark = pytest.mark.gpu

F_DT, F_K, F_RANGE = 0.25, 48, 2.0
MS, NP = 8, 64                          # the padding of the oracle's per-query layouts


def _pp(hiplib):
    pp = hiplib.default_plan_params()
    pp.seed = lc.SEED
    return pp


@pytest.fixture(scope="module")
def arena(hiplib):
    grid, res, org, S, E = lc.chain()["scene"]
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl0 = hiplib.Planner(h, len(E), lc.R)
    plain = pl0.plan(S, E, pp=_pp(hiplib))
    yield dict(h=h, S=S, E=E, Q=len(E), plain=plain, pl0=pl0)
    pl0.close()
    h.close()


def _same_outputs(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _oracle_inputs(hiplib, plain, order=None, extra_reject=None):
    """the chain as the joint oracle's plans entry takes it, the queries in `order` (default: the call's); a query the device found
    no layout group for has no candidates"""
    per = lc.chain()["per"]
    order = list(range(len(per))) if order is None else order
    Q, R = len(order), lc.R
    n_seg, sg, pn = np.zeros(Q, np.int32), np.zeros((Q, MS), np.int32), np.zeros((Q, MS), np.int32)
    pdt, co, cost, elig = np.zeros((Q, R, MS)), np.zeros((Q, R, NP, 6, 2)), np.zeros((Q, R)), np.zeros((Q, R), np.int32)
    for i, q in enumerate(order):
        c = per[q]
        if c is None or plain["plan_status"][q] == hiplib.PLAN_LAYOUT_UNSUPPORTED:
            continue
        lay, M = c["layout"], len(c["layout"].piece_nums)
        n_seg[i], sg[i, :M], pn[i, :M] = M, lay.singuls, lay.piece_nums
        pdt[i, :, :M], co[i, :, :lay.n_pieces] = c["dts"], c["coeffs"]
        cost[i] = c["solve"]["final_cost"]
        elig[i] = (np.asarray(c["solve"]["success"]) != 0) & (np.asarray(c["collision"]) == 0)
        if extra_reject is not None:
            elig[i] &= extra_reject[q] == 0
    return n_seg, sg, pn, pdt, co, cost, elig


def _ref(hiplib, plain, margin, rng=F_RANGE, **kw):
    return pj.select_plans(*_oracle_inputs(hiplib, plain, **kw), 0.0, F_DT, F_K, margin, rng, order=2)


def _check(hiplib, arena, pl, ref, plain_rows=True):
    out = pl.plan(arena["S"], arena["E"], pp=_pp(hiplib))
    got = pl.last_joint(arena["Q"])
    jc.same(dict(got, winner=ref["winner"]), ref)
    assert np.array_equal(got["blocked"] != 0, got["conflict_sample"] >= 0)
    assert np.array_equal(out["winner"], ref["winner"]), (out["winner"], ref["winner"])
    ok = ref["winner"] >= 0
    assert np.array_equal(out["plan_status"][ok], np.full(ok.sum(), hiplib.PLAN_OK))
    had = arena["plain"]["winner"] >= 0
    assert (out["plan_status"][had & ~ok] == hiplib.PLAN_NO_VALID_RESTART).all()
    if plain_rows:
        for k in ("r_final_cost", "r_status", "r_success", "r_iters", "r_evals", "r_collision", "r_first_sample"):
            assert np.array_equal(out[k], arena["plain"][k], equal_nan=True), k
    return out, got


def test_off_is_a_planner_without_it(hiplib, arena):
    Q = arena["Q"]
    pl = hiplib.Planner(arena["h"], Q, lc.R)
    pl.set_joint_selection(False)                               # off before it was ever on
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), arena["plain"])
    pl.set_joint_selection(True)                                # on, the conflict filter off: nothing of it runs
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), arena["plain"])
    with pytest.raises(hiplib.DftpavError) as e:
        pl.last_joint(Q)
    assert e.value.code == hiplib.E_INVALID
    pl.set_conflict_filter(0.5, F_RANGE, F_DT, F_K)
    pl.set_joint_selection(False)                               # the filter on, joint selection off: the filter alone (an empty table)
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), arena["plain"])
    with pytest.raises(hiplib.DftpavError):
        pl.last_joint(Q)
    pl.close()


def test_the_same_query_twice(hiplib, arena):
    """the second query's restarts all start in the first's winner at k = 0: it ends without a plan, the first is unchanged"""
    plain, Q = arena["plain"], arena["Q"]
    q = int(np.flatnonzero(plain["winner"] >= 0)[0])
    S2, E2 = arena["S"][[q, q]], arena["E"][[q, q]]
    pl = hiplib.Planner(arena["h"], 2, lc.R)
    twin = pl.plan(S2, E2, pp=_pp(hiplib))                      # (the sampler keys its streams by the query's index: not plain's restarts)
    assert twin["winner"][0] >= 0 and twin["winner"][1] >= 0
    pl.set_conflict_filter(0.3, F_RANGE, F_DT, F_K)
    pl.set_joint_selection(True)
    out = pl.plan(S2, E2, pp=_pp(hiplib))
    rows = pl.last_joint(2)
    assert out["winner"][0] == twin["winner"][0] and out["plan_status"][0] == hiplib.PLAN_OK
    for k in out:
        if np.ndim(out[k]) >= 1 and np.shape(out[k])[0] == 2:
            assert np.array_equal(out[k][0], twin[k][0], equal_nan=True), k
    assert out["winner"][1] == -1 and out["plan_status"][1] == hiplib.PLAN_NO_VALID_RESTART and not out["coeffs"][1].any()
    assert rows["blocked"].tolist() == [[0] * lc.R, [1] * lc.R]
    assert (rows["conflict_sample"][1] == 0).all() and (rows["conflict_partner"][1] == 0).all() and (rows["min_sep"][1] == 0.0).all()
    assert np.isposinf(rows["min_sep"][0]).all()
    ms = arena["h"].joint_last_ms()
    assert min(ms) > 0.0
    pl.close()


MARGIN = 0.3


def test_on_the_arena_queries(hiplib, arena):
    """The fourteen arena queries all START IN THE SAME STATE, so every candidate overlaps every winner in front of it at k = 0 (min_sep
    0.0 throughout, from the oracle): any margin >= 0 is larger than every pairwise distance at k = 0, and only the first query with a
    plan keeps one.  No margin lies between two separations of this scene; the case of a winner that moves to a dearer restart is
    covered on crafted poses (tests/test_gpu_joint_select.py), not here."""
    plain, Q = arena["plain"], arena["Q"]
    free = _ref(hiplib, plain, -1.0)                            # nobody is blocked: every candidate against the unfiltered winners
    seps = np.unique(free["min_sep"][np.isfinite(free["min_sep"])])
    print("separations from the winners in front, nobody blocked:", seps.tolist(), "winners", free["winner"].tolist())
    assert np.array_equal(free["winner"], np.where(plain["plan_status"] == hiplib.PLAN_OK, plain["winner"], -1))
    first = int(np.flatnonzero(free["winner"] >= 0)[0])
    pl = hiplib.Planner(arena["h"], Q, lc.R)
    pl.set_joint_selection(True)
    for margin, rng in ((MARGIN, F_RANGE), (0.0, 0.0), (1000.0, 1000.0)):
        ref = _ref(hiplib, plain, margin, rng)
        assert (ref["winner"] >= 0).sum() == 1 and ref["winner"][first] == free["winner"][first]
        assert (ref["conflict_sample"][first + 1:][np.isfinite(ref["min_sep"][first + 1:])] == 0).all()
        pl.set_conflict_filter(margin, rng, F_DT, F_K)
        out, got = _check(hiplib, arena, pl, ref)
        for k in ("final_cost", "coeffs", "x", "iters"):
            assert np.array_equal(out[k][first], plain[k][first]), k
        _same_outputs(_check(hiplib, arena, pl, ref)[0], out)   # rows and flags do not leak between calls
    pl.set_conflict_filter(-0.5, F_RANGE, F_DT, F_K)            # a negative margin switches the filter, and joint selection with it, off
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), plain)
    ms = arena["h"].joint_last_ms()
    assert min(ms) > 0.0
    # a call of fewer queries, in another order: priority is the call's order
    pl.set_conflict_filter(MARGIN, F_RANGE, F_DT, F_K)
    order = [q for q in range(Q) if free["winner"][q] >= 0][::-1][:3]
    sub = pl.plan(arena["S"][order], arena["E"][order], pp=_pp(hiplib))
    rows = pl.last_joint(len(order))
    won = np.flatnonzero(sub["winner"] >= 0)                    # (restarts are drawn by the query's index in the call: not the chain's)
    assert len(won) == 1 and rows["blocked"][won[0] + 1:].all() and not rows["blocked"][:won[0] + 1].any()
    assert (rows["conflict_partner"][won[0] + 1:] == won[0]).all()
    pl.close()


# ---- two vehicles side by side (tests/joint_cases.py: plan_scene), 1.3 m between the flanks at the start.  From the chain of CPU oracles
# and the joint oracle alone (order 2, range 6, dt 0.25, K 48): query 0's cheapest restart is 2; the separations of query 1's four
# restarts from it are 0.589, 0.612, 0.475, 0.871 m, and query 1's cheapest restart is 2 as well.  A margin of 0.53 m lies strictly
# between 0.475 and 0.589: query 1 moves to restart 0, which is dearer, and query 0 is unchanged.  The tests assert these properties
# from the oracles before the device runs.
S_RANGE, S_MARGIN = 6.0, 0.53


@pytest.fixture(scope="module")
def side(hiplib):
    ch = jc.plan_chain()
    grid, res, org, S, E = ch["scene"]
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl0 = hiplib.Planner(h, len(E), jc.PLAN_R)
    plain = pl0.plan(S, E, pp=_pp(hiplib))
    yield dict(h=h, S=S, E=E, Q=len(E), plain=plain, per=ch["per"])
    pl0.close()
    h.close()


def _side_ref(side, margin, reject=None):
    per, Q, R = side["per"], side["Q"], jc.PLAN_R
    n_seg, sg, pn = np.zeros(Q, np.int32), np.zeros((Q, MS), np.int32), np.zeros((Q, MS), np.int32)
    pdt, co, cost, elig = np.zeros((Q, R, MS)), np.zeros((Q, R, NP, 6, 2)), np.zeros((Q, R)), np.zeros((Q, R), np.int32)
    for q, c in enumerate(per):
        lay, M = c["layout"], len(c["layout"].piece_nums)
        n_seg[q], sg[q, :M], pn[q, :M] = M, lay.singuls, lay.piece_nums
        pdt[q, :, :M], co[q, :, :lay.n_pieces] = c["dts"], c["coeffs"]
        cost[q] = c["solve"]["final_cost"]
        elig[q] = (np.asarray(c["solve"]["success"]) != 0) & (np.asarray(c["collision"]) == 0)
        if reject is not None:
            elig[q] &= reject[q] == 0
    return pj.select_plans(n_seg, sg, pn, pdt, co, cost, elig, 0.0, F_DT, F_K, margin, S_RANGE, order=2), cost, elig


def _side_check(hiplib, side, pl, ref):
    out = pl.plan(side["S"], side["E"], pp=_pp(hiplib))
    got = pl.last_joint(side["Q"])
    jc.same(dict(got, winner=ref["winner"]), ref)
    assert np.array_equal(out["winner"], ref["winner"]), (out["winner"], ref["winner"])
    for q, c in enumerate(side["per"]):
        w = ref["winner"][q]
        assert out["plan_status"][q] == (hiplib.PLAN_OK if w >= 0 else hiplib.PLAN_NO_VALID_RESTART)
        if w >= 0:
            assert out["final_cost"][q] == c["solve"]["final_cost"][w] and np.array_equal(out["coeffs"][q, :c["layout"].n_pieces], c["coeffs"][w]), q
    for k in ("r_final_cost", "r_status", "r_success", "r_iters", "r_evals", "r_collision", "r_first_sample"):
        assert np.array_equal(out[k], side["plain"][k], equal_nan=True), k
    return out, got


def test_a_margin_between_two_separations(hiplib, side):
    """one winner moves to a dearer restart, one query is unchanged, both keep a plan; winners, rows and blocked equal the oracle"""
    per = side["per"]
    assert all(c is not None for c in per) and (side["plain"]["plan_status"] == hiplib.PLAN_OK).all()
    free, cost, _ = _side_ref(side, -1.0)                       # nobody blocked: the separations from the winners in front
    seps = np.sort(free["min_sep"][1])
    print("separations of query 1 from query 0's winner:", free["min_sep"][1].tolist(), "winners", free["winner"].tolist(), "margin", S_MARGIN)
    assert np.array_equal(free["winner"], side["plain"]["winner"])
    assert seps[0] < S_MARGIN < seps[1] and free["min_sep"][1, free["winner"][1]] == seps[0]     # strictly between two of them
    ref, _, _ = _side_ref(side, S_MARGIN)
    w0, w1 = free["winner"][1], ref["winner"][1]
    assert ref["winner"][0] == free["winner"][0] and w1 >= 0 and w1 != w0 and cost[1, w1] > cost[1, w0]
    assert ref["blocked"][1].sum() == 1 and ref["blocked"][1, w0] == 1
    pl = hiplib.Planner(side["h"], side["Q"], jc.PLAN_R)
    pl.set_conflict_filter(S_MARGIN, S_RANGE, F_DT, F_K)
    _same_outputs(pl.plan(side["S"], side["E"], pp=_pp(hiplib)), side["plain"])      # joint selection off: both keep their cheapest
    pl.set_joint_selection(True)
    out, got = _side_check(hiplib, side, pl, ref)
    for k in ("final_cost", "coeffs", "x", "iters"):
        assert np.array_equal(out[k][0], side["plain"][k][0]), k                     # query 0 unchanged
    _same_outputs(_side_check(hiplib, side, pl, ref)[0], out)
    pl.set_conflict_filter(seps[0] * 0.5, S_RANGE, F_DT, F_K)   # below every separation: nobody is blocked, rows against the winners
    _same_outputs(_side_check(hiplib, side, pl, _side_ref(side, seps[0] * 0.5)[0])[0], side["plain"])
    pl.close()


def test_a_larger_K_after_a_smaller_one(hiplib, side):
    """joint selection on, the filter set for K = 4, a call, then set for K = F_K: the filter's and the joint stage's poses are
    allocated again for the larger K, and winners, blocked and rows of the next call equal the oracle at F_K"""
    ref, _, _ = _side_ref(side, S_MARGIN)
    assert ref["conflict_sample"].max() >= 4                    # the one conflict lies at a clock the first allocation has no poses for
    pl = hiplib.Planner(side["h"], side["Q"], jc.PLAN_R)
    pl.set_conflict_filter(S_MARGIN, S_RANGE, F_DT, 4)
    pl.set_joint_selection(True)
    _same_outputs(pl.plan(side["S"], side["E"], pp=_pp(hiplib)), side["plain"])       # (within four clocks nobody is blocked)
    assert not pl.last_joint(side["Q"])["blocked"].any()
    pl.set_conflict_filter(S_MARGIN, S_RANGE, F_DT, F_K)
    _side_check(hiplib, side, pl, ref)
    pl.close()


def test_composition_with_the_limit_filter(hiplib, side):
    """A restart the limit filter rejects cannot win and cannot block.  A forward speed limit of 5.0 m/s rejects query 0's cheapest
    restart (and two more); query 0 takes the one that is left, and query 1 is blocked by THAT restart's poses: its winner differs
    from the one it would have were the rejected restart still the blocker."""
    from oracle_limits import pylimits as plim
    per, Q = side["per"], side["Q"]
    lim = hiplib.default_limits()
    lim.max_forward_vel, lim.max_backward_vel, lim.max_forward_cur, lim.max_backward_cur = 5.0, 2.01, 1.01, 1.01
    rej = np.array([1 - plim.check_batch(c["layout"].singuls, c["layout"].piece_nums, c["coeffs"], c["dts"], lc.CHECK_DT, lim, order=2)["feasible"]
                    for c in per])
    alone, cost, elig = _side_ref(side, S_MARGIN)
    ref, _, _ = _side_ref(side, S_MARGIN, reject=rej)
    # were eligibility ignored in the joint stage: blocked by the unfiltered winner's poses, the limit flags applied afterwards
    wrong = [lc.select(cost[q], elig[q], alone["blocked"][q] | rej[q]) for q in range(Q)]
    print("limit rejects", rej.tolist(), "joint alone", alone["winner"].tolist(), "both", ref["winner"].tolist(), "were it to block", wrong)
    assert rej[0, alone["winner"][0]] == 1 and 0 < rej[0].sum() < jc.PLAN_R and not rej[1].any()
    assert ref["winner"][0] >= 0 and ref["winner"][0] != alone["winner"][0] and ref["winner"][1] >= 0
    assert ref["winner"][1] != wrong[1] and ref["winner"][1] != alone["winner"][1]
    assert not np.array_equal(ref["blocked"][1], alone["blocked"][1])
    pl = hiplib.Planner(side["h"], Q, jc.PLAN_R)
    pl.set_conflict_filter(S_MARGIN, S_RANGE, F_DT, F_K)
    pl.set_joint_selection(True)
    pl.set_limit_filter(lim, lc.CHECK_DT)
    out, got = _side_check(hiplib, side, pl, ref)
    assert np.array_equal(pl.last_limits(Q)["feasible"], 1 - rej)
    pl.set_limit_filter(None)
    _side_check(hiplib, side, pl, alone)
    pl.close()


# ---- through dftpav_replan_tick: the two vehicles of the scene above as two empty slots with ego states, so both slots plan in ONE tick,
# in slot order (the tick's query list, hence the priority), from the scene's start states towards its goals; t_now + budget = 0 is the
# adoption clock.  The scene and both expectations come from the oracles above: without joint selection both slots adopt their cheapest
# restart, 0.475 m apart at their nearest clock; with it slot 1 adopts restart 0, 0.589 m from slot 0's plan.
T_TICK, BUDGET = -0.5, 0.5
EXEC_KEYS = ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "duration", "start_time", "end_time", "end_state")


def _tick_planner(hiplib, side, joint):
    """a planner of two empty slots whose table exists (a plan installed and cleared again), the conflict filter on"""
    from dftpav_amd import replan_scenes as rs
    pp = _pp(hiplib)
    pl = hiplib.Planner(side["h"], side["Q"], jc.PLAN_R)
    c = side["per"][0]
    plan = dict(singul=c["layout"].singuls, piece_nums=c["layout"].piece_nums, coeff_dt=c["dts"][0], coeffs=c["coeffs"][0],
                end_state=side["E"][0], t_start=0.0)
    pad = rs.padded(dict(slots=[plan]), pp.max_seg, pp.max_pieces)
    pl.install(pad["slots"], pad["n_seg"], pad["singul"], pad["piece_nums"], pad["coeff_dt"], pad["coeffs"], pad["end_states"], t_start=0.0)
    pl.clear([0])
    pl.set_conflict_filter(S_MARGIN, S_RANGE, F_DT, F_K)
    pl.set_joint_selection(joint)
    return pl, pp


def _ego(side):
    S = side["S"]
    return np.concatenate([S, np.zeros((len(S), 2))], axis=1)   # x, y, angle, velocity, steer, acceleration


def _executing_is(pl, s, c, r, t_start):
    e = pl.executing(s)
    M, n = len(c["layout"].piece_nums), c["layout"].n_pieces
    return (e["n_seg"] == M and e["start_time"][0] == t_start and np.array_equal(e["coeffs"][:n], c["coeffs"][r])
            and np.array_equal(e["coeff_dt"][:M], c["dts"][r]))


def test_two_slots_replan_in_one_tick(hiplib, side):
    per = side["per"]
    free, cost, _ = _side_ref(side, -1.0)
    ref, _, _ = _side_ref(side, S_MARGIN)
    w_off, w_on = free["winner"], ref["winner"]
    near, clear_of = free["min_sep"][1, w_off[1]], ref["min_sep"][1, w_on[1]]
    assert near <= S_MARGIN < clear_of and w_on[0] == w_off[0] and w_on[1] != w_off[1] and w_on[1] >= 0      # the scene, from the oracles
    clocks = (T_TICK + BUDGET, F_DT, F_K, S_MARGIN, S_RANGE)
    # joint selection off: both adopt, and the check of the table reports them within the margin
    pl, pp = _tick_planner(hiplib, side, False)
    tk = pl.tick(T_TICK, BUDGET, end_states=side["E"], ego_states=_ego(side), pp=pp)
    assert np.array_equal(tk["query_slot"], [0, 1]) and tk["check"]["replan"].tolist() == [1, 1]
    assert np.array_equal(tk["plan"]["winner"], w_off) and (tk["plan"]["plan_status"] == hiplib.PLAN_OK).all()
    assert all(_executing_is(pl, s, per[s], w_off[s], T_TICK + BUDGET) for s in (0, 1))
    rows = pl.check_conflicts(*clocks)
    print("off: adopted", tk["plan"]["winner"].tolist(), "table min_sep", rows["min_sep"].tolist(), "conflict_sample", rows["conflict_sample"].tolist())
    assert rows["min_sep"][0] == rows["min_sep"][1] == near and (rows["conflict_sample"] >= 0).all()
    assert rows["conflict_partner"].tolist() == [1, 0]
    with pytest.raises(hiplib.DftpavError):
        pl.last_joint(2)
    pl.close()
    # on: the lower-priority slot takes another restart, and the check finds nothing within the margin between the two
    pl, pp = _tick_planner(hiplib, side, True)
    tk = pl.tick(T_TICK, BUDGET, end_states=side["E"], ego_states=_ego(side), pp=pp)
    assert np.array_equal(tk["query_slot"], [0, 1]) and tk["check"]["replan"].tolist() == [1, 1]
    assert np.array_equal(tk["plan"]["winner"], w_on) and (tk["plan"]["plan_status"] == hiplib.PLAN_OK).all()
    jc.same(dict(pl.last_joint(2), winner=w_on), ref)
    assert all(_executing_is(pl, s, per[s], w_on[s], T_TICK + BUDGET) for s in (0, 1))
    rows = pl.check_conflicts(*clocks)
    print("on: adopted", tk["plan"]["winner"].tolist(), "table min_sep", rows["min_sep"].tolist(), "conflict_sample", rows["conflict_sample"].tolist())
    assert rows["min_sep"][0] == rows["min_sep"][1] == clear_of and (rows["conflict_sample"] == -1).all()
    # the reverse slot order is the reverse priority: the vehicles exchanged between the slots, slot 0 keeps its cheapest restart
    pl.clear([0, 1])
    ego, goals = _ego(side)[::-1].copy(), side["E"][::-1].copy()
    tk = pl.tick(T_TICK, BUDGET, end_states=goals, ego_states=ego, pp=pp)
    joint = pl.last_joint(2)
    assert np.array_equal(tk["query_slot"], [0, 1]) and not joint["blocked"][0].any() and tk["plan"]["winner"][0] >= 0
    rows = pl.check_conflicts(*clocks)
    print("exchanged: adopted", tk["plan"]["winner"].tolist(), "blocked", joint["blocked"].tolist(), "table min_sep", rows["min_sep"].tolist())
    assert (rows["conflict_sample"] == -1).all()                # whoever adopted: nothing within the margin between the two
    pl.close()


def test_a_second_tick_with_both_slots_executing(hiplib, side):
    """Own slots and the table test beside joint selection: after the tick above both slots execute; an obstacle dropped on each path flags
    both at t = 0.5, and both replan in one tick from their desired states at t = 1.0.  Each new plan is tested against the other's OLD
    plan (its own excused) and against the other's new plan if that one wins.  Whatever each slot ends with -- its new plan or the one
    it kept -- every pairing was tested at the clocks 1.0 + k dt, k < K - 4 (old against old in the first tick, at the same clocks), so
    the check of the table finds nothing within the margin."""
    grid, res, org = jc.plan_chain()["scene"][:3]
    pl, pp = _tick_planner(hiplib, side, True)
    pl.tick(T_TICK, BUDGET, end_states=side["E"], ego_states=_ego(side), pp=pp)
    before = [pl.executing(s) for s in (0, 1)]
    xs, ys = org[0] + np.arange(grid.shape[1]) * res, org[1] + np.arange(grid.shape[0]) * res
    after = grid.copy()
    for e in before:
        n = int(e["piece_nums"][:e["n_seg"]].sum())
        mid = e["coeffs"][n // 2, 0]                            # where the piece half way down the plan starts
        after[np.ix_((ys >= mid[1] - 0.25) & (ys <= mid[1] + 0.25), (xs >= mid[0] - 0.25) & (xs <= mid[0] + 0.25))] = 80
    side["h"].set_grid_map(after, res, org)
    try:
        tk = pl.tick(0.5, BUDGET, pp=pp)
        assert tk["check"]["collision"].tolist() == [1, 1] and np.array_equal(tk["query_slot"], [0, 1])
        joint, table = pl.last_joint(2), pl.last_conflicts(2)
        now = [pl.executing(s) for s in (0, 1)]
        adopted = [now[s]["start_time"][0] == 1.0 for s in (0, 1)]
        print("second tick: status", tk["plan"]["plan_status"].tolist(), "winner", tk["plan"]["winner"].tolist(), "adopted", adopted,
              "table-test rejects", (table["conflict_sample"] >= 0).astype(int).tolist(), "blocked", joint["blocked"].tolist())
        for s in (0, 1):
            assert adopted[s] == (tk["plan"]["winner"][s] >= 0)
            if not adopted[s]:                                  # it keeps its old plan, bit for bit
                assert all(np.asarray(before[s][k]).tobytes() == np.asarray(now[s][k]).tobytes() for k in EXEC_KEYS)
            assert (table["conflict_partner"][s][table["conflict_sample"][s] >= 0] == 1 - s).all()       # never its own slot
        assert not joint["blocked"][0].any()
        rows = pl.check_conflicts(1.0, F_DT, F_K - 4, S_MARGIN, S_RANGE)
        print("table min_sep", rows["min_sep"].tolist())
        assert (rows["conflict_sample"] == -1).all() and (rows["min_sep"] > S_MARGIN).all()
    finally:
        side["h"].set_grid_map(grid, res, org)
        pl.close()
