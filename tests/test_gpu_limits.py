"""Solved plans against the kinematic limits on the device (limits.hip): dftpav_batch_check_limits on solved batches and on crafted
coefficients, dftpav_planner_check_limits on the executing table, and the limit filter of dftpav_plan_queries / dftpav_replan_tick
-- every field equal to oracle_limits in order 2 (tests/limits_cases.py holds the chain of CPU oracles the filter is held against)."""
import ctypes as C
import math

import numpy as np
import pytest

import limits_cases as lc
from dftpav_amd import replan_scenes as rs
from dftpav_amd import scenarios as sc
from dftpav_amd.pods import LayoutSpec
from oracle_limits import pylimits as plim

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
EXEC_KEYS = ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "duration", "start_time", "end_time", "end_state", "hist", "have_hist")


def _limits(hiplib, **kw):
    l = hiplib.default_limits()
    for k, v in kw.items():
        setattr(l, k, v)
    return l


def _all_inf(hiplib):
    return _limits(hiplib, **{k: INF for k in plim.LIMIT_FIELDS})


def _set_coeffs(hiplib, bt, co, dt):
    fn = hiplib.lib().dftpav_debug_batch_set_coeffs
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    co, dt = np.ascontiguousarray(co, dtype=np.float64), np.ascontiguousarray(dt, dtype=np.float64)
    assert fn(bt._b, co.ctypes.data_as(C.c_void_p), dt.ctypes.data_as(C.c_void_p)) == 0


def _crafted(hiplib, h, piece_nums, singuls, co, dt, check_dt, limits):
    """device and oracle rows of crafted coefficients [B][Ntot][6][2] / piece durations [B][M]"""
    co = np.ascontiguousarray(co, dtype=np.float64)
    bt = hiplib.Batch(h, LayoutSpec(list(piece_nums), list(singuls), 4), co.shape[0])
    _set_coeffs(hiplib, bt, co, dt)
    got = bt.check_limits(check_dt, limits)
    bt.close()
    ref = plim.check_batch(singuls, piece_nums, co, dt, check_dt, limits, order=2)
    assert lc.same_rows(got, ref), (got, ref)
    return got, ref


def straight(speed, n_pieces, dT, direction=1.0):
    co = np.zeros((n_pieces, 6, 2))
    for p in range(n_pieces):
        co[p, 0, 0] = direction * speed * dT * p
        co[p, 1, 0] = direction * speed
    return co


@pytest.mark.parametrize("pieces,sing,B,steps,more_than_256", [([2], [1], 8, (0.05, 0.0371), False), ([3, 2], [1, -1], 8, (0.05, 0.0371), False),
                                                               ([16], [1], 3, (0.02, 0.0137), True)])   # ~6 s of 16 pieces: > 256 samples
def test_solved_batches_equal_the_oracle(hiplib, pieces, sing, B, steps, more_than_256):
    p = hiplib.default_params()
    s = sc.make_scenario(pieces, sing, 8, 8, B, seed=300 + len(pieces) + pieces[0], n_obs=10)
    s.apply_resolution(p)
    h = hiplib.Handle(p)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    bt.solve()
    co, dts = bt.coeffs()
    lim = hiplib.default_limits(p)
    for dt in steps:                               # the second divides no duration
        got = bt.check_limits(dt, lim)
        ref = plim.check_batch(sing, pieces, co, dts, dt, lim, order=2)
        print(pieces, dt, "samples", ref["n_samples"].tolist(), "max", got["max_abs"][0].tolist(), "arg", got["arg"][0].tolist(),
              "violated", got["violated"].sum(0).tolist())
        assert lc.same_rows(got, ref), (pieces, dt)
        assert (ref["n_samples"] > 256).all() == more_than_256 and np.isfinite(got["max_abs"]).all() and (got["arg"] >= 0).all()
    assert h.limits_last_ms() > 0.0
    # the pointers of dftpav_limits_out may be NULL, one by one
    out = hiplib.LimitsOut(s.B)
    out.c.max_abs = None
    out.c.violated = None
    fn = hiplib.lib().dftpav_batch_check_limits
    fn.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    assert fn(bt._b, steps[1], C.byref(lim), C.byref(out.c)) == 0
    assert np.array_equal(out.a["arg"], ref["arg"]) and np.array_equal(out.a["feasible"], ref["feasible"]) and not out.a["max_abs"].any()
    bt.close()
    h.close()


def test_crafted_coefficients(hiplib):
    h = hiplib.Handle()
    lim = hiplib.default_limits()
    # straight motion at exactly 5.0 m/s: every sample ties, arg 0; the limit is strict
    co = straight(5.0, 4, 1.0)[None]
    got, _ = _crafted(hiplib, h, [4], [1], co, [[1.0]], 0.05, lim)
    assert got["max_abs"][0].tolist() == [5.0, 0.0, 0.0, 0.0, 0.0] and got["arg"][0].tolist() == [0] * 5
    assert not got["violated"].any() and got["feasible"][0] == 1
    got, _ = _crafted(hiplib, h, [4], [1], co, [[1.0]], 0.05, _limits(hiplib, max_forward_vel=math.nextafter(5.0, 0.0)))
    assert got["violated"][0].tolist() == [1, 0, 0, 0, 0] and got["feasible"][0] == 0 and got["arg"][0, 0] == 0
    # the same in reverse, at the backward limit
    co = straight(2.0, 4, 1.0, direction=-1.0)[None]
    got, _ = _crafted(hiplib, h, [4], [-1], co, [[1.0]], 0.05, lim)
    assert got["max_abs"][0, 0] == 2.0 and got["arg"][0, 0] == 0 and got["feasible"][0] == 1
    got, _ = _crafted(hiplib, h, [4], [-1], co, [[1.0]], 0.05, _limits(hiplib, max_backward_vel=math.nextafter(2.0, 0.0)))
    assert got["violated"][0].tolist() == [1, 0, 0, 0, 0]
    got, _ = _crafted(hiplib, h, [4], [-1], co, [[1.0]], 0.05, _limits(hiplib, max_forward_vel=1.0))      # the forward limit is not read
    assert got["feasible"][0] == 1
    # a piece at rest (with an acceleration): the branch applies, every quantity is 0
    z = np.zeros((1, 2, 6, 2))
    z[0, :, 0] = (3.0, 4.0)
    z[0, 0, 2] = (3e-5, 1e-5)
    z[0, 0, 1] = (1e-7, 0.0)                                # |dsigma| < 1e-6 at the first samples
    got, ref = _crafted(hiplib, h, [2], [1], z, [[0.001]], 0.0004, lim)
    assert got["max_abs"][0, 1:].tolist() == [0.0] * 4 and 0.0 < got["max_abs"][0, 0] < 1e-6 and got["feasible"][0] == 1
    z[0, 0, 1:3] = 0.0
    got, _ = _crafted(hiplib, h, [2], [1], z, [[1.0]], 0.05, lim)
    assert not got["max_abs"].any() and (got["arg"] == 0).all() and got["feasible"][0] == 1
    # a NaN coefficient in the last piece: violated whatever the limit, arg the first NaN sample, later samples do not replace it
    co = straight(1.0, 3, 1.0)
    co[2, 3, 1] = NAN
    got, ref = _crafted(hiplib, h, [3], [1], np.stack([co, straight(1.0, 3, 1.0)]), [[1.0], [1.0]], 0.05, _all_inf(hiplib))
    t, k = 0.0, 0
    while not t - 1.0 > 1.0:                                # locatePieceIdx moves on to the last piece once t - 1.0 > 1.0
        t += 0.05
        k += 1
    assert np.isnan(got["max_abs"][0]).all() and (got["arg"][0] == k).all() and (got["violated"][0] == 1).all() and got["feasible"][0] == 0
    # +inf limits never fire for a number (the second trajectory, and a fast one)
    assert not got["violated"][1].any() and got["feasible"][1] == 1
    got, _ = _crafted(hiplib, h, [4], [1], straight(1e6, 4, 1.0)[None], [[1.0]], 0.05, _all_inf(hiplib))
    assert not got["violated"].any() and got["max_abs"][0, 0] == 1e6
    h.close()


def test_samples_past_the_table_of_sample_times(hiplib):
    """A segment with more samples than the 4096 the host tabulates: the count and the times past the table's end are the running
    sum continued on the device.  |velocity| rises to the end (1 m/s + 0.5 m/s^2 over 4 pieces of 1 s), so its arg lies there."""
    n_pieces, dT, v0, a, check_dt = 4, 1.0, 1.0, 0.5, 0.0009
    co = np.zeros((1, n_pieces, 6, 2))
    for p in range(n_pieces):
        t = p * dT
        co[0, p, :3, 0] = (v0 * t + 0.5 * a * t * t, v0 + a * t, 0.5 * a)
    h = hiplib.Handle()
    got, ref = _crafted(hiplib, h, [n_pieces], [1], co, [[dT]], check_dt, hiplib.default_limits())
    print("n_samples", ref["n_samples"].tolist(), "max", got["max_abs"][0].tolist(), "arg", got["arg"][0].tolist())
    duration, t, n = 0.0, 0.0, 0
    for _ in range(n_pieces):
        duration += dT
    while t < duration:
        t += check_dt
        n += 1
    assert n > 4096 and ref["n_samples"][0] == n
    assert ref["arg"][0, 0] > 4096 and got["arg"][0, 0] == n - 1 and got["feasible"][0] == 1
    h.close()


def _oracle_on_table(pl, n_slots, check_dt, limits):
    """the oracle on dftpav_planner_executing's read-back of every slot"""
    ex = [pl.executing(s) for s in range(n_slots)]
    return ex, plim.check_table([e["n_seg"] for e in ex], [e["singul"] for e in ex], [e["piece_nums"] for e in ex],
                                [e["coeff_dt"] for e in ex], np.array([e["coeffs"] for e in ex]), check_dt, limits, order=2)


def _same_table(a, b):
    return all(np.array_equal(np.asarray(x[k]), np.asarray(y[k])) for x, y in zip(a, b) for k in EXEC_KEYS)


FILTER = dict(max_forward_vel=5.01, max_backward_vel=2.01, max_forward_cur=1.01, max_backward_cur=1.01)


def test_table_variant(hiplib, oracle):
    grid, res, org, S, E = lc.chain()["scene"]
    Q = len(E)
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl = hiplib.Planner(h, Q, lc.R)
    lim = _limits(hiplib, **FILTER)
    empty = pl.check_limits(0.05, lim)                      # before the table was filled once
    assert not empty["max_abs"].any() and (empty["arg"] == -1).all() and not empty["violated"].any() and not empty["feasible"].any()
    scene = rs.crafted(oracle.minco_generate)
    pad = rs.padded(scene)
    for k in range(len(pad["slots"])):
        sl = slice(k, k + 1)
        pl.install(pad["slots"][sl], pad["n_seg"][sl], pad["singul"][sl], pad["piece_nums"][sl], pad["coeff_dt"][sl], pad["coeffs"][sl],
                   pad["end_states"][sl], t_start=pad["t_start"][k])
    for dt in (0.05, 0.0371):
        ex, ref = _oracle_on_table(pl, Q, dt, lim)
        got = pl.check_limits(dt, lim)
        assert lc.same_rows(got, ref), dt
        assert _same_table(ex, [pl.executing(s) for s in range(Q)])                  # the table is unchanged, byte for byte
    occupied = np.array([e["n_seg"] > 0 for e in ex])
    assert occupied.sum() == 9 and (got["arg"][~occupied] == -1).all() and not got["max_abs"][~occupied].any()
    assert not got["feasible"][~occupied].any() and (got["arg"][occupied] >= 0).all()
    assert any(e["n_seg"] >= 2 and -1 in e["singul"][:e["n_seg"]] for e in ex)     # gear-shift plans among them
    # plan() with the filter on, then adopt: the slots' rows are the winners' rows of the call, bit for bit
    pp = hiplib.default_plan_params()
    pp.seed = lc.SEED
    pl.set_limit_filter(lim, lc.CHECK_DT)
    out = pl.plan(S, E, pp=pp)
    last = pl.last_limits(Q)
    queries, slots = [0, 1, 3, 4], [10, 11, 12, 13]
    ad = pl.adopt(queries, slots, t_start=3.0, pp=pp)
    assert ad.tolist() == [1, 1, 1, 0]                       # (query 4 has no feasible restart: see test_limit_filter)
    ex, ref = _oracle_on_table(pl, Q, lc.CHECK_DT, lim)
    got = pl.check_limits(lc.CHECK_DT, lim)
    assert lc.same_rows(got, ref)
    for q, s in zip(queries[:3], slots[:3]):
        w = int(out["winner"][q])
        assert w >= 0 and got["feasible"][s] == 1
        for k in lc.FIELDS:
            assert np.array_equal(got[k][s], last[k][q, w]), (q, k)
    assert got["arg"][13].tolist() == [-1] * 5 and ex[13]["n_seg"] == 0
    pl.close()
    h.close()


# The limits of FILTER and the queries they hit were chosen on the CPU from the oracle chain's own per-restart maxima:
#   import limits_cases as lc; from dftpav_amd import capi
#   l = capi.default_limits(); l.max_forward_vel, l.max_backward_vel, l.max_forward_cur, l.max_backward_cur = 5.01, 2.01, 1.01, 1.01
#   m = lc.chain_limits(l)
#   for q, e in enumerate(lc.chain()["per"]):
#       if e: print(q, lc.select(e["solve"]["final_cost"], e["solve"]["success"], e["collision"]),
#                   lc.select(e["solve"]["final_cost"], e["solve"]["success"], e["collision"] | (1 - m["feasible"][q])))
CHANGED = {1: (1, 3), 3: (1, 3), 8: (2, 3)}       # query: (winner without the filter, winner with it -- a dearer, feasible restart)
NO_VALID = {4: 3, 7: 3, 10: 0}                    # query: winner without the filter; with it every restart is rejected
KEPT = {0: 0, 2: 0, 5: 1, 6: 3, 9: 2, 11: 0}      # query: the winner either way


def test_limit_filter(hiplib):
    ch = lc.chain()
    grid, res, org, S, E = ch["scene"]
    Q = len(E)
    lim = _limits(hiplib, **FILTER)
    ref = lc.chain_limits(lim)
    pp = hiplib.default_plan_params()
    pp.seed = lc.SEED
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl0 = hiplib.Planner(h, Q, lc.R)                        # a planner that never had a filter
    plain = pl0.plan(S, E, pp=pp)
    with pytest.raises(hiplib.DftpavError) as e:
        pl0.last_limits(Q)                                  # that call ran without the filter
    assert e.value.code == hiplib.E_INVALID
    pl0.close()
    pl = hiplib.Planner(h, Q, lc.R)
    pl.set_limit_filter(lim, lc.CHECK_DT)
    out = pl.plan(S, E, pp=pp)
    last = pl.last_limits(Q)
    seen = dict(changed=0, none=0, kept=0)
    for q, c in enumerate(ch["per"]):
        if c is None or out["plan_status"][q] == hiplib.PLAN_LAYOUT_UNSUPPORTED:
            assert out["winner"][q] == -1 and (last["arg"][q] == -1).all() and not last["max_abs"][q].any() and not last["feasible"][q].any(), q
            continue
        r = c["solve"]
        w0 = lc.select(r["final_cost"], r["success"], c["collision"])
        w1 = lc.select(r["final_cost"], r["success"], c["collision"] | (1 - ref["feasible"][q]))
        print(q, "winner", w0, "->", w1, "device", plain["winner"][q], "->", out["winner"][q], "feasible", last["feasible"][q].tolist())
        assert plain["winner"][q] == w0 and out["winner"][q] == w1, q
        assert out["plan_status"][q] == (hiplib.PLAN_OK if w1 >= 0 else hiplib.PLAN_NO_VALID_RESTART), q
        for k in lc.FIELDS:
            assert np.array_equal(last[k][q], ref[k][q]), (q, k)
        assert np.array_equal(out["r_collision"][q], c["collision"]) and np.array_equal(out["r_first_sample"][q], c["first"]), q
        for k in ("r_final_cost", "r_status", "r_success", "r_iters", "r_evals", "r_collision", "r_first_sample"):
            assert np.array_equal(out[k][q], plain[k][q]), (q, k)
        if q in CHANGED:
            assert (w0, w1) == CHANGED[q] and r["final_cost"][w1] > r["final_cost"][w0] and ref["feasible"][q, w1] == 1
            assert out["final_cost"][q] == r["final_cost"][w1] and np.array_equal(out["coeffs"][q, :c["layout"].n_pieces], c["coeffs"][w1])
            seen["changed"] += 1
        elif q in NO_VALID:
            assert w0 == NO_VALID[q] and w1 == -1 and not out["coeffs"][q].any()
            seen["none"] += 1
        else:
            assert w0 == w1 == KEPT[q] and np.array_equal(out["coeffs"][q], plain["coeffs"][q])
            seen["kept"] += 1
    assert seen == dict(changed=len(CHANGED), none=len(NO_VALID), kept=len(KEPT))
    # a refused change of the filter leaves it as it is
    for bad_l, bad_dt in ((_limits(hiplib, max_latacc=NAN), 0.05), (_limits(hiplib, max_steer=0.0), 0.05), (lim, 0.0), (lim, NAN), (lim, INF)):
        with pytest.raises(hiplib.DftpavError) as e:
            pl.set_limit_filter(bad_l, bad_dt)
        assert e.value.code == hiplib.E_INVALID
    again = pl.plan(S, E, pp=pp)
    for k in out:
        assert np.array_equal(again[k], out[k], equal_nan=True), k
    assert lc.same_rows(pl.last_limits(Q), last)
    # the filter set back to NULL: the bits of a planner that never had one
    pl.set_limit_filter(None)
    off = pl.plan(S, E, pp=pp)
    for k in plain:
        assert np.array_equal(off[k], plain[k], equal_nan=True), k
    pl.close()
    h.close()


def test_tick_with_the_filter_keeps_the_plan_of_a_rejected_replanning(hiplib):
    """every restart of a replanning violates a velocity limit of 0.01 m/s: the query ends NO_VALID_RESTART and the slot keeps its plan,
    byte for byte; the same tick with the filter off replaces it"""
    grid, res, org, S, E = lc.chain()["scene"]
    Q = len(E)
    pp = hiplib.default_plan_params()
    pp.seed = lc.SEED
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl = hiplib.Planner(h, Q, lc.R)
    out = pl.plan(S, E, pp=pp)
    ok = np.flatnonzero((out["plan_status"] == hiplib.PLAN_OK) & (out["winner"] >= 0))
    pl.adopt(ok, ok, t_start=0.0, pp=pp)
    before = [pl.executing(q) for q in range(Q)]
    total = {int(q): float(before[q]["end_time"][before[q]["n_seg"] - 1]) for q in ok}
    c = min([q for q in total if before[q]["n_seg"] == 1], key=lambda q: total[q])   # the shortest plan of one gear segment
    pl.clear([q for q in range(Q) if q != c])
    # at 0.4 of it with the goal moved by 0.6 m: near, no turn point ahead, the target moved -- CheckReplan asks for a new plan
    t_now, budget = 0.4 * total[c], 0.5
    goals = E.copy()
    goals[c, 0] += 0.6
    pl.set_limit_filter(_limits(hiplib, max_forward_vel=0.01, max_backward_vel=0.01), lc.CHECK_DT)
    tk = pl.tick(t_now, budget, end_states=goals, pp=pp)
    assert tk["query_slot"].tolist() == [c]
    print("plan_status with the filter:", tk["plan"]["plan_status"].tolist(), "r_success", tk["plan"]["r_success"].tolist())
    last = pl.last_limits(1)
    assert tk["plan"]["plan_status"][0] == hiplib.PLAN_NO_VALID_RESTART and tk["plan"]["winner"][0] == -1
    assert tk["plan"]["r_success"][0].any() and not last["feasible"][0].any() and (last["violated"][0, :, 0] == 1).all()
    assert all(np.array_equal(np.asarray(pl.executing(c)[k]), np.asarray(before[c][k])) for k in EXEC_KEYS)
    pl.set_limit_filter(None)
    tk2 = pl.tick(t_now, budget, end_states=goals, pp=pp)
    assert tk2["query_slot"].tolist() == [c] and tk2["plan"]["plan_status"][0] == hiplib.PLAN_OK
    for k in ("r_final_cost", "r_success", "r_collision", "r_first_sample"):
        assert np.array_equal(tk2["plan"][k], tk["plan"][k]), k
    ex = pl.executing(c)
    assert ex["start_time"][0] == t_now + budget and np.array_equal(ex["coeffs"], tk2["plan"]["coeffs"][0])
    pl.close()
    h.close()


def test_refusals_leave_outputs_and_state_untouched(hiplib):
    p = hiplib.default_params()
    s = sc.make_scenario([2], [1], 8, 8, 2, seed=5, n_obs=10)
    s.apply_resolution(p)
    h = hiplib.Handle(p)
    bt = hiplib.Batch(h, s.layout, s.B)
    lim = hiplib.default_limits(p)
    fb = hiplib.lib().dftpav_batch_check_limits
    fb.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    fp = hiplib.lib().dftpav_planner_check_limits
    fp.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]

    def untouched(fn, obj, n, dt, l):
        out = hiplib.LimitsOut(n)
        for a in out.a.values():
            a[...] = 77
        assert fn(obj, dt, C.byref(l) if l is not None else None, C.byref(out.c)) == hiplib.E_INVALID
        assert all((a == 77).all() for a in out.a.values())

    untouched(fb, bt._b, s.B, 0.05, lim)                     # nothing uploaded, nothing solved
    bt.upload(s)
    untouched(fb, bt._b, s.B, 0.05, lim)                     # no solved coefficients
    bt.solve()
    good = bt.check_limits(0.05, lim)
    bad = [(0.0, lim), (-0.05, lim), (NAN, lim), (INF, lim), (0.05, None)]
    for f in plim.LIMIT_FIELDS:
        bad += [(0.05, _limits(hiplib, **{f: 0.0})), (0.05, _limits(hiplib, **{f: -1.0})), (0.05, _limits(hiplib, **{f: NAN}))]
    for dt, l in bad:
        untouched(fb, bt._b, s.B, dt, l)
    assert fb(bt._b, 0.05, C.byref(lim), None) == hiplib.E_INVALID
    assert lc.same_rows(bt.check_limits(0.05, lim), good)    # and the batch is as it was
    pl = hiplib.Planner(h, 3, 2)
    for dt, l in bad:
        untouched(fp, pl._p, 3, dt, l)
    with pytest.raises(hiplib.DftpavError) as e:
        pl.last_limits(1)                                    # no call to read
    assert e.value.code == hiplib.E_INVALID
    pl.close()
    bt.close()
    h.close()
