"""The read-out contract of every device timer behind the C-ABI: what each *_last_ms entry point (and dftpav_planner_info's stage_ms)
answers before any call has fed it -- DFTPAV_E_INVALID with the output untouched, or DFTPAV_OK with 0.0 -- and after exactly one
call that feeds it; what the two-part read-outs answer after a call that timed only one part; and the two orders of calls that once
depended on another entry point having created the events.  The read-outs are called raw, with -1.0 in every output beforehand.
No magnitude of a time is asserted."""
import ctypes as C

import numpy as np
import pytest

from dftpav_amd import replan_scenes as rs
from dftpav_amd import scenarios as sc

pytestmark = pytest.mark.gpu

UNTOUCHED = -1.0
RES, ORIGIN = 1.0, (-68.0, 12.0)      # 32 x 32 cells round the lanes of replan_scenes: x in [-68, -36], y in [12, 44]
T_NOW = 100.0
K = 2


def _grid():
    g = np.zeros((32, 32), dtype=np.uint8)
    g[2:4, 5:8] = 80                  # a few occupied cells, 12 m from the lane the plans run on
    return g


def _read(hiplib, name, obj, n_out=1, tail=()):
    """(return code, the floats left in outputs that held UNTOUCHED) of a read-out (object, float * n_out, further pointers)"""
    outs = [C.c_float(UNTOUCHED) for _ in range(n_out)]
    fn = getattr(hiplib.lib(), name)
    fn.argtypes = [C.c_void_p] + [C.POINTER(C.c_float)] * n_out + [C.c_void_p] * len(tail)
    fn.restype = C.c_int
    rc = fn(obj, *[C.byref(o) for o in outs], *tail)
    return rc, [float(o.value) for o in outs]


def _stage_ms(hiplib, pl):
    ms = np.full(4, UNTOUCHED, dtype=np.float32)
    fn = hiplib.lib().dftpav_planner_info
    fn.argtypes = [C.c_void_p] * 5
    fn.restype = C.c_int
    return fn(pl._p, None, None, None, ms.ctypes.data_as(C.c_void_p)), ms.astype(np.float64).tolist()


def _reported(v):
    return np.isfinite(v) and v >= 0.0


def _handle(hiplib, with_map=True):
    s = sc.baseline_config(1, B=2)
    h = hiplib.Handle(s.apply_resolution(hiplib.default_params()))
    if with_map:
        h.set_grid_map(_grid(), RES, ORIGIN)
    return h, s


def _solved(hiplib, with_map=True):
    """the 8-piece forward problem, B = 2, solved once in the default order on a fresh handle"""
    h, s = _handle(hiplib, with_map)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    bt.solve()
    return h, bt


def _planner(hiplib, oracle, install=True):
    """a planner of two slots on a fresh handle with the map; one plan along lane 1 installed in slot 0, a second into its 12 s"""
    h = hiplib.Handle()
    h.set_grid_map(_grid(), RES, ORIGIN)
    pl = hiplib.Planner(h, 2, 1)
    if install:
        plan = rs.plan_a(oracle.minco_generate, 1)
        plan["t_start"], plan["hist"] = T_NOW - 1.0, None
        pad = rs.padded(dict(slots=[plan, None]))
        pl.install(pad["slots"], pad["n_seg"], pad["singul"], pad["piece_nums"], pad["coeff_dt"], pad["coeffs"], pad["end_states"],
                   t_start=pad["t_start"][0])
    return h, pl


# ------------------------------------------------- before any timed call
def test_handle_read_outs_before_any_timed_call(hiplib):
    h, _ = _handle(hiplib)
    for name in ("dftpav_corridor_last_ms", "dftpav_limits_last_ms", "dftpav_goal_field_last_ms"):
        assert _read(hiplib, name, h._h) == (hiplib.E_INVALID, [UNTOUCHED]), name
    assert _read(hiplib, "dftpav_rs_table_last_ms", h._h, 1, (None,)) == (hiplib.E_INVALID, [UNTOUCHED])
    assert _read(hiplib, "dftpav_clearance_last_ms", h._h, 2) == (hiplib.OK, [0.0, 0.0])
    assert _read(hiplib, "dftpav_conflicts_last_ms", h._h, 2) == (hiplib.OK, [0.0, 0.0])
    h.close()


def test_planner_read_outs_before_any_timed_call(hiplib, oracle):
    h, pl = _planner(hiplib, oracle)
    assert _read(hiplib, "dftpav_replan_last_ms", pl._p, 2) == (hiplib.OK, [0.0, 0.0])
    assert _read(hiplib, "dftpav_publish_last_ms", pl._p) == (hiplib.OK, [0.0])
    assert _stage_ms(hiplib, pl) == (hiplib.OK, [0.0] * 4)
    assert _read(hiplib, "dftpav_conflicts_last_ms", h._h, 2) == (hiplib.OK, [0.0, 0.0])   # (installing a plan feeds nothing)
    pl.close()
    h.close()


def test_batch_read_out_before_any_solve(hiplib):
    h, s = _handle(hiplib)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    assert _read(hiplib, "dftpav_batch_last_solve_ms", bt._b) == (hiplib.E_INVALID, [UNTOUCHED])
    bt.close()
    h.close()


# ------------------------------------------------- after exactly one call that feeds the timer
def test_solve_ms_after_one_solve(hiplib):
    h, bt = _solved(hiplib)
    rc, (ms,) = _read(hiplib, "dftpav_batch_last_solve_ms", bt._b)
    assert rc == hiplib.OK and _reported(ms)
    assert _read(hiplib, "dftpav_corridor_last_ms", h._h) == (hiplib.E_INVALID, [UNTOUCHED])   # a solve is no corridor-family call
    bt.close()
    h.close()


def test_corridor_ms_after_one_corridor_call(hiplib):
    h, _ = _handle(hiplib)
    h.corridor_rectangles([[-60.0, 28.0, 0.0]])
    rc, (ms,) = _read(hiplib, "dftpav_corridor_last_ms", h._h)
    assert rc == hiplib.OK and _reported(ms)
    h.close()


def test_limits_ms_after_one_check(hiplib):
    h, bt = _solved(hiplib)
    bt.check_limits(0.05)
    rc, (ms,) = _read(hiplib, "dftpav_limits_last_ms", h._h)
    assert rc == hiplib.OK and _reported(ms)
    bt.close()
    h.close()


def test_limits_ms_after_one_check_of_the_table(hiplib, oracle):
    h, pl = _planner(hiplib, oracle)
    pl.check_limits(0.05)
    rc, (ms,) = _read(hiplib, "dftpav_limits_last_ms", h._h)
    assert rc == hiplib.OK and _reported(ms)
    pl.close()
    h.close()


def test_clearance_ms_first_check_builds_the_field_and_the_second_does_not(hiplib):
    h, bt = _solved(hiplib)
    bt.check_clearance(0.05)
    rc, (field, check) = _read(hiplib, "dftpav_clearance_last_ms", h._h, 2)
    assert rc == hiplib.OK and _reported(field) and _reported(check)
    # a second check on the same map builds no field: the field's pair of events is not recorded again, and field_ms goes on
    # reporting the last build -- the same two events, so the same value
    bt.check_clearance(0.05)
    rc, (field2, check2) = _read(hiplib, "dftpav_clearance_last_ms", h._h, 2)
    assert rc == hiplib.OK and field2 == field and _reported(check2)
    bt.close()
    h.close()


def test_clearance_ms_after_one_check_of_the_table(hiplib, oracle):
    h, pl = _planner(hiplib, oracle)
    pl.check_clearance(0.05)
    rc, (field, check) = _read(hiplib, "dftpav_clearance_last_ms", h._h, 2)
    assert rc == hiplib.OK and _reported(field) and _reported(check)
    pl.close()
    h.close()


def test_conflict_ms_poses_alone_then_the_whole_check(hiplib, oracle):
    h, pl = _planner(hiplib, oracle)
    pl.sample_poses(T_NOW, 0.5, K)
    rc, (pose, pair) = _read(hiplib, "dftpav_conflicts_last_ms", h._h, 2)
    assert rc == hiplib.OK and _reported(pose) and pair == 0.0
    pl.check_conflicts(T_NOW, 0.5, K)
    rc, (pose, pair) = _read(hiplib, "dftpav_conflicts_last_ms", h._h, 2)
    assert rc == hiplib.OK and _reported(pose) and _reported(pair)
    pl.sample_poses(T_NOW, 0.5, K)      # the poses alone again: the pair time of the call before is no longer reported
    rc, (pose, pair) = _read(hiplib, "dftpav_conflicts_last_ms", h._h, 2)
    assert rc == hiplib.OK and _reported(pose) and pair == 0.0
    pl.close()
    h.close()


def test_conflict_ms_after_one_check(hiplib, oracle):
    h, pl = _planner(hiplib, oracle)
    pl.check_conflicts(T_NOW, 0.5, K)
    rc, (pose, pair) = _read(hiplib, "dftpav_conflicts_last_ms", h._h, 2)
    assert rc == hiplib.OK and _reported(pose) and _reported(pair)
    pl.close()
    h.close()


def test_goal_field_ms_after_one_build(hiplib):
    h, _ = _handle(hiplib)
    h.goal_field([[-50.0, 28.0]], fetch=False)
    rc, (ms,) = _read(hiplib, "dftpav_goal_field_last_ms", h._h)
    assert rc == hiplib.OK and _reported(ms)
    h.close()


def test_rs_table_ms_after_one_build(hiplib):
    h, _ = _handle(hiplib, with_map=False)
    assert h.rs_table(max_cur=1.0, n_yaw=4, extent=1.0, cell=0.5).shape == (4, 5, 5)
    builds = C.c_int(-1)
    rc, (ms,) = _read(hiplib, "dftpav_rs_table_last_ms", h._h, 1, (C.byref(builds),))
    assert rc == hiplib.OK and _reported(ms) and builds.value == 1
    h.close()


def test_replan_ms_check_alone_then_a_tick(hiplib, oracle):
    h, pl = _planner(hiplib, oracle)
    pl.check(T_NOW, 0.5)
    rc, (check, tick) = _read(hiplib, "dftpav_replan_last_ms", pl._p, 2)
    assert rc == hiplib.OK and _reported(check) and tick == 0.0
    out = pl.tick(T_NOW, 0.5)
    assert len(out["query_slot"]) == 0      # the plan has 11 s left on a free lane: the tick is its check alone
    rc, (check, tick) = _read(hiplib, "dftpav_replan_last_ms", pl._p, 2)
    assert rc == hiplib.OK and _reported(check) and _reported(tick)
    pl.close()
    h.close()


def test_replan_ms_after_one_tick(hiplib, oracle):
    h, pl = _planner(hiplib, oracle)
    pl.tick(T_NOW, 0.5)
    rc, (check, tick) = _read(hiplib, "dftpav_replan_last_ms", pl._p, 2)
    assert rc == hiplib.OK and _reported(check) and _reported(tick)      # (a tick runs the check)
    pl.close()
    h.close()


def test_publish_ms_after_one_publish(hiplib, oracle):
    h, pl = _planner(hiplib, oracle)
    pl.publish([T_NOW, T_NOW + 0.01])
    rc, (ms,) = _read(hiplib, "dftpav_publish_last_ms", pl._p)
    assert rc == hiplib.OK and _reported(ms)
    pl.close()
    h.close()


def test_stage_ms_after_one_plan(hiplib, oracle):
    h, pl = _planner(hiplib, oracle, install=False)
    out = pl.plan([[-60.0, 28.0, 0.0, 0.0]], [[-48.0, 28.0, 0.0, 0.0]])
    print("plan_status", out["plan_status"])
    rc, ms = _stage_ms(hiplib, pl)
    assert rc == hiplib.OK and all(_reported(v) for v in ms)
    rc, (cor,) = _read(hiplib, "dftpav_corridor_last_ms", h._h)      # the planner's stages are not the handle's corridor span
    assert (rc, cor) == (hiplib.E_INVALID, UNTOUCHED)
    pl.close()
    h.close()


# ------------------------------------------------- orders of calls that must not depend on another entry point
def test_validate_as_the_first_step_call_after_the_map(hiplib):
    h, bt = _solved(hiplib)
    col, first = bt.validate(0.05, 0.1)
    assert col.shape == (2,) and first.shape == (2,)
    rc, (ms,) = _read(hiplib, "dftpav_corridor_last_ms", h._h)
    assert rc == hiplib.OK and _reported(ms)
    bt.close()
    h.close()


def test_limits_on_a_handle_that_never_had_a_map(hiplib):
    h, bt = _solved(hiplib, with_map=False)
    out = bt.check_limits(0.05)
    assert out["feasible"].shape == (2,)
    rc, (ms,) = _read(hiplib, "dftpav_limits_last_ms", h._h)
    assert rc == hiplib.OK and _reported(ms)
    assert _read(hiplib, "dftpav_corridor_last_ms", h._h) == (hiplib.E_INVALID, [UNTOUCHED])
    bt.close()
    h.close()
