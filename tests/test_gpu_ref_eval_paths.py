"""Which pass of ref_eval (dftpav_amd/csrc/solver_ref.hip) an evaluation takes, proved case by case.

What the active terms of an evaluation add to gdC, gdT and the costs is stated once (chain_add, ref_order_common.h) and walked by three
passes: the 16-lane serial pass and the wide pass of the WAVE shape, the window pass of the TEAM shape.  Which pass runs depends on
the number of active terms alone, so every case here asserts that number before it compares bits:

  * the evaluation (Batch.eval) is bit-equal in cost and gradient to the restatement (oracle.OracleProblem, order 2; order 0 where there
    is neither a junction nor an obstacle);
  * the evaluation launch does not write the profile (Prof::start: solves only), so the same point is then SOLVED with
    lbfgs_g_epsilon = 1e300: lbfgs_optimize returns after its first evaluation, which is the evaluation above (evals == 1, the same
    cost), and slot 9 / 10 of read_profile() are that evaluation's active terms / "its records went past the LDS window".

The thresholds are read from ref_order_common.h, not repeated here.  The point of a case is the scenario's own x0: the waypoints of the
scenario are displaced (seeded) before the upload, so eval, solve and oracle start from the same x.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dftpav_amd import scenarios as sc

pytestmark = pytest.mark.gpu

_HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dftpav_amd", "csrc", "ref_order_common.h")


def _threshold(name):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(_HDR).read())
    assert m, name
    return int(m.group(1))


_KIND = {"team": 0, "wave": 1, "quad": 5}   # RefKind of device_types.h (5: the QUAD shape for several segments)


def _assert_planned_shape(hiplib, monkeypatch, p, s, shape, S=0):
    """DFTPAV_REF_SHAPE only asks: the plan is asked what a batch like this one takes (the evaluation of a QUAD plan runs in its
    WAVE shape, capi.cpp: the read-outs)."""
    fn = hiplib.lib().dftpav_debug_reference_plan
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 8)()
    monkeypatch.setenv("DFTPAV_REF_SHAPE", shape)
    assert fn(C.byref(s.layout.c_struct()), C.byref(p), S, s.B, 256, out) == 0
    monkeypatch.delenv("DFTPAV_REF_SHAPE")
    assert int(out[0]) == 1 and int(out[1]) == _KIND[shape], (shape, list(out))


def _first_evaluation(hiplib, monkeypatch, s, shape, surround=False):
    """-> (p, f, g, x, terms, slot 10, batch, handle) of the evaluation at the scenario's x0 in the given shape"""
    p = hiplib.default_params()
    s.apply_resolution(p)
    p.lbfgs_g_epsilon = 1e300      # the solve ends after its first evaluation (lbfgs.hpp:537-541)
    _assert_planned_shape(hiplib, monkeypatch, p, s, shape, S=len(s.surround.start_time) if surround else 0)
    h = hiplib.Handle(p)
    if surround:
        h.set_surround(s.surround)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    monkeypatch.setenv("DFTPAV_REF_SHAPE", shape)
    bt.set_order(hiplib.ORDER_REFERENCE)
    monkeypatch.delenv("DFTPAV_REF_SHAPE")
    x = bt.x0()
    f, g = bt.eval(x)
    bt.profile(True)
    r = bt.solve()
    prof = bt.read_profile()
    bt.profile(False)
    assert (r["evals"] == 1).all() and np.array_equal(r["final_cost"], f) and np.array_equal(r["x"], x)
    return p, f, g, x, prof[:, 9], prof[:, 10], bt, h


def _displaced_cfg3(B, sigma, seed):
    """the configs[2] layout (16 pieces, 33 points per piece, H = 4: 528 points), every inner waypoint moved by N(0, sigma)"""
    if sigma == 0.0:   # at x0 a trajectory has 0 ... 60 active terms: the rows that have some and keep them all in the LDS window
        return sc.baseline_config(3, B=32).subset(_FEW_TERM_ROWS[:B])
    s = sc.baseline_config(3, B=B)
    if sigma > 0.0:
        s.inner_pts = np.ascontiguousarray(s.inner_pts + np.random.default_rng(seed).normal(0.0, sigma, s.inner_pts.shape))
    return s


# rows of baseline_config(3, B=32) that have 26, 28, 22 and 15 active terms at x0 (its 32 rows have 0 ... 136; kRecWave is 48)
_FEW_TERM_ROWS = [3, 8, 9, 11]

# (shape, displacement of the waypoints in metres, seed)
_CASES = {
    "wave_serial_in_lds": ("wave", 0.0, 0),
    "wave_serial_past_window": ("wave", 0.7, 5),
    "wave_wide": ("wave", 30.0, 7),
    "team_one_window": ("team", 0.7, 5),
    "team_several_windows": ("team", 30.0, 7),
}


@pytest.mark.parametrize("case", list(_CASES))
def test_every_chain_pass_is_reached_and_has_the_reference_bits(hiplib, oracle, monkeypatch, case):
    """configs[2] layout, 4 trajectories.  x0: a few active terms; waypoints moved by N(0, 0.7): hundreds; by N(0, 30): most points
    lie far outside their corridor, four vertices against two or more half-planes each and the feasibility terms -- thousands."""
    shape, sigma, seed = _CASES[case]
    rec_wave, serial_max, list_cap = _threshold("kRecWave"), _threshold("kSerialMax"), _threshold("kListCapTeam")
    s = _displaced_cfg3(4, sigma, seed)
    p, f, g, x, terms, past, bt, h = _first_evaluation(hiplib, monkeypatch, s, shape)
    print(case, "active terms", terms.tolist(), "past the window", past.tolist())
    if case == "wave_serial_in_lds":
        assert ((terms > 0) & (terms <= rec_wave)).all(), terms
        assert (past == 0).all()
    elif case == "wave_serial_past_window":
        assert ((terms > rec_wave) & (terms <= serial_max)).all(), terms
        assert (past == 1).all()
    elif case == "wave_wide":
        assert (terms > serial_max).all(), terms
    elif case == "team_one_window":
        assert ((terms > 0) & (terms <= list_cap)).all(), terms
    else:
        assert (terms > list_cap).all(), terms
    for b in range(s.B):
        for order in (0, 2):   # one segment, no obstacle: no libm call, both orders are the reference's bits
            fo, go = oracle.OracleProblem(p, s, b, order=order).eval(x[b])
            assert f[b] == fo and np.array_equal(g[b], go), (case, b, order, f[b], fo)
    bt.close()
    h.close()


def _two_segments_among_cars(B):
    """7 + 6 pieces with a gear shift among the four cars of dynamicObs.yaml, obstacle clocks that differ from the ego's (the layout and
    seed of test_gear_shifts_with_moving_obstacles_in_reference_order)"""
    s = sc.make_scenario([7, 6], [1, -1], 12, 16, B, seed=81, with_moving=True, n_obs=25, start_centre=(-38.0, 5.0))
    s.surround.start_time[:] = [0.5, 0.0, 1.5, 0.25]
    s.t_now = 0.6
    return s


@pytest.mark.parametrize("shape", ["wave", "team"])
def test_obstacle_terms_on_the_second_segment(hiplib, oracle, monkeypatch, shape):
    """Two segments (7 + 6 pieces) among the four moving cars: an obstacle term of segment 1 adds `* pieceid`, `* Nseg` and one more
    addend per previous segment to that segment's gdT (traj_optimizer.cpp:1663-1676).  Every trajectory of the case has the
    moving-obstacle cost of segment 1 above zero (dftpav_batch_cost_terms)."""
    s = _two_segments_among_cars(64).subset(_SECOND_SEGMENT_ROWS)
    p, f, g, x, terms, past, bt, h = _first_evaluation(hiplib, monkeypatch, s, shape, surround=True)
    _, seg = bt.cost_terms(x)
    print(shape, "active terms", terms.tolist(), "moving-obstacle cost of segment 1", seg[:, 1, hiplib.TERM_SURROUND].tolist())
    assert (seg[:, 1, hiplib.TERM_SURROUND] > 0.0).all(), seg[:, :, hiplib.TERM_SURROUND]
    assert (terms > 0).all()
    for b in range(s.B):
        fo, go = oracle.OracleProblem(p, s, b, order=2).eval(x[b])
        assert f[b] == fo and np.array_equal(g[b], go), (shape, b, f[b], fo, np.abs(g[b] - go).max())
    bt.close()
    h.close()


# rows of _two_segments_among_cars(64) whose second segment meets an obstacle at x0: costs(1) of segment 1 is 19 721, 22 888, 4 466, 20 964
_SECOND_SEGMENT_ROWS = [0, 2, 4, 6]


@pytest.mark.parametrize("mem", [8, 12])
@pytest.mark.parametrize("shape", ["wave", "quad"])
def test_recursion_ring_wraps_inside_a_block(hiplib, oracle, monkeypatch, shape, mem):
    """Both double-buffered block loops of the two-loop recursion -- two_loop<CAP, EXACT> of the WAVE shape (blocks of 8 pairs) and
    q4m_two_loop of the gear-shift QUAD shape (blocks of 4): solves long enough to fill the history and wrap its ring.  mem = 8: one block of 8 exactly; mem = 12: the ring wraps inside a
    block of 8 and of 4.  BASELINE configs[1] (8 + 8 pieces with a gear shift), 3 trajectories, bit-equal to order 2."""
    p = hiplib.default_params()
    s = sc.baseline_config(2, B=3)
    s.apply_resolution(p)
    p.lbfgs_mem_size = mem
    _assert_planned_shape(hiplib, monkeypatch, p, s, shape)
    h = hiplib.Handle(p)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    monkeypatch.setenv("DFTPAV_REF_SHAPE", shape)
    bt.set_order(hiplib.ORDER_REFERENCE)
    monkeypatch.delenv("DFTPAV_REF_SHAPE")
    r = bt.solve()
    want = oracle.solve_batch(p, s, nthreads=3, order=2)
    assert (want["iters"] > 16).all(), want["iters"]
    for k in ("final_cost", "x", "status", "iters", "evals", "hist_sum", "success"):
        assert np.array_equal(r[k], want[k]), (shape, mem, k)
    bt.close()
    h.close()
