"""Every exit of the L-BFGS control of the reference order (dftpav_amd/csrc/lbfgs_control.h: lbfgs_advance, one state machine for
every solve shape) on every shape that runs it: the params that make lbfgs_optimize / line_search_lewisoverton leave through each of
their reachable returns (lbfgs.hpp:276-390, 524-745), solved in the TEAM, WAVE (two widths of the chain), QUAD (one segment: two
widths; several segments) and generic (n > 64) kernels, every field of every solve BIT-EQUAL to the restatement (oracle order 2).

Not reachable with finite inputs and not here: -1005 (an ascent direction), -1006 (a step <= 0), -1012 (a cost that is inf / nan).
"""
import numpy as np
import pytest

from dftpav_amd import scenarios as sc
from terms_cases import reference_plan

pytestmark = pytest.mark.gpu

KEYS = ("final_cost", "x", "status", "iters", "evals", "hist_sum", "success")
WAVE = {"DFTPAV_REF_SHAPE": "wave", "DFTPAV_REF_SLOTS": "2"}   # + a slice of 3, then 17 iterations (test_wave_shape_and_ring_are_bit_identical)
QUAD = {"DFTPAV_REF_SHAPE": "quad", "DFTPAV_REF_QUAD_WAVES": "1"}
QUAD_RING = {"DFTPAV_REF_SLOTS": "2", "DFTPAV_REF_SLICE": "5"}  # slices of 5 EVALUATIONS: suspend and resume fall inside line searches

# shape: pieces, gears, n, the kind of launch the plan must report (0 TEAM, 1 WAVE, 3 QUAD, 5 QUAD for several segments), what forces it
SHAPES = {
    "team_n15": ((8,), (1,), 15, 0, {}),
    "wave_n15": ((8,), (1,), 15, 1, WAVE),
    "wave_n39": ((20,), (1,), 39, 1, WAVE),
    "quad_n15": ((8,), (1,), 15, 3, QUAD),
    "quad_n31": ((16,), (1,), 31, 3, QUAD),
    "quad_n33_two_segments": ((8, 8), (1, -1), 33, 5, QUAD),
    "generic_n79": ((40,), (1,), 79, 0, {}),
}
# case: the params that force the exit, the status every trajectory ends with
CASES = {
    "max_iterations": ({"lbfgs_max_iterations": 3}, -1008),
    "max_linesearch": ({"lbfgs_max_linesearch": 2}, -1009),
    "min_step": ({"lbfgs_min_step": 0.5}, -1011),
    "max_step": ({"lbfgs_max_step": 1e-3}, -1010),
    "machine_prec": ({"lbfgs_machine_prec": 0.6}, -1007),
    "g_epsilon": ({"lbfgs_g_epsilon": 1e9}, 0),
    "past_delta": ({"lbfgs_past": 1, "lbfgs_delta": 0.1}, 1),
    "cautious_factor": ({"lbfgs_cautious_factor": 1e6}, 1),   # updates are refused: directions from a history that is not extended
}
RING_CASES = ("cautious_factor", "machine_prec")   # the QUAD shapes run these through a sliced ring


def _problem(hiplib, pieces, gears, case):
    p = hiplib.default_params()
    s = sc.make_scenario(list(pieces), list(gears), 4, 4, B=4, seed=11)
    s.apply_resolution(p)
    for name, value in CASES[case][0].items():
        setattr(p, name, value)
    return p, s


_WANT = {}


def _want(hiplib, oracle, pieces, gears, case):
    """the restatement's solves of a layout under a case's params: computed once, shared by the shapes of that layout, never changed"""
    key = (pieces, gears, case)
    if key not in _WANT:
        p, s = _problem(hiplib, pieces, gears, case)
        want = oracle.solve_batch(p, s, nthreads=4, order=2)
        for k in KEYS:
            want[k].setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_exit_of_the_control_on_every_shape(hiplib, oracle, monkeypatch, shape, case):
    pieces, gears, n, kind, env = SHAPES[shape]
    want = _want(hiplib, oracle, pieces, gears, case)
    status = CASES[case][1]
    if n != 39:   # (the layouts whose oracle runs were read when the cases were chosen; at n = 39 the oracle's status is the expectation)
        assert (want["status"] == status).all(), (shape, case, want["status"])
        if case == "g_epsilon":
            assert (want["evals"] == 1).all() and (want["iters"] == 0).all(), (shape, want["evals"], want["iters"])
        if case == "past_delta":   # (past = 1: the test of lbfgs.hpp:642-659 applies from k = 1 on, and one row of the n = 31 layout stops there)
            assert ((want["iters"] >= 1) & (want["iters"] <= 9)).all(), (shape, want["iters"])
        if case == "cautious_factor":
            assert ((want["evals"] >= 170) & (want["evals"] <= 2100)).all() and (want["hist_sum"] == 0).all(), (shape, want["evals"], want["hist_sum"])
    p, s = _problem(hiplib, pieces, gears, case)
    assert s.layout.n_vars == n
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    if env is QUAD and case in RING_CASES:
        for name, value in QUAD_RING.items():
            monkeypatch.setenv(name, value)
    for slice_ in ((3, 17) if env is WAVE else (None,)):
        if slice_ is not None:
            monkeypatch.setenv("DFTPAV_REF_SLICE", str(slice_))
        assert reference_plan(s, p) == kind, (shape, "the plan did not pick the shape under test")
        h = hiplib.Handle(p)
        bt = hiplib.Batch(h, s.layout, s.B)
        bt.upload(s)
        bt.set_order(hiplib.ORDER_REFERENCE)
        r = bt.solve()
        bt.close()
        h.close()
        for k in KEYS:
            assert np.array_equal(r[k], want[k]), (shape, case, slice_, k, r[k], want[k])
