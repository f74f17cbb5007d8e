"""The interior steps of the QUAD shape's four substitution sweeps at 16 pieces in SELECT form (dftpav_amd/csrc/solver_ref4.hip:
sweep4_split): every lane runs every interior step on its own block of the table and its own rows, and only the step's owner keeps
the result (R = own ? acc : R); the table rows of a traversal's last end block are requested in front of its second loop.

Bar: every evaluation's cost and gradient, and every output of every solve (x, cost, status, iterations, evaluations, hist_sum,
success), BIT-EQUAL to the restatement of the reference in order 2 (oracle/pyoracle.py; one segment has no junction angle, so
order 0 gives the same solves and is compared too).  Reference order, QUAD shape forced (the plan is asked what it picked).

What can go wrong in this form and which case would show it: a lane that is not the owner keeps a row (any case: the solve and
solveAdj results of every piece enter g); a lane of a row that is not there takes part (1, 3 and 5 trajectories: waves with one and
with three rows present, a full wave beside a single row); the rows requested ahead are another block's or arrive late (the last
end block closes every traversal: all cases).  On each of the kernel's three instances (the sweeps are compiled into each):
<true, true> -- H = 4, help_eps = 0, rectangle corridors, BASELINE configs[3]'s layout --, <true, false> (DFTPAV_RECT_CORRIDOR=0)
and <false, false> (help_eps != 0).  15 pieces still take the plain traversal (quad_common.h: quad_sweep) and keep its bits.

Shapes: 16 pieces with K = 4 points per piece (n = 31), a memory of 8 and six iterations: both end blocks, the fourteen interior
steps and the hand-over between the two sets run in every evaluation of every row that is there.
"""
import ctypes as C

import numpy as np
import pytest

from dftpav_amd import scenarios as sc

pytestmark = pytest.mark.gpu

KEYS = ("final_cost", "x", "status", "iters", "evals", "hist_sum", "success")
INSTANCES = ("fast_rect", "fast_general", "plain")


def _instance(s, instance):
    if instance == "fast_general":
        return (("DFTPAV_RECT_CORRIDOR", "0"),)
    if instance == "plain":
        s.help_eps = 1e-3
    return ()


def _check(hiplib, oracle, monkeypatch, p, s, env, pieces=16, n_points=3):
    s.apply_resolution(p)
    p.lbfgs_mem_size = 8
    p.lbfgs_max_iterations = 6
    want = oracle.solve_batch(p, s, nthreads=8, order=2)
    env = (("DFTPAV_REF_SHAPE", "quad"), ("DFTPAV_REF_QUAD_WAVES", "1")) + tuple(env)
    for k, v in env:
        monkeypatch.setenv(k, v)
    h = hiplib.Handle(p)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    bt.set_order(hiplib.ORDER_REFERENCE)
    fn = hiplib.lib().dftpav_debug_reference_plan
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 8)()
    assert fn(C.byref(s.layout.c_struct()), C.byref(p), 0, s.B, 256, out) == 0
    assert int(out[1]) == 3, "the plan did not pick the QUAD shape"
    for k, _ in env:
        monkeypatch.delenv(k)
    rng = np.random.default_rng(31 * s.B + len(env))
    x0 = bt.x0()
    assert x0.shape[1] == 2 * pieces - 1  # (n = 2 N - 1: the layout has the pieces the case is about)
    for x in (x0, x0 + rng.normal(0, 0.2, x0.shape), x0 + rng.normal(0, 0.7, x0.shape))[:n_points]:
        f, g = bt.eval(x)
        for b in range(s.B):
            fo, go = oracle.OracleProblem(p, s, b, order=2).eval(x[b])
            assert f[b] == fo and np.array_equal(g[b], go), (s.B, b)
    bt.set_hand_over(0)  # the QUAD launch finishes every trajectory itself
    r = bt.solve()
    bt.close()
    h.close()
    print("B", s.B, "iters", r["iters"], "evals", r["evals"])
    for k in KEYS:
        assert np.array_equal(r[k], want[k]), (s.B, k)
    # not vacuous: the adjoint sweeps ran on gradients that moved the point
    assert (want["iters"] >= 2).all() and (r["evals"] >= 2).all(), (want["iters"], r["evals"])
    want0 = oracle.solve_batch(p, s, nthreads=8, order=0)
    for k in KEYS:
        assert np.array_equal(r[k], want0[k]), (s.B, k, "order 0")


@pytest.mark.parametrize("instance", INSTANCES)
@pytest.mark.parametrize("B", [1, 3, 4, 5])
def test_sixteen_pieces(hiplib, oracle, monkeypatch, B, instance):
    """One row, three rows, a full wave, a full wave and a single row."""
    p = hiplib.default_params()
    s = sc.make_scenario([16], [1], 4, 4, B, seed=2600 + B, n_obs=30)
    _check(hiplib, oracle, monkeypatch, p, s, _instance(s, instance), pieces=16)


@pytest.mark.parametrize("instance", INSTANCES)
def test_baseline_layout(hiplib, oracle, monkeypatch, instance):
    """BASELINE configs[3]'s own layout and corridors (rectangles: the value line's instance by default), five trajectories."""
    p = hiplib.default_params()
    s = sc.baseline_config(3, B=5)
    _check(hiplib, oracle, monkeypatch, p, s, _instance(s, instance), n_points=1)


def test_fifteen_pieces_take_the_plain_traversal(hiplib, oracle, monkeypatch):
    """N = 15: quad_sweep, one lane per piece with both dimensions on it -- untouched, the same bits."""
    p = hiplib.default_params()
    s = sc.make_scenario([15], [1], 4, 4, 5, seed=2615, n_obs=30)
    _check(hiplib, oracle, monkeypatch, p, s, (), pieces=15)
