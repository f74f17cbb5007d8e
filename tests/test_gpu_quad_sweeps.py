"""The four substitution sweeps of the QUAD shape at 16 pieces (dftpav_amd/csrc/solver_ref4.hip: sweep4_split) after their diet: the
two end blocks of a traversal stand outside the loops, a loop of seven interior steps per set holds interior code only, and every
step ends by fetching the neighbour's rows for the next one.

Bar: every evaluation's cost and gradient, and every output of every solve (x, cost, status, iterations, evaluations, hist_sum,
success), BIT-EQUAL to the restatement of the reference (oracle/pyoracle.py, order 0).  Reference order, QUAD shape forced
(DFTPAV_REF_SHAPE=quad; the plan is asked what it picked).

Shapes: the smallest at which the split sweep can go wrong -- 16 pieces with K = 4 points per piece (n = 31), so that both end blocks
and the hand-over between the two sets at the ninth step (row_ror) run in every row that is there; 4 and 8 trajectories (one full wave,
two), 1 and 3 (a wave with rows that are not there: EXEC holds whole rows only), 5 (a full wave and one with a single row).  Other
piece counts take the plain traversal beside it (quad_common.h: quad_sweep, the one solver_ref4m.hip runs for several segments): 15
(its longest), 8, 3 (one interior block) and 2 (both blocks are end blocks, and the prefetched interior table is its zero branch).
A memory of 8 and a handful of iterations per solve.
"""
import ctypes as C

import numpy as np
import pytest

from dftpav_amd import scenarios as sc

pytestmark = pytest.mark.gpu

KEYS = ("final_cost", "x", "status", "iters", "evals", "hist_sum", "success")
MAX_ITER = 6


def _check(hiplib, oracle, monkeypatch, pieces, B, order2_too=False):
    p = hiplib.default_params()
    s = sc.make_scenario([pieces], [1], 4, 4, B, seed=1600 + 16 * pieces + B, n_obs=30)
    s.apply_resolution(p)
    p.lbfgs_mem_size = 8
    p.lbfgs_max_iterations = MAX_ITER
    want = oracle.solve_batch(p, s, nthreads=8, order=0)
    monkeypatch.setenv("DFTPAV_REF_SHAPE", "quad")
    monkeypatch.setenv("DFTPAV_REF_QUAD_WAVES", "1")
    h = hiplib.Handle(p)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    bt.set_order(hiplib.ORDER_REFERENCE)
    fn = hiplib.lib().dftpav_debug_reference_plan
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 8)()
    assert fn(C.byref(s.layout.c_struct()), C.byref(p), 0, s.B, 256, out) == 0
    assert int(out[1]) == 3, "the plan did not pick the QUAD shape"
    monkeypatch.delenv("DFTPAV_REF_SHAPE")
    monkeypatch.delenv("DFTPAV_REF_QUAD_WAVES")
    assert bt.x0().shape[1] == 2 * pieces - 1
    rng = np.random.default_rng(16 * pieces + B)
    for x in (bt.x0(), bt.x0() + rng.normal(0, 0.2, bt.x0().shape), bt.x0() + rng.normal(0, 0.7, bt.x0().shape)):
        f, g = bt.eval(x)
        for b in range(s.B):
            fo, go = oracle.OracleProblem(p, s, b, order=0).eval(x[b])
            assert f[b] == fo and np.array_equal(g[b], go), (pieces, B, b)
    bt.set_hand_over(0)  # the QUAD launch finishes every trajectory itself
    r = bt.solve()
    print("pieces", pieces, "B", B, "iters", r["iters"], "evals", r["evals"])
    for k in KEYS:
        assert np.array_equal(r[k], want[k]), (pieces, B, k)
    assert (r["evals"] >= 2).all(), r["evals"]  # (a solve is more than its first evaluation)
    if order2_too:  # the restatement with correctly rounded cos / sin: one segment has no junction angle, so the same solves
        want2 = oracle.solve_batch(p, s, nthreads=8, order=2)
        for k in KEYS:
            assert np.array_equal(r[k], want2[k]), (pieces, B, k, "order 2")
        # not vacuous: the adjoint sweeps ran on a gradient that the point terms touched (the oracle alone: 6 iterations in every row)
        assert (want2["iters"] >= 2).all() and (r["iters"] >= 2).all(), r["iters"]
    bt.close()
    h.close()


@pytest.mark.parametrize("B", [4, 8])
def test_full_waves(hiplib, oracle, monkeypatch, B):
    """One full wave, then two: both end blocks and the ninth step's hand-over in all four rows."""
    _check(hiplib, oracle, monkeypatch, 16, B)


@pytest.mark.parametrize("B", [1, 3])
def test_rows_that_are_not_there(hiplib, oracle, monkeypatch, B):
    """A wave with one row and with three: the lanes of the missing rows are off in every step, the fetches included."""
    _check(hiplib, oracle, monkeypatch, 16, B)


def test_a_full_wave_and_a_single_row(hiplib, oracle, monkeypatch):
    _check(hiplib, oracle, monkeypatch, 16, 5)


@pytest.mark.parametrize("pieces", [15, 8, 2, 3])
def test_other_piece_counts_take_the_generic_sweep(hiplib, oracle, monkeypatch, pieces):
    """N != 16: quad_sweep with one segment, one lane per piece and both dimensions on it -- the restatement's bits (order 0 and
    order 2), at least two iterations in every row."""
    _check(hiplib, oracle, monkeypatch, pieces, 5, order2_too=True)
