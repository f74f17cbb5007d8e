"""The parked terms of the QUAD shape (dftpav_amd/csrc/solver_ref4.hip: q4_eval): what an active term adds to gdT and to the two costs
lives in one LDS pool per trajectory (kQPool = 64 entries in arrival order) and is chained afterwards in (piece, point, term) order
through a permutation table; a trajectory with more terms than the pool holds sends the surplus to global scratch and the wave
takes the piece-by-piece path.

Bar: every evaluation's cost and gradient, and every output of every solve (x, cost, status, iterations, evaluations, hist_sum,
success), BIT-EQUAL to the restatement of the reference (oracle/pyoracle.py, order 0).  Reference order, QUAD shape forced.

The term counts a case depends on come from the restatement, not from the kernel: active_terms() (tests/quad_cases.py) applies the activation tests
of addPVAGradCost2CT (oracle/dftpav_oracle.c: violaPos / violaVel / violaAcc / violaCurL / violaCurR > 0) to the coefficients the
oracle formed at the evaluated point (OracleProblem.coeffs), and the oracle's own corridor and feasibility costs are zero exactly
when no term is active.  The counts are steered by the durations of the rows under one velocity limit: a row with a third of its nominal duration
breaks the limit at every point, the nominal one at none, longer ones meet the acceleration and curvature limits at their ends.

Shapes: 16 pieces with 8 points per piece (n = 31) in batches of 1, 3, 4 and 5 trajectories (a wave with missing rows, a full
wave, a second wave with one row); 15 and 8 pieces (the generic sweep, Kd != K end pieces); five half-planes per point (the
instance that is not FAST); one solve in slices of five evaluations through the ring (suspended and resumed).
"""
import ctypes as C

import numpy as np
import pytest

from dftpav_amd import scenarios as sc
from dftpav_amd.pods import LayoutSpec
from quad_cases import active_terms

pytestmark = pytest.mark.gpu

KEYS = ("final_cost", "x", "status", "iters", "evals", "hist_sum", "success")
POOL = 64   # kQPool
DENSE = 24  # kDense (quad_common.h)
WINDOW = 7  # what a piece kept in LDS before the pool
VMAX = 4.0  # the velocity limit of every case: just above the nominal cruise speed
# duration scales of a row and what they give at 16 pieces (classes(), asserted per test): nothing active; two terms in one piece;
# a piece beyond the old window among some twenty terms; 174 terms (every point breaks the velocity limit)
NONE, FEW, BUSY, OVER = 1.0, 2.2, 3.0, 1.0 / 3.0


def classes(counts, costs):
    """What a row is, from the restatement's counts [B][N][J] and costs: "none" (and both penalty costs exactly zero), "few" (at
    most what one piece's window held, in all), "busy" (a piece beyond the old window, the total within the pool), "some", "over"
    (beyond the pool)."""
    out = []
    for cnt, cost in zip(counts, costs):
        per = cnt.sum(axis=1)
        tot = int(per.sum())
        if tot == 0:
            assert cost == (0.0, 0.0), cost
        out.append("none" if tot == 0 else "over" if tot > POOL else "busy" if per.max() > WINDOW else "few" if tot <= WINDOW else "some")
    return out


def _scene(pieces, K, Kd, scales, seed, H=4):
    """One trajectory per entry of scales: the same path, its duration the nominal one times the entry."""
    B = len(scales)
    s = sc.make_scenario([pieces], [1], K, Kd, B, seed=seed, n_obs=30, n_hyp=1, restart_sigma=0.0, dur_scale=(1.0, 1.0))
    s.init_Ts *= np.asarray(scales, dtype=np.float64)[:, None]
    if H != 4:  # further half-planes: copies of the first ones, moved inwards and rescaled (tests/terms_cases.py: "generic")
        cor = np.zeros((B, s.n_points, H, 4))
        cor[:, :, :4] = s.corridor
        cor[:, :, 4:] = s.corridor[:, :, :H - 4]
        cor[:, :, 4:, 2:] -= 0.2 * s.corridor[:, :, :H - 4, :2]
        cor[:, :, 4:, :2] *= 3.0
        s = sc.Scenario(s.name, LayoutSpec(s.layout.piece_nums, s.layout.singuls, H=H), s.K, s.Kd, B, s.ini_states, s.fin_states,
                        s.inner_pts, s.init_Ts, np.ascontiguousarray(cor))
    return s


def _params(hiplib, s):
    p = hiplib.default_params()
    s.apply_resolution(p)
    p.max_forward_vel = VMAX
    p.lbfgs_mem_size = 8
    p.lbfgs_max_iterations = 6
    return p


def _run(hiplib, oracle, monkeypatch, p, s, want, in_place=None, env=(), longest=2):
    """Evaluations at x0 and solves, QUAD shape against the restatement.  want: the rows' classes at x0, asserted from the
    restatement's counts; in_place: whether some round of a wave has more terms than the dense list holds."""
    x0 = np.stack([oracle.OracleProblem(p, s, b, order=0).x0() for b in range(s.B)])
    got = [active_terms(oracle, p, s, b, x0[b]) for b in range(s.B)]
    counts = np.stack([g[0] for g in got])
    rounds = [int(counts[w:w + 4].sum(axis=(0, 1)).max()) for w in range(0, s.B, 4)]
    print("terms per row", counts.sum(axis=(1, 2)), "largest piece", counts.sum(axis=2).max(axis=1), "largest round of a wave", rounds)
    assert classes(counts, [g[1] for g in got]) == list(want)
    if in_place is not None:
        assert (max(rounds) > DENSE) == in_place, rounds
    want = oracle.solve_batch(p, s, nthreads=8, order=0)
    monkeypatch.setenv("DFTPAV_REF_SHAPE", "quad")
    monkeypatch.setenv("DFTPAV_REF_QUAD_WAVES", "1")
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
    monkeypatch.delenv("DFTPAV_REF_SHAPE")
    monkeypatch.delenv("DFTPAV_REF_QUAD_WAVES")
    for k, _ in env:
        monkeypatch.delenv(k)
    assert np.array_equal(bt.x0(), x0)
    rng = np.random.default_rng(s.B)
    for x in (x0, x0 + rng.normal(0, 0.2, x0.shape)):
        f, g = bt.eval(x)
        for b in range(s.B):
            fo, go = oracle.OracleProblem(p, s, b, order=0).eval(x[b])
            assert f[b] == fo and np.array_equal(g[b], go), (s.B, b)
    bt.set_hand_over(0)  # the QUAD launch finishes every trajectory itself
    r = bt.solve()
    print("B", s.B, "iters", r["iters"], "evals", r["evals"])
    for k in KEYS:
        assert np.array_equal(r[k], want[k]), (s.B, k)
    assert (want["evals"] >= 2).all() and want["evals"].max() >= longest, want["evals"]
    bt.close()
    h.close()


def test_no_active_term(hiplib, oracle, monkeypatch):
    """Nothing is parked: the chain pass has no trip."""
    s = _scene(16, 8, 8, [NONE] * 3, seed=41)
    _run(hiplib, oracle, monkeypatch, _params(hiplib, s), s, ["none"] * 3, in_place=False)


def test_a_few_terms_in_one_piece(hiplib, oracle, monkeypatch):
    s = _scene(16, 8, 8, [FEW], seed=41)
    _run(hiplib, oracle, monkeypatch, _params(hiplib, s), s, ["few"], in_place=False)


@pytest.mark.parametrize("B", [1, 4, 5])
def test_a_piece_beyond_the_old_window(hiplib, oracle, monkeypatch, B):
    """Every row has a piece with more than seven terms (what went to global memory before) and fewer than kQPool in all: the dense
    path with one row, a full wave, and a second wave of one row."""
    s = _scene(16, 8, 8, [BUSY] * B, seed=41)
    _run(hiplib, oracle, monkeypatch, _params(hiplib, s), s, ["busy"] * B)


def test_overflowing_row_among_rows_with_few_and_none(hiplib, oracle, monkeypatch):
    """One wave: a row with more terms than the pool holds (the piece-by-piece path, its surplus in global scratch) beside a busy
    row, one with two terms and one with none."""
    s = _scene(16, 8, 8, [FEW, OVER, NONE, BUSY], seed=41)
    _run(hiplib, oracle, monkeypatch, _params(hiplib, s), s, ["few", "over", "none", "busy"], in_place=False)


@pytest.mark.parametrize("B", [3, 4])
def test_rounds_taken_in_place(hiplib, oracle, monkeypatch, B):
    """Every row breaks the limit at every point: a round of the wave has more terms than the dense list holds, so the in-place path
    numbers the pool's slots, and every row overflows its pool."""
    s = _scene(16, 8, 8, [OVER] * B, seed=41)
    _run(hiplib, oracle, monkeypatch, _params(hiplib, s), s, ["over"] * B, in_place=True)


@pytest.mark.parametrize("pieces,want", [(15, ["none", "over", "busy", "over", "over"]), (8, ["none", "over", "some", "some", "over"])])
def test_other_piece_counts(hiplib, oracle, monkeypatch, pieces, want):
    """N != 16 with Kd != K: the generic sweep, end pieces with more points than the others; a second wave of one row."""
    s = _scene(pieces, 6, 9, [NONE, OVER, 10.0, 0.6, OVER], seed=41 + pieces)
    _run(hiplib, oracle, monkeypatch, _params(hiplib, s), s, want)


def test_five_half_planes(hiplib, oracle, monkeypatch):
    """H = 5: the instance that is not FAST (29 terms per point)."""
    s = _scene(16, 8, 8, [BUSY, OVER, NONE], seed=41, H=5)
    _run(hiplib, oracle, monkeypatch, _params(hiplib, s), s, ["busy", "over", "none"])


def test_suspended_and_resumed(hiplib, oracle, monkeypatch):
    """One persistent wave, slices of five evaluations, solves of more than 64 evaluations: the pool and the permutation are
    scratch of one evaluation, nothing of them has to survive a trip through the ring."""
    s = _scene(16, 8, 8, [BUSY, OVER, NONE, FEW, BUSY], seed=41)
    p = _params(hiplib, s)
    p.lbfgs_max_iterations = 80
    _run(hiplib, oracle, monkeypatch, p, s, ["busy", "over", "none", "few", "busy"], env=(("DFTPAV_REF_SLOTS", "1"), ("DFTPAV_REF_SLICE", "5")),
         longest=65)
