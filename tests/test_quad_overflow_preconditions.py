"""What the cases of tests/test_gpu_quad_parked_overflow.py need in order to mean anything, from the restatement alone (no GPU): base
scenes without an active term at x0, the forced terms counted by quad_cases.active_terms exactly where and as many as forced, the
totals around the pool's size and the block's, rows without a term beside overflowed ones, the split of a row's pieces between pool
and scratch in arrival order, the plan's kind and workgroup for the forced shape, and the five-half-plane scene beyond the pool."""
import numpy as np
import pytest

import quad_cases as qc
import test_gpu_quad_parked_overflow as tp


@pytest.mark.parametrize("name", sorted(tp.CASES))
def test_cases_are_not_vacuous(hiplib, oracle, monkeypatch, name):
    pieces, rows = tp.CASES[name]
    p, s, x0, counts = tp.build(hiplib, oracle, pieces, rows)
    assert counts.shape == (len(rows), pieces, max(tp.K, tp.KD) + 1) and s.layout.H == 4
    tp.precondition(name, counts)
    monkeypatch.setenv("DFTPAV_REF_SHAPE", "quad")
    monkeypatch.setenv("DFTPAV_REF_QUAD_WAVES", "1")
    assert qc.plan_readout(hiplib, s, p)[:3] == [1, 3, 64]
    # the solves the GPU cases compare: every one takes more than one evaluation
    assert (oracle.solve_batch(p, s, nthreads=8, order=2)["evals"] >= 2).all()


@pytest.mark.parametrize("name", ["piece_cases", "four_rows_70_97_141_203"])
def test_help_eps_cases_are_not_vacuous(hiplib, oracle, name):
    """help_eps = 1e-3 (the instance that is not FAST) forces the same terms, and moves the gradient"""
    pieces, rows = tp.CASES[name]
    p, s, x0, counts = tp.build(hiplib, oracle, pieces, rows, 1e-3)
    p0, s0, _, counts0 = tp.build(hiplib, oracle, pieces, rows)
    tp.precondition(name, counts)
    assert np.array_equal(counts, counts0) and s.help_eps == 1e-3 and s0.help_eps == 0.0
    x1 = x0 + np.random.default_rng(s.B).normal(0, 0.05, x0.shape)
    assert any(not np.array_equal(oracle.OracleProblem(p, s, b, order=2).eval(x1[b])[1], oracle.OracleProblem(p0, s0, b, order=2).eval(x1[b])[1])
               for b in range(s.B))


def test_the_piece_row_splits_as_described(hiplib, oracle):
    """the row of the piece cases: 60 pool entries from point 1, piece 7 across the pool's end, piece 2 wholly in scratch"""
    _, _, _, counts = tp.build(hiplib, oracle, 16, tp.CASES["piece_cases"][1])
    a, c = tp.pool_split(counts[0])
    assert list(c) == [21, 0, 7, 15, 0, 15, 0, 9, 0, 0, 0, 0, 0, 0, 0, 18]
    assert list(a) == [15, 0, 0, 15, 0, 15, 0, 4, 0, 0, 0, 0, 0, 0, 0, 15]


def test_five_half_planes_scene_overflows(hiplib, oracle):
    _, s4, x0, _ = tp.build(hiplib, oracle, 16, tp.CASES["piece_cases"][1])
    s = qc.extra_planes(s4, 5)
    p = tp.params_of(hiplib, s)
    tot = np.array([qc.active_terms(oracle, p, s, b, x0[b], order=2)[0].sum() for b in range(s.B)])
    assert tot.max() > tp.POOL and tot.max() % tp.BLOCK != 0 and (tot > tp.POOL).sum() >= 2, tot
