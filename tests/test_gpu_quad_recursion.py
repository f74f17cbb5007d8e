"""The two-loop recursion of the QUAD shape (dftpav_amd/csrc/solver_ref4.hip: q4_two_loop) after its diet: blocks of eight history
rows read as consecutive rows from one address (a block that crosses the end of the ring comes from the mirror of the ring's ends,
DevBatch::histM), (ys, 1 / ys) of a pair carried as element 31 of its row, no select in front of the chains.

Bar: every output of every solve (x, cost, status, iterations, evaluations, hist_sum, success) BIT-EQUAL to the WAVE shape
(DFTPAV_REF_SHAPE=wave, solver_ref.hip: code this change does not touch) and to the restatement in order 2 (oracle/pyoracle.py).

Shapes: the smallest at which this code can go wrong -- 8-16 trajectories of BASELINE configs[3]'s layout (16 pieces, n = 31), L-BFGS
memories of 8 (= the block), 12 (no multiple of it) and 20 (more than two blocks) with several times as many iterations, so that pairs
land in both mirrored ranges and blocks cross the ring's end in both loops; layouts of 4 and 10 pieces (n = 7, 19: the second register
of a vector is all padding / part padding).

Hand-over: test_hand_over_resumes_from_the_ring runs an isolated batch of 192 trajectories of a 4-piece layout whose last 64 go to
the WAVE shape, which resumes them from the ring in histS and from histR (it never sees the mirror); it must equal the all-WAVE run.
"""
import numpy as np
import pytest

from dftpav_amd import scenarios as sc

pytestmark = pytest.mark.gpu

KEYS = ("final_cost", "x", "status", "iters", "evals", "hist_sum", "success")


def _solve(hiplib, monkeypatch, p, s, shape, env=(), hand_over=0):
    """One reference-order solve of the batch in the given shape (the plan is chosen by set_order, from the environment)."""
    monkeypatch.setenv("DFTPAV_REF_SHAPE", shape)
    for k, v in env:
        monkeypatch.setenv(k, v)
    h = hiplib.Handle(p)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    bt.set_order(hiplib.ORDER_REFERENCE)
    monkeypatch.delenv("DFTPAV_REF_SHAPE")
    for k, _ in env:
        monkeypatch.delenv(k)
    bt.set_hand_over(hand_over)
    r = bt.solve()
    r2 = bt.solve()  # the history and its mirror are left as the first solve wrote them: a second solve starts on them
    for k in KEYS:
        assert np.array_equal(r[k], r2[k]), ("second solve", shape, k)
    bt.close()
    h.close()
    return r


def _check(hiplib, oracle, monkeypatch, p, s, mem, env=()):
    p.lbfgs_mem_size = mem
    want = oracle.solve_batch(p, s, nthreads=8, order=2)
    rw = _solve(hiplib, monkeypatch, p, s, "wave")
    rq = _solve(hiplib, monkeypatch, p, s, "quad", env=(("DFTPAV_REF_QUAD_WAVES", "1"),) + tuple(env))
    print("mem", mem, "iters", rq["iters"], "evals", rq["evals"], "hist_sum", rq["hist_sum"])
    for k in KEYS:
        assert np.array_equal(rq[k], rw[k]), ("QUAD against WAVE", mem, k)
        assert np.array_equal(rq[k], want[k]), ("QUAD against the restatement", mem, k)
    return rq


def _rows_differ(r, mem):
    """The trajectories that share a wave (four consecutive ones: every row in a row of its own from the start) have different
    history depths and are in different phases: their iteration and evaluation counts differ, and every one of them runs several
    times round the ring."""
    it, ev = r["iters"], r["evals"]
    assert (it > 3 * mem).sum() >= len(it) // 2, (mem, it)
    for w in range(0, len(it) - 3, 4):
        assert len(set(it[w:w + 4].tolist())) > 1 and len(set(ev[w:w + 4].tolist())) > 1, (w, it[w:w + 4], ev[w:w + 4])
    # (evaluations per iteration differ too: some row is in its line search while another runs the recursion)
    assert len(set((ev - it).tolist())) > 1


@pytest.mark.parametrize("mem", [8, 12, 20])
def test_ring_wraps_through_both_mirrors(hiplib, oracle, monkeypatch, mem):
    """configs[3]'s layout (n = 31) with a memory equal to the block, no multiple of it, and more than two blocks."""
    p = hiplib.default_params()
    s = sc.baseline_config(3, B=12)
    s.apply_resolution(p)
    r = _check(hiplib, oracle, monkeypatch, p, s, mem)
    _rows_differ(r, mem)


def test_ring_wraps_through_the_ring_of_suspended_rows(hiplib, oracle, monkeypatch):
    """The same through the batch's ring: one persistent wave, slices of 5 evaluations -- a trajectory's history and mirror are
    written by one slice and read by the next, from whichever row pops it."""
    p = hiplib.default_params()
    s = sc.baseline_config(3, B=9)
    s.apply_resolution(p)
    _check(hiplib, oracle, monkeypatch, p, s, 12, env=(("DFTPAV_REF_SLOTS", "1"), ("DFTPAV_REF_SLICE", "5")))


@pytest.mark.parametrize("pieces,mem", [(4, 8), (10, 12)])
def test_padding_in_the_second_register(hiplib, oracle, monkeypatch, pieces, mem):
    """n = 7: the second register of a vector is all padding (its chain is left out); n = 19: part padding -- its products enter the
    chain unselected and must be zeros."""
    p = hiplib.default_params()
    s = sc.make_scenario([pieces], [1], 9, 14, 8, seed=600 + pieces, n_obs=30)
    s.apply_resolution(p)
    r = _check(hiplib, oracle, monkeypatch, p, s, mem)
    assert r["x"].shape[1] == 2 * pieces - 1
    assert (r["iters"] > mem).any(), r["iters"]


def test_true_divisions_read_the_pair_from_the_row(hiplib, oracle, monkeypatch):
    """The EXACT instantiation (true divisions from the first iteration on) takes (ys, 1 / ys) from element 31 too."""
    p = hiplib.default_params()
    s = sc.baseline_config(3, B=8)
    s.apply_resolution(p)
    _check(hiplib, oracle, monkeypatch, p, s, 12, env=(("DFTPAV_REF_EXACT_DIV", "1"),))


def test_hand_over_resumes_from_the_ring(hiplib, monkeypatch):
    """An isolated batch whose last 64 trajectories finish in the WAVE shape: bit-equal to the all-WAVE run."""
    p = hiplib.default_params()
    s = sc.make_scenario([4], [1], 9, 14, 192, seed=77, n_obs=30)
    s.apply_resolution(p)
    p.lbfgs_mem_size = 12
    rw = _solve(hiplib, monkeypatch, p, s, "wave")
    rq = _solve(hiplib, monkeypatch, p, s, "quad", hand_over=-1,
                env=(("DFTPAV_REF_QUAD_HANDOVER", "64"), ("DFTPAV_REF_SLOTS", "8"), ("DFTPAV_REF_SLICE", "6")))
    for k in KEYS:
        assert np.array_equal(rq[k], rw[k]), k
