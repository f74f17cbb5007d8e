"""The two block forms of the QUAD shape's two-loop recursion (dftpav_amd/csrc/solver_ref4.hip: q4_first_steps / q4_second_steps): a
block of eight history steps in which no row's bound falls runs as one body under one mask (q4_first_block / q4_second_block: the
block's alphas stored behind it in 16-byte writes and read at its head), a block with a bound inside it asks step by step.

Bar: every output of every solve (x, cost, status, iterations, evaluations, hist_sum, success) BIT-EQUAL to the restatement in
order 2 (oracle/pyoracle.py), on the kernel's three instances (INSTANCES below; the vector-length cases run on the default one).

Shapes: ONE wave of four trajectories (or fewer: absent rows) of BASELINE configs[3]'s layout (16 pieces, n = 31), so that the four
rows' bounds differ inside one pass and a block is full for one row, partial for another and out for a third.  A row's bound grows
by one with every accepted pair: a solve whose rows accept A pairs takes every bound 1 .. min(A, mem) -- 7, 8, 9, 15, 16, 17 and 24
among them -- and A follows from the solve's hist_sum (the sum of the bounds), which each case asserts, so that a case cannot stop
covering its block form unnoticed.  The counts are the restatement's (the CPU), against which the device is then compared.

Not reachable: n = 32 (the instances with (ys, 1 / ys) read from histR) -- a single-segment layout has n = 2 N - 1, odd; and a
row that switches to true division in the middle of a solve -- no input here produces a ys outside 2^-500 .. 2^500, so the division
route is the forced one (DFTPAV_REF_EXACT_DIV=1) for all rows.
"""
import numpy as np
import pytest

from dftpav_amd import scenarios as sc

pytestmark = pytest.mark.gpu

KEYS = ("final_cost", "x", "status", "iters", "evals", "hist_sum", "success")


def _accepted(hist_sum, mem):
    """Pairs a row accepted, from the sum of its bounds: hist_sum = sum over j = 1 .. A of min(j, mem)."""
    a, s = 0, 0
    while s < hist_sum:
        a += 1
        s += min(a, mem)
    assert s == hist_sum, (hist_sum, mem)
    return a


def _quad(hiplib, monkeypatch, p, s, env=()):
    env = (("DFTPAV_REF_SHAPE", "quad"), ("DFTPAV_REF_QUAD_WAVES", "1")) + tuple(env)
    for k, v in env:
        monkeypatch.setenv(k, v)
    h = hiplib.Handle(p)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    bt.set_order(hiplib.ORDER_REFERENCE)
    for k, _ in env:
        monkeypatch.delenv(k)
    r = bt.solve()
    bt.close()
    h.close()
    return r


def _check(hiplib, oracle, monkeypatch, p, s, mem, env=(), reach=0):
    """reach: the bound that at least two rows of the wave must reach, and at least one row must stay short of the others."""
    p.lbfgs_mem_size = mem
    want = oracle.solve_batch(p, s, nthreads=8, order=2)
    acc = [_accepted(int(hs), mem) for hs in want["hist_sum"]]
    print("mem", mem, "iters", want["iters"], "evals", want["evals"], "accepted pairs", acc)
    if reach:
        assert sum(a >= reach for a in acc) >= min(2, s.B), (reach, acc)
    if s.B > 1:  # the rows are in different places: bounds and phases differ inside a pass
        assert len(set(acc)) > 1 and len(set((want["evals"] - want["iters"]).tolist())) > 1, (acc, want["evals"], want["iters"])
    got = _quad(hiplib, monkeypatch, p, s, env)
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (mem, env, k)
    return want, acc


# The three instances of ref4_kernel, each with its own compiled copy of both block forms: <true, true> (H = 4, help_eps = 0, rectangle
# corridors: the default), <true, false> (the corridors taken as general half-planes), <false, false> (help_eps != 0: not FAST)
INSTANCES = ("fast_rect", "fast_general", "plain")


def _scene(B, instance):
    s = sc.baseline_config(3, B=B)
    env = ()
    if instance == "fast_general":
        env = (("DFTPAV_RECT_CORRIDOR", "0"),)
    elif instance == "plain":
        s.help_eps = 1e-3
    return s, env


@pytest.mark.parametrize("instance", INSTANCES)
@pytest.mark.parametrize("mem,reach", [(8, 8), (12, 12), (20, 20), (256, 24)])
def test_bounds_across_the_block_border(hiplib, oracle, monkeypatch, mem, reach, instance):
    """mem 8: the bound stops at the block's size (7: partial, 8: full); 12, 20: it stops inside the second / third block, and more
    iterations than mem read the blocks from the mirror; 256: the ring never wraps and the bounds run through 7, 8, 9, 15, 16, 17, 24.
    On each of the kernel's three instances."""
    p = hiplib.default_params()
    s, env = _scene(4, instance)
    s.apply_resolution(p)
    want, acc = _check(hiplib, oracle, monkeypatch, p, s, mem, env=env, reach=reach)
    if mem < 256:
        assert (want["iters"] > 2 * mem).sum() >= 2, want["iters"]


@pytest.mark.parametrize("instance", ["fast_rect", "plain"])
@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_absent_rows_and_rows_in_their_line_search(hiplib, oracle, monkeypatch, B, instance):
    """A wave with one, two and three rows present (B = 5: a full wave and one row): the decision between the block forms is taken
    over the rows that are in the recursion, and a row in its line search has no say in it."""
    p = hiplib.default_params()
    s, env = _scene(B, instance)
    s.apply_resolution(p)
    _check(hiplib, oracle, monkeypatch, p, s, 256, env=env, reach=24)


@pytest.mark.parametrize("pieces,n", [(4, 7), (10, 19), (16, 31)])
def test_vector_lengths(hiplib, oracle, monkeypatch, pieces, n):
    """n = 7: one chain per sum (the bodies built for n <= 16); n = 19, 31: two."""
    p = hiplib.default_params()
    s = sc.make_scenario([pieces], [1], 9, 14, 4, seed=600 + pieces, n_obs=30)
    s.apply_resolution(p)
    want, acc = _check(hiplib, oracle, monkeypatch, p, s, 12, reach=12)
    assert want["x"].shape[1] == n


@pytest.mark.parametrize("instance", INSTANCES)
def test_true_divisions_in_both_block_forms(hiplib, oracle, monkeypatch, instance):
    p = hiplib.default_params()
    s, env = _scene(4, instance)
    s.apply_resolution(p)
    _check(hiplib, oracle, monkeypatch, p, s, 20, env=env + (("DFTPAV_REF_EXACT_DIV", "1"),), reach=20)


@pytest.mark.parametrize("instance", INSTANCES)
def test_suspended_and_resumed_rows(hiplib, oracle, monkeypatch, instance):
    """Slices of 3 evaluations through the batch's ring, one persistent wave: a row's alphas are what its LDS holds, written and read
    inside one recursion; nothing of a block survives a suspension in registers."""
    p = hiplib.default_params()
    s, env = _scene(6, instance)
    s.apply_resolution(p)
    _check(hiplib, oracle, monkeypatch, p, s, 20, env=env + (("DFTPAV_REF_SLOTS", "1"), ("DFTPAV_REF_SLICE", "3")), reach=20)
