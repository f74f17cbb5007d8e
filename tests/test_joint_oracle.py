"""The CPU yardstick of joint selection (oracle_conflict/joint_oracle.cpp) against a brute-force restatement of the rule in plain Python
(tests/joint_cases.py): random poses, the dependency chain, the two orders, blocked == (conflict_sample >= 0); and its second entry,
which evaluates the poses from plans as the candidate oracle does."""
import numpy as np
import pytest

import joint_cases as jc
from oracle_conflict import pycandidate as pcand
from oracle_conflict import pyjoint as pj


@pytest.mark.parametrize("seed", range(12))
def test_random_poses_equal_the_brute_force_rule(seed):
    rng = np.random.default_rng(1000 + seed)
    Q, R, K = int(rng.integers(1, 7)), int(rng.integers(1, 5)), int(rng.integers(1, 6))
    poses, cost, elig = jc.random_scene(seed, K, Q, R, spread=3.0)
    hits = 0
    for margin, rng_m in ((0.5, 2.0), (0.0, 0.0), (3.0, 3.0), (-1.0, 2.0)):
        ref = jc.brute(poses, cost, elig, margin, rng_m)
        for order in (0, 2):                                    # no call of libm but sqrt: the orders agree on every index and bit
            got = pj.select(poses, cost, elig, margin, rng_m, order=order)
            jc.same(got, ref)
            assert np.array_equal(got["blocked"] != 0, got["conflict_sample"] >= 0)
        hits += int(ref["blocked"].sum())
        if margin < 0.0:
            assert not ref["blocked"].any()                     # a negative margin: never
    print("seed", seed, "Q R K", Q, R, K, "blocked", hits)


def test_random_scenes_block_someone():
    """the scenes above are not empty of conflicts"""
    n = 0
    for seed in range(12):
        poses, cost, elig = jc.random_scene(seed, 3, 6, 4, spread=3.0)
        n += int(pj.select(poses, cost, elig, 0.5, 2.0)["blocked"].sum())
    assert n > 20, n


@pytest.mark.parametrize("K", [1, 3])
def test_only_winners_block(K):
    poses, cost, elig, margin, rng_m = jc.chain(K)
    got = pj.select(poses, cost, elig, margin, rng_m)
    jc.same(got, jc.brute(poses, cost, elig, margin, rng_m))
    assert got["winner"].tolist() == [0, 1, 1]
    assert got["blocked"].tolist() == [[0, 0], [1, 0], [1, 0]]
    assert got["conflict_partner"].tolist() == [[-1, -1], [0, -1], [1, -1]] and got["conflict_sample"][1, 0] == 0
    assert abs(got["min_sep"][1, 0] - 0.12) < 1e-12 and got["min_sep"][2, 0] == got["min_sep"][1, 0]
    elig[0] = 0                                                 # q0 without an eligible restart: all three change
    flipped = pj.select(poses, cost, elig, margin, rng_m)
    jc.same(flipped, jc.brute(poses, cost, elig, margin, rng_m))
    assert flipped["winner"].tolist() == [-1, 0, 0] and not flipped["blocked"].any()
    assert np.isposinf(flipped["min_sep"][:2]).all()            # nobody won below q0 and q1
    assert flipped["sep_partner"][2].tolist() == [-1, -1]       # q1's cheapest is 50 m away: outside the broad phase


def test_ties_nan_costs_and_the_broad_phase():
    poses, cost, elig = jc.apart(2, 3, 3)
    cost[0] = [2.0, 1.0, 1.0]                                   # a tie: the lowest r
    cost[1] = [np.nan, 3.0, 3.0]                                # a NaN cost never wins
    jc.put(poses, 0, 1, 0.0, 0.0)
    jc.put(poses, 2, 0, 3.0, 0.0)                               # overlaps q0's winner, the centres 3 m apart
    got = pj.select(poses, cost, elig, 0.5, 2.0)
    assert got["winner"].tolist() == [1, 1, 1] and got["blocked"][2].tolist() == [1, 0, 0] and got["min_sep"][2, 0] == 0.0
    # range + 2 rad below the centre distance: the pair contributes nothing although the boxes overlap
    rad = np.sqrt(0.25 * jc.L ** 2 + 0.25 * jc.W ** 2)
    near = pj.select(poses, cost, elig, -2.4, 3.0 - 2.0 * rad - 1e-9)
    assert near["winner"].tolist() == [1, 1, 0] and not near["blocked"].any() and np.isposinf(near["min_sep"]).all()
    jc.same(near, jc.brute(poses, cost, elig, -2.4, 3.0 - 2.0 * rad - 1e-9))


def test_plans_entry_uses_the_candidate_pose(oracle):
    """straight runs as candidates: the poses are the candidate oracle's, and the selection is that of the poses-in entry on them"""
    from dftpav_amd import conflict_scenes as cs
    gen = oracle.minco_generate
    Q, R, K, dt, t_call = 4, 2, 9, 0.5, 3.0
    runs = [[cs._run(gen, (-10.0 + 2.0 * q, 3.0 * r + 1.3 * q), (10.0 + 2.0 * q, 3.0 * r + 1.3 * q), 0.0, n_pieces=4) for r in range(R)] for q in range(Q)]
    runs[2] = None                                              # a query outside every layout group
    MS, NP = 2, 6
    n_seg, sg, pn = np.zeros(Q, np.int32), np.zeros((Q, MS), np.int32), np.zeros((Q, MS), np.int32)
    pdt, co = np.zeros((Q, R, MS)), np.zeros((Q, R, NP, 6, 2))
    for q, rr in enumerate(runs):
        if rr is None:
            continue
        n_seg[q], sg[q, :1], pn[q, :1] = 1, rr[0]["singul"], rr[0]["piece_nums"]
        for r, p in enumerate(rr):
            pdt[q, r, :1], co[q, r, :4] = p["coeff_dt"], p["coeffs"]
    cost = np.tile([1.0, 2.0], (Q, 1))
    elig = np.ones((Q, R), np.int32)
    elig[2] = 0
    for order in (0, 2):
        got = pj.select_plans(n_seg, sg, pn, pdt, co, cost, elig, t_call, dt, K, 0.3, 2.0, order=order)
        for q, rr in enumerate(runs):
            if rr is None:
                assert np.isnan(got["poses"][:, q]).all()
                continue
            ref = pcand.poses(rr[0]["singul"], rr[0]["piece_nums"], pdt[q, :, :1], co[q, :, :4], t_call, t_call, dt, K, order=order)
            assert np.array_equal(got["poses"][:, q].view(np.int64), ref.view(np.int64)), (order, q)
        jc.same(got, pj.select(got["poses"], cost, elig, 0.3, 2.0, order=order))
        jc.same(got, jc.brute(got["poses"], cost, elig, 0.3, 2.0))
        assert got["winner"][2] == -1 and got["blocked"].any() and got["winner"].tolist() != [0, 0, -1, 0]
    assert np.array_equal(pj.select_plans(n_seg, sg, pn, pdt, co, cost, elig, t_call, dt, K, 0.3, 2.0, order=0)["winner"], got["winner"])
