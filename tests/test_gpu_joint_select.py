"""The kernels of joint selection (joint_select.hip) through dftpav_debug_joint_select, on crafted poses of a few boxes: winners, blocked
and the five rows bit-equal to oracle_conflict/joint_oracle.cpp in order 2."""
import ctypes as C
import itertools

import numpy as np
import pytest

import joint_cases as jc
from oracle_conflict import pyjoint as pj

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def h(hiplib):
    handle = hiplib.Handle()
    yield handle
    handle.close()


def _both(hiplib, h, poses, cost, elig, margin, rng):
    got = hiplib.debug_joint_select(h, poses, cost, elig, margin, rng)
    ref = pj.select(poses, cost, elig, margin, rng, order=2)
    jc.same(got, ref)
    assert np.array_equal(got["blocked"] != 0, got["conflict_sample"] >= 0)
    return got


def test_only_winners_block(hiplib, h):
    poses, cost, elig, margin, rng = jc.chain(1)
    got = _both(hiplib, h, poses, cost, elig, margin, rng)
    assert got["winner"].tolist() == [0, 1, 1] and got["blocked"].tolist() == [[0, 0], [1, 0], [1, 0]]
    assert got["conflict_partner"].tolist() == [[-1, -1], [0, -1], [1, -1]]
    ms = h.joint_last_ms()
    assert ms[0] == 0.0 and ms[1] > 0.0 and ms[2] > 0.0          # no pose kernel ran
    elig[0] = 0                                                 # flipping q0's eligibility changes all three
    got = _both(hiplib, h, poses, cost, elig, margin, rng)
    assert got["winner"].tolist() == [-1, 0, 0] and not got["blocked"].any()


def test_nobody_eligible_and_nan_poses_block_nobody(hiplib, h):
    poses, cost, elig = jc.apart(2, 4, 2)
    for q in range(4):                                          # every query's cheapest restart on the same spot
        jc.put(poses, q, 0, 0.0, 0.0)
    got = _both(hiplib, h, poses, cost, elig, 0.5, 2.0)
    assert got["winner"].tolist() == [0, 1, 1, 1] and got["blocked"][:, 0].tolist() == [0, 1, 1, 1]
    elig[0] = 0                                                 # q0 wins nothing and blocks nobody: q1 takes the spot
    poses[:, 2] = NAN                                           # q2 of NaN poses is never blocked, wins, and blocks nobody
    got = _both(hiplib, h, poses, cost, elig, 0.5, 2.0)
    assert got["winner"].tolist() == [-1, 0, 0, 1] and got["blocked"][:, 0].tolist() == [0, 0, 0, 1]
    assert got["conflict_partner"][3, 0] == 1 and np.isposinf(got["min_sep"][2]).all()
    poses[0, 1, 0, 2] = NAN                                     # one component at one sample: that sample takes no part
    got = _both(hiplib, h, poses, cost, elig, 0.5, 2.0)
    assert got["conflict_sample"][3, 0] == 1


@pytest.mark.parametrize("K", [1, 2, 5, 257])
def test_conflict_at_the_last_sample_only(hiplib, h, K):
    poses, cost, elig = jc.apart(K, 2, 2)
    jc.put(poses, 0, 0, 0.0, 0.0)
    jc.put(poses, 1, 0, 5.0, 0.0, k=K - 1)                      # arrives in front of q0's winner at the last clock
    got = _both(hiplib, h, poses, cost, elig, 0.5, 2.0)
    assert got["winner"].tolist() == [0, 1] and got["conflict_sample"][1, 0] == K - 1 and got["sep_sample"][1, 0] == K - 1
    jc.put(poses, 1, 0, 5.0 + 0.5, 0.0, k=K - 1)                # 0.62 m: inside the broad phase, outside the margin
    got = _both(hiplib, h, poses, cost, elig, 0.5, 2.0)
    assert got["winner"].tolist() == [0, 0] and not got["blocked"].any() and got["sep_sample"][1, 0] == K - 1


# Q * R = 63, 64, 65, 130; R = 3 with a query astride 63 | 64 (candidates 63, 64, 65) and one astride 127 | 128 (126, 127, 128)
@pytest.mark.parametrize("Q,R", [(21, 3), (16, 4), (64, 1), (13, 5), (65, 2), (22, 3), (43, 3)])
def test_tile_edges(hiplib, h, Q, R):
    K = 3
    for seed in (0, 1):
        poses, cost, elig = jc.random_scene(100 * Q + seed, K, Q, R)
        got = _both(hiplib, h, poses, cost, elig, 0.5, 2.0)
        assert got["blocked"].any()
    # partners across the tile edges and between the first and the last query: candidate b, its query's cheapest, stands in front of
    # candidate a, the winner of a's query
    poses, cost, elig = jc.apart(K, Q, R)
    pairs = [(0, Q * R - 1)] + [(a, a + 1) for a in (63, 127) if a + 1 < Q * R and a // R != (a + 1) // R]
    if R == 3 and Q * R > 64:
        pairs += [(61, 64)] if Q == 22 else [(61, 64), (124, 127)]   # a restart of the query astride the edge against the query below
    for n, (a, b) in enumerate(pairs):
        cost[a // R, a % R] = cost[b // R, b % R] = 0.5
        jc.put(poses, a // R, a % R, 0.0, 50.0 * n)
        jc.put(poses, b // R, b % R, 5.0, 50.0 * n, k=K - 1)
    got = _both(hiplib, h, poses, cost, elig, 0.5, 2.0)
    for a, b in pairs:
        assert got["winner"][a // R] == a % R and got["blocked"][b // R, b % R] == 1 and got["winner"][b // R] != b % R, (a, b)
        assert got["conflict_partner"][b // R, b % R] == a // R and got["conflict_sample"][b // R, b % R] == K - 1, (a, b)
    assert got["blocked"].sum() == len(pairs)


def test_ties_nan_costs_and_the_broad_phase(hiplib, h):
    poses, cost, elig = jc.apart(2, 3, 3)
    cost[0] = [2.0, 1.0, 1.0]
    cost[1] = [NAN, 3.0, 3.0]
    jc.put(poses, 0, 1, 0.0, 0.0)
    jc.put(poses, 2, 0, 3.0, 0.0)                               # overlaps q0's winner, the centres 3 m apart
    got = _both(hiplib, h, poses, cost, elig, 0.5, 2.0)
    assert got["winner"].tolist() == [1, 1, 1] and got["blocked"][2].tolist() == [1, 0, 0] and got["min_sep"][2, 0] == 0.0
    rad = np.sqrt(0.25 * jc.L ** 2 + 0.25 * jc.W ** 2)
    cut = 3.0 - 2.0 * rad - 1e-9                                # range + 2 rad just below the centre distance, the margin below that
    got = _both(hiplib, h, poses, cost, elig, -2.4, cut)
    assert got["winner"].tolist() == [1, 1, 0] and not got["blocked"].any() and np.isposinf(got["min_sep"]).all()


def test_symmetry(hiplib, h):
    """exchanging the order of two queries exchanges who is blocked, with the same min_sep bits"""
    poses, cost, elig = jc.apart(3, 2, 1)
    jc.put(poses, 0, 0, 0.3, 0.1, heading=0.4)
    jc.put(poses, 1, 0, 4.1, 3.2, heading=-1.1)
    jc.put(poses, 1, 0, 3.9, 2.6, k=2, heading=-0.9)
    a = _both(hiplib, h, poses, cost, elig, 1.0, 3.0)
    b = _both(hiplib, h, poses[:, ::-1].copy(), cost, elig, 1.0, 3.0)
    for got in (a, b):
        assert got["winner"].tolist() == [0, -1] and got["blocked"].tolist() == [[0], [1]] and got["conflict_partner"][1, 0] == 0
    assert 0.0 < a["min_sep"][1, 0] <= 1.0 and a["min_sep"][1, 0].tobytes() == b["min_sep"][1, 0].tobytes()
    assert a["sep_sample"][1, 0] == b["sep_sample"][1, 0]


ARGS = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]


def _raw(hiplib):
    fn = hiplib.lib().dftpav_debug_joint_select
    fn.argtypes = ARGS
    return fn


def test_null_output_pointers(hiplib, h):
    poses, cost, elig = jc.random_scene(5, 3, 6, 4, spread=3.0)
    full = hiplib.debug_joint_select(h, poses, cost, elig, 0.5, 2.0)
    assert full["blocked"].any()
    fn = _raw(hiplib)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    n = 0
    for keep in itertools.product((False, True), repeat=8):     # winner, blocked, out, and the five pointers of out
        if keep[2] and not any(keep[3:]) or not keep[2] and any(keep[3:]):
            continue
        out = hiplib.ConflictOut(6, 4)
        w, b = np.full(6, 77, np.int32), np.full((6, 4), 77, np.int32)
        for a in out.a.values():
            a[...] = 77
        for k, on in zip(jc.FIELDS, keep[3:]):
            if not on:
                setattr(out.c, k, None)
        rc = fn(h._h, 6, 4, 3, ptr(poses), ptr(cost), ptr(elig), 0.5, 2.0, ptr(w) if keep[0] else None, ptr(b) if keep[1] else None,
                C.byref(out.c) if keep[2] else None)
        assert rc == hiplib.OK, keep
        assert np.array_equal(w, full["winner"]) if keep[0] else (w == 77).all()
        assert np.array_equal(b, full["blocked"]) if keep[1] else (b == 77).all()
        for k, on in zip(jc.FIELDS, keep[3:]):
            assert np.array_equal(out.a[k], full[k]) if on else (out.a[k] == 77).all(), (keep, k)
        n += 1
    assert n == 4 * 32


def test_refusals_write_nothing(hiplib, h):
    poses, cost, elig = jc.random_scene(6, 2, 3, 2, spread=3.0)
    good = hiplib.debug_joint_select(h, poses, cost, elig, 0.5, 2.0)
    ms = h.joint_last_ms()
    fn = _raw(hiplib)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = hiplib.ConflictOut(3, 2)
    w, b = np.full(3, 77, np.int32), np.full((3, 2), 77, np.int32)
    for a in out.a.values():
        a[...] = 77
    ok = dict(h=h._h, Q=3, R=2, K=2, poses=ptr(poses), cost=ptr(cost), elig=ptr(elig), margin=0.5, range=2.0)
    bad = [dict(h=None), dict(poses=None), dict(cost=None), dict(elig=None), dict(Q=0), dict(Q=-1), dict(R=0), dict(K=0), dict(K=-1), dict(K=4097),
           dict(margin=NAN), dict(margin=2.5), dict(range=INF), dict(range=NAN), dict(margin=INF), dict(margin=INF, range=INF)]
    big = [dict(Q=8193, R=1), dict(Q=4097, R=2), dict(Q=2049, R=1, K=2048), dict(Q=1025, R=1, K=4096)]   # beyond the two design bounds
    for case, code in [(c, hiplib.E_INVALID) for c in bad] + [(c, hiplib.E_UNSUPPORTED) for c in big]:
        a = dict(ok, **case)
        assert fn(a["h"], a["Q"], a["R"], a["K"], a["poses"], a["cost"], a["elig"], a["margin"], a["range"], ptr(w), ptr(b), C.byref(out.c)) == code, case
    assert (w == 77).all() and (b == 77).all() and all((a == 77).all() for a in out.a.values())
    assert h.joint_last_ms() == ms                              # nothing ran
    jc.same(hiplib.debug_joint_select(h, poses, cost, elig, 0.5, 2.0), good)
    pl = hiplib.Planner(h, 3, 2)
    fs = hiplib.lib().dftpav_planner_set_joint_selection
    fs.argtypes = [C.c_void_p, C.c_int]
    assert fs(None, 1) == hiplib.E_INVALID and fs(pl._p, 2) == hiplib.E_INVALID and fs(pl._p, -1) == hiplib.E_INVALID
    with pytest.raises(hiplib.DftpavError) as e:
        pl.last_joint(3)                                        # no call ran with joint selection
    assert e.value.code == hiplib.E_INVALID
    pl.close()
    wide = hiplib.Planner(h, 4097, 2)                           # 8194 candidates
    with pytest.raises(hiplib.DftpavError) as e:
        wide.set_joint_selection(True)
    assert e.value.code == hiplib.E_UNSUPPORTED
    wide.set_joint_selection(False)
    wide.close()
    deep = hiplib.Planner(h, 2049, 1)                           # 2049 candidates: K = 2048 passes 2^22
    deep.set_joint_selection(True)
    with pytest.raises(hiplib.DftpavError) as e:
        deep.set_conflict_filter(0.5, 2.0, 0.1, 2048)
    assert e.value.code == hiplib.E_UNSUPPORTED
    deep.set_conflict_filter(0.5, 2.0, 0.1, 2047)
    deep.set_joint_selection(False)
    deep.set_conflict_filter(0.5, 2.0, 0.1, 2048)
    with pytest.raises(hiplib.DftpavError) as e:
        deep.set_joint_selection(True)                          # the filter's K passes the bound now
    assert e.value.code == hiplib.E_UNSUPPORTED
    deep.close()
