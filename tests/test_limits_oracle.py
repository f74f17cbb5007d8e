"""CPU checks of the kinematic-limits oracle (oracle_limits/limits_oracle.cpp): the quantities of Piece::getVel / getAcc / getLatAcc /
getCurv / getSteer (poly_traj_utils.hpp:247-300) over CheckReplan's samples (traj_server_ros.cpp:385-386), their maxima, where they
are first reached, and the limit tests.  The reference holds no expected values for this step; these are property checks against
the read-out oracle (oracle/states_oracle.cpp) and a plain loop, and each special case of the device kernel is shown to occur."""
import math

import numpy as np
import pytest

from dftpav_amd import replan_scenes as rs
from dftpav_amd import scenarios as sc
from oracle_limits import pylimits as pl

INF = float("inf")
DEFAULT = dict(max_forward_vel=5.0, max_backward_vel=2.0, max_forward_acc=8.0, max_backward_acc=4.0, max_forward_cur=1.0,
               max_backward_cur=1.0, max_latacc=5.0, max_steer=INF)


def straight(speed, n_pieces, dT, direction=1.0):
    """[n_pieces][6][2]: motion along x at exactly `speed`: every sample has the same |velocity|, every other quantity is 0"""
    co = np.zeros((n_pieces, 6, 2))
    for p in range(n_pieces):
        co[p, 0, 0] = direction * speed * dT * p
        co[p, 1, 0] = direction * speed
    return co


@pytest.fixture(scope="module")
def gear_shift(oracle, hiplib):
    """a 3 + 2 plan, forward then reverse, solved by the oracle in order 2: coeffs [B][5][6][2], piece_dt [B][2]"""
    p = hiplib.default_params()
    s = sc.make_scenario([3, 2], [1, -1], 8, 8, 2, seed=41, n_obs=10)
    s.apply_resolution(p)
    r = oracle.solve_batch(p, s, nthreads=2, order=2)
    co, dts = [], []
    for b in range(s.B):
        pr = oracle.OracleProblem(p, s, b, order=2)
        pr.eval(r["x"][b])
        c, t = pr.coeffs()
        co.append(c)
        dts.append(t)
    return np.array(co), np.array(dts)


def _plain_loop(samples, n):
    """max |q| and its first index by a plain loop over the oracle's per-sample values"""
    m, a = [0.0] * 5, [-1] * 5
    for k in range(n):
        for j in range(5):
            v = abs(float(samples[k, 3 + j]))
            if a[j] < 0 or v > m[j]:
                m[j], a[j] = v, k
    return m, a


def test_samples_equal_the_read_out_oracle(oracle, gear_shift):
    """The per-sample curvature, velocity, acceleration and steer behind the maxima are BIT-EQUAL to the columns of
    oracle.sample_states (Trajectory::GetState, poly_traj_utils.hpp:378-406) at the same local times: getStateExpPos divides by
    singul * norm where the getters multiply by singul, which changes no bit (largest difference observed: 0.0).  Each segment is
    read on its own with a dyadic step, so that GetState's t0 + k * dt is the running sum t += dt exactly."""
    co, dts = gear_shift
    dt = 0.0625
    r = pl.check_batch([1, -1], [3, 2], co, dts, dt, DEFAULT, order=2, max_samples=1024)
    largest = 0.0
    for b in range(co.shape[0]):
        n = int(r["n_samples"][b])
        sm = r["samples"][b, :n]
        assert n > 20 and set(sm[:, 1].tolist()) == {0.0, 1.0}
        p0 = 0
        for i, (N, sg) in enumerate(((3, 1), (2, -1))):
            rows = sm[sm[:, 1] == i]
            st, nv = oracle.sample_states(co[b:b + 1, p0:p0 + N], [[dts[b, i]]], [N], [sg], sample_dt=dt, n_samples=len(rows),
                                          filter_singularity=False, order=2)
            assert nv[0] == len(rows) and np.array_equal(st[0, :, 0], rows[:, 0])
            for col, j in ((4, 3 + 3), (5, 3 + 0), (6, 3 + 1), (7, 3 + 4)):   # curvature, velocity, acceleration, steer
                largest = max(largest, float(np.max(np.abs(st[0, :, col] - rows[:, j]))))
                assert np.array_equal(st[0, :, col], rows[:, j]), (b, i, col)
            p0 += N
        assert (sm[sm[:, 1] == 1][:, 3] < 0).all() and (sm[sm[:, 1] == 0][1:, 3] > 0).all()   # the reverse segment drives backwards
    print("largest difference to sample_states:", largest)


@pytest.mark.parametrize("dt", [0.05, 0.0625, 0.0371])
def test_maxima_and_first_indices_equal_a_plain_loop(gear_shift, dt):
    co, dts = gear_shift
    r = pl.check_batch([1, -1], [3, 2], co, dts, dt, DEFAULT, order=2, max_samples=2048)
    for b in range(co.shape[0]):
        n = int(r["n_samples"][b])
        m, a = _plain_loop(r["samples"][b], n)
        assert r["max_abs"][b].tolist() == m and r["arg"][b].tolist() == a
        # the local time of a sample: the running sum, walked down by locatePieceIdx's subtractions
        k0 = int(np.sum(r["samples"][b, :n, 1] == 0))
        t, k = 0.0, 0
        while t < dts[b, 0] + dts[b, 0] + dts[b, 0]:
            assert r["samples"][b, k, 0] == t
            t += dt
            k += 1
        assert k == k0


def test_orders_agree_on_the_discrete_outputs(gear_shift):
    co, dts = gear_shift
    for dt in (0.05, 0.0371):
        a = pl.check_batch([1, -1], [3, 2], co, dts, dt, DEFAULT, order=0)
        b = pl.check_batch([1, -1], [3, 2], co, dts, dt, DEFAULT, order=2)
        for k in ("arg", "violated", "feasible"):
            assert np.array_equal(a[k], b[k]), k
        assert np.allclose(a["max_abs"], b["max_abs"], rtol=1e-14, atol=0)


def test_a_plan_that_starts_at_rest_takes_the_branch(oracle):
    seg = rs._segment(oracle.minco_generate, (0.0, 0.0), (6.0, 2.0), 3, 1.0, 1, 0.0, 0.5)
    c = seg["coeffs"].copy()
    c[0, 2] = (0.3, 0.1)                  # an acceleration at rest: without the branch the curvature would divide by zero
    r = pl.check_batch([1], [3], c[None], [[1.0]], 0.05, DEFAULT, order=2, max_samples=64)
    s0 = r["samples"][0, 0]
    assert s0[0] == 0.0 and (s0[3:8] == 0.0).all()          # |dsigma| < 1e-6: velocity 0, and the other four by their branch
    assert (r["samples"][0, 1:60, 3] > 0).all() and np.isfinite(r["max_abs"]).all()
    # a piece at rest altogether: every quantity 0 at every sample, arg 0
    z = np.zeros((1, 2, 6, 2))
    z[0, :, 0] = (3.0, 4.0)
    r = pl.check_batch([1], [2], z, [[1.0]], 0.05, DEFAULT, order=2)
    assert not r["max_abs"].any() and (r["arg"] == 0).all() and r["feasible"][0] == 1


def test_ties_go_to_the_first_sample_and_the_limit_is_strict():
    co = straight(5.0, 4, 1.0)[None]
    r = pl.check_batch([1], [4], co, [[1.0]], 0.05, DEFAULT, order=2, max_samples=128)
    n = int(r["n_samples"][0])
    assert n == 81 and (r["samples"][0, :n, 3] == 5.0).all()        # every sample ties (80 steps of 0.05 sum to just under 4.0)
    assert r["max_abs"][0, 0] == 5.0 and r["arg"][0].tolist() == [0] * 5 and r["feasible"][0] == 1
    below = dict(DEFAULT, max_forward_vel=math.nextafter(5.0, 0.0))
    r = pl.check_batch([1], [4], co, [[1.0]], 0.05, below, order=2)
    assert r["violated"][0].tolist() == [1, 0, 0, 0, 0] and r["feasible"][0] == 0


def test_a_reverse_segment_is_judged_by_the_backward_limits():
    fwd, back = straight(3.0, 2, 1.0), straight(3.0, 2, 1.0, direction=-1.0)
    back[:, 0, 0] += 6.0
    co = np.concatenate([fwd, back])[None]
    r = pl.check_batch([1, -1], [2, 2], co, [[1.0, 1.0]], 0.05, DEFAULT, order=2, max_samples=128)
    sm = r["samples"][0, :int(r["n_samples"][0])]
    assert (sm[sm[:, 1] == 0][:, 3] == 3.0).all() and (sm[sm[:, 1] == 1][:, 3] == -3.0).all() and (sm[:, 1] == 1).sum() >= 40
    assert r["violated"][0, 0] == 1 and r["arg"][0, 0] == 0          # 3 m/s: allowed forwards, not backwards; the maximum ties from sample 0
    r = pl.check_batch([1, 1], [2, 2], co, [[1.0, 1.0]], 0.05, DEFAULT, order=2)
    assert r["violated"][0, 0] == 0
    r = pl.check_batch([1, -1], [2, 2], co, [[1.0, 1.0]], 0.05, dict(DEFAULT, max_backward_vel=3.0), order=2)
    assert r["violated"][0, 0] == 0 and r["feasible"][0] == 1


def test_durations_off_the_grid_and_more_than_256_samples():
    co = straight(1.0, 2, 0.5)[None]
    r = pl.check_batch([1], [2], co, [[0.5]], 0.3, DEFAULT, order=2, max_samples=16)
    assert r["n_samples"][0] == 4 and r["samples"][0, :4, 0].tolist() == [0.0, 0.3, 0.6, 0.3 + 0.3 + 0.3]   # 0.9 < 1.0, 1.2 is not
    co = straight(1.0, 16, 1.0)
    co[15, 1, 0], co[15, 2, 0] = 1.0, 0.5                # the last piece accelerates: the maximum lies past sample 256
    r = pl.check_batch([1], [16], co[None], [[1.0]], 0.05, DEFAULT, order=2, max_samples=512)
    n = int(r["n_samples"][0])
    assert n >= 320 and r["arg"][0, 0] == n - 1 > 256 and r["arg"][0, 1] >= 300
    m, a = _plain_loop(r["samples"][0], n)
    assert r["max_abs"][0].tolist() == m and r["arg"][0].tolist() == a


def test_nan_rule_and_empty_plans():
    co = straight(1.0, 3, 1.0)
    co[2, 3, 1] = float("nan")
    r = pl.check_batch([1], [3], co[None], [[1.0]], 0.05, dict(DEFAULT, max_forward_vel=INF, max_latacc=INF), order=2, max_samples=64)
    first = int(np.flatnonzero(np.isnan(r["samples"][0, :60, 3]))[0])
    t, k = 0.0, 0
    while not t - 1.0 > 1.0:                              # locatePieceIdx moves on to the last piece once t - 1.0 > 1.0
        t += 0.05
        k += 1
    assert first == k and k in (40, 41)                   # the first sample on the NaN piece, by the running sum
    assert np.isnan(r["max_abs"][0]).all() and (r["arg"][0] == first).all() and (r["violated"][0] == 1).all() and r["feasible"][0] == 0
    e = pl.check_table([0], np.zeros((1, 8)), np.zeros((1, 8)), np.zeros((1, 8)), np.zeros((1, 4, 6, 2)), 0.05, DEFAULT)
    assert not e["max_abs"].any() and (e["arg"] == -1).all() and not e["violated"].any() and e["feasible"][0] == 0
