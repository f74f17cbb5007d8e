"""The list of active terms of the QUAD shape (dftpav_amd/csrc/solver_ref4.hip: q4_eval, flush; quad_common.h: DenseLds): the lanes
of a wave list the active terms their points have, round by round, and the list is emptied -- every entry evaluated by one lane, the
owners adding their results in list order -- when a round's terms no longer fit behind what it holds, and by the extra round.  A round
with more terms than the list holds is taken in place.  kDense, the list's length, is read from the library.

Bar: every evaluation's cost and gradient and every output of every solve (x, cost, status, iterations, evaluations, hist_sum,
success) BIT-EQUAL to the restatement of the reference (oracle/pyoracle.py, order 2).  Reference order, QUAD shape forced.

How the cases are made: every trajectory is the same path at its nominal duration, which has NO active term at its initial point (asserted).
Terms are then switched on one by one through the corridor: at a chosen constraint point a half-plane keeps its normal and is pulled
in round the initial path, to lie between the footprint's vertices (their positions from the restatement's coefficients at the initial
point), so that exactly the wanted number of the point's vertex-against-plane terms is active -- five for a plane pulled in behind all
five vertices.  Every threshold lies at least 5e-7 from the nearest vertex; the activation test's own rounding is some 1e-14.  The term counts
[trajectory][piece][point] of the finished corridor are counted again over all points and planes, and what the wave does with them --
the sizes of its flushes, the rounds it takes in place -- follows from the counts by the rule above (waves()); each case asserts that before
anything is compared.  A count that cannot be reached fails the test.

Shapes: 16 pieces with 9 points each (n = 31), batches of 4 and 5 trajectories.  Instances: "rect" (H = 4, rectangles: the instance
the bench runs), "planes" (H = 4, one normal turned: no rectangles), "h3" and "h5" (three and five half-planes: the generic instance).
"""
import ctypes as C

import numpy as np
import pytest

from dftpav_amd import scenarios as sc
from dftpav_amd.pods import LayoutSpec

pytestmark = pytest.mark.gpu

KEYS = ("final_cost", "x", "status", "iters", "evals", "hist_sum", "success")
POOL = 64    # kQPool
VMAX = 4.0   # the velocity limit: just above the nominal cruise speed (tests/test_gpu_quad_parked.py)
N, K = 16, 8
ORDER = 2
INSTANCES = ("rect", "planes", "h3", "h5")
_cache = {}


def _scene(B, inst):
    s = sc.make_scenario([N], [1], K, K, B, seed=41, n_obs=30, n_hyp=1, restart_sigma=0.0, dur_scale=(1.0, 1.0))
    H = {"h3": 3, "h5": 5}.get(inst, 4)
    if H != 4:  # h5: a copy of the first plane, moved inwards and rescaled (tests/test_gpu_quad_parked.py); h3: the first three
        cor = np.zeros((B, s.n_points, H, 4))
        cor[:, :, :min(H, 4)] = s.corridor[:, :, :min(H, 4)]
        if H > 4:
            cor[:, :, 4:] = s.corridor[:, :, :H - 4]
            cor[:, :, 4:, 2:] -= 0.2 * s.corridor[:, :, :H - 4, :2]
            cor[:, :, 4:, :2] *= 3.0
        s = sc.Scenario(s.name, LayoutSpec(s.layout.piece_nums, s.layout.singuls, H=H), s.K, s.Kd, B, s.ini_states, s.fin_states,
                        s.inner_pts, s.init_Ts, np.ascontiguousarray(cor))
    if inst == "planes":  # one normal of the batch turned by a milliradian, at a point no case uses: the batch is no batch of rectangles
        n = s.corridor[0, 15 * (K + 1) + 4, 2, :2].copy()
        c, sn = np.cos(1e-3), np.sin(1e-3)
        s.corridor[0, 15 * (K + 1) + 4, 2, :2] = (c * n[0] - sn * n[1], sn * n[0] + c * n[1])
    return s


def _params(hiplib, s):
    p = hiplib.default_params()
    s.apply_resolution(p)
    p.max_forward_vel = VMAX
    p.lbfgs_mem_size = 8
    p.lbfgs_max_iterations = 6
    return p


def _geometry(oracle, p, s, x):
    """Of trajectory 0 at x, from the restatement's coefficients: feas [N][K + 1] active feasibility terms per point, vert [N][K + 1][5][2]
    the footprint's vertices there, live [N][K + 1] whether the point has terms at all (addPVAGradCost2CT's tests)."""
    o = oracle.OracleProblem(p, s, 0, order=ORDER)
    o.eval(x)
    c, dt = o.coeffs()
    sg = s.layout.singuls[0]
    vmax, amax, cmax = p.max_forward_vel, p.max_forward_acc, p.max_forward_cur
    W, Lg, dcr = p.veh_width + 2 * p.half_margin, p.veh_length + 2 * p.half_margin, p.veh_d_cr
    le = [(dcr + Lg / 2, W / 2), (dcr + Lg / 2, -W / 2), (dcr - Lg / 2, -W / 2), (dcr - Lg / 2, W / 2), (dcr + Lg / 2, W / 2)]
    feas = np.zeros((N, K + 1), dtype=np.int64)
    vert = np.zeros((N, K + 1, 5, 2))
    live = np.zeros((N, K + 1), dtype=bool)
    for i in range(N):
        step, s1 = dt[0] / K, 0.0
        for j in range(K + 1):
            b0 = np.array([1.0, s1, s1 ** 2, s1 ** 3, s1 ** 4, s1 ** 5])
            b1 = np.array([0.0, 1.0, 2 * s1, 3 * s1 ** 2, 4 * s1 ** 3, 5 * s1 ** 4])
            b2 = np.array([0.0, 0.0, 2.0, 6 * s1, 12 * s1 ** 2, 20 * s1 ** 3])
            s1 += step
            sig, ds, dds = b0 @ c[i], b1 @ c[i], b2 @ c[i]
            v = float(np.hypot(ds[0], ds[1]))
            if v < 1e-4 or (i == 0 and j == 0) or (i == N - 1 and j == K):
                continue
            live[i, j] = True
            zh1 = float(dds @ ds)
            zh3 = float(dds[1] * ds[0] - dds[0] * ds[1])
            cur = zh3 / (v * v + s.help_eps) ** 1.5
            feas[i, j] = int(v * v - vmax * vmax > 0) + int(zh1 * zh1 / (v * v) - amax * amax > 0) + int(cur - cmax > 0) + int(-cur - cmax > 0)
            R = sg * np.array([[ds[0], -ds[1]], [ds[1], ds[0]]]) / v
            for u, (lx, ly) in enumerate(le):
                vert[i, j, u] = sig + R @ np.array([lx, ly])
    return feas, vert, live


def _counts(geo, cor_b):
    """[N][K + 1] active terms per point of a trajectory with corridor cor_b [points][H][4]: every vertex against every half-plane."""
    feas, vert, live = geo
    cor = np.array(cor_b, dtype=np.float64)
    cor[:, :, :2] /= np.linalg.norm(cor[:, :, :2], axis=2, keepdims=True)
    out = feas.copy()
    for i in range(N):
        for j in range(K + 1):
            if not live[i, j]:
                continue
            for col in cor[i * (K + 1) + j]:
                for bpt in vert[i, j]:
                    out[i, j] += int(col[0] * (bpt[0] - col[2]) + col[1] * (bpt[1] - col[3]) > 0)
    return out


def _pull(geo, cor_b, i, j, m):
    """Switches on exactly m corridor terms of point j of piece i: whole planes behind all five vertices, and one plane between the
    vertices for the rest (vertices 0 and 4 are one corner: a plane has them both or neither)."""
    _, vert, live = geo
    assert live[i, j] and 0 < m <= 5 * cor_b.shape[1], (i, j, m)
    pid = i * (K + 1) + j
    free = list(range(cor_b.shape[1]))

    def put(k, outside):
        n = cor_b[pid, k, :2] / np.linalg.norm(cor_b[pid, k, :2])
        pr = np.sort(vert[i, j] @ n)[::-1]
        if outside == 5:
            t = pr[4] - 0.25
        else:
            if pr[outside - 1] - pr[outside] < 1e-6:
                return False
            t = 0.5 * (pr[outside - 1] + pr[outside])
        cor_b[pid, k, 2:] = n * t
        free.remove(k)
        return True

    if m % 5:
        assert any(put(k, m % 5) for k in list(free)), "no half-plane of point (%d, %d) separates %d of the vertices" % (i, j, m % 5)
    for _ in range(m // 5):
        assert put(free[0], 5)


def _spread(geo, s, rows, j, total, per):
    """total terms in round j: per terms a point, dealt to the rows in turn, piece by piece (1 .. 14), the remainder at the last point."""
    at = [(b, i) for i in range(1, N - 1) for b in rows]
    for b, i in at:
        if total <= 0:
            break
        _pull(geo, s.corridor[b], i, j, min(per, total))
        total -= per
    assert total <= 0, "round %d does not hold that many terms" % j


def waves(counts, T):
    """What every wave does with counts [B][N][K + 1] (q4_eval's rule, list length T): (rows, sizes of its flushes in order, rounds taken
    in place as (round, terms, the size of the flush in front of it or 0))."""
    out = []
    for w in range(0, len(counts), 4):
        listed, flushes, in_place = 0, [], []
        for j, tot in enumerate(counts[w:w + 4].sum(axis=(0, 1))):
            tot, front = int(tot), 0
            if listed > 0 and listed + tot > T:
                flushes.append(listed)
                front, listed = listed, 0
            if tot > T:
                in_place.append((j, tot, front))
            else:
                listed += tot
        if listed > 0:
            flushes.append(listed)
        out.append((len(counts[w:w + 4]), flushes, in_place))
    return out


def _dense(hiplib):
    fn = hiplib.lib().dftpav_debug_quad_list_capacity
    fn.argtypes, fn.restype = [], C.c_int
    T = int(fn())
    assert T % 8 == 0 and 8 <= T <= 64, T
    return T


def _case(hiplib, oracle, inst, B, build):
    """The scene of a case: build(geo, s, T) pulls the half-planes in.  Returns (p, s, x0, counts, T); the geometry and x0 of an
    instance are computed once."""
    T = _dense(hiplib)
    s = _scene(B, inst)
    p = _params(hiplib, s)
    if inst not in _cache:
        x0 = oracle.OracleProblem(p, s, 0, order=ORDER).x0()
        _cache[inst] = (x0, _geometry(oracle, p, s, x0))
    x0, geo = _cache[inst]
    assert all(_counts(geo, s.corridor[b]).sum() == 0 for b in range(B)), "the nominal trajectory has active terms"
    build(geo, s, T)
    counts = np.stack([_counts(geo, s.corridor[b]) for b in range(B)])
    print("terms per row", counts.sum(axis=(1, 2)), "per round of the first wave", counts[:4].sum(axis=(0, 1)), "waves", waves(counts, T))
    return p, s, np.stack([x0] * B), counts, T


def _compare(hiplib, oracle, monkeypatch, p, s, x0):
    """Evaluations at x0 and beside it, and solves: the QUAD shape against the restatement."""
    for b in range(s.B):
        assert np.array_equal(oracle.OracleProblem(p, s, b, order=ORDER).x0(), x0[b])
    want = oracle.solve_batch(p, s, nthreads=8, order=ORDER)
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
    assert np.array_equal(bt.x0(), x0)
    rng = np.random.default_rng(s.B)
    for x in (x0, x0 + rng.normal(0, 0.2, x0.shape)):
        f, g = bt.eval(x)
        for b in range(s.B):
            fo, go = oracle.OracleProblem(p, s, b, order=ORDER).eval(x[b])
            assert f[b] == fo and np.array_equal(g[b], go), (s.B, b)
    bt.set_hand_over(0)  # the QUAD launch finishes every trajectory itself
    r = bt.solve()
    for k in KEYS:
        assert np.array_equal(r[k], want[k]), (s.B, k)
    assert (want["evals"] >= 2).all(), want["evals"]
    bt.close()
    h.close()


@pytest.mark.parametrize("inst", INSTANCES)
def test_exactly_full(hiplib, oracle, monkeypatch, inst):
    """(a) the list reaches exactly kDense entries -- all but four in one round, over the four rows -- and is flushed once, by the
    extra round."""
    def build(geo, s, T):
        _spread(geo, s, range(4), 2, T - 4, 5)
        _pull(geo, s.corridor[2], 5, 5, 4)
    p, s, x0, counts, T = _case(hiplib, oracle, inst, 4, build)
    assert waves(counts, T) == [(4, [T], [])]
    _compare(hiplib, oracle, monkeypatch, p, s, x0)


@pytest.mark.parametrize("inst", INSTANCES)
def test_one_over(hiplib, oracle, monkeypatch, inst):
    """(b) kDense + 1 entries: a later round's single term no longer fits behind the full list -- two flushes, the second of one entry."""
    def build(geo, s, T):
        _spread(geo, s, range(4), 2, T - 4, 5)
        _pull(geo, s.corridor[2], 5, 5, 4)
        _pull(geo, s.corridor[3], 9, 7, 1)
    p, s, x0, counts, T = _case(hiplib, oracle, inst, 4, build)
    assert waves(counts, T) == [(4, [T, 1], [])]
    _compare(hiplib, oracle, monkeypatch, p, s, x0)


@pytest.mark.parametrize("inst", INSTANCES)
def test_round_in_place_behind_a_list(hiplib, oracle, monkeypatch, inst):
    """(c) a round with kDense + 6 terms while the list holds seven: the seven are flushed, the round is taken in place (its pool slots
    numbered behind them), three later terms are listed again."""
    def build(geo, s, T):
        _pull(geo, s.corridor[0], 2, 1, 7)
        _spread(geo, s, range(4), 3, T + 6, 10)
        _pull(geo, s.corridor[1], 4, 6, 3)
    p, s, x0, counts, T = _case(hiplib, oracle, inst, 4, build)
    assert waves(counts, T) == [(4, [7, 3], [(3, T + 6, 7)])]
    _compare(hiplib, oracle, monkeypatch, p, s, x0)


@pytest.mark.parametrize("inst", INSTANCES)
def test_one_row_present(hiplib, oracle, monkeypatch, inst):
    """(d) a second wave with one row: its sixteen lanes take a list of kDense - 3 entries in several passes, then one of eight."""
    def build(geo, s, T):
        _pull(geo, s.corridor[0], 3, 2, 5)
        _spread(geo, s, [4], 2, T - 3, 5)
        _spread(geo, s, [4], 6, 8, 4)
    p, s, x0, counts, T = _case(hiplib, oracle, inst, 5, build)
    assert T - 3 > 16
    assert waves(counts, T) == [(4, [5], []), (1, [T - 3, 8], [])]
    _compare(hiplib, oracle, monkeypatch, p, s, x0)


@pytest.mark.parametrize("inst", INSTANCES)
def test_overflowing_row_beside_an_empty_one(hiplib, oracle, monkeypatch, inst):
    """(e) a row with 70 terms (more than kQPool: its pool slots are numbered across the flushes, the last six go to global scratch)
    in a wave with an empty row and two rows of a few terms."""
    def build(geo, s, T):
        for j, tot in ((1, 20), (2, 20), (3, 20), (5, 10)):
            _spread(geo, s, [1], j, tot, 10)
        _pull(geo, s.corridor[2], 7, 2, 5)
        _pull(geo, s.corridor[2], 8, 4, 2)
        _pull(geo, s.corridor[3], 12, 3, 3)
    p, s, x0, counts, T = _case(hiplib, oracle, inst, 4, build)
    assert counts.sum(axis=(1, 2)).tolist() == [0, 70, 7, 3] and 70 > POOL
    (rows, flushes, in_place), = waves(counts, T)
    assert rows == 4 and sum(flushes) == 80 and not in_place
    _compare(hiplib, oracle, monkeypatch, p, s, x0)
