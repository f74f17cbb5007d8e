"""dftpav_plan_queries on the device: fourteen start / goal queries on the default arena (dftpav_amd/search_scenes.py:
arena_plan_queries -- the twelve arena goals, one goal inside an obstacle, one closer than 1 m), several layouts in one call,
against (1) the chain of CPU oracles in order 2, search -> resample -> restart oracle -> corridor -> solve -> validate, and
(2) the separate public calls made one layout at a time; the selection rule on crafted arrays; independence of the queries
from one another, reuse of the cached batches, and the error paths."""
import numpy as np
import pytest

from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import FrontendParams, LayoutSpec
from dftpav_amd.scenarios import Scenario
from oracle_search import pysearch as ps

pytestmark = pytest.mark.gpu

R = 4          # restarts per query in the oracle comparisons (every one of them is solved on the CPU too)
SEED = 7
K, KD = 16, 32
PER_RESTART = ("r_final_cost", "r_status", "r_success", "r_iters", "r_evals", "r_collision", "r_first_sample")


def _pp(hiplib):
    pp = hiplib.default_plan_params()
    pp.seed = SEED
    return pp


def _layout_of(row, q):
    M = int(row["n_seg"][q])
    return LayoutSpec([int(v) for v in row["piece_nums"][q, :M]], [int(v) for v in row["singul"][q, :M]], 4)


def _hypothesis(fe, h, lay):
    """(inner [n_inner], durations [M], poses [Npts][3]) of hypothesis h of a front-end result"""
    M, pn = lay.M, lay.piece_nums
    inner = np.concatenate([fe["inner_pts"][h, i, :pn[i] - 1].reshape(-1) for i in range(M)])
    durs = fe["piece_dt"][h, :M] * fe["piece_nums"][h, :M]
    states = np.concatenate([fe["states"][h, i, :fe["n_states"][h, i]] for i in range(M)])
    return inner, durs, states


def _restarts_of(sample, q, inner, durs):
    """the R restarts of query q: the sampler keys its streams by (seed, hypothesis, restart), and the hypothesis is the query's
    index in the call -- so the hypothesis goes in as row q of q + 1 rows"""
    a = np.zeros((q + 1, inner.size))
    d = np.ones((q + 1, durs.size))
    a[q], d[q] = inner, durs
    oi, od = sample(a, d, R, seed=SEED)
    return oi[q * R:(q + 1) * R].copy(), od[q * R:(q + 1) * R].copy()


def _scenario(lay, fe, h, inner_r, durs_r, corridor):
    npts = lay.n_points(K, KD)
    M = lay.M
    return Scenario("plan", lay, K, KD, R, np.repeat(fe["ini_states"][h:h + 1, :M], R, 0).copy(),
                    np.repeat(fe["fin_states"][h:h + 1, :M], R, 0).copy(), inner_r, durs_r,
                    corridor if corridor is not None else np.zeros((R, npts, 4, 4)))


def _select(cost, success, collision):
    """the selection rule, restated: among restarts that succeeded and do not collide the smallest cost; a NaN never wins; ties
    go to the lowest index; -1 if none qualifies"""
    cost, ok = np.asarray(cost, dtype=np.float64), (np.asarray(success) != 0) & (np.asarray(collision) == 0)
    ok = ok & ~np.isnan(cost)
    w = np.full(cost.shape[0], -1, dtype=np.int32)
    for q in range(cost.shape[0]):
        idx = np.flatnonzero(ok[q])
        if idx.size:
            w[q] = idx[np.argmin(cost[q, idx])]      # argmin: the first of equal minima
    return w


@pytest.fixture(scope="module")
def scene():
    return ss.arena_plan_queries()


@pytest.fixture(scope="module")
def planned(hiplib, scene):
    """one call of dftpav_plan_queries on the scene, and the handle / planner it ran on"""
    grid, res, org, S, E = scene
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl = hiplib.Planner(h, len(E), R)
    out = pl.plan(S, E, pp=_pp(hiplib))
    yield h, pl, out
    pl.close()
    h.close()


@pytest.fixture(scope="module")
def chain(hiplib, oracle, scene):
    """the chain of oracles in order 2, query by query: dict(search, arrived, per query None or dict(layout, results ...))"""
    grid, res, org, S, E = scene
    p = hiplib.default_params()
    Q = len(E)
    o = ps.kino_search(grid, res, org, S, E, order=2, nthreads=8)
    arrived = np.hypot(E[:, 0] - S[:, 0], E[:, 1] - S[:, 1]) < 1.0
    fp = FrontendParams.default(K=K, Kd=KD)
    per = [None] * Q
    for q in range(Q):
        if arrived[q] or o["status"][q] != 2:
            continue
        n = int(o["path_len"][q])
        fe = oracle.frontend_resample(o["paths"][q:q + 1, :n].copy(), o["path_len"][q:q + 1].copy(), S[q:q + 1], E[q:q + 1],
                                      np.zeros((1, 2)), fp, order=2)
        if not 1 <= fe["n_seg"][0] <= 8:
            per[q] = dict(fe=fe, layout=None)
            continue
        lay = _layout_of(fe, 0)
        inner, durs, states = _hypothesis(fe, 0, lay)
        assert states.shape[0] == lay.n_points(K, KD)
        inner_r, durs_r = _restarts_of(oracle.sample_restarts, q, inner, durs)
        cor = oracle.corridor_rectangles(grid, res, org, states, order=2)
        s = _scenario(lay, fe, 0, inner_r, durs_r, np.repeat(cor[None], R, 0))
        r = oracle.solve_batch(p, s, nthreads=8, order=2)
        co, dts = [], []
        for b in range(R):
            pr = oracle.OracleProblem(p, s, b, order=2)
            pr.eval(r["x"][b])
            a, d = pr.coeffs()
            co.append(a)
            dts.append(d)
        co, dts = np.array(co), np.array(dts)
        col, first = oracle.validate_trajectories(grid, res, org, co, dts, lay.piece_nums, lay.singuls, order=2)
        per[q] = dict(fe=fe, layout=lay, solve=r, coeffs=co, dts=dts, collision=col, first=first)
    return dict(search=o, arrived=arrived, per=per)


def _key(lay):
    return (tuple(lay.piece_nums.tolist()), tuple(lay.singuls.tolist()))


def test_scene_meets_the_conditions(hiplib, chain):
    """by the oracle chain alone: >= 3 distinct layouts, one of them with M >= 2, a NO_PATH, an ARRIVED, and at most two queries
    outside the padding or the reference order's limits"""
    layouts, odd, no_path = set(), 0, 0
    for q, c in enumerate(chain["per"]):
        if chain["arrived"][q]:
            continue
        if c is None:
            no_path += 1
        elif c["layout"] is None:
            odd += 1
        else:
            layouts.add(_key(c["layout"]))
    print("layouts:", sorted(layouts), "no path:", no_path, "arrived:", int(chain["arrived"].sum()), "outside:", odd)
    assert len(layouts) >= 3 and any(len(k[0]) >= 2 for k in layouts)
    assert no_path >= 1 and chain["arrived"].sum() >= 1 and odd <= 2


def test_against_the_oracle_chain(hiplib, planned, chain):
    h, pl, out = planned
    o = chain["search"]
    assert np.array_equal(out["search_status"], o["status"])
    assert np.array_equal(out["search_iters"], o["iters"])
    assert np.array_equal(out["search_path_len"], o["path_len"])
    n_plans, odd = 0, 0
    for q, c in enumerate(chain["per"]):
        st = int(out["plan_status"][q])
        if chain["arrived"][q]:
            assert st == hiplib.PLAN_ARRIVED, q
            continue
        if c is None:
            assert st == hiplib.PLAN_NO_PATH and out["winner"][q] == -1, q
            continue
        if c["layout"] is None:
            assert st == hiplib.PLAN_TOO_MANY_SEGMENTS, q
            odd += 1
            continue
        if st == hiplib.PLAN_LAYOUT_UNSUPPORTED:
            odd += 1
            continue
        lay, r = c["layout"], c["solve"]
        M, n = lay.M, lay.n_vars
        assert out["n_seg"][q] == M and np.array_equal(out["singul"][q, :M], lay.singuls), q
        assert np.array_equal(out["piece_nums"][q, :M], lay.piece_nums) and np.array_equal(out["piece_dt"][q, :M], c["fe"]["piece_dt"][0, :M]), q
        for a, b in (("r_final_cost", r["final_cost"]), ("r_status", r["status"]), ("r_iters", r["iters"]), ("r_evals", r["evals"]),
                     ("r_success", r["success"]), ("r_collision", c["collision"]), ("r_first_sample", c["first"])):
            print(q, a, out[a][q], b)
            assert np.array_equal(out[a][q], b), (q, a)
        w = int(_select(r["final_cost"][None], r["success"][None], c["collision"][None])[0])
        assert out["winner"][q] == w, q
        assert st == (hiplib.PLAN_OK if w >= 0 else hiplib.PLAN_NO_VALID_RESTART), q
        if w >= 0:
            n_plans += 1
            assert out["final_cost"][q] == r["final_cost"][w] and out["iters"][q] == r["iters"][w], q
            assert np.array_equal(out["x"][q, :n], r["x"][w]) and not out["x"][q, n:].any(), q
            assert np.array_equal(out["coeffs"][q, :lay.n_pieces], c["coeffs"][w]) and not out["coeffs"][q, lay.n_pieces:].any(), q
            assert np.array_equal(out["coeff_dt"][q, :M], c["dts"][w]), q
    assert odd <= 2 and n_plans >= 3
    # every winner obeys the rule, given the per-restart arrays returned
    solved = np.isin(out["plan_status"], (hiplib.PLAN_OK, hiplib.PLAN_NO_VALID_RESTART))
    assert np.array_equal(out["winner"][solved], _select(out["r_final_cost"], out["r_success"], out["r_collision"])[solved])
    assert (out["winner"][~solved] == -1).all()
    info = pl.info()
    print("groups:", info["group_sizes"], "batches:", info["n_batches"], "stage ms:", info["stage_ms"])
    assert len(info["group_sizes"]) >= 3 and info["n_batches"] == len(info["group_sizes"])


def test_against_the_separate_public_calls(hiplib, planned, scene):
    """the same quantities through kino_search, frontend_resample, sample_restarts, Batch.upload (host set-up), corridor_from_states,
    the reference-order solve, coeffs and validate, one layout at a time"""
    grid, res, org, S, E = scene
    h, pl, out = planned
    Q = len(E)
    sr = h.kino_search(S, E)
    assert np.array_equal(out["search_status"], sr["status"]) and np.array_equal(out["search_iters"], sr["iters"])
    assert np.array_equal(out["search_path_len"], sr["path_len"])
    arrived = np.hypot(E[:, 0] - S[:, 0], E[:, 1] - S[:, 1]) < 1.0
    use = np.flatnonzero((sr["status"] == 2) & ~arrived)
    fp = FrontendParams.default(K=K, Kd=KD)
    mp = int(sr["path_len"].max())
    fe = h.frontend_resample(sr["paths"][use, :mp].copy(), sr["path_len"][use].copy(), S[use], E[use], np.zeros((len(use), 2)), fp)
    g = hiplib.plan_group_layouts(np.full(len(use), 2, dtype=np.int32), fe["n_seg"], fe["singul"], fe["piece_nums"])
    atan2_only = []
    for gi, f in enumerate(g["group_first"]):
        members = np.flatnonzero(g["group"] == gi)
        lay = _layout_of(fe, f)
        if out["plan_status"][use[f]] == hiplib.PLAN_LAYOUT_UNSUPPORTED:
            continue
        B = len(members) * R
        inner_r, durs_r, states = [], [], []
        for m in members:
            inner, durs, st = _hypothesis(fe, m, lay)
            a, d = _restarts_of(h.sample_restarts, int(use[m]), inner, durs)
            inner_r.append(a)
            durs_r.append(d)
            states.append(st)
        npts = lay.n_points(K, KD)
        s = Scenario("plan-public", lay, K, KD, B, np.repeat(fe["ini_states"][members, :lay.M], R, 0).copy(),
                     np.repeat(fe["fin_states"][members, :lay.M], R, 0).copy(), np.concatenate(inner_r), np.concatenate(durs_r),
                     np.zeros((B, npts, 4, 4)))
        bt = hiplib.Batch(h, lay, B)
        bt.upload(s, with_corridor=False)
        bt.corridor_from_states(np.array(states), n_restarts=R)
        bt.set_order(hiplib.ORDER_REFERENCE)
        r = bt.solve()
        co, dts = bt.coeffs()
        col, first = bt.validate()
        # where the host libm's atan2 of a junction angle is not correctly rounded the host set-up starts from another x0:
        # reported with its arguments, the oracle chain stays the contract for those queries
        x0 = bt.x0().reshape(len(members), R, -1)
        ang = slice(lay.n_vars - (lay.M - 1), lay.n_vars)
        fin = s.fin_states.reshape(len(members), R, lay.M, 6)
        bt.close()
        for k, m in enumerate(members):
            q = int(use[m])
            if lay.M > 1:
                cr = hiplib_cr_atan2(hiplib, fin[k, 0, :-1, 3], fin[k, 0, :-1, 2])
                if not np.array_equal(cr, x0[k, 0, ang]):
                    atan2_only.append((q, fin[k, 0, :-1, 3].tolist(), fin[k, 0, :-1, 2].tolist()))
                    continue
            sl = slice(k * R, (k + 1) * R)
            for a, b in (("r_final_cost", r["final_cost"]), ("r_status", r["status"]), ("r_success", r["success"]), ("r_iters", r["iters"]),
                         ("r_evals", r["evals"]), ("r_collision", col), ("r_first_sample", first)):
                assert np.array_equal(out[a][q], b[sl]), (q, a)
            w = int(out["winner"][q])
            assert w == int(_select(r["final_cost"][None, sl], r["success"][None, sl], col[None, sl])[0]), q
            if w >= 0:
                t = k * R + w
                assert np.array_equal(out["x"][q, :lay.n_vars], r["x"][t]) and out["final_cost"][q] == r["final_cost"][t], q
                assert np.array_equal(out["coeffs"][q, :lay.n_pieces], co[t]) and np.array_equal(out["coeff_dt"][q, :lay.M], dts[t]), q
    print("queries left to the oracle chain (host atan2 not correctly rounded at y, x):", atan2_only)
    assert len(atan2_only) < len(use)


def hiplib_cr_atan2(hiplib, y, x):
    import ctypes as C
    y = np.ascontiguousarray(y, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    o = np.zeros_like(y)
    fn = hiplib.lib().dftpav_debug_cr_atan2
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    fn(len(y), y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p))
    return o


@pytest.mark.parametrize("n_restarts", [1, 7, 64, 100])
def test_selection_rule(hiplib, n_restarts):
    rng = np.random.default_rng(n_restarts)
    h = hiplib.Handle()
    nq, Rr = 40, n_restarts
    cost = rng.integers(0, 6, (nq, Rr)).astype(np.float64)     # few distinct values: ties everywhere
    suc = (rng.random((nq, Rr)) < 0.7).astype(np.int32)
    col = (rng.random((nq, Rr)) < 0.3).astype(np.int32)
    suc[0] = 0                                   # all failed
    col[1], suc[1] = 1, 1                        # all colliding
    cost[2], suc[2], col[2] = 3.0, 1, 0          # every restart ties: the first one
    cost[3], suc[3], col[3] = np.nan, 1, 0       # only NaN: none
    cost[4], suc[4], col[4] = np.inf, 1, 0       # only +inf: the first one
    cost[5], suc[5], col[5] = np.nan, 1, 0
    cost[5, Rr - 1] = np.inf                     # NaN everywhere but an +inf at the end: that one
    cost[6], suc[6], col[6] = 2.0, 1, 0
    cost[6, Rr - 1] = -1.0                       # the minimum in the last lane used
    cost[7], suc[7], col[7] = 5.0, 1, 0
    cost[7, Rr // 2] = 0.0
    suc[7, Rr // 2] = 0                          # the cheapest failed: not it
    cost[8], suc[8], col[8] = 0.0, 1, 0
    cost[8, 0] = -0.0                            # -0.0 == 0.0: a tie, the lowest index
    cost[9], suc[9], col[9] = -np.inf, 1, 1
    cost[9, Rr - 1], col[9, Rr - 1] = np.nan, 0  # the only free restart is a NaN: none
    w = hiplib.debug_plan_select(h, cost, suc, col)
    ref = _select(cost, suc, col)
    assert np.array_equal(w, ref)
    assert w[0] == -1 and w[1] == -1 and w[2] == 0 and w[3] == -1 and w[4] == 0 and w[9] == -1
    assert w[5] == Rr - 1 and w[6] == Rr - 1
    h.close()


def test_permutation_reuse_and_subsets(hiplib, planned, scene):
    grid, res, org, S, E = scene
    h, pl, out = planned
    pp = _pp(hiplib)
    n0 = pl.info()["n_batches"]
    again = pl.plan(S, E, pp=pp)                   # a second identical call: the same bits, no new batch
    for k in out:
        assert np.array_equal(out[k], again[k], equal_nan=True), k
    assert pl.info()["n_batches"] == n0
    # independence: the search, the layout and the plan of a query do not depend on its neighbours.  (A query's restarts are keyed
    # by its index in the call, so a permuted call is compared with restart 0 -- the hypothesis itself -- which no key touches;
    # the queries that keep their index are compared in full.)
    perm = np.arange(len(E))[::-1].copy()
    mid = len(E) // 2
    perm[mid], perm[-1 - mid] = perm[-1 - mid], perm[mid]
    pm = pl.plan(S[perm], E[perm], pp=pp)
    for k in ("plan_status", "n_seg", "singul", "piece_nums", "piece_dt", "search_status", "search_iters", "search_path_len"):
        assert np.array_equal(pm[k], out[k][perm]), k
    for k in PER_RESTART:
        assert np.array_equal(pm[k][:, 0], out[k][perm][:, 0], equal_nan=True), k
    fixed = np.flatnonzero(perm == np.arange(len(E)))
    for k in out:
        assert np.array_equal(pm[k][fixed], out[k][fixed], equal_nan=True), k
    assert pl.info()["n_batches"] == n0
    # a subset of the queries, at the same indices, on the cached batches
    nsub = len(E) - 5
    sub = pl.plan(S[:nsub], E[:nsub], pp=pp)
    for k in out:
        assert np.array_equal(sub[k], out[k][:nsub], equal_nan=True), k
    assert pl.info()["n_batches"] == n0


def test_permuted_queries_with_one_restart_permute_bit_for_bit(hiplib, scene):
    """with the hypothesis alone (n_restarts = 1: no key is drawn from) every output of a permuted call is the permuted output"""
    grid, res, org, S, E = scene
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl = hiplib.Planner(h, len(E), 1)
    pp = _pp(hiplib)
    a = pl.plan(S, E, pp=pp)
    perm = np.random.default_rng(3).permutation(len(E))
    b = pl.plan(S[perm], E[perm], pp=pp)
    for k in a:
        assert np.array_equal(b[k], a[k][perm], equal_nan=True), k
    assert (a["plan_status"] == hiplib.PLAN_OK).sum() >= 3
    pl.close()
    h.close()


def test_a_restart_below_mini_T_refuses_the_query(hiplib, scene):
    """dur_lo = dur_hi = 1e-3 with two restarts: restart 0 keeps its durations, restart 1 of every solved query falls below mini_T
    (plan.hip: mini_t_flag) -- the query is reported without a plan, its compact outputs zero, its restart 0 as in a plain call;
    the queries that never reach a solve, and a plain call afterwards, are untouched by it"""
    grid, res, org, S, E = scene
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl = hiplib.Planner(h, len(E), 2)
    plain = pl.plan(S, E, pp=_pp(hiplib))
    short = _pp(hiplib)
    short.dur_lo = short.dur_hi = 1e-3
    out = pl.plan(S, E, pp=short)
    solved = np.isin(plain["plan_status"], (hiplib.PLAN_OK, hiplib.PLAN_NO_VALID_RESTART))
    print("solved by the plain call:", np.flatnonzero(solved).tolist(), "status", plain["plan_status"].tolist(), "->", out["plan_status"].tolist())
    assert solved.sum() >= 3 and (~solved).sum() >= 2 and (plain["plan_status"] == hiplib.PLAN_OK).sum() >= 3
    # the bound of the scene: a segment shorter than 100 s times 1e-3 is below the default mini_T
    assert h.params.mini_T == 0.1
    seg = out["piece_dt"] * out["piece_nums"]
    for q in np.flatnonzero(solved):
        M = int(out["n_seg"][q])
        assert M >= 1 and (seg[q, :M] > 0.0).all() and (seg[q, :M] < 100.0).all(), (q, seg[q, :M])
    for q in np.flatnonzero(solved):
        assert out["plan_status"][q] == hiplib.PLAN_NO_VALID_RESTART and out["winner"][q] == -1, q
        assert out["final_cost"][q] == 0.0 and out["iters"][q] == 0, q
        assert not out["x"][q].any() and not out["coeffs"][q].any() and not out["coeff_dt"][q].any(), q
        for k in PER_RESTART:
            assert np.array_equal(out[k][q, 0], plain[k][q, 0], equal_nan=True), (q, k)
    for k in plain:
        assert np.array_equal(out[k][~solved], plain[k][~solved], equal_nan=True), k
    again = pl.plan(S, E, pp=_pp(hiplib))
    for k in plain:
        assert np.array_equal(again[k], plain[k], equal_nan=True), k
    pl.close()
    h.close()


def test_errors_leave_the_planner_usable(hiplib, scene):
    grid, res, org, S, E = scene
    h = hiplib.Handle()
    with pytest.raises(hiplib.DftpavError) as e:
        hiplib.Planner(h, 4, 0)                   # n_restarts < 1
    assert e.value.code == hiplib.E_INVALID
    pl = hiplib.Planner(h, 2, 2)
    pp = _pp(hiplib)
    with pytest.raises(hiplib.DftpavError) as e:
        pl.plan(S[:2], E[:2], pp=pp)              # no map
    assert e.value.code == hiplib.E_INVALID
    h.set_grid_map(grid, res, org)
    with pytest.raises(hiplib.DftpavError) as e:
        pl.plan(S[:3], E[:3], pp=pp)              # Q > max_queries
    assert e.value.code == hiplib.E_INVALID
    bad = _pp(hiplib)
    bad.max_seg = 9
    with pytest.raises(hiplib.DftpavError) as e:
        pl.plan(S[:2], E[:2], pp=bad)
    assert e.value.code == hiplib.E_INVALID
    r = pl.plan(S[:2], E[:2], pp=pp)              # and the planner still plans
    assert np.isin(r["plan_status"], (hiplib.PLAN_OK, hiplib.PLAN_NO_VALID_RESTART)).all() and (r["search_status"] == 2).all()
    assert np.array_equal(r["winner"], _select(r["r_final_cost"], r["r_success"], r["r_collision"]))
    assert pl.plan(S[:0], E[:0], pp=pp)["plan_status"].shape == (0,)
    pl.close()
    h.close()
