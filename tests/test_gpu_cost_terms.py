"""dftpav_batch_cost_terms (solver_ref.hip: kModeTerms) and the residual-penalty filter of dftpav_plan_queries / dftpav_replan_tick
(plan.hip: penalty_gate_kernel) on the device.  Every comparison is equality of bits: the terms against the restatement's
OracleProblem.eval + cost_terms in order 2, the cost of dftpav_batch_eval against the terms recomposed in the reference's
association (tests/terms_cases.py: recompose), the filter against the oracle chain with the same rule.  The scenes, their
preconditions and the caps are held by tests/test_cost_terms_cpu.py on the CPU."""
import ctypes as C

import numpy as np
import pytest

import limits_cases as lc
import terms_cases as tc

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
SOLVE_KEYS = ("x", "final_cost", "status", "success", "iters", "evals", "hist_sum")
EXEC_KEYS = ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "duration", "start_time", "end_time", "end_state", "hist", "have_hist")


def _batch(hiplib, p, s):
    h = hiplib.Handle(p)
    if s.surround is not None:
        h.set_surround(s.surround)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    bt.set_order(hiplib.ORDER_REFERENCE)
    return h, bt


def _check_point(bt, p, s, x, oracle_idx):
    """the identity with dftpav_batch_eval on every trajectory, the oracle on those of oracle_idx; -> (terms, seg_terms)"""
    terms, seg = bt.cost_terms(x)
    f, _ = bt.eval(x)
    assert terms.shape == (s.B, 5) and seg.shape == (s.B, s.layout.M, 5)
    for b in range(s.B):
        assert tc.recompose(terms[b], seg[b]) == f[b], b
        assert np.array_equal(tc.chained(seg[b]), terms[b]), b
    for b in oracle_idx:
        fo, to = tc.oracle_terms(p, s, int(b), x[int(b)])
        print(int(b), "terms", terms[b].tolist(), "oracle", to.tolist())
        assert f[b] == fo and np.array_equal(terms[b], to), b
        if s.layout.M == 1:
            assert np.array_equal(seg[b, 0], to), b
    return terms, seg


@pytest.mark.parametrize("name", ["team", "gear", "sur", "generic"])
def test_terms_equal_the_oracle_in_the_team_shape(hiplib, oracle, name):
    """tests 1, 2, 3 and 5 of the issue: one segment of 2 pieces; 3 + 2 pieces with a gear shift (two rows of seg_terms whose chained
    sums are terms); the 2 pieces among moving cars (the SUR instance); six half-planes per point (the generic form)"""
    p, s, xs = tc.scene(name)
    assert tc.reference_plan(s, p, 4 if s.surround is not None else 0) == 0
    h, bt = _batch(hiplib, p, s)
    for x in xs:
        _check_point(bt, p, s, x, range(s.B))
    bt.close()
    h.close()


def test_wave_shape(hiplib, oracle, monkeypatch):
    """2 pieces among the moving cars at the smallest batch that leaves the TEAM shape: one wave per trajectory.  Evaluation only.
    Then the instance without moving obstacles, which no batch of 2 pieces takes by itself (it goes to the QUAD shape), by the
    developer option."""
    p, s, xs = tc.scene("wave")
    assert tc.reference_plan(s, p, 4) == 1
    assert tc.reference_plan(s, p, 4, B=tc.N_WAVE - 1) == 0    # one trajectory fewer: still TEAM
    q = tc.scene("team")
    h, bt = _batch(hiplib, p, s)
    _check_point(bt, p, s, xs[0], np.linspace(0, s.B - 1, 16).astype(int))
    bt.close()
    h.close()
    monkeypatch.setenv("DFTPAV_REF_SHAPE", "wave")
    p, s, xs = q
    assert tc.reference_plan(s, p, 0) == 1
    h, bt = _batch(hiplib, p, s)
    for x in xs:
        _check_point(bt, p, s, x, range(s.B))
    bt.close()
    h.close()


def test_quad_planned_batch_is_served_by_the_team_wave_kernel(hiplib, oracle):
    """a batch whose solves and evaluations run the QUAD kernel: the terms call succeeds (through the WAVE shape of its plan), gives
    what a TEAM-planned batch gives on the same data, and recomposes to the QUAD kernel's cost"""
    p, s, xs = tc.scene("quad")
    assert tc.reference_plan(s, p, 0) == 3
    h, bt = _batch(hiplib, p, s)
    terms, seg = _check_point(bt, p, s, xs[0], range(4))      # dftpav_batch_eval runs the QUAD kernel here
    s4 = s.subset(range(4))
    assert tc.reference_plan(s4, p, 0) == 0
    b4 = hiplib.Batch(h, s4.layout, 4)
    b4.upload(s4)
    b4.set_order(hiplib.ORDER_REFERENCE)
    t4, g4 = b4.cost_terms(xs[0][:4])
    assert np.array_equal(t4, terms[:4]) and np.array_equal(g4, seg[:4])
    b4.close()
    bt.close()
    h.close()


def test_terms_of_the_solution_and_refusals(hiplib, oracle):
    p, s, xs = tc.scene("gear")
    h, bt = _batch(hiplib, p, s)
    fn = hiplib.lib().dftpav_batch_cost_terms
    fn.argtypes = [C.c_void_p] * 4
    t77, g77 = np.full((s.B, 5), 77.0), np.full((s.B, 2, 5), 77.0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert fn(bt._b, None, ptr(t77), ptr(g77)) == hiplib.E_INVALID          # before any solve
    assert (t77 == 77.0).all() and (g77 == 77.0).all()
    r = bt.solve()
    terms, seg = bt.cost_terms()
    tx, gx = bt.cost_terms(r["x"])
    assert np.array_equal(terms, tx) and np.array_equal(seg, gx)
    for b in range(s.B):
        fo, to = tc.oracle_terms(p, s, b, r["x"][b])
        assert np.array_equal(terms[b], to) and tc.recompose(terms[b], seg[b]) == fo == r["final_cost"][b], b
    only_t = np.zeros((s.B, 5))
    assert fn(bt._b, None, ptr(only_t), None) == 0 and np.array_equal(only_t, terms)      # either output may be NULL
    only_g = np.zeros((s.B, 2, 5))
    assert fn(bt._b, None, None, ptr(only_g)) == 0 and np.array_equal(only_g, seg)
    again = bt.results()
    for k in SOLVE_KEYS:
        assert np.array_equal(again[k], r[k]), k                            # the results of the solve are untouched
    # the device order does not keep the penalty classes apart: refused, nothing written, the batch still usable
    bt.set_order(hiplib.ORDER_DEVICE)
    assert fn(bt._b, ptr(np.ascontiguousarray(xs[1])), ptr(t77), ptr(g77)) == hiplib.E_UNSUPPORTED
    assert fn(bt._b, None, ptr(t77), ptr(g77)) == hiplib.E_UNSUPPORTED
    assert (t77 == 77.0).all() and (g77 == 77.0).all()
    fd, _ = bt.eval(xs[1])
    assert np.isfinite(fd).all()
    bt.set_order(hiplib.ORDER_REFERENCE)
    f, _ = bt.eval(xs[1])
    t2, g2 = bt.cost_terms(xs[1])
    assert all(tc.recompose(t2[b], g2[b]) == f[b] for b in range(s.B))
    # what dftpav_batch_eval refuses: a batch nothing was uploaded to
    b2 = hiplib.Batch(h, s.layout, s.B)
    b2.set_order(hiplib.ORDER_REFERENCE)
    assert fn(b2._b, ptr(np.ascontiguousarray(xs[1])), ptr(t77), ptr(g77)) == hiplib.E_INVALID
    assert (t77 == 77.0).all() and (g77 == 77.0).all()
    b2.close()
    bt.close()
    h.close()


def test_gate_hook(hiplib):
    h = hiplib.Handle()
    for caps, terms, flags_in, rejected in tc.gate_cases():
        fo, rj = hiplib.debug_penalty_gate(h, terms, caps, flags_in)
        want_fo, want_rj = tc.gate_rule(terms, caps, flags_in)
        assert np.array_equal(rj, want_rj) and np.array_equal(rj, rejected) and np.array_equal(fo, want_fo), (rj, fo)
    # more than one workgroup
    rng = np.random.default_rng(3)
    t = rng.uniform(0.0, 2.0, (1000, 5))
    t[rng.integers(0, 1000, 40), rng.integers(2, 5, 40)] = NAN
    fi = rng.integers(0, 2, 1000).astype(np.int32)
    caps = hiplib.PenaltyCaps(1.5, 1.0, INF)
    fo, rj = hiplib.debug_penalty_gate(h, t, caps, fi)
    want_fo, want_rj = tc.gate_rule(t, caps, fi)
    assert np.array_equal(rj, want_rj) and np.array_equal(fo, want_fo) and 0 < rj.sum() < 1000
    h.close()


# ---- the planner
def _pp(hiplib):
    pp = hiplib.default_plan_params()
    pp.seed = lc.SEED
    return pp


@pytest.fixture(scope="module")
def arena(hiplib, oracle):
    """the fourteen arena queries, a handle with their map, and the outputs of a planner that never had a filter"""
    grid, res, org, S, E = lc.chain()["scene"]
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl0 = hiplib.Planner(h, len(E), lc.R)
    plain = pl0.plan(S, E, pp=_pp(hiplib))
    yield dict(h=h, S=S, E=E, Q=len(E), plain=plain, pl0=pl0, n_batches=pl0.info()["n_batches"])
    pl0.close()
    h.close()


def _same_outputs(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_filter_set_and_taken_back_is_a_planner_without_one(hiplib, arena):
    pl = hiplib.Planner(arena["h"], arena["Q"], lc.R)
    pl.set_penalty_filter(hiplib.PenaltyCaps(**tc.CAPS))
    pl.set_penalty_filter(None)
    off = pl.plan(arena["S"], arena["E"], pp=_pp(hiplib))
    _same_outputs(off, arena["plain"])
    assert pl.info()["n_batches"] == arena["n_batches"]
    for planner in (pl, arena["pl0"]):
        with pytest.raises(hiplib.DftpavError) as e:
            planner.last_cost_terms(arena["Q"])                 # that call ran without the filter
        assert e.value.code == hiplib.E_INVALID
    pl.close()


def test_caps_of_infinity_change_nothing_and_record_the_terms(hiplib, arena):
    ch = lc.chain()
    T, scen = tc.chain_terms()
    Q = arena["Q"]
    pl = hiplib.Planner(arena["h"], Q, lc.R)
    pl.set_penalty_filter(hiplib.PenaltyCaps())
    out = pl.plan(arena["S"], arena["E"], pp=_pp(hiplib))
    _same_outputs(out, arena["plain"])
    assert pl.info()["n_batches"] == arena["n_batches"]
    terms, rej = pl.last_cost_terms(Q)
    assert not rej.any()
    solved = 0
    for q, c in enumerate(ch["per"]):
        if c is None or out["plan_status"][q] == hiplib.PLAN_LAYOUT_UNSUPPORTED:
            assert not terms[q].any(), q
            continue
        assert np.array_equal(terms[q], T[q]), q                # the oracle chain's terms
        bt = hiplib.Batch(arena["h"], c["layout"], lc.R)         # and the public call on a batch of the query's layout
        bt.upload(scen[q])
        bt.set_order(hiplib.ORDER_REFERENCE)
        tb, _ = bt.cost_terms(c["solve"]["x"])
        bt.close()
        assert np.array_equal(terms[q], tb), q
        solved += 1
    assert solved >= 10
    pl.close()


def test_caps_chosen_on_the_cpu(hiplib, arena):
    ch = lc.chain()
    T, _ = tc.chain_terms()
    Q, plain = arena["Q"], arena["plain"]
    caps = hiplib.PenaltyCaps(**tc.CAPS)
    want_rej = tc.gate_rule(T.reshape(-1, 5), caps, np.zeros(Q * lc.R, np.int32))[1].reshape(Q, lc.R)
    pl = hiplib.Planner(arena["h"], Q, lc.R)
    pl.set_penalty_filter(caps)
    out = pl.plan(arena["S"], arena["E"], pp=_pp(hiplib))
    terms, rej = pl.last_cost_terms(Q)
    lim = hiplib.default_limits()
    lim.max_forward_vel, lim.max_backward_vel, lim.max_forward_cur, lim.max_backward_cur = 5.01, 2.01, 1.01, 1.01   # tests/test_gpu_limits.py: FILTER
    feas = lc.chain_limits(lim)["feasible"]
    pl.set_limit_filter(lim, lc.CHECK_DT)
    both = pl.plan(arena["S"], arena["E"], pp=_pp(hiplib))
    terms_b, rej_b = pl.last_cost_terms(Q)
    assert np.array_equal(terms_b, terms) and np.array_equal(rej_b, rej)
    seen = dict(changed=0, none=0, kept=0)
    differs = 0
    for q, c in enumerate(ch["per"]):
        if c is None or out["plan_status"][q] == hiplib.PLAN_LAYOUT_UNSUPPORTED:
            assert out["winner"][q] == -1 and not terms[q].any() and not rej[q].any(), q
            continue
        r = c["solve"]
        w0 = lc.select(r["final_cost"], r["success"], c["collision"])
        w1 = lc.select(r["final_cost"], r["success"], c["collision"] | want_rej[q])
        w2 = lc.select(r["final_cost"], r["success"], c["collision"] | want_rej[q] | (1 - feas[q]))
        print(q, "winner", w0, "->", w1, "with the limits too", w2, "device", plain["winner"][q], "->", out["winner"][q], both["winner"][q])
        assert np.array_equal(terms[q], T[q]) and np.array_equal(rej[q], want_rej[q]), q
        assert plain["winner"][q] == w0 and out["winner"][q] == w1 and both["winner"][q] == w2, q
        for o, w in ((out, w1), (both, w2)):
            assert o["plan_status"][q] == (hiplib.PLAN_OK if w >= 0 else hiplib.PLAN_NO_VALID_RESTART), q
            assert np.array_equal(o["r_collision"][q], c["collision"]) and np.array_equal(o["r_first_sample"][q], c["first"]), q
            for k in ("r_final_cost", "r_status", "r_success", "r_iters", "r_evals", "r_collision", "r_first_sample"):
                assert np.array_equal(o[k][q], plain[k][q]), (q, k)
            if w >= 0:
                assert o["final_cost"][q] == r["final_cost"][w] and np.array_equal(o["coeffs"][q, :c["layout"].n_pieces], c["coeffs"][w]), q
            else:
                assert not o["coeffs"][q].any(), q
        differs += w2 != w1
        if q in tc.CHANGED:
            assert (w0, w1) == tc.CHANGED[q] and r["final_cost"][w1] > r["final_cost"][w0]
            seen["changed"] += 1
        elif q in tc.NO_VALID:
            assert w0 == tc.NO_VALID[q] and w1 == -1
            seen["none"] += 1
        else:
            assert w0 == w1 == tc.KEPT[q] and np.array_equal(out["coeffs"][q], plain["coeffs"][q])
            seen["kept"] += 1
    assert seen == dict(changed=len(tc.CHANGED), none=len(tc.NO_VALID), kept=len(tc.KEPT))
    assert differs > 0                                           # the limit filter adds rejections of its own
    # ---- refusals: negative or NaN caps and NULL outputs leave the planner and its last results as they are
    for bad in (hiplib.PenaltyCaps(-1.0, INF, INF), hiplib.PenaltyCaps(INF, NAN, INF), hiplib.PenaltyCaps(INF, INF, -1e-300),
                hiplib.PenaltyCaps(NAN, NAN, NAN)):
        with pytest.raises(hiplib.DftpavError) as e:
            pl.set_penalty_filter(bad)
        assert e.value.code == hiplib.E_INVALID
    fn = hiplib.lib().dftpav_planner_last_cost_terms
    fn.argtypes = [C.c_void_p] * 3
    assert fn(pl._p, None, None) == hiplib.E_INVALID
    t2, r2 = pl.last_cost_terms(Q)
    assert np.array_equal(t2, terms) and np.array_equal(r2, rej)
    pl.set_limit_filter(None)
    again = pl.plan(arena["S"], arena["E"], pp=_pp(hiplib))      # the caps are still CAPS
    _same_outputs(again, out)
    pl.set_penalty_filter(hiplib.PenaltyCaps(0.0, 0.0, 0.0))     # legal: no residual penalty at all
    pl.set_penalty_filter(None)
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), plain)
    pl.close()


def test_tick_with_the_filter_keeps_the_plan_of_a_rejected_replanning(hiplib, arena):
    """caps of 0.0: every restart of the replanning keeps some residual penalty, the query ends NO_VALID_RESTART and the slot keeps
    its plan, byte for byte; the same tick with the filter off replaces it"""
    Q, E = arena["Q"], arena["E"]
    pp = _pp(hiplib)
    pl = hiplib.Planner(arena["h"], Q, lc.R)
    out = pl.plan(arena["S"], E, pp=pp)
    ok = np.flatnonzero((out["plan_status"] == hiplib.PLAN_OK) & (out["winner"] >= 0))
    pl.adopt(ok, ok, t_start=0.0, pp=pp)
    before = [pl.executing(q) for q in range(Q)]
    total = {int(q): float(before[q]["end_time"][before[q]["n_seg"] - 1]) for q in ok}
    c = min([q for q in total if before[q]["n_seg"] == 1], key=lambda q: total[q])   # the shortest plan of one gear segment
    pl.clear([q for q in range(Q) if q != c])
    t_now, budget = 0.4 * total[c], 0.5
    goals = E.copy()
    goals[c, 0] += 0.6
    pl.set_penalty_filter(hiplib.PenaltyCaps(0.0, 0.0, 0.0))
    tk = pl.tick(t_now, budget, end_states=goals, pp=pp)
    assert tk["query_slot"].tolist() == [c]
    terms, rej = pl.last_cost_terms(1)
    print("plan_status with the filter:", tk["plan"]["plan_status"].tolist(), "r_success", tk["plan"]["r_success"].tolist(), "terms", terms[0].tolist())
    want = tc.gate_rule(terms[0], hiplib.PenaltyCaps(0.0, 0.0, 0.0), np.zeros(lc.R, np.int32))[1]
    assert np.array_equal(rej[0], want) and rej[0].all() and tk["plan"]["r_success"][0].any()
    assert tk["plan"]["plan_status"][0] == hiplib.PLAN_NO_VALID_RESTART and tk["plan"]["winner"][0] == -1
    assert all(np.array_equal(np.asarray(pl.executing(c)[k]), np.asarray(before[c][k])) for k in EXEC_KEYS)
    pl.set_penalty_filter(None)
    tk2 = pl.tick(t_now, budget, end_states=goals, pp=pp)
    assert tk2["query_slot"].tolist() == [c] and tk2["plan"]["plan_status"][0] == hiplib.PLAN_OK
    for k in ("r_final_cost", "r_success", "r_collision", "r_first_sample"):
        assert np.array_equal(tk2["plan"][k], tk["plan"][k]), k
    ex = pl.executing(c)
    assert ex["start_time"][0] == t_now + budget and np.array_equal(ex["coeffs"], tk2["plan"]["coeffs"][0])
    pl.close()
