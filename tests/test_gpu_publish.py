"""The 100 Hz publisher on the device: dftpav_planner_publish on the crafted scene of dftpav_amd/publish_scenes.py, states,
codes and the written-back state bit-equal to oracle_publish in order 2 (the full clock list, one tick, one chunk plus one
tick, the list cut into two calls); the table and the check untouched by it; the publisher's state across dftpav_replan_tick on
the arena scene of tests/test_gpu_replan.py; clear; and the refusals."""
import numpy as np
import pytest

from dftpav_amd import publish_scenes as ps
from dftpav_amd import search_scenes as ss
from oracle_publish import pypublish as pp

pytestmark = pytest.mark.gpu

R = 2
SEED = 7
EXEC_KEYS = ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "duration", "start_time", "end_time", "end_state", "hist", "have_hist")


@pytest.fixture(scope="module")
def scene(oracle):
    return ps.crafted(oracle.minco_generate)


def _oracle_table(scene):
    T = pp.Table(ps.N_SLOTS)
    for s, p in enumerate(scene["slots"]):
        if p is None:
            continue
        T.install(s, p["singul"], p["piece_nums"], p["coeff_dt"], p["coeffs"], p["t_start"])
        if p["ctrl_hist"] is not None:
            T.set_ctrl_history(s, *p["ctrl_hist"])
    return T


@pytest.fixture(scope="module")
def full(scene):
    """the oracle's run of the full clock list, computed once: (outputs, the table with the final publisher state)"""
    T = _oracle_table(scene)
    return pp.publish(T, scene["clocks"], order=2), T


def _install_scene(pl, scene):
    pad = ps.padded(scene)
    for k in range(len(pad["slots"])):          # one call per plan: each has its own t_start
        sl = slice(k, k + 1)
        pl.install(pad["slots"][sl], pad["n_seg"][sl], pad["singul"][sl], pad["piece_nums"][sl], pad["coeff_dt"][sl], pad["coeffs"][sl],
                   pad["end_states"][sl], t_start=pad["t_start"][k])
    for s, p in enumerate(scene["slots"]):
        if p is not None and p["ctrl_hist"] is not None:
            pl.set_ctrl_history([s], [p["ctrl_hist"][0]], [p["ctrl_hist"][1]])


def _planner(hiplib, scene):
    h = hiplib.Handle()
    pl = hiplib.Planner(h, ps.N_SLOTS, R)
    _install_scene(pl, scene)
    return h, pl


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_state(pl, T):
    """the publisher's state of every slot, read back, against the oracle table's: bit for bit"""
    for s in range(T.slots):
        st = pl.publisher_state(s)
        assert (st["exe_index"], st["have_hist"]) == (int(T.exe_index[s]), int(T.have[s])), s
        assert np.array_equal(_bits(st["hist"]), _bits(T.hist[s])), s


def _same_rows(got, ref, n=None):
    sl = slice(None, n)
    assert np.array_equal(got["published"], ref["published"][sl])
    assert np.array_equal(_bits(got["states"]), _bits(ref["states"][sl]))       # bit for bit, the sign of a zero included


def _same_exec(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in EXEC_KEYS)


@pytest.mark.parametrize("n", ["full", 1, ps.CHUNK + 1])
def test_publish_equals_the_oracle(hiplib, scene, full, n):
    clocks = scene["clocks"] if n == "full" else scene["clocks"][:n]
    if n == "full":
        ref, T = full
    else:
        T = _oracle_table(scene)
        ref = pp.publish(T, clocks, order=2)
    h, pl = _planner(hiplib, scene)
    _same_state(pl, _oracle_table(scene))                     # after install + set_ctrl_history
    assert pl.publish_last_ms() == 0.0
    got = pl.publish(clocks)
    print("published codes per slot:", [np.bincount(got["published"][:, s], minlength=3).tolist() for s in range(ps.N_SLOTS)])
    _same_rows(got, ref)
    _same_state(pl, T)
    assert got["published"].max() == 2 and pl.publish_last_ms() > 0.0          # slot 6 is filtered from the first tick on
    pl.close()
    h.close()


def test_split_calls_and_null_outputs(hiplib, scene, full):
    ref, T = full
    cut = scene["split"]
    h, pl = _planner(hiplib, scene)
    a = pl.publish(scene["clocks"][:cut])
    b = pl.publish(scene["clocks"][cut:])
    _same_rows(dict(published=np.concatenate([a["published"], b["published"]]), states=np.concatenate([a["states"], b["states"]])), ref)
    _same_state(pl, T)
    pl.close()
    # either output may be NULL: the state advances all the same
    h2, pl2 = _planner(hiplib, scene)
    only_codes = pl2.publish(scene["clocks"][:cut], want_states=False)
    assert only_codes["states"] is None and np.array_equal(only_codes["published"], ref["published"][:cut])
    none = pl2.publish(scene["clocks"][cut:], want_states=False, want_published=False)
    assert none["states"] is None and none["published"] is None
    _same_state(pl2, T)
    pl2.close()
    h2.close()
    h.close()


def test_table_and_check_untouched_clear_and_refusals(hiplib, scene, full):
    ref, T = full
    grid, res, org, _, _ = ss.arena()
    h, pl = _planner(hiplib, scene)
    h.set_grid_map(grid, res, org)
    fresh = hiplib.Planner(h, ps.N_SLOTS, R)
    with pytest.raises(hiplib.DftpavError) as e:                 # before the table was filled once
        fresh.publish(scene["clocks"][:4])
    assert e.value.code == hiplib.E_INVALID
    st = fresh.publisher_state(3)
    assert (st["exe_index"], st["have_hist"]) == (0, 0) and not st["hist"].any() and fresh.padding() == (0, 0)
    fresh.close()
    before = [pl.executing(s) for s in range(ps.N_SLOTS)]
    check_before = pl.check(ps.T0, 0.5)
    cut = scene["split"]
    pl.publish(scene["clocks"][:cut])
    T1 = _oracle_table(scene)
    pp.publish(T1, scene["clocks"][:cut])
    _same_state(pl, T1)
    # the refusals: state and table stay as they were
    bad = [np.zeros(0), np.zeros(hiplib.PUBLISH_MAX_TICKS + 1), np.array([ps.T0, float("nan")])]
    for clocks in bad:
        with pytest.raises(hiplib.DftpavError) as e:
            pl.publish(clocks)
        assert e.value.code == hiplib.E_INVALID
    for fn in (lambda: pl.set_ctrl_history([8], [0.0], [0.0]), lambda: pl.set_ctrl_history([ps.N_SLOTS], [0.0], [0.0]),
               lambda: pl.publisher_state(ps.N_SLOTS), lambda: pl.publisher_state(-1)):      # an empty slot; out of range
        with pytest.raises(hiplib.DftpavError) as e:
            fn()
        assert e.value.code == hiplib.E_INVALID
    _same_state(pl, T1)
    assert all(_same_exec(before[s], pl.executing(s)) for s in range(ps.N_SLOTS))          # publish wrote nothing into the table
    check_after = pl.check(ps.T0, 0.5)
    for k in check_before:
        assert np.array_equal(check_before[k], check_after[k]), k                          # the check derives its index from its clock
    # and the rest of the list still gives the single call's rows
    got = pl.publish(scene["clocks"][cut:])
    assert np.array_equal(got["published"], ref["published"][cut:]) and np.array_equal(_bits(got["states"]), _bits(ref["states"][cut:]))
    _same_state(pl, T)
    # clear drops the state; install starts it anew
    assert pl.publisher_state(6)["have_hist"] == 1 and pl.publisher_state(6)["exe_index"] == int(T.exe_index[6]) > 0
    pl.clear([6, 7])
    for s in (6, 7):
        st = pl.publisher_state(s)
        assert (st["exe_index"], st["have_hist"]) == (0, 0) and not st["hist"].any()
    assert pl.publisher_state(1)["exe_index"] == int(T.exe_index[1]) > 0
    b1 = before[1]
    pl.install([1], [b1["n_seg"]], b1["singul"][None], b1["piece_nums"][None], b1["coeff_dt"][None], b1["coeffs"][None], b1["end_state"][None],
               t_start=b1["start_time"][0])
    st = pl.publisher_state(1)
    assert (st["exe_index"], st["have_hist"]) == (0, 0) and not st["hist"].any()
    got = pl.publish(scene["clocks"][:3])
    assert not got["published"][:, [6, 7, 8]].any() and np.array_equal(got["published"][:, 1], ref["published"][:3, 1])
    pl.close()
    h.close()


def _pub_states(pl, Q):
    return [pl.publisher_state(q) for q in range(Q)]


def _same_pub(a, b):
    return (a["exe_index"], a["have_hist"]) == (b["exe_index"], b["have_hist"]) and np.array_equal(_bits(a["hist"]), _bits(b["hist"]))


def test_publisher_state_across_the_tick(hiplib):
    grid, res, org, S, E = ss.arena_plan_queries()
    Q = len(E)
    ppar = hiplib.default_plan_params()
    ppar.seed = SEED
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl = hiplib.Planner(h, Q, R)
    out = pl.plan(S, E, pp=ppar)
    ok = (out["plan_status"] == hiplib.PLAN_OK) & (out["winner"] >= 0)
    adopted = np.flatnonzero(ok)
    assert len(adopted) >= 3
    pl.adopt(np.arange(Q), np.arange(Q), t_start=0.0, pp=ppar)
    for q in range(Q):                                              # a plain adopt into an empty slot: index 0, no history
        st = pl.publisher_state(q)
        assert (st["exe_index"], st["have_hist"]) == (0, 0) and not st["hist"].any()
    pl.set_ctrl_history(adopted, -0.01 * np.ones(len(adopted)), 0.01 * (1 + adopted))
    before = [pl.executing(q) for q in range(Q)]
    # ---- the scene of tests/test_gpu_replan.py: the clock at 0.4 of the shortest one-segment plan, an obstacle on the path of plan a, one
    # on the goal of plan b (no path: the slot keeps its plan), the goal of plan c moved
    total = {int(q): float(before[q]["end_time"][before[q]["n_seg"] - 1]) for q in adopted}
    single = [q for q in total if before[q]["n_seg"] == 1] or list(total)
    c = min(single, key=lambda q: total[q])
    t_now, budget = 0.4 * total[c], 0.5
    others = [q for q in total if q != c and total[q] > t_now + 1.0]
    assert len(others) >= 2
    a, b = others[0], others[-1]
    after = grid.copy()
    xs, ys = org[0] + np.arange(grid.shape[1]) * res, org[1] + np.arange(grid.shape[0]) * res

    def drop(x, y, half):
        after[np.ix_((ys >= y - half) & (ys <= y + half), (xs >= x - half) & (xs <= x + half))] = 80
    na = int(out["piece_nums"][a, :out["n_seg"][a]].sum())
    mid = out["coeffs"][a, (2 * na) // 3, 0]
    drop(mid[0], mid[1], 0.4)
    drop(E[b, 0], E[b, 1], 2.0)
    goals = E.copy()
    goals[c, 0] += 0.6
    h.set_grid_map(after, res, org)
    # the publisher has run up to the tick's clock, and one tick far ahead: every occupied slot's index is 1 or more then
    pl.publish([t_now - 0.01, t_now, 1e6])
    pub0 = _pub_states(pl, Q)
    assert all(pub0[q]["exe_index"] >= 1 and pub0[q]["have_hist"] == 1 for q in adopted)
    tk = pl.tick(t_now, budget, end_states=goals, pp=ppar)
    stamp = t_now + budget
    new_ok = (tk["plan"]["plan_status"] == hiplib.PLAN_OK) & (tk["plan"]["winner"] >= 0)
    swapped = [int(s) for s, good in zip(tk["query_slot"], new_ok) if good]
    print("flagged:", tk["query_slot"].tolist(), "adopted by the tick:", swapped)
    assert len(swapped) >= 1 and b in tk["query_slot"].tolist() and b not in swapped
    pub1 = _pub_states(pl, Q)
    for q in range(Q):
        if q in swapped:                                           # exe_traj_index_ = 0 (:177), ctrl_state_hist_ kept
            assert pl.executing(q)["start_time"][0] == stamp
            assert pub1[q]["exe_index"] == 0 and pub1[q]["have_hist"] == 1 and np.array_equal(_bits(pub1[q]["hist"]), _bits(pub0[q]["hist"])), q
        else:                                                      # kept its plan, or empty: unchanged
            assert _same_pub(pub1[q], pub0[q]), q
    # ---- first plans through the tick: three slots emptied, every empty slot gets its ego state
    empt = [int(q) for q in adopted if q not in (a, b, c)][:3] or [int(a)]
    pl.clear(empt)
    ego = np.zeros((Q, 6))
    ego[:, :4] = S
    ego[:, 2] += 0.001 * np.arange(Q)                              # an angle of its own per slot
    was_empty = [q for q in range(Q) if pl.executing(q)["n_seg"] == 0]
    pub2 = _pub_states(pl, Q)
    tk2 = pl.tick(t_now, budget, end_states=goals, ego_states=ego, pp=ppar)
    ok2 = (tk2["plan"]["plan_status"] == hiplib.PLAN_OK) & (tk2["plan"]["winner"] >= 0)
    swapped2 = [int(s) for s, good in zip(tk2["query_slot"], ok2) if good]
    first = [q for q in swapped2 if q in was_empty]
    print("first plans:", first, "of the empty", was_empty, "replanned:", [q for q in swapped2 if q not in was_empty])
    assert len(first) >= 1
    pub3 = _pub_states(pl, Q)
    for q in range(Q):
        if q in first:                                             # seeded as the desired-state history is
            assert pub3[q]["exe_index"] == 0 and pub3[q]["have_hist"] == 1 and np.array_equal(pub3[q]["hist"], [stamp, ego[q, 2]]), q
        elif q in swapped2:
            assert pub3[q]["exe_index"] == 0 and pub3[q]["have_hist"] == pub2[q]["have_hist"]
            assert np.array_equal(_bits(pub3[q]["hist"]), _bits(pub2[q]["hist"])), q
        else:
            assert _same_pub(pub3[q], pub2[q]), q
    # ---- a following publish equals the oracle run on the table read back
    T = pp.Table(Q, *pl.padding())
    for q in range(Q):
        ex = pl.executing(q)
        M = ex["n_seg"]
        if M == 0:
            continue
        T.install(q, ex["singul"][:M], ex["piece_nums"][:M], ex["coeff_dt"][:M], ex["coeffs"], ex["start_time"][0])
        T.exe_index[q], T.have[q], T.hist[q] = pub3[q]["exe_index"], pub3[q]["have_hist"], pub3[q]["hist"]
    clocks = np.concatenate([stamp + 0.01 * np.arange(40), stamp + 2.0 + 1.5 * np.arange(12)])
    ref = pp.publish(T, clocks, order=2)
    got = pl.publish(clocks)
    assert ref["published"][:40, first].all()
    _same_rows(got, ref)
    _same_state(pl, T)
    pl.close()
    h.close()
