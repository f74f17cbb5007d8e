"""The replan loop on the device: dftpav_replan_check on the crafted scene of dftpav_amd/replan_scenes.py, every field bit-equal
to oracle_replan in order 2 and the collision fields to dftpav_batch_validate; the executing table (install / adopt / clear /
executing); dftpav_replan_tick on adopted plans of search_scenes.arena_plan_queries with obstacles dropped and a goal moved,
against the oracle's flags and a separate dftpav_plan_queries call; a second identical tick; and the refusals."""
import ctypes as C

import numpy as np
import pytest

from dftpav_amd import replan_scenes as rs
from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import LayoutSpec
from oracle_replan import pyreplan as pr

pytestmark = pytest.mark.gpu

R = 2
SEED = 7
CHECK_KEYS = pr.INTS + ("desired", "start_state", "start_ctrl")
EXEC_KEYS = ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "duration", "start_time", "end_time", "end_state", "hist", "have_hist")


def _pp(hiplib):
    pp = hiplib.default_plan_params()
    pp.seed = SEED
    return pp


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in EXEC_KEYS)


def _chain(piece_nums, coeff_dt, t_start):
    rows, world = [], float(t_start)
    for N, dt in zip(piece_nums, coeff_dt):
        d = 0.0
        for _ in range(int(N)):
            d += float(dt)
        rows.append((d, world, world + d))
        world = world + d
    return np.array(rows).reshape(-1, 3)


def _install_scene(pl, scene):
    pad = rs.padded(scene)
    for k in range(len(pad["slots"])):          # one call per plan: each has its own t_start
        sl = slice(k, k + 1)
        pl.install(pad["slots"][sl], pad["n_seg"][sl], pad["singul"][sl], pad["piece_nums"][sl], pad["coeff_dt"][sl], pad["coeffs"][sl],
                   pad["end_states"][sl], t_start=pad["t_start"][k])
    for s, p in enumerate(scene["slots"]):
        if p is not None and p["hist"] is not None:
            pl.set_history([s], [p["hist"][0]], [p["hist"][1]])
    return pad


def _oracle_table(scene):
    T = pr.Table(rs.N_SLOTS)
    for s, p in enumerate(scene["slots"]):
        if p is None:
            continue
        T.install(s, p["singul"], p["piece_nums"], p["coeff_dt"], p["coeffs"], p["end_state"], p["t_start"])
        if p["hist"] is not None:
            T.set_history(s, *p["hist"])
    return T


def _validate_on_device(hiplib, h, singul, piece_nums, coeffs, coeff_dt, sample_dt=0.05):
    """dftpav_batch_validate of one plan uploaded as a batch of its layout (test hook dftpav_debug_batch_set_coeffs)"""
    lay = LayoutSpec([int(v) for v in piece_nums], [int(v) for v in singul], 4)
    bt = hiplib.Batch(h, lay, 1)
    fn = hiplib.lib().dftpav_debug_batch_set_coeffs
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    co = np.ascontiguousarray(coeffs[:lay.n_pieces], dtype=np.float64)
    dt = np.ascontiguousarray(coeff_dt[:lay.M], dtype=np.float64)
    assert fn(bt._b, co.ctypes.data_as(C.c_void_p), dt.ctypes.data_as(C.c_void_p)) == 0
    col, first = bt.validate(sample_dt=sample_dt, vertex_res=0.1)
    bt.close()
    return int(col[0]), int(first[0])


@pytest.fixture(scope="module")
def scene(oracle):
    return rs.crafted(oracle.minco_generate)


def test_check_equals_the_oracle_and_the_validation(hiplib, scene):
    h = hiplib.Handle()
    h.set_grid_map(scene["grid"], scene["resolution"], scene["origin"])
    pl = hiplib.Planner(h, rs.N_SLOTS, R)
    _install_scene(pl, scene)
    T = _oracle_table(scene)
    goals = np.array([p["end_state"] if p is not None else np.zeros(4) for p in scene["slots"]])
    goals2 = goals.copy()
    goals2[4, 1] += 1.0
    for kw in (dict(ego_states=scene["ego_states"]), dict(), dict(ego_states=scene["ego_states"], end_states=goals2)):
        got = pl.check(scene["t_now"], scene["budget"], **kw)
        ref = pr.replan_check(scene["grid"], scene["resolution"], scene["origin"], T, scene["t_now"], scene["budget"], order=2, **kw)
        for k in CHECK_KEYS:
            print(k, got[k].tolist() if got[k].ndim == 1 else "")
            assert np.array_equal(got[k], ref[k]), (k, sorted(kw))
    got = pl.check(scene["t_now"], scene["budget"], ego_states=scene["ego_states"])
    assert got["replan"].sum() >= 3 and got["collision"].sum() >= 1 and got["complete"].sum() == 1
    n = 0
    for s, p in enumerate(scene["slots"]):
        if p is None or got["complete"][s]:
            continue
        col, first = _validate_on_device(hiplib, h, p["singul"], p["piece_nums"], p["coeffs"], p["coeff_dt"])
        assert (got["collision"][s], got["first_sample"][s]) == (col, first), s
        n += 1
    assert n >= 8
    # the map of before the obstacle was dropped: no collision anywhere; and another clock
    h.set_grid_map(scene["grid_before"], scene["resolution"], scene["origin"])
    for t_now in (scene["t_now"], scene["t_now"] + 1.7, scene["t_now"] - 3.0):
        got = pl.check(t_now, scene["budget"], ego_states=scene["ego_states"])
        ref = pr.replan_check(scene["grid_before"], scene["resolution"], scene["origin"], T, t_now, scene["budget"], ego_states=scene["ego_states"])
        for k in CHECK_KEYS:
            assert np.array_equal(got[k], ref[k]), (k, t_now)
        assert got["collision"].sum() == 0
    ms = pl.replan_last_ms()
    print("check kernel ms:", ms[0])
    assert ms[0] > 0.0
    pl.close()
    h.close()


def test_check_refuses_an_outline_beyond_its_table_and_stays_usable(hiplib, scene):
    """A vertex_res that needs 4096 outline spacings or more is refused with E_UNSUPPORTED before anything is enqueued; the next
    check with the ordinary values returns exactly what it returned before the refused one."""
    h = hiplib.Handle()
    h.set_grid_map(scene["grid"], scene["resolution"], scene["origin"])
    pl = hiplib.Planner(h, rs.N_SLOTS, R)
    _install_scene(pl, scene)
    before = pl.check(scene["t_now"], scene["budget"], ego_states=scene["ego_states"])
    p = h.params
    too_fine = (max(p.veh_length, p.veh_width) + 1.0) / 5000.0
    assert hiplib.debug_validation_table(p, 0.05, too_fine, 4096)[0] == hiplib.E_UNSUPPORTED
    with pytest.raises(hiplib.DftpavError) as e:
        pl.check(scene["t_now"], scene["budget"], ego_states=scene["ego_states"], vertex_res=too_fine)
    assert e.value.code == hiplib.E_UNSUPPORTED
    after = pl.check(scene["t_now"], scene["budget"], ego_states=scene["ego_states"])
    for k in CHECK_KEYS:
        assert np.array_equal(before[k], after[k]), k
    assert before["collision"].sum() >= 1   # (the scene's check is not trivially empty)
    pl.close()
    h.close()


N_TABLE = 4096      # sample times the host tabulates (validation_table); later ones continue the running sum on the device
LONG_DT = 0.0009    # 4 s of plan: 4445 samples


@pytest.fixture(scope="module")
def long_plan(oracle):
    """One plan whose collision samples run past the table of sample times: 4 pieces of 1 s straight along +x at 2 m/s from the
    origin, and a wall across the map that the front of the vehicle (3.455 m ahead of the pose) only reaches at t ~ 3.82 s.  With
    the oracle's verdict (order 2) at LONG_DT, computed once."""
    co = np.zeros((4, 6, 2))
    co[:, 0, 0] = 2.0 * np.arange(4)
    co[:, 1, 0] = 2.0
    plan = dict(singul=[1], piece_nums=[4], coeff_dt=[1.0], coeffs=co, end_state=[8.0, 0.0, 0.0, 0.0], t_start=0.0, hist=None)
    grid = np.zeros((50, 120), dtype=np.uint8)       # 0.2 m cells from (-5, -5): x up to 19 m
    grid[:, 81] = 80                                 # x in [11.1, 11.3)
    scene = dict(slots=[plan], grid=grid, resolution=0.2, origin=(-5.0, -5.0))
    col, first = oracle.validate_trajectories(grid, 0.2, (-5.0, -5.0), co[None], [[1.0]], [4], [1], sample_dt=LONG_DT, order=2)
    scene["validate"] = (int(col[0]), int(first[0]))
    assert col[0] == 1 and first[0] > N_TABLE         # the verdict cannot come from the table alone
    return scene


def _samples_below(duration, dt):
    t, k = 0.0, 0
    while t < duration:                               # traj_server_ros.cpp:386
        t += dt
        k += 1
    return k


def test_validate_past_the_sample_table(hiplib, long_plan):
    """dftpav_batch_validate where a segment has more samples than the host tabulates: the count and the times past the table's end
    are the continued running sum, the first colliding sample lies there, equal to oracle.validate in order 2."""
    h = hiplib.Handle()
    h.set_grid_map(long_plan["grid"], long_plan["resolution"], long_plan["origin"])
    pl = hiplib.Planner(h, 1, R)
    _install_long(pl, long_plan)
    assert _samples_below(float(pl.executing(0)["duration"][0]), LONG_DT) > N_TABLE
    p = long_plan["slots"][0]
    got = _validate_on_device(hiplib, h, p["singul"], p["piece_nums"], p["coeffs"], np.array(p["coeff_dt"]), sample_dt=LONG_DT)
    print("validate:", got, "oracle:", long_plan["validate"])
    assert got == long_plan["validate"]
    pl.close()
    h.close()


def _install_long(pl, long_plan):
    pad = rs.padded(long_plan)
    pl.install(pad["slots"], pad["n_seg"], pad["singul"], pad["piece_nums"], pad["coeff_dt"], pad["coeffs"], pad["end_states"], t_start=0.0)


def test_check_past_the_sample_table(hiplib, long_plan):
    """dftpav_replan_check on the same plan in a slot of the table: every field equal to oracle_replan, the collision fields to
    the validation's."""
    h = hiplib.Handle()
    h.set_grid_map(long_plan["grid"], long_plan["resolution"], long_plan["origin"])
    pl = hiplib.Planner(h, 1, R)
    _install_long(pl, long_plan)
    assert _samples_below(float(pl.executing(0)["duration"][0]), LONG_DT) > N_TABLE
    p = long_plan["slots"][0]
    T = pr.Table(1)
    T.install(0, p["singul"], p["piece_nums"], p["coeff_dt"], p["coeffs"], p["end_state"], p["t_start"])
    got = pl.check(0.5, 0.5, check_dt=LONG_DT)
    ref = pr.replan_check(long_plan["grid"], long_plan["resolution"], long_plan["origin"], T, 0.5, 0.5, check_dt=LONG_DT, order=2)
    print("check:", int(got["collision"][0]), int(got["first_sample"][0]), "oracle_replan:", int(ref["collision"][0]), int(ref["first_sample"][0]))
    for k in CHECK_KEYS:
        assert np.array_equal(got[k], ref[k]), k
    assert (int(got["collision"][0]), int(got["first_sample"][0])) == long_plan["validate"]
    pl.close()
    h.close()


def test_install_executing_round_trip_and_refusals(hiplib, scene):
    h = hiplib.Handle()
    pl = hiplib.Planner(h, rs.N_SLOTS, R)
    assert pl.executing(3)["n_seg"] == 0 and pl.padding() == (0, 0)    # before anything was installed
    with pytest.raises(hiplib.DftpavError) as e:
        pl.check(0.0)                                          # no map, no table
    assert e.value.code == hiplib.E_INVALID
    pad = _install_scene(pl, scene)
    for k, s in enumerate(pad["slots"]):
        ex = pl.executing(int(s))
        p = scene["slots"][s]
        M = int(pad["n_seg"][k])
        for key in ("singul", "piece_nums", "coeff_dt", "coeffs"):
            assert np.array_equal(ex[key], pad[key][k]), (s, key)
        assert ex["n_seg"] == M and np.array_equal(ex["end_state"], pad["end_states"][k])
        rows = _chain(pad["piece_nums"][k, :M], pad["coeff_dt"][k, :M], pad["t_start"][k])
        assert np.array_equal(ex["duration"][:M], rows[:, 0]) and np.array_equal(ex["start_time"][:M], rows[:, 1])
        assert np.array_equal(ex["end_time"][:M], rows[:, 2]) and ex["start_time"][0] == pad["t_start"][k]
        assert not ex["duration"][M:].any() and not ex["start_time"][M:].any() and not ex["end_time"][M:].any()
        if p["hist"] is None:
            assert ex["have_hist"] == 0 and not ex["hist"].any()
        else:
            assert ex["have_hist"] == 1 and np.array_equal(ex["hist"], p["hist"])
    assert pl.executing(7)["n_seg"] == 0
    before = [pl.executing(s) for s in range(rs.N_SLOTS)]
    one = slice(0, 1)
    args = lambda **kw: {**dict(slots=pad["slots"][one], n_seg=pad["n_seg"][one], singul=pad["singul"][one], piece_nums=pad["piece_nums"][one],
                                coeff_dt=pad["coeff_dt"][one], coeffs=pad["coeffs"][one], end_states=pad["end_states"][one]), **kw}
    bad = [args(slots=[rs.N_SLOTS]), args(slots=[-1]), args(n_seg=[9]), args(n_seg=[0]),                     # slot out of range, n_seg > max_seg
           args(singul=pad["singul"][one, :4], piece_nums=pad["piece_nums"][one, :4], coeff_dt=pad["coeff_dt"][one, :4],
                coeffs=pad["coeffs"][one, :4 * 64]),                                                          # another padding: max_seg 4
           args(coeffs=pad["coeffs"][one, :8 * 32])]                                                          # max_pieces 32
    for a in bad:
        with pytest.raises(hiplib.DftpavError) as e:
            pl.install(**a)
        assert e.value.code == hiplib.E_INVALID
    two = slice(0, 2)
    with pytest.raises(hiplib.DftpavError) as e:                                                             # a slot named twice
        pl.install([4, 4], pad["n_seg"][two], pad["singul"][two], pad["piece_nums"][two], pad["coeff_dt"][two], pad["coeffs"][two], pad["end_states"][two])
    assert e.value.code == hiplib.E_INVALID
    for fn in (lambda: pl.set_history([7], [0.0], [0.0]), lambda: pl.clear([rs.N_SLOTS]), lambda: pl.executing(rs.N_SLOTS),
               lambda: pl.adopt([0], [0])):                                                                  # empty slot; out of range; no plan() to adopt from
        with pytest.raises(hiplib.DftpavError) as e:
            fn()
        assert e.value.code == hiplib.E_INVALID
    pp4 = _pp(hiplib)
    pp4.max_seg = 4
    h.set_grid_map(scene["grid"], scene["resolution"], scene["origin"])
    with pytest.raises(hiplib.DftpavError) as e:
        pl.tick(scene["t_now"], scene["budget"], pp=pp4)                                                     # the tick's plans would have another padding
    assert e.value.code == hiplib.E_INVALID
    assert all(_same(before[s], pl.executing(s)) for s in range(rs.N_SLOTS))                                  # a refused call changed nothing
    assert pl.padding() == (8, 64)
    # and the planner is still usable: the check gives the oracle's answer, clear empties
    got = pl.check(scene["t_now"], scene["budget"])
    ref = pr.replan_check(scene["grid"], scene["resolution"], scene["origin"], _oracle_table(scene), scene["t_now"], scene["budget"])
    for k in CHECK_KEYS:
        assert np.array_equal(got[k], ref[k]), k
    pl.clear([1, 3])
    for s in (1, 3):
        ex = pl.executing(s)
        assert ex["n_seg"] == 0 and not any(np.asarray(ex[k]).any() for k in EXEC_KEYS)
    got = pl.check(scene["t_now"], scene["budget"])
    assert got["occupied"][1] == 0 and got["occupied"][3] == 0 and got["occupied"][4] == 1 and got["replan"][3] == 0
    pl.close()
    h.close()


@pytest.fixture(scope="module")
def arena_scene():
    return ss.arena_plan_queries()


def _table_from_plan(out, goals, t_start, slots_of_query):
    Q = len(goals)
    T = pr.Table(Q)
    for q, s in slots_of_query.items():
        M = int(out["n_seg"][q])
        pn = out["piece_nums"][q, :M]
        T.install(s, out["singul"][q, :M], pn, out["coeff_dt"][q, :M], out["coeffs"][q, :int(pn.sum())], goals[q], t_start)
    return T


def test_adopt_and_tick(hiplib, arena_scene):
    grid, res, org, S, E = arena_scene
    Q = len(E)
    pp = _pp(hiplib)
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl = hiplib.Planner(h, Q, R)
    out = pl.plan(S, E, pp=pp)
    ok = (out["plan_status"] == hiplib.PLAN_OK) & (out["winner"] >= 0)
    assert ok.sum() >= 3 and (~ok).sum() >= 2
    # ---- adopt: query q into slot q
    T0 = 0.0
    ad = pl.adopt(np.arange(Q), np.arange(Q), t_start=T0, pp=pp)
    assert np.array_equal(ad, ok.astype(np.int32))
    for q in range(Q):
        ex = pl.executing(q)
        if not ok[q]:
            assert ex["n_seg"] == 0
            continue
        M = int(out["n_seg"][q])
        assert ex["n_seg"] == M and np.array_equal(ex["singul"], out["singul"][q]) and np.array_equal(ex["piece_nums"], out["piece_nums"][q])
        assert np.array_equal(ex["coeffs"], out["coeffs"][q]) and np.array_equal(ex["coeff_dt"], out["coeff_dt"][q])
        rows = _chain(out["piece_nums"][q, :M], out["coeff_dt"][q, :M], T0)
        assert np.array_equal(ex["duration"][:M], rows[:, 0]) and np.array_equal(ex["start_time"][:M], rows[:, 1]) and np.array_equal(ex["end_time"][:M], rows[:, 2])
        assert np.array_equal(ex["end_state"], E[q]) and ex["have_hist"] == 0
    # a shifted adoption: another start, another slot; the slot's former plan is replaced
    q0, q1 = np.flatnonzero(ok)[:2]
    pl.adopt([q0], [q1], t_start=2.5, pp=pp)
    ex = pl.executing(int(q1))
    assert np.array_equal(ex["coeffs"], out["coeffs"][q0]) and ex["start_time"][0] == 2.5 and np.array_equal(ex["end_state"], E[q0])
    pl.adopt([q1], [q1], t_start=T0, pp=pp)
    before = [pl.executing(q) for q in range(Q)]
    n_batches = pl.info()["n_batches"]
    # ---- the tick: the clock at 0.4 of the shortest plan of one gear segment; an obstacle on the path of one plan, one on the goal of
    # another (its replanning finds no path: the end is not free), and the goal of that shortest plan moved by 0.6 m
    adopted = np.flatnonzero(ok)
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
    mid = out["coeffs"][a, (2 * na) // 3, 0]            # where a piece two thirds down plan a starts
    drop(mid[0], mid[1], 0.4)
    drop(E[b, 0], E[b, 1], 2.0)
    goals = E.copy()
    goals[c, 0] += 0.6
    h.set_grid_map(after, res, org)
    slot_of = {int(q): int(q) for q in adopted}
    ref = pr.replan_check(after, res, org, _table_from_plan(out, E, T0, slot_of), t_now, budget, end_states=goals, order=2)
    flagged = np.flatnonzero(ref["replan"])
    print("flagged by the oracle:", flagged.tolist(), "a, b, c:", a, b, c, "t_now:", t_now)
    assert ref["collision"][a] == 1 and ref["collision"][b] == 1 and ref["is_near"][c] == 1 and ref["target_moved"][c] == 1
    assert ref["replan"][c] == 1 or ref["is_close_turnpoint"][c] == 1
    tk = pl.tick(t_now, budget, end_states=goals, pp=pp)
    for k in CHECK_KEYS:
        assert np.array_equal(tk["check"][k], ref[k]), k
    assert np.array_equal(tk["query_slot"], flagged)
    # the plans: a separate call with the oracle's start states and controls at t_now + budget, on a planner of its own
    pl2 = hiplib.Planner(h, Q, R)
    sep = pl2.plan(ref["start_state"][flagged], goals[flagged], start_ctrl=ref["start_ctrl"][flagged], pp=pp, t_now=t_now + budget)
    pl2.close()
    for k in sep:
        assert np.array_equal(tk["plan"][k], sep[k], equal_nan=True), k
    new_ok = (sep["plan_status"] == hiplib.PLAN_OK) & (sep["winner"] >= 0)
    print("plan_status of the tick:", sep["plan_status"].tolist())
    kb = int(np.flatnonzero(flagged == b)[0])
    assert sep["plan_status"][kb] == hiplib.PLAN_NO_PATH and new_ok.sum() >= 1
    stamp = t_now + budget
    for q in range(Q):
        ex = pl.executing(q)
        k = np.flatnonzero(flagged == q)
        if k.size == 0 or not new_ok[k[0]]:
            assert _same(ex, before[q]), q                  # not flagged, or its planning failed: the old plan, byte for byte
            continue
        k = int(k[0])
        M = int(sep["n_seg"][k])
        assert ex["n_seg"] == M and np.array_equal(ex["singul"], sep["singul"][k]) and np.array_equal(ex["piece_nums"], sep["piece_nums"][k])
        assert np.array_equal(ex["coeffs"], sep["coeffs"][k]) and np.array_equal(ex["coeff_dt"], sep["coeff_dt"][k])
        rows = _chain(sep["piece_nums"][k, :M], sep["coeff_dt"][k, :M], stamp)
        assert ex["start_time"][0] == stamp and np.array_equal(ex["start_time"][:M], rows[:, 1]) and np.array_equal(ex["end_time"][:M], rows[:, 2])
        assert np.array_equal(ex["duration"][:M], rows[:, 0]) and np.array_equal(ex["end_state"], goals[q])
        assert ex["have_hist"] == 1 and np.array_equal(ex["hist"], [stamp, ref["desired"][q, 3]])
    ms = pl.replan_last_ms()
    print("check ms, tick ms:", ms)
    # ---- a second identical tick on the restored table: the same bits, no new batch for layouts already met
    nb1 = pl.info()["n_batches"]
    pl.clear(np.arange(Q))
    for q in adopted:
        bq = before[q]
        pl.install([q], [bq["n_seg"]], bq["singul"][None], bq["piece_nums"][None], bq["coeff_dt"][None], bq["coeffs"][None], bq["end_state"][None],
                   t_start=bq["start_time"][0])
    assert all(_same(before[q], pl.executing(q)) for q in range(Q))
    tk2 = pl.tick(t_now, budget, end_states=goals, pp=pp)
    for k in CHECK_KEYS:
        assert np.array_equal(tk2["check"][k], tk["check"][k]), k
    assert np.array_equal(tk2["query_slot"], tk["query_slot"])
    for k in sep:
        assert np.array_equal(tk2["plan"][k], tk["plan"][k], equal_nan=True), k
    assert pl.info()["n_batches"] == nb1 >= n_batches
    # a tick in which nothing is flagged plans nothing
    h.set_grid_map(grid, res, org)
    pl.clear(np.arange(Q))
    pl.install([c], [before[c]["n_seg"]], before[c]["singul"][None], before[c]["piece_nums"][None], before[c]["coeff_dt"][None],
               before[c]["coeffs"][None], before[c]["end_state"][None], t_start=T0)
    tk3 = pl.tick(0.1, budget, pp=pp)
    assert tk3["query_slot"].size == 0 and tk3["check"]["replan"].sum() == 0 and _same(pl.executing(c), before[c])
    # and the empty slots get their first plans from their ego states: ego_states has a row for every slot, so every empty slot is
    # flagged (slot c alone holds a plan, and needs nothing at this clock); the oracle says which
    empty = [q for q in range(Q) if q != c]
    ego = np.zeros((Q, 6))
    ego[:, :4] = S
    first_goals = E.copy()
    first_goals[0] = E[int(adopted[0])]
    pl.clear([0])
    ref4 = pr.replan_check(grid, res, org, _table_from_plan(out, E, T0, {c: c}), 0.1, budget, end_states=first_goals, ego_states=ego, order=2)
    assert np.flatnonzero(ref4["replan"]).tolist() == empty
    tk4 = pl.tick(0.1, budget, end_states=first_goals, ego_states=ego, pp=pp)
    for k in CHECK_KEYS:
        assert np.array_equal(tk4["check"][k], ref4[k]), k
    assert tk4["query_slot"].tolist() == empty and np.array_equal(tk4["check"]["start_state"][empty], S[empty])
    print("plan_status of the first plans:", tk4["plan"]["plan_status"].tolist())
    assert tk4["plan"]["plan_status"][0] in (hiplib.PLAN_OK, hiplib.PLAN_NO_VALID_RESTART)
    assert _same(pl.executing(c), before[c])
    for k, q in enumerate(empty):
        ex = pl.executing(q)
        if tk4["plan"]["plan_status"][k] == hiplib.PLAN_OK and tk4["plan"]["winner"][k] >= 0:
            assert ex["n_seg"] >= 1 and ex["start_time"][0] == 0.1 + budget and ex["have_hist"] == 1 and np.array_equal(ex["hist"], [0.1 + budget, S[q, 2]])
            assert np.array_equal(ex["coeffs"], tk4["plan"]["coeffs"][k]) and np.array_equal(ex["end_state"], first_goals[q])
        else:
            assert ex["n_seg"] == 0, q                      # no winner: the slot stays empty
    pl.close()
    h.close()
