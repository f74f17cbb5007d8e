"""The CPU restatement of the 100 Hz publisher (oracle_publish/publish_oracle.cpp) against what already exists -- the state
read-out of oracle/ and a plain-Python restatement of the index walk and the filter chain -- on the crafted scene of
dftpav_amd/publish_scenes.py; the scene against its own conditions, by the oracle alone; and the refusals of the entry points
that need no device.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from dftpav_amd import publish_scenes as ps
from oracle_publish import pypublish as pp


@pytest.fixture(scope="module")
def scene(oracle):
    return ps.crafted(oracle.minco_generate)


def table_of(scene):
    T = pp.Table(ps.N_SLOTS)
    for s, p in enumerate(scene["slots"]):
        if p is None:
            continue
        T.install(s, p["singul"], p["piece_nums"], p["coeff_dt"], p["coeffs"], p["t_start"])
        if p["ctrl_hist"] is not None:
            T.set_ctrl_history(s, *p["ctrl_hist"])
    return T


@pytest.fixture(scope="module")
def run2(scene):
    T = table_of(scene)
    out = pp.publish(T, scene["clocks"], order=2)
    out["final"] = T
    return out


def _times(p):
    """the chain of traj_container.hpp:58-73 in Python floats: per segment duration, start, end"""
    rows, world = [], p["t_start"]
    for N, dt in zip(p["piece_nums"], p["coeff_dt"]):
        d = 0.0
        for _ in range(int(N)):
            d += float(dt)
        rows.append((d, world, world + d))
        world = world + d
    return rows


def _normalize(a):
    tmp = a
    tmp -= float((a >= math.pi) * 2) * math.pi
    tmp += float((a < -math.pi) * 2) * math.pi
    return tmp


def test_index_and_codes_equal_a_python_restatement(scene, run2):
    """the index walk (traj_server_ros.cpp:248-252) and the filter chain (:335-356, :257-258) in plain Python, fed with the
    angle and velocity GetState gave"""
    clocks = scene["clocks"]
    max_rate = float.fromhex("0x1.fffffffffffffp-1") / 2.85 * 0.1          # tan(M_PI / 4), correctly rounded (and what glibc returns)
    for s, p in enumerate(scene["slots"]):
        if p is None:
            assert not run2["published"][:, s].any() and (run2["index"][:, s] == -1).all()
            continue
        rows = _times(p)
        last = len(rows) - 1
        exe, hist = 0, p["ctrl_hist"]
        for k, t in enumerate(clocks):
            t = float(t)
            want_idx, want_code, want_angle = -1, 0, 0.0
            if exe <= last and not rows[exe][0] < 1e-5:
                if rows[exe][2] <= t:
                    exe += 1
                if exe <= last:
                    want_idx = exe
                    assert run2["t_local"][k, s] == t - rows[exe][1]
                    angle, vel = float(run2["raw_angle"][k, s]), float(run2["states"][k, s, 5])
                    want_code = 1
                    if hist is not None and abs(vel) < 0.1 and abs(_normalize(angle - hist[1])) > max_rate * (t - hist[0]):
                        angle, want_code = hist[1], 2
                    hist, want_angle = (t, angle), angle
            got = (int(run2["index"][k, s]), int(run2["published"][k, s]))
            assert got == (want_idx, want_code), (s, k, got)
            assert run2["states"][k, s, 3] == want_angle and run2["states"][k, s, 0] == (t if want_code else 0.0)
            if not want_code:
                assert not run2["states"][k, s].any()
        F = run2["final"]
        assert F.exe_index[s] == exe and F.have[s] == int(hist is not None)
        if hist is not None:
            assert tuple(F.hist[s]) == hist


def test_unfiltered_rows_equal_the_state_oracle(oracle, scene, run2):
    """on ticks with code 1 the row is oracle.sample_states on that segment as a one-segment trajectory at that local time (one
    sample, the filter off; sample_states publishes nothing before 0 or at / past the segment's end: the clamped and the negative
    times are held to it on the piece alone, given a duration that contains the local time)"""
    n_in = n_clamped = 0
    seen = set()
    for s, p in enumerate(scene["slots"]):
        if p is None:
            continue
        rows = _times(p)
        for k in np.flatnonzero(run2["published"][:, s] == 1):
            i, t = int(run2["index"][k, s]), float(run2["t_local"][k, s])
            if (s, i, t) in seen:
                continue
            seen.add((s, i, t))
            p0, N = int(p["piece_nums"][:i].sum()), int(p["piece_nums"][i])
            row = run2["states"][k, s]
            assert row[0] == scene["clocks"][k]
            if 0.0 <= t < rows[i][0]:
                st, nv = oracle.sample_states(p["coeffs"][None, p0:p0 + N], p["coeff_dt"][None, i:i + 1], [N], [int(p["singul"][i])], t0=t,
                                              sample_dt=1.0, n_samples=1, filter_singularity=False, order=2)
                n_in += 1
            elif t >= rows[i][0]:
                tt = rows[i][0]                       # GetState clamps to the total duration, locatePieceIdx lands in the last piece
                for _ in range(N - 1):
                    tt -= float(p["coeff_dt"][i])
                dt2 = np.array([[2.0 * float(p["coeff_dt"][i])]])
                st, nv = oracle.sample_states(p["coeffs"][None, p0 + N - 1:p0 + N], dt2, [1], [int(p["singul"][i])], t0=tt, sample_dt=1.0,
                                              n_samples=1, filter_singularity=False, order=2)
                n_clamped += 1
            else:
                continue                              # before the plan's start: test_scene_meets_its_conditions
            assert nv[0] == 1
            assert np.array_equal(row[1:], st[0, 0, 1:]), (s, k)
    assert n_in >= 500 and n_clamped >= 1


def _runs(mask):
    """lengths of the runs of consecutive True"""
    out, n = [], 0
    for m in list(mask) + [False]:
        if m:
            n += 1
        elif n:
            out.append(n)
            n = 0
    return out


def test_scene_meets_its_conditions(scene, run2):
    """every case the scene is there for occurs, by the oracle alone (order 2)"""
    o, want, clocks = run2, scene["expect"], scene["clocks"]
    slot = {case: s for s, case in want.items()}
    assert len(slot) == ps.N_SLOTS == len(want)
    K = len(clocks)
    tick = lambda t: int(np.flatnonzero(clocks == t)[0])
    assert K <= 300 and K > ps.CHUNK + 1 and 0 < scene["split"] < K and scene["split"] % ps.CHUNK != 0
    s = slot["inside_segment"]
    rows = _times(scene["slots"][s])
    assert (o["published"][:, s] == 1).all() and (o["index"][:, s] == 0).all()
    assert (o["t_local"][:, s] > 0.0).all() and (o["t_local"][:, s] < rows[0][0]).all()
    s = slot["end_time_exact"]
    rows = _times(scene["slots"][s])
    k = tick(rows[0][2])                                   # a clock exactly on the end of segment 0: the <= of :248
    assert o["index"][k - 1, s] == 0 and o["index"][k, s] == 1 and o["t_local"][k, s] == 0.0 and o["published"][k, s] >= 1
    s = slot["one_step_per_tick"]
    rows = _times(scene["slots"][s])
    assert len(rows) == 3
    k = next(k for k in range(1, K) if clocks[k] - clocks[k - 1] > rows[1][0])
    assert clocks[k - 1] < rows[0][2] and clocks[k] >= rows[1][2]          # from inside segment 0 to past the end of segment 1
    assert o["index"][k - 1, s] == 0 and o["index"][k, s] == 1 and o["index"][k + 1, s] == 2
    assert o["t_local"][k, s] > rows[1][0]                                 # GetState clamps: the end of the middle segment
    p = scene["slots"][s]
    c = p["coeffs"][int(p["piece_nums"][:2].sum()) - 1]
    end = sum(c[j] * float(p["coeff_dt"][1]) ** j for j in range(6))
    assert np.allclose(o["states"][k, s, 1:3], end, rtol=0, atol=1e-9) and o["states"][k, s, 5] < 0.0
    s = slot["before_start"]
    before = clocks < scene["slots"][s]["t_start"]
    assert before.sum() > ps.CHUNK and (o["published"][before, s] >= 1).all() and (o["t_local"][before, s] < 0.0).all()
    assert (o["index"][before, s] == 0).all() and np.isfinite(o["states"][before, s]).all()
    s = slot["reverse_segment"]
    rev = o["index"][:, s] == 1
    assert scene["slots"][s]["singul"][1] == -1 and rev.sum() > ps.CHUNK and (o["states"][rev, s, 5] < 0.0).all()
    s = slot["standstill_on_start"]
    k = tick(scene["slots"][s]["t_start"])
    row = o["states"][k, s]
    assert o["t_local"][k, s] == 0.0 and o["raw_angle"][k, s] == 0.0 and row[5] == 0.0             # atan2(0, 0); |v| < 1e-6
    assert row[4] == 0.0 and row[6] == 0.0 and row[7] == 0.0
    assert o["published"][k, s] == 2 and row[3] == o["states"][k - 1, s, 3] and abs(row[3]) == math.pi   # the history angle restored
    s = slot["gear_shift_run"]
    code2 = o["published"][:, s] == 2
    hist_angle = scene["slots"][s]["ctrl_hist"][1]
    assert max(_runs(code2)) >= 2 and code2[ps.CHUNK - 1] and code2[ps.CHUNK] and code2[0]        # straddles the chunk boundary
    assert code2[scene["split"] - 1] and code2[scene["split"]]                                    # and the cut of the split call
    assert (o["states"][code2, s, 3] == hist_angle).all() and (np.abs(o["states"][code2, s, 5]) < 0.1).all()
    assert (np.abs(o["raw_angle"][code2, s] - hist_angle) > 0.29).all()
    k = tick(ps.GEAR_SHIFT)
    assert o["index"][k - 1, s] == 0 and o["index"][k, s] == 1 and o["states"][k - 1, s, 5] > 0.0 > o["states"][k, s, 5]
    assert np.allclose(np.abs(o["states"][k, s, 5]), 0.05, rtol=0, atol=1e-9)
    assert (o["published"][:, s] == 1).sum() >= 5                                                  # and the run ends
    s = slot["completes_mid_call"]
    rows = _times(scene["slots"][s])
    k = tick(rows[-1][2])
    assert (o["published"][:k, s] >= 1).all() and not o["published"][k:, s].any() and not o["states"][k:, s].any()
    assert (clocks[k:] < rows[-1][2]).any()                # a later clock inside the plan again: the slot stays silent
    assert run2["final"].exe_index[s] == len(rows)
    s = slot["empty"]
    assert scene["slots"][s] is None and not o["published"][:, s].any() and not o["states"][:, s].any()
    assert run2["final"].have[s] == 0 and run2["final"].exe_index[s] == 0
    s = slot["no_history"]
    assert scene["slots"][s]["ctrl_hist"] is None and o["published"][0, s] == 1 and o["states"][0, s, 3] == o["raw_angle"][0, s]
    T = table_of(scene)
    pp.publish(T, scene["clocks"][:1])
    assert T.have[s] == 1 and tuple(T.hist[s]) == (clocks[0], o["states"][0, s, 3])
    # a clock that goes back is among them
    assert (np.diff(clocks) < 0.0).any()


def test_orders_agree_on_the_discrete_outputs(scene, run2):
    T = table_of(scene)
    out0 = pp.publish(T, scene["clocks"], order=0)
    assert np.array_equal(out0["published"], run2["published"]) and np.array_equal(out0["index"], run2["index"])
    assert np.array_equal(T.exe_index, run2["final"].exe_index) and np.array_equal(T.have, run2["final"].have)
    assert np.array_equal(out0["t_local"], run2["t_local"])
    assert np.allclose(out0["states"], run2["states"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("cut", ["split", 1, ps.CHUNK, ps.CHUNK + 1])
def test_two_consecutive_calls_give_the_rows_of_one(scene, run2, cut):
    cut = scene["split"] if cut == "split" else cut
    T = table_of(scene)
    a = pp.publish(T, scene["clocks"][:cut])
    b = pp.publish(T, scene["clocks"][cut:])
    for k in ("states", "published", "index", "t_local", "raw_angle"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), run2[k]), k
    F = run2["final"]
    assert np.array_equal(T.exe_index, F.exe_index) and np.array_equal(T.hist, F.hist) and np.array_equal(T.have, F.have)


def test_entry_points_refuse_without_a_planner(hiplib):
    """the C-ABI's refusals that need no device: a NULL planner"""
    L = hiplib.lib()
    t = (C.c_double * 2)(0.0, 0.01)
    one = (C.c_int * 1)(0)
    L.dftpav_planner_publish.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dftpav_planner_publisher_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dftpav_planner_set_ctrl_history.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dftpav_publish_last_ms.argtypes = [C.c_void_p, C.c_void_p]
    ms = C.c_float(1.0)
    assert L.dftpav_planner_publish(None, 2, t, None, None) == hiplib.E_INVALID
    assert L.dftpav_planner_publisher_state(None, 0, None, None, None) == hiplib.E_INVALID
    assert L.dftpav_planner_set_ctrl_history(None, 1, one, t, t) == hiplib.E_INVALID
    assert L.dftpav_publish_last_ms(None, C.byref(ms)) == hiplib.E_INVALID
    for name in ("publish", "publisher_state", "set_ctrl_history", "publish_last_ms"):
        assert callable(getattr(hiplib.Planner, name))
    assert ps.CHUNK == 256
