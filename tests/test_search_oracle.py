"""The CPU restatement of the hybrid A* front end (oracle_search/kino_search_oracle.cpp): KinoAstar::search + getKinoPath's
2D retry + getKinoNode up to SampleTraj, on the scenes of dftpav_amd/search_scenes.py.  Each test names the oracle order it
uses (0: libm, 1: the kernel's correctly rounded functions replayed on the host, 2: binary128-rounded).

Orders 0, 1 and 2 agree on every discrete output (status, shot_success, used_3d, budget_hit, iters, nodes_used, n_nodes,
path_len, the nodes' steer / arc / singul) for every scene here, the default-arena goals included
(test_orders_agree_on_the_discrete_outputs); order 1 equals order 2 bit for bit in every field."""
import numpy as np
import pytest

from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import SearchParams
from oracle_search import pysearch as ps

import search_cases as sc

REACH_END, NO_PATH = 2, 3
DISCRETE = ("status", "shot_success", "used_3d", "budget_hit", "iters", "nodes_used", "n_nodes", "path_len")


def _run(scene, sp=None, order=2, **kw):
    name, g, res, org, st, en = scene
    r = ps.kino_search(g, res, org, st[None], en[None], sp=sp, order=order, **kw)
    return {k: (v[0] if v.ndim > 1 else int(v[0])) for k, v in r.items()}


def _collides(g, res, org, pose, sp):
    """the search's own collision test of one pose: a search from it to itself (early exit when occupied)"""
    r = ps.kino_search(g, res, org, np.array([[pose[0], pose[1], pose[2], 0.0]]), np.array([[pose[0] + 200.0, 0.0, 0.0, 0.0]]),
                       sp=sp.copy(max_iters=0, retry_2d=0), order=2)
    return r["nodes_used"][0] == 0


def test_heap_matches_std_priority_queue():
    """kino_heap.h against std::priority_queue with in-place key changes and many ties, >= 1e5 operations per seed"""
    for seed in (1, 2, 3):
        assert ps.heap_selftest(seed, 150000) == -1


def test_empty_map_shot_from_the_start():
    """order 2: a start at rest on an empty map: the shot from the start node succeeds before any pop"""
    r = _run(ss.empty())
    assert r["status"] == REACH_END and r["shot_success"] == 1 and r["iters"] == 0 and r["nodes_used"] == 1
    assert r["n_nodes"] == 1 and r["used_3d"] == 1 and r["budget_hit"] == 0
    _, _, _, _, st, en = ss.empty()
    path = r["paths"][:r["path_len"]]
    assert np.array_equal(path[0], st[:3]) and np.array_equal(path[-1], en[:3])
    steps = np.hypot(*np.diff(path[:, :2], axis=0).T)
    assert (steps < 0.2 + 1e-9).all() and r["path_len"] > 20         # [start] + shot samples every checkl + goal


def test_moving_start_expands_with_its_own_gear_first():
    """order 2: a start moving forwards expands first with the arcs map_resl and 2 map_resl only (kino_astar.cpp:143-151)"""
    sp = SearchParams.default()
    r = _run(ss.moving_start())
    assert r["status"] == REACH_END and r["iters"] >= 1 and r["n_nodes"] >= 2
    first = r["nodes"][1]
    assert first[4] in (sp.map_resl, sp.map_resl + sp.map_resl) and first[5] == 1.0
    assert r["nodes"][0][5] == 1.0                                     # getSingularity(1.5)


def test_reverse_scene_has_a_reverse_node():
    """order 2: rolling backwards towards a goal behind: the first expansion is reverse only, a node with singul -1"""
    r = _run(ss.reverse())
    assert r["status"] == REACH_END
    nodes = r["nodes"][:r["n_nodes"]]
    assert (nodes[1:, 5] == -1.0).any() and nodes[1, 4] < 0.0


@pytest.mark.parametrize("scene", [ss.wall_gap(), ss.moving_start(), ss.reverse()], ids=lambda s: s[0])
def test_nodes_are_state_transits_and_the_path_is_free(scene):
    """order 2: every returned node is stateTransit(parent, input) bit for bit, and every SampleTraj pose up to the shot is free"""
    name, g, res, org, st, en = scene
    sp = SearchParams.default()
    r = _run(scene)
    assert r["status"] == REACH_END
    nodes = r["nodes"][:r["n_nodes"]]
    for j in range(1, len(nodes)):
        want = ps.state_transit(nodes[j - 1][:3], nodes[j][3:5], sp.wheel_base, order=2)
        assert np.array_equal(nodes[j][:3], want), j
    n_rough = 1 + (len(nodes) - 1) * sp.check_num
    for pose in r["paths"][:n_rough]:
        assert not _collides(g, res, org, pose, sp)


def test_wall_gap_needs_a_search():
    """order 2: the wall blocks the direct shot: the answer is a searched path that ends on a free shot"""
    r = _run(ss.wall_gap())
    assert r["status"] == REACH_END and r["shot_success"] == 1 and r["iters"] > 10 and r["n_nodes"] > 3


@pytest.mark.parametrize("scene", [ss.occupied_start(), ss.occupied_goal()], ids=lambda s: s[0])
def test_occupied_start_or_goal_is_no_path(scene):
    """order 2: kino_astar.cpp:43-52, in the 3D search and in the 2D retry"""
    r = _run(scene)
    assert r["status"] == NO_PATH and r["iters"] == 0 and r["nodes_used"] == 0 and r["used_3d"] == 0
    r = _run(scene, sp=SearchParams.default().copy(retry_2d=0))
    assert r["status"] == NO_PATH and r["iters"] == 0 and r["used_3d"] == 1


def test_enclosed_start_exhausts_the_open_set():
    """order 2: NO_PATH from the 3D search (no retry) and from the 2D retry, without the budget"""
    r3 = _run(ss.enclosed(), sp=SearchParams.default().copy(retry_2d=0))
    assert r3["status"] == NO_PATH and r3["used_3d"] == 1 and r3["budget_hit"] == 0 and r3["iters"] > 0
    r2 = _run(ss.enclosed())
    assert r2["status"] == NO_PATH and r2["used_3d"] == 0 and r2["budget_hit"] == 0 and r2["iters"] > 0
    assert r2["iters"] == r2["nodes_used"]                             # every node was popped


def test_budget():
    """order 2: max_iters stands for the wall clock: the time-out branch (kino_astar.cpp:115-132)"""
    sp = SearchParams.default().copy(max_iters=5, retry_2d=0)
    r = _run(ss.wall_gap(), sp=sp)
    assert r["status"] == REACH_END and r["budget_hit"] == 1 and r["shot_success"] == 0 and r["iters"] == 5
    _, _, _, _, st, en = ss.wall_gap()
    assert r["path_len"] == 1 + (r["n_nodes"] - 1) * sp.check_num     # no shot, no goal appended
    assert not np.array_equal(r["paths"][r["path_len"] - 1], en[:3])
    r = _run(ss.wall_gap(), sp=sp.copy(max_iters=0))
    assert r["status"] == NO_PATH and r["budget_hit"] == 1 and r["iters"] == 0


def test_node_pool_exhaustion():
    """order 2: use_node_num_ == allocate_num is NO_PATH ("run out of memory", kino_astar.cpp:270-274)"""
    r = _run(ss.wall_gap(), sp=SearchParams.default().copy(allocate_num=40, retry_2d=0))
    assert r["status"] == NO_PATH and r["nodes_used"] == 40 and r["budget_hit"] == 0


def test_default_arena_goals_need_a_search():
    """order 2: the goals of search_scenes.ARENA_GOALS are free, their direct shot from the ego start collides (the answer
    took pops), and the search reaches them"""
    grid, res, org, start, goals = ss.arena()
    r = ps.kino_search(grid, res, org, np.repeat(start[None], len(goals), 0), goals, order=2, nthreads=4)
    assert (r["status"] == REACH_END).all() and (r["iters"] > 0).all() and (r["shot_success"] == 1).all()
    assert not r["budget_hit"].any()


def test_orders_agree_on_the_discrete_outputs():
    """orders 0, 1, 2 on every scene: the discrete outputs agree; order 1 == order 2 in every field"""
    scenes = ss.small_scenes()
    grid, res, org, start, goals = ss.arena()
    runs = [(s[1], s[2], s[3], s[4][None], s[5][None]) for s in scenes]
    runs.append((grid, res, org, np.repeat(start[None], len(goals), 0), goals))
    for g, rs_, o, st, en in runs:
        out = [ps.kino_search(g, rs_, o, st, en, order=k, nthreads=4) for k in (0, 1, 2)]
        for k in DISCRETE:
            assert np.array_equal(out[0][k], out[2][k]) and np.array_equal(out[1][k], out[2][k]), k
        assert np.array_equal(out[0]["nodes"][..., 3:], out[2]["nodes"][..., 3:])
        for k in out[2]:
            assert np.array_equal(out[1][k], out[2][k]), k


# ---- the cases of search_cases.py: each meets the condition it is there for (the device runs them in test_gpu_search.py) ----------

def _q(case, q=0):
    """the discrete outputs of query q of a case, the changed parameters, the whole result"""
    r = sc.oracle(case)
    return {k: int(r[k][q]) for k in DISCRETE}, sc.CASES[case][1], r


def _others_as_default(r, last=11):
    """every arena goal but `last` answers as in the default run, in every field"""
    d = sc.oracle("default-arena")
    keep = np.arange(len(d["status"])) != last
    for k in d:
        assert np.array_equal(r[k][keep], d[k][keep]), k


@pytest.mark.parametrize("case", [c for c in sc.BUDGET if "wall-gap" in c])
def test_case_budget_wall_gap(case):
    """order 2: the time-out branch at iteration 0 (the start node is terminal: NO_PATH, retried in 2D), 1, 5 and 30"""
    o, ch, r = _q(case)
    m = ch["max_iters"]
    assert o["budget_hit"] == 1 and o["iters"] == m and o["shot_success"] == 0
    if m == 0:
        assert o["status"] == NO_PATH and o["nodes_used"] == 1 and o["used_3d"] == 1 - ch["retry_2d"]
        assert o["n_nodes"] == 0 and o["path_len"] == 0
    else:
        assert o["status"] == REACH_END and o["used_3d"] == 1
        assert o["path_len"] == 1 + (o["n_nodes"] - 1) * 5 == {1: 6, 5: 21, 30: 26}[m]   # no shot, no goal appended
        assert not np.array_equal(r["paths"][0, o["path_len"] - 1], ss.wall_gap()[5][:3])


def test_case_budget_arena():
    """order 2, max_iters = 50: goal 11 (84 iterations at the default) ends on the budget, the others as before: a mixed launch"""
    o, ch, r = _q("budget-arena-max_iters=50", 11)
    assert o["status"] == REACH_END and o["budget_hit"] == 1 and o["shot_success"] == 0 and o["iters"] == 50
    assert o["path_len"] == 1 + (o["n_nodes"] - 1) * 5
    _others_as_default(r)
    assert not r["budget_hit"][:11].any() and (r["shot_success"][:11] == 1).all()


@pytest.mark.parametrize("case", [c for c in sc.POOL if "wall-gap" in c])
def test_case_pool_wall_gap(case):
    """order 2: the pool runs out in the middle of an expansion, in 3D and again in the 2D retry (allocate_num = 40, 64: tables of
    128 slots a third and a half full); with 200 nodes (a table of 512) the 2D retry reaches the goal over the same pool"""
    o, ch, r = _q(case)
    a = ch["allocate_num"]
    if a == 200 and ch["retry_2d"]:
        assert o["status"] == REACH_END and o["used_3d"] == 0 and o["nodes_used"] == 134 and o["path_len"] == 84
        assert o["shot_success"] == 1
        first = _q(case.replace("retry_2d=1", "retry_2d=0"))[0]
        assert first["status"] == NO_PATH and first["nodes_used"] == 200          # the 3D pass that came before
    else:
        assert o["status"] == NO_PATH and o["nodes_used"] == a and o["used_3d"] == 1 - ch["retry_2d"]
        assert o["n_nodes"] == 0 and o["path_len"] == 0
    assert o["budget_hit"] == 0


@pytest.mark.parametrize("case", [c for c in sc.POOL if "arena" in c])
def test_case_pool_arena(case):
    """order 2, allocate_num = 300 (a table of 1024): goal 11 (448 nodes at the default) runs out of nodes in 3D, the others answer
    as before; the 2D retry reaches it"""
    o, ch, r = _q(case, 11)
    if ch["retry_2d"]:
        assert o["status"] == REACH_END and o["used_3d"] == 0 and o["nodes_used"] == 143 and o["shot_success"] == 1
    else:
        assert o["status"] == NO_PATH and o["used_3d"] == 1 and o["nodes_used"] == 300
        assert o["n_nodes"] == 0 and o["path_len"] == 0 and not r["nodes"][11].any() and not r["paths"][11].any()
    _others_as_default(r)
    assert (r["status"][:11] == REACH_END).all() and (r["nodes_used"][:11] < 300).all()


@pytest.mark.parametrize("case", list(sc.BOUNDS))
def test_case_bounds(case):
    """order 2: a search space that ends close to the scene: the goal is reached, but expansions were rejected on the way (the
    iteration count is not the default run's)"""
    o, ch, r = _q(case)
    d = _q("default-wall-gap")[0]
    assert o["status"] == REACH_END and o["shot_success"] == 1 and d["iters"] == 53
    assert o["iters"] == {30.0: 50, 26.0: 55, 24.2: 54}[ch["map_size_x"]] != d["iters"]


@pytest.mark.parametrize("case", list(sc.PARAMS))
def test_case_parameters(case):
    """order 2: one search parameter off its default: the goal is reached, by another search than the default's"""
    (name, value), = sc.CASES[case][1].items()
    base = "default-arena" if sc.CASES[case][0] == "arena" else "default-wall-gap"
    r, d = sc.oracle(case), sc.oracle(base)
    assert getattr(SearchParams.default(), name) != value
    assert (r["status"] == REACH_END).all() and (r["shot_success"] == 1).all() and not r["budget_hit"].any()
    if name == "traj_steer_change_penalty":
        assert not np.array_equal(r["paths"], d["paths"]) and not np.array_equal(r["nodes"][..., 3], d["nodes"][..., 3])
    else:
        assert not all(np.array_equal(r[k], d[k]) for k in r)
    if case == "lambda_heu=1.0":
        assert r["nodes_used"][0] == 1737


@pytest.mark.parametrize("case", list(sc.YAWS))
def test_case_yaws(case):
    """order 2: start and goal yaws outside [-pi, pi), wrapped once as the reference wraps them: the goal is reached"""
    o, ch, r = _q(case)
    yaw = sc.CASES[case][2]
    assert o["status"] == REACH_END and o["shot_success"] == 1 and 400 <= o["nodes_used"] <= 2110
    assert r["nodes"][0, 0, 2] == yaw                                   # the node keeps the yaw as given
    once = yaw - 2 * np.pi * (yaw >= np.pi) + 2 * np.pi * (yaw < -np.pi)
    assert r["paths"][0, 0, 2] == once and (-np.pi <= once < np.pi) == (abs(yaw) < 3 * np.pi)


def test_case_maze():
    """order 2: search_scenes.maze() at MAZE_MAX_ITERS ends on the budget with 5337 nodes, a heap thousands deep"""
    o, ch, r = _q("maze")
    assert ch["max_iters"] == ss.MAZE_MAX_ITERS == 2000
    assert o["status"] == REACH_END and o["budget_hit"] == 1 and o["shot_success"] == 0 and o["iters"] == 2000
    assert o["nodes_used"] == 5337 and o["path_len"] == 1 + (o["n_nodes"] - 1) * 5 and o["n_nodes"] > 1
    assert "maze" not in [s[0] for s in ss.small_scenes()]
    name, g, res, org, st, en = ss.maze()
    less = ps.kino_search(g, res, org, st[None], en[None], sp=SearchParams.default().copy(max_iters=1500), order=2)
    assert less["nodes_used"][0] < 5000                                 # 2000 is the smallest multiple of 500 that gives 5000


def test_search_slots(hiplib):
    """dftpav_debug_search_slots, the workspace arithmetic search_setup uses (no device): 100 bytes of pool, heap and path list per
    node and 4 per table slot (the power of two >= 2 allocate_num), as many queries in flight as 6 GiB hold"""
    import ctypes as C
    fn = hiplib.lib().dftpav_debug_search_slots
    fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    fn.restype = C.c_int

    def slots(n, **kw):
        sp = SearchParams.default().copy(**kw)
        s, b = C.c_int(-1), C.c_size_t(0)
        assert fn(C.byref(sp), n, C.byref(s), C.byref(b)) == hiplib.OK
        return s.value, b.value

    s, per = slots(100000)
    assert per == 100 * 100000 + 4 * 262144 + 256 and s == ((6 << 30) - 6 * 256) // per == 583 > 400
    assert slots(12) == (12, per) and slots(583)[0] == 583 and slots(584)[0] == 583
    s, per = slots(32, allocate_num=4194304)
    assert per == 100 * 4194304 + 4 * 8388608 + 256 and s == 14 < 32
    assert slots(1, allocate_num=40) == (1, 100 * 40 + 4 * 128 + 256) and slots(1, allocate_num=64)[1] == 100 * 64 + 4 * 128 + 256
    assert slots(1, allocate_num=65)[1] == 100 * 65 + 4 * 256 + 256
    assert slots(5, allocate_num=1 << 28) == (1, 100 * (1 << 28) + 4 * (1 << 29) + 256)   # more than 6 GiB per query: one slot
    sp = SearchParams.default()
    assert fn(C.byref(sp), 0, None, None) == hiplib.E_INVALID and fn(None, 1, None, None) == hiplib.E_INVALID
    assert fn(C.byref(sp.copy(allocate_num=1)), 1, None, None) == hiplib.E_INVALID
    assert fn(C.byref(sp), 1, None, None) == hiplib.OK


def test_default_search_params_match_the_library(hiplib):
    """pods.SearchParams.default() is dftpav_default_search_params, field for field (the library loads without a GPU)"""
    import ctypes as C
    c = SearchParams()
    hiplib.lib().dftpav_default_search_params(C.byref(c))
    d = SearchParams.default()
    for f, _ in SearchParams._fields_:
        assert getattr(c, f) == getattr(d, f), f
