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


def test_default_search_params_match_the_library(hiplib):
    """pods.SearchParams.default() is dftpav_default_search_params, field for field (the library loads without a GPU)"""
    import ctypes as C
    c = SearchParams()
    hiplib.lib().dftpav_default_search_params(C.byref(c))
    d = SearchParams.default()
    for f, _ in SearchParams._fields_:
        assert getattr(c, f) == getattr(d, f), f
