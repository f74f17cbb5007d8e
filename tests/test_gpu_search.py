"""dftpav_kino_search on the device against the CPU restatement in order 2 (oracle_search/), bit for bit in every output field,
on a batch of every scene of dftpav_amd/search_scenes.py; on the cases of search_cases.py, the branches that the default parameters
and searches that end well never take; with more queries than workspace slots; then the default-arena chain with a real search in
front: kino_search -> frontend_resample -> corridor_from_states -> reference-order solve -> validate."""
import numpy as np
import pytest

from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import FrontendParams, LayoutSpec, SearchParams
from dftpav_amd.scenarios import Scenario
from oracle_search import pysearch as ps

import search_cases as sc

pytestmark = pytest.mark.gpu


def _arena_batch(copies=4):
    """the default-arena goals from the ego start, `copies` times over (the small scenes run on maps of their own)"""
    grid, res, org, start, goals = ss.arena()
    en = np.concatenate([goals] * copies)
    st = np.repeat(start[None], len(en), 0)
    return grid, res, org, st, en


def _compare(r, o):
    for k in o:
        assert np.array_equal(r[k], o[k]), k


@pytest.mark.parametrize("variant", ["default", "use3d=0", "retry_2d=0"])
def test_batch_matches_the_oracle(hiplib, variant):
    sp = SearchParams.default()
    if variant == "use3d=0":
        sp = sp.copy(use3d=0)
    elif variant == "retry_2d=0":
        sp = sp.copy(retry_2d=0)
    h = hiplib.Handle()
    # every small scene, each on its own map, 8 copies per scene (64 queries) ...
    for name, g, res, org, st, en in ss.small_scenes():
        h.set_grid_map(g, res, org)
        S, E = np.repeat(st[None], 8, 0), np.repeat(en[None], 8, 0)
        r = h.kino_search(S, E, sp=sp)
        o = ps.kino_search(g, res, org, S[:1], E[:1], sp=sp, order=2)
        for k in o:
            assert np.array_equal(r[k], np.repeat(o[k], 8, 0)), (name, k)
    # ... and 48 default-arena queries
    grid, res, org, S, E = _arena_batch()
    h.set_grid_map(grid, res, org)
    r = h.kino_search(S, E, sp=sp)
    o = ps.kino_search(grid, res, org, S, E, sp=sp, order=2, nthreads=8)
    _compare(r, o)
    assert (r["status"] == 2).all()
    h.close()


@pytest.fixture(scope="module")
def scene_handles(hiplib):
    """one handle per scene of search_cases.py, kept for the module: the cases of a scene follow one another over one workspace,
    whatever allocate_num each asks for"""
    handles = {}
    yield handles, hiplib
    for h in handles.values():
        h.close()


@pytest.mark.parametrize("case", sc.NEW_CASES)
def test_case_matches_the_oracle(scene_handles, case):
    """the branches only the CPU restatement took before (search_cases.py: the budget exit, node-pool exhaustion with its 2D retry
    in a crowded hash table, the bounds of the search space, every parameter off its default, yaws to wrap, a search of 5337 nodes):
    every output field bit-equal to the restatement in order 2.  tests/test_search_oracle.py holds each case to its condition."""
    handles, hiplib = scene_handles
    grid, res, org, S, E, sp = sc.queries(case)
    scene = sc.CASES[case][0]
    if scene not in handles:
        handles[scene] = hiplib.Handle()
        handles[scene].set_grid_map(grid, res, org)
    r = handles[scene].kino_search(S, E, sp=sp)
    _compare(r, sc.oracle(case))


def test_more_queries_than_slots_and_workspace_reuse(hiplib):
    """32 queries with allocate_num = 4194304 fit 14 at a time into the 6 GiB of workspace: three launches, the later ones writing
    the outputs of q0 + block over the slots of the first; before and after it a call at the default parameters, the workspace grown
    and then reused.  No search here uses more than 448 nodes, far below either pool size, and no output depends on allocate_num
    otherwise: the large call equals the default run's rows, cycled."""
    import ctypes as C
    big = SearchParams.default().copy(allocate_num=4194304)
    fn = hiplib.lib().dftpav_debug_search_slots
    fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    slots = C.c_int(0)
    assert fn(C.byref(big), 32, C.byref(slots), None) == hiplib.OK and slots.value == 14
    grid, res, org, S, E, _ = sc.queries("default-arena")
    o = sc.oracle("default-arena")
    assert o["nodes_used"].max() == 448
    idx = np.arange(32) % len(S)
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    first = h.kino_search(S, E)
    cycled = h.kino_search(S[idx], E[idx], sp=big)
    again = h.kino_search(S, E)
    _compare(first, o)
    _compare(again, o)
    _compare(again, first)
    for k in o:
        assert np.array_equal(cycled[k], o[k][idx]), k
    h.close()


def test_truncated_outputs_report_the_true_length(hiplib):
    name, g, res, org, st, en = ss.wall_gap()
    h = hiplib.Handle()
    h.set_grid_map(g, res, org)
    full = h.kino_search(st[None], en[None])
    cut = h.kino_search(st[None], en[None], max_nodes=3, max_path=10)
    assert cut["path_len"][0] == full["path_len"][0] > 10 and cut["n_nodes"][0] == full["n_nodes"][0] > 3
    assert np.array_equal(cut["paths"][0], full["paths"][0, :10]) and np.array_equal(cut["nodes"][0], full["nodes"][0, :3])
    h.close()


def test_no_map_is_invalid(hiplib):
    h = hiplib.Handle()
    with pytest.raises(hiplib.DftpavError) as e:
        h.kino_search(np.zeros((1, 4)), np.ones((1, 4)))
    assert e.value.code == hiplib.E_INVALID
    h.close()


def test_two_calls_give_the_same_bits(hiplib):
    grid, res, org, S, E = _arena_batch(copies=2)
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    a = h.kino_search(S, E)
    b = h.kino_search(S, E)
    _compare(a, b)
    assert h.corridor_last_ms() > 0.0
    h.close()


def test_default_arena_chain_with_a_search_in_front(hiplib, oracle):
    """test_default_map.py with a real search in front: a goal the direct shot cannot reach; every stage bit-equal to the
    oracle chain, the solves succeed and the validation is clean"""
    grid, res, org, start, goals = ss.arena()
    goal = goals[3:4]
    K, Kd, B = 16, 32, 4
    p = hiplib.default_params()
    p.traj_resolution, p.des_traj_resolution = K, Kd
    h = hiplib.Handle(p)
    h.set_grid_map(grid, res, org)
    st = start[None].copy()
    r = h.kino_search(st, goal)
    o = ps.kino_search(grid, res, org, st, goal, order=2)
    _compare(r, o)
    assert r["status"][0] == 2 and r["iters"][0] > 0
    n = int(r["path_len"][0])
    paths, plen = r["paths"][:, :n].copy(), r["path_len"].copy()
    fp = FrontendParams.default(K=K, Kd=Kd)
    fe = h.frontend_resample(paths, plen, st, goal, np.zeros((1, 2)), fp)
    fo = oracle.frontend_resample(paths, plen, st, goal, np.zeros((1, 2)), fp, order=2)
    for k in fo:
        assert np.array_equal(fe[k], fo[k]), k
    M = int(fe["n_seg"][0])
    pn = [int(x) for x in fe["piece_nums"][0, :M]]
    sg = [int(x) for x in fe["singul"][0, :M]]
    lay = LayoutSpec(pn, sg, 4)
    npts = lay.n_points(K, Kd)
    states = np.concatenate([fe["states"][0, i, :fe["n_states"][0, i]] for i in range(M)])
    assert states.shape[0] == npts
    inner = np.concatenate([fe["inner_pts"][0, i, :pn[i] - 1].reshape(-1) for i in range(M)])
    durs = fe["piece_dt"][0, :M] * fe["piece_nums"][0, :M]
    s = Scenario("search-chain", lay, K, Kd, B, np.repeat(fe["ini_states"][0:1, :M], B, 0).copy(),
                 np.repeat(fe["fin_states"][0:1, :M], B, 0).copy(), np.repeat(inner[None], B, 0).copy(),
                 np.repeat(durs[None], B, 0).copy(), np.zeros((B, npts, 4, 4)))
    bt = hiplib.Batch(h, lay, B)
    bt.upload(s, with_corridor=False)
    bt.corridor_from_states(np.repeat(states[None], B, 0))
    bt.set_order(hiplib.ORDER_REFERENCE)
    res_ = bt.solve()
    s.corridor = np.repeat(oracle.corridor_rectangles(grid, res, org, states, order=2)[None], B, 0)
    ro = oracle.solve_batch(p, s, nthreads=4, order=2)
    for k in ("final_cost", "x", "status", "iters", "evals"):
        assert np.array_equal(res_[k], ro[k]), k
    assert res_["success"].all()
    col, first = bt.validate()
    co, dts = bt.coeffs()
    oc, of = oracle.validate_trajectories(grid, res, org, co, dts, lay.piece_nums, lay.singuls, order=2)
    assert np.array_equal(col, oc) and np.array_equal(first, of) and not col.any()
    bt.close()
    h.close()
