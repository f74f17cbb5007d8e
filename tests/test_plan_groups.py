"""The host half of dftpav_plan_queries that needs no device: the grouping of queries by layout (dftpav_plan_group_layouts), the
default parameters (dftpav_default_plan_params against the defaults of the stages) and the entry points without a handle."""
import ctypes as C

import numpy as np
import pytest

from dftpav_amd import pods

REACH, NO_PATH = 2, 3


def _rows(rows, max_seg=4):
    a = np.zeros((len(rows), max_seg), dtype=np.int32)
    for i, r in enumerate(rows):
        a[i, :len(r)] = r
    return a


def test_identical_layouts_share_a_group_and_first_appearance_orders_them(hiplib):
    pn = _rows([[3, 2], [6], [3, 2], [2, 2, 2], [6], [3, 2]])
    sg = _rows([[1, -1], [-1], [1, -1], [1, -1, 1], [-1], [1, -1]])
    r = hiplib.plan_group_layouts([REACH] * 6, [2, 1, 2, 3, 1, 2], sg, pn)
    assert r["group"].tolist() == [0, 1, 0, 2, 1, 0]
    assert r["group_first"].tolist() == [0, 1, 3]
    assert (r["plan_status"] == hiplib.PLAN_OK).all()


def test_layouts_that_differ_only_in_singul_or_in_pieces_do_not(hiplib):
    pn = _rows([[3, 2], [3, 2], [3, 3], [3]])
    sg = _rows([[1, -1], [-1, 1], [1, -1], [1]])
    r = hiplib.plan_group_layouts([REACH] * 4, [2, 2, 2, 1], sg, pn)
    assert r["group"].tolist() == [0, 1, 2, 3] and r["group_first"].tolist() == [0, 1, 2, 3]


def test_entries_past_n_seg_do_not_count(hiplib):
    pn = _rows([[3, 2, 9, 9], [3, 2, 0, 0]])
    sg = _rows([[1, -1, 7, 7], [1, -1, 0, 0]])
    r = hiplib.plan_group_layouts([REACH, REACH], [2, 2], sg, pn)
    assert r["group"].tolist() == [0, 0] and r["group_first"].tolist() == [0]


def test_no_path_and_over_padded_queries_get_no_group_and_their_status(hiplib):
    pn = _rows([[3, 2], [0], [2, 2, 2, 2], [3, 2], [4], [0]])
    sg = _rows([[1, -1], [0], [1, -1, 1, -1], [1, -1], [1], [0]])
    status = [REACH, NO_PATH, REACH, REACH, REACH, REACH]
    n_seg = [2, 0, 5, 2, 1, 0]          # query 2 found five segments for a padding of four; query 5 none at all
    r = hiplib.plan_group_layouts(status, n_seg, sg, pn)
    assert r["group"].tolist() == [0, -1, -1, 0, 1, -1]
    assert r["group_first"].tolist() == [0, 4]
    assert r["plan_status"].tolist() == [hiplib.PLAN_OK, hiplib.PLAN_NO_PATH, hiplib.PLAN_TOO_MANY_SEGMENTS, hiplib.PLAN_OK,
                                         hiplib.PLAN_OK, hiplib.PLAN_TOO_MANY_SEGMENTS]


def test_a_first_query_without_a_group_does_not_take_group_zero(hiplib):
    pn = _rows([[0], [5], [5]])
    sg = _rows([[0], [1], [1]])
    r = hiplib.plan_group_layouts([NO_PATH, REACH, REACH], [0, 1, 1], sg, pn)
    assert r["group"].tolist() == [-1, 0, 0] and r["group_first"].tolist() == [1]


def test_empty_input(hiplib):
    r = hiplib.plan_group_layouts(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32))
    assert r["group"].shape == (0,) and r["group_first"].shape == (0,) and r["plan_status"].shape == (0,)
    fn = hiplib.lib().dftpav_plan_group_layouts
    fn.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 8
    ng = C.c_int(-1)
    assert fn(0, 4, None, None, None, None, None, None, C.byref(ng), None) == hiplib.OK and ng.value == 0
    assert fn(0, 4, None, None, None, None, None, None, None, None) == hiplib.E_INVALID      # nowhere to put the count
    assert fn(2, 4, None, None, None, None, None, None, C.byref(ng), None) == hiplib.E_INVALID  # queries without tables
    assert fn(-1, 4, None, None, None, None, None, None, C.byref(ng), None) == hiplib.E_INVALID
    assert fn(0, 0, None, None, None, None, None, None, C.byref(ng), None) == hiplib.E_INVALID


def test_planner_create_without_a_handle_or_a_device(hiplib):
    L = hiplib.lib()
    L.dftpav_planner_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    out = C.c_void_p(1)
    assert L.dftpav_planner_create(None, 4, 4, C.byref(out)) == hiplib.E_INVALID and not out.value
    with pytest.raises(hiplib.DftpavError) as e:
        hiplib.Planner(None, 4, 4)
    assert e.value.code == hiplib.E_INVALID
    L.dftpav_plan_queries.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_double, C.c_void_p]
    assert L.dftpav_plan_queries(None, None, None, None, None, 0, 0.0, None) == hiplib.E_INVALID
    L.dftpav_planner_info.argtypes = [C.c_void_p] * 5
    assert L.dftpav_planner_info(None, None, None, None, None) == hiplib.E_INVALID
    L.dftpav_debug_plan_select.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    assert L.dftpav_debug_plan_select(None, 1, 1, None, None, None, None) == hiplib.E_INVALID
    L.dftpav_planner_destroy.argtypes = [C.c_void_p]
    L.dftpav_planner_destroy.restype = None
    L.dftpav_planner_destroy(None)      # a null planner is ignored, as a null handle is
    import torch
    if not torch.cuda.is_available():   # no device: no handle to create a planner on, and no fallback
        with pytest.raises(hiplib.DftpavError) as e:
            hiplib.Planner(hiplib.Handle(), 4, 4)
        assert e.value.code == hiplib.E_NO_DEVICE


def _fields(s):
    return {n: getattr(s, n) for n, _ in s._fields_}


def test_default_plan_params_are_the_defaults_of_the_stages(hiplib):
    L = hiplib.lib()
    L.dftpav_abi_sizeof_plan_params.restype = C.c_int
    L.dftpav_abi_sizeof_plan_out.restype = C.c_int
    assert L.dftpav_abi_sizeof_plan_params() == C.sizeof(pods.PlanParams)
    assert L.dftpav_abi_sizeof_plan_out() == C.sizeof(pods.PlanOutC)
    pp = hiplib.default_plan_params()
    sp = pods.SearchParams()
    L.dftpav_default_search_params.argtypes = [C.c_void_p]
    L.dftpav_default_search_params.restype = None
    L.dftpav_default_search_params(C.byref(sp))
    assert _fields(pp.search) == _fields(sp) == _fields(pods.SearchParams.default())
    assert _fields(pp.frontend) == _fields(pods.FrontendParams.default())
    p = hiplib.default_params()       # the front end resamples at the solver's resolutions and with its limits
    assert (pp.frontend.traj_res, pp.frontend.dense_traj_res) == (p.traj_resolution, p.des_traj_resolution)
    assert (pp.frontend.max_forward_vel, pp.frontend.max_forward_acc) == (p.max_forward_vel, p.max_forward_acc)
    assert (pp.frontend.max_backward_vel, pp.frontend.max_backward_acc) == (p.max_backward_vel, p.max_backward_acc)
    import inspect
    d = {k: v.default for k, v in inspect.signature(hiplib.Handle.sample_restarts).parameters.items()}
    assert (pp.sigma, pp.dur_lo, pp.dur_hi, pp.seed) == (d["sigma"], d["lo"], d["hi"], d["seed"])
    d = {k: v.default for k, v in inspect.signature(hiplib.Batch.validate).parameters.items()}
    assert (pp.check_dt, pp.vertex_res) == (d["sample_dt"], d["vertex_res"])
    d = {k: v.default for k, v in inspect.signature(pods.FrontendOut.__init__).parameters.items()}
    assert (pp.max_seg, pp.max_pieces) == (d["max_seg"], d["max_pieces"])
    d = {k: v.default for k, v in inspect.signature(hiplib.Handle.kino_search).parameters.items()}
    assert pp.max_path == d["max_path"]
