"""C-ABI of the replan loop without a device: every new entry point refuses a null planner with DFTPAV_E_INVALID, the output POD
has the compiled layout, and the header, the export list and the library agree.  (The refusals that need a planner -- slot out
of range, n_seg > max_seg, another padding -- need a device: tests/test_gpu_replan.py.)"""
import ctypes as C
import os
import re

import numpy as np

from dftpav_amd import pods

NEW = ("dftpav_planner_install", "dftpav_planner_adopt", "dftpav_planner_set_history", "dftpav_planner_clear",
       "dftpav_planner_executing", "dftpav_planner_padding", "dftpav_replan_check", "dftpav_replan_tick", "dftpav_replan_last_ms")


def test_new_entries_are_declared_exported_and_cited(hiplib):
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "dftpav_hip.h")).read()
    L = hiplib.lib()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in hiplib.EXPORTS and getattr(L, name) is not None, name
    # the citation comment the other entries carry: the reference's lines the loop replaces
    block = hdr[hdr.index("the replan loop"):hdr.index("One-shot convenience")]
    for cite in ("traj_server_ros.cpp:149-158", ":359-402", ":445-461", ":335-356", "traj_manager.cpp:74-75", "traj_container.hpp:58-73",
                 "traj_manager.cpp:618-625", ":472-484", "traj_manager.cpp:631-637"):
        assert cite in block, cite


def test_replan_out_matches_the_compiled_layout(hiplib):
    L = hiplib.lib()
    L.dftpav_abi_sizeof_replan_out.restype = C.c_int
    assert L.dftpav_abi_sizeof_replan_out() == C.sizeof(pods.ReplanOutC)
    out = pods.ReplanOut(3)
    assert set(out.arrays()) == {n for n, _ in pods.ReplanOutC._fields_}
    assert out.arrays()["desired"].shape == (3, 8) and out.arrays()["start_state"].shape == (3, 4) and out.arrays()["start_ctrl"].shape == (3, 2)


def test_null_planner_is_invalid_everywhere(hiplib):
    L = hiplib.lib()
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    one = np.zeros(1, dtype=np.int32)
    buf = np.zeros(8 * 64 * 12)
    ip, dp = one.ctypes.data_as(vp), buf.ctypes.data_as(vp)
    pp = hiplib.default_plan_params()
    out = pods.ReplanOut(1)
    calls = {
        "dftpav_planner_install": ([vp, i, vp, i, i, vp, vp, vp, vp, vp, vp, d], (None, 1, ip, 8, 64, ip, ip, ip, dp, dp, dp, 0.0)),
        "dftpav_planner_adopt": ([vp, i, vp, vp, d, vp], (None, 1, ip, ip, 0.0, None)),
        "dftpav_planner_set_history": ([vp, i, vp, vp, vp], (None, 1, ip, dp, dp)),
        "dftpav_planner_clear": ([vp, i, vp], (None, 1, ip)),
        "dftpav_planner_executing": ([vp, i] + [vp] * 11, (None, 0) + (None,) * 11),
        "dftpav_planner_padding": ([vp, vp, vp], (None, None, None)),
        "dftpav_replan_check": ([vp, d, d, vp, vp, d, d, vp], (None, 0.0, 0.5, None, None, 0.05, 0.1, C.byref(out.c))),
        "dftpav_replan_tick": ([vp, vp, d, d] + [vp] * 6, (None, C.byref(pp), 0.0, 0.5, None, None, None, None, None, None)),
        "dftpav_replan_last_ms": ([vp, vp, vp], (None, None, None)),
    }
    assert set(calls) == set(NEW)
    for name, (argtypes, args) in calls.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, C.c_int
        assert fn(*args) == hiplib.E_INVALID, name
