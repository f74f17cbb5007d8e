"""ctypes loader of the CPU restatement of the hybrid A* front end -- TEST INFRASTRUCTURE (kino_search_oracle.cpp).

Only tests/ and scripts/ import this."""
import ctypes as C
import os

import numpy as np

from dftpav_amd.pods import SearchOut, SearchParams
from oracle_shared.loader import Loader


def _declare(L):
    L.oracle_kino_search.restype = None
    L.oracle_kino_search.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.oracle_kino_search_field.restype = None
    L.oracle_kino_search_field.argtypes = L.oracle_kino_search.argtypes + [C.c_void_p, C.c_void_p, C.c_double]
    L.oracle_kino_search_heu.restype = None
    L.oracle_kino_search_heu.argtypes = L.oracle_kino_search_field.argtypes + [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double]
    L.oracle_rs_table.restype = None
    L.oracle_rs_table.argtypes = [C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p]
    L.oracle_rs_slot.restype = None
    L.oracle_rs_slot.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.oracle_state_transit.restype = None
    L.oracle_state_transit.argtypes = [C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    L.heap_selftest.restype = C.c_longlong
    L.heap_selftest.argtypes = [C.c_ulonglong, C.c_longlong]


_load = Loader(os.path.dirname(os.path.abspath(__file__)), "libkino_search_oracle.so",
               ("kino_search_oracle.cpp", "../oracle/step_trig.h", "../dftpav_amd/csrc/kino_heap.h", "../dftpav_amd/csrc/rs_math.h",
                "../dftpav_amd/csrc/cr_trig.h", "../include/dftpav_hip.h"), _declare)
build, lib = _load.build, _load.lib


def kino_search(grid, resolution, origin, start_states, end_states, sp=None, order=2, max_nodes=512, max_path=4096,
                nthreads=1, fields=None, field_of=None, unit=0.0, field_entry=False, rs_tab=None, rs_extent=0.0, rs_cell=1.0,
                rs_scale=1.0, heu_entry=False):
    """getKinoPath (KinoAstar::search with its 2D retry) + getKinoNode up to SampleTraj for n queries: the dict of
    dftpav_amd.pods.SearchOut.  start_states / end_states [n][4] (x, y, yaw, v).

    fields (int32 [k][size_y][size_x]), field_of ([n], -1: none; default: query q reads field q, or all the one field) and unit: the
    heuristic of dftpav_set_search_heuristic through oracle_kino_search_field (oracle_goalfield.pygoalfield.search_fields makes the
    three).  Off by default: oracle_kino_search.  field_entry=True takes the new entry without a field.

    rs_tab (float64 [n_yaw][n][n], from rs_table below, of rs_extent and rs_cell) and rs_scale: the Reeds-Shepp term of
    dftpav_set_search_rs_heuristic through oracle_kino_search_heu, with or without fields.  heu_entry=True takes that entry without
    a table."""
    g = np.ascontiguousarray(grid, dtype=np.uint8)
    st = np.ascontiguousarray(start_states, dtype=np.float64).reshape(-1, 4)
    en = np.ascontiguousarray(end_states, dtype=np.float64).reshape(-1, 4)
    sp = sp if sp is not None else SearchParams.default()
    out = SearchOut(st.shape[0], max_nodes, max_path)
    args = (g.ctypes.data, g.shape[1], g.shape[0], float(resolution), float(origin[0]), float(origin[1]), C.addressof(sp), st.ctypes.data,
            en.ctypes.data, st.shape[0], int(order), int(nthreads), C.addressof(out.c))
    call = lib().oracle_kino_search_field
    if rs_tab is not None or heu_entry:
        tab = np.ascontiguousarray(rs_tab, dtype=np.float64) if rs_tab is not None else None
        if tab is not None:
            half = int(np.ceil(float(rs_extent) / float(rs_cell)))
            assert tab.ndim == 3 and tab.shape[1] == tab.shape[2] == 2 * half + 1
        tail = (tab.ctypes.data if tab is not None else None, tab.shape[0] if tab is not None else 0, float(rs_extent), float(rs_cell),
                float(rs_scale))
        call = lambda *a: lib().oracle_kino_search_heu(*a, *tail)       # noqa: E731
    if fields is None and not field_entry and call is lib().oracle_kino_search_field:
        lib().oracle_kino_search(*args)
    elif fields is None:
        call(*args, None, None, 0.0)
    else:
        f = np.ascontiguousarray(fields, dtype=np.int32).reshape((-1,) + g.shape)
        if field_of is None:
            assert f.shape[0] in (1, st.shape[0])
            field_of = np.arange(st.shape[0]) if f.shape[0] == st.shape[0] else np.zeros(st.shape[0])
        fo = np.ascontiguousarray(field_of, dtype=np.int32).reshape(-1)
        assert fo.shape[0] == st.shape[0] and fo.max() < f.shape[0]
        call(*args, f.ctypes.data, fo.ctypes.data, float(unit))
    return out.arrays()


def rs_table(rho, n_yaw=72, extent=15.0, cell=0.25, order=2):
    """oracle_rs_table: the Reeds-Shepp cost-to-go table float64 [n_yaw][n][n], n = 2 ceil(extent / cell) + 1: entry (k, j, i) is
    rho * the normalised length of the shortest path from ((i - half) cell, (j - half) cell, k 2 pi / n_yaw) to (0, 0, 0)."""
    half = int(np.ceil(float(extent) / float(cell)))
    out = np.zeros((int(n_yaw), 2 * half + 1, 2 * half + 1))
    lib().oracle_rs_table(int(order), float(rho), int(n_yaw), float(extent), float(cell), out.ctypes.data)
    return out


def rs_slot(goal, poses, n_yaw, extent, cell, order=2):
    """The lookup rule of the search with a table: for poses [m][3] and a goal [3], the flat offset into the table each pose reads,
    -1 where it reads nothing."""
    g = np.ascontiguousarray(goal, dtype=np.float64)[:3].copy()
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(p.shape[0], dtype=np.int64)
    lib().oracle_rs_slot(int(order), int(n_yaw), float(extent), float(cell), g.ctypes.data, p.ctypes.data, p.shape[0], out.ctypes.data)
    return out


def state_transit(state0, ctrl, wheel_base=2.85, order=2):
    """KinoAstar::stateTransit (kino_astar.cpp:21-36) in the given order: (x, y, yaw) of (steer, arc) from state0."""
    s0 = np.ascontiguousarray(state0, dtype=np.float64)[:3].copy()
    u = np.ascontiguousarray(ctrl, dtype=np.float64)[:2].copy()
    o = np.zeros(3)
    lib().oracle_state_transit(int(order), float(wheel_base), s0.ctypes.data, u.ctypes.data, o.ctypes.data)
    return o


def heap_selftest(seed, n_ops):
    """kino_heap.h against std::priority_queue: -1, or the first operation after which they differ."""
    return int(lib().heap_selftest(int(seed), int(n_ops)))
