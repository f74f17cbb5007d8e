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
    L.oracle_state_transit.restype = None
    L.oracle_state_transit.argtypes = [C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    L.heap_selftest.restype = C.c_longlong
    L.heap_selftest.argtypes = [C.c_ulonglong, C.c_longlong]


_load = Loader(os.path.dirname(os.path.abspath(__file__)), "libkino_search_oracle.so",
               ("kino_search_oracle.cpp", "../oracle/step_trig.h", "../dftpav_amd/csrc/kino_heap.h", "../dftpav_amd/csrc/rs_math.h",
                "../dftpav_amd/csrc/cr_trig.h", "../include/dftpav_hip.h"), _declare)
build, lib = _load.build, _load.lib


def kino_search(grid, resolution, origin, start_states, end_states, sp=None, order=2, max_nodes=512, max_path=4096,
                nthreads=1, fields=None, field_of=None, unit=0.0, field_entry=False):
    """getKinoPath (KinoAstar::search with its 2D retry) + getKinoNode up to SampleTraj for n queries: the dict of
    dftpav_amd.pods.SearchOut.  start_states / end_states [n][4] (x, y, yaw, v).

    fields (int32 [k][size_y][size_x]), field_of ([n], -1: none; default: query q reads field q, or all the one field) and unit: the
    heuristic of dftpav_set_search_heuristic through oracle_kino_search_field (oracle_goalfield.pygoalfield.search_fields makes the
    three).  Off by default: oracle_kino_search.  field_entry=True takes the new entry without a field."""
    g = np.ascontiguousarray(grid, dtype=np.uint8)
    st = np.ascontiguousarray(start_states, dtype=np.float64).reshape(-1, 4)
    en = np.ascontiguousarray(end_states, dtype=np.float64).reshape(-1, 4)
    sp = sp if sp is not None else SearchParams.default()
    out = SearchOut(st.shape[0], max_nodes, max_path)
    args = (g.ctypes.data, g.shape[1], g.shape[0], float(resolution), float(origin[0]), float(origin[1]), C.addressof(sp), st.ctypes.data,
            en.ctypes.data, st.shape[0], int(order), int(nthreads), C.addressof(out.c))
    if fields is None and not field_entry:
        lib().oracle_kino_search(*args)
    elif fields is None:
        lib().oracle_kino_search_field(*args, None, None, 0.0)
    else:
        f = np.ascontiguousarray(fields, dtype=np.int32).reshape((-1,) + g.shape)
        if field_of is None:
            assert f.shape[0] in (1, st.shape[0])
            field_of = np.arange(st.shape[0]) if f.shape[0] == st.shape[0] else np.zeros(st.shape[0])
        fo = np.ascontiguousarray(field_of, dtype=np.int32).reshape(-1)
        assert fo.shape[0] == st.shape[0] and fo.max() < f.shape[0]
        lib().oracle_kino_search_field(*args, f.ctypes.data, fo.ctypes.data, float(unit))
    return out.arrays()


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
