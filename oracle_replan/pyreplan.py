"""ctypes loader of the CPU restatement of the replan loop -- TEST INFRASTRUCTURE (replan_oracle.cpp).

Only tests/ and scripts/ import this."""
import ctypes as C
import os

import numpy as np

from oracle_shared.loader import Loader


INTS = ("occupied", "complete", "exe_index", "is_close_turnpoint", "is_near", "target_moved", "collision", "first_sample", "replan")


def _declare(L):
    L.oracle_replan_check.restype = None
    L.oracle_replan_check.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int]
                                      + [C.c_void_p] * 9 + [C.c_double, C.c_double, C.c_void_p, C.c_void_p]
                                      + [C.c_double] * 6 + [C.c_int] + [C.c_void_p] * 7)


_load = Loader(os.path.dirname(os.path.abspath(__file__)), "libreplan_oracle.so",
               ("replan_oracle.cpp", "../oracle_shared/ref_objects.h", "../oracle/step_trig.h", "../dftpav_amd/csrc/cr_trig.h"), _declare)
build, lib = _load.build, _load.lib


class Table:
    """The executing table on the host, padded as the device's: a slot is empty (n_seg 0) or holds one plan."""

    def __init__(self, slots, max_seg=8, max_pieces=64):
        i32 = np.int32
        self.slots, self.max_seg, self.max_pieces = int(slots), int(max_seg), int(max_pieces)
        self.n_seg = np.zeros(slots, i32)
        self.singul = np.zeros((slots, max_seg), i32)
        self.piece_nums = np.zeros((slots, max_seg), i32)
        self.coeff_dt = np.zeros((slots, max_seg))
        self.coeffs = np.zeros((slots, max_seg * max_pieces, 6, 2))
        self.end_state = np.zeros((slots, 4))
        self.hist = np.zeros((slots, 2))
        self.have_hist = np.zeros(slots, i32)
        self.t_start = np.zeros(slots)

    def install(self, slot, singul, piece_nums, coeff_dt, coeffs, end_state, t_start):
        """one plan: singul / piece_nums / coeff_dt [M], coeffs [sum piece_nums][6][2]"""
        M = len(piece_nums)
        self.clear(slot)
        self.n_seg[slot] = M
        self.singul[slot, :M] = singul
        self.piece_nums[slot, :M] = piece_nums
        self.coeff_dt[slot, :M] = coeff_dt
        co = np.asarray(coeffs, dtype=np.float64)
        self.coeffs[slot, :co.shape[0]] = co
        self.end_state[slot] = end_state
        self.t_start[slot] = t_start

    def set_history(self, slot, stamp, angle):
        self.hist[slot] = (stamp, angle)
        self.have_hist[slot] = 1

    def clear(self, slot):
        for a in (self.n_seg, self.singul, self.piece_nums, self.coeff_dt, self.coeffs, self.end_state, self.hist, self.have_hist, self.t_start):
            a[slot] = 0


def replan_check(grid, resolution, origin, table, t_now, budget=0.5, end_states=None, ego_states=None, veh=(1.90, 4.88, 1.015),
                 wheel_base=2.85, check_dt=0.05, vertex_res=0.1, order=2):
    """One tick of the reference's loop for every slot of `table`: the dict of dftpav_amd.pods.ReplanOut, plus duration / start_time /
    end_time [slots][max_seg], pidx and t_local [slots] (the segment and the local time the desired state was read at)."""
    T = table
    S = T.slots
    g = np.ascontiguousarray(grid, dtype=np.uint8)
    en = None if end_states is None else np.ascontiguousarray(end_states, dtype=np.float64).reshape(S, 4)
    eg = None if ego_states is None else np.ascontiguousarray(ego_states, dtype=np.float64).reshape(S, 6)
    o_int = np.zeros((len(INTS), S), dtype=np.int32)
    des, st, ct = np.zeros((S, 8)), np.zeros((S, 4)), np.zeros((S, 2))
    times = np.zeros((S, T.max_seg, 3))
    pidx, tl = np.zeros(S, dtype=np.int32), np.zeros(S)
    ptr = lambda a: None if a is None else a.ctypes.data
    arrs = [np.ascontiguousarray(a) for a in (T.n_seg, T.singul, T.piece_nums, T.coeff_dt, T.coeffs, T.end_state, T.hist, T.have_hist, T.t_start)]
    lib().oracle_replan_check(g.ctypes.data, g.shape[1], g.shape[0], float(resolution), float(origin[0]), float(origin[1]), S, T.max_seg,
                              T.max_pieces, *[ptr(a) for a in arrs], float(t_now), float(budget), ptr(en), ptr(eg), float(veh[0]),
                              float(veh[1]), float(veh[2]), float(wheel_base), float(check_dt), float(vertex_res), int(order),
                              ptr(o_int), ptr(des), ptr(st), ptr(ct), ptr(times), ptr(pidx), ptr(tl))
    out = {k: o_int[i].copy() for i, k in enumerate(INTS)}
    out.update(desired=des, start_state=st, start_ctrl=ct, duration=times[:, :, 0].copy(), start_time=times[:, :, 1].copy(),
               end_time=times[:, :, 2].copy(), pidx=pidx, t_local=tl)
    return out
