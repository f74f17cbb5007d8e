"""ctypes loader of the CPU restatement of the 100 Hz publisher -- TEST INFRASTRUCTURE (publish_oracle.cpp).

Only tests/ and scripts/ import this."""
import ctypes as C
import os

import numpy as np

from oracle_shared.loader import Loader


def _declare(L):
    L.oracle_publish.restype = None
    L.oracle_publish.argtypes = [C.c_int] * 3 + [C.c_void_p] * 9 + [C.c_int, C.c_void_p, C.c_double, C.c_int] + [C.c_void_p] * 5


_load = Loader(os.path.dirname(os.path.abspath(__file__)), "libpublish_oracle.so",
               ("publish_oracle.cpp", "../oracle_shared/ref_objects.h", "../oracle/step_trig.h", "../dftpav_amd/csrc/cr_trig.h"), _declare)
build, lib = _load.build, _load.lib


class Table:
    """The executing plans on the host, padded as the device's table, with the publisher's state of every slot: exe_index, the
    back of the control history hist (stamp, angle) and have."""

    def __init__(self, slots, max_seg=8, max_pieces=64):
        i32 = np.int32
        self.slots, self.max_seg, self.max_pieces = int(slots), int(max_seg), int(max_pieces)
        self.n_seg = np.zeros(slots, i32)
        self.singul = np.zeros((slots, max_seg), i32)
        self.piece_nums = np.zeros((slots, max_seg), i32)
        self.coeff_dt = np.zeros((slots, max_seg))
        self.coeffs = np.zeros((slots, max_seg * max_pieces, 6, 2))
        self.t_start = np.zeros(slots)
        self.exe_index = np.zeros(slots, i32)
        self.hist = np.zeros((slots, 2))
        self.have = np.zeros(slots, i32)

    def install(self, slot, singul, piece_nums, coeff_dt, coeffs, t_start):
        """one plan: singul / piece_nums / coeff_dt [M], coeffs [>= sum piece_nums][6][2]; the publisher starts on segment 0
        without history"""
        M = len(piece_nums)
        self.clear(slot)
        self.n_seg[slot] = M
        self.singul[slot, :M] = singul
        self.piece_nums[slot, :M] = piece_nums
        self.coeff_dt[slot, :M] = coeff_dt
        co = np.asarray(coeffs, dtype=np.float64)
        self.coeffs[slot, :co.shape[0]] = co
        self.t_start[slot] = t_start

    def set_ctrl_history(self, slot, stamp, angle):
        self.hist[slot] = (stamp, angle)
        self.have[slot] = 1

    def clear(self, slot):
        for a in (self.n_seg, self.singul, self.piece_nums, self.coeff_dt, self.coeffs, self.t_start, self.exe_index, self.hist, self.have):
            a[slot] = 0


def publish(table, clocks, wheel_base=2.85, order=2):
    """One PublishData call per clock and slot, in order; advances the publisher's state of `table` in place.  -> dict(states
    [K][slots][8], published [K][slots], index [K][slots] (the segment read, -1: none), t_local, raw_angle [K][slots] (the time
    handed to GetState and the angle it gave))"""
    T = table
    S = T.slots
    t = np.ascontiguousarray(clocks, dtype=np.float64).reshape(-1)
    K = t.shape[0]
    states = np.zeros((K, S, 8))
    pub, idx = np.zeros((K, S), dtype=np.int32), np.zeros((K, S), dtype=np.int32)
    tl, raw = np.zeros((K, S)), np.zeros((K, S))
    ro = [np.ascontiguousarray(a) for a in (T.n_seg, T.singul, T.piece_nums, T.coeff_dt, T.coeffs, T.t_start)]
    for a in (T.exe_index, T.hist, T.have):
        assert a.flags["C_CONTIGUOUS"]
    lib().oracle_publish(S, T.max_seg, T.max_pieces, *[a.ctypes.data for a in ro], T.exe_index.ctypes.data, T.hist.ctypes.data,
                         T.have.ctypes.data, K, t.ctypes.data, float(wheel_base), int(order), states.ctypes.data, pub.ctypes.data,
                         idx.ctypes.data, tl.ctypes.data, raw.ctypes.data)
    return dict(states=states, published=pub, index=idx, t_local=tl, raw_angle=raw)
