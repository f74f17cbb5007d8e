"""ctypes wrapper of the CPU yardstick of joint selection -- TEST INFRASTRUCTURE (joint_oracle.cpp, libjoint_oracle.so).

Only tests/ and scripts/ import this."""
import ctypes as C
import os

import numpy as np

from oracle_shared.loader import Loader

FIELDS = ("min_sep", "sep_sample", "sep_partner", "conflict_sample", "conflict_partner")
VEH = (1.90, 4.88, 1.015)     # veh_width, veh_length, veh_d_cr of the default parameters


def _declare(L):
    outs = [C.c_void_p] * 7
    L.oracle_joint_select.restype = None
    L.oracle_joint_select.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_double, C.c_double, C.c_void_p, C.c_int] + outs
    L.oracle_joint_select_plans.restype = None
    L.oracle_joint_select_plans.argtypes = ([C.c_int] * 4 + [C.c_void_p] * 7 + [C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                                                                C.c_void_p, C.c_int] + outs + [C.c_void_p])


_load = Loader(os.path.dirname(os.path.abspath(__file__)), "libjoint_oracle.so",
               ("joint_oracle.cpp", "../oracle_shared/ref_objects.h", "../oracle/step_trig.h", "../dftpav_amd/csrc/cr_trig.h"), _declare)
build, lib = _load.build, _load.lib


def _outs(Q, R):
    out = dict(winner=np.zeros(Q, dtype=np.int32), blocked=np.zeros((Q, R), dtype=np.int32), min_sep=np.zeros((Q, R)),
               **{k: np.zeros((Q, R), dtype=np.int32) for k in FIELDS[1:]})
    return out, [out[k].ctypes.data for k in ("winner", "blocked") + FIELDS]


def _check(margin, range):
    margin = float(margin)
    rng = margin if range is None else float(range)
    if margin != margin or not np.isfinite(rng) or rng < margin:
        raise ValueError("margin must be a number, range finite and >= margin")
    return margin, rng


def select(poses, cost, eligible, margin, range=None, veh=VEH, order=2):
    """poses [K][Q][R][4] = cx, cy, cs, sn, cost and eligible [Q][R] -> dict(winner [Q], blocked [Q][R], the five rows [Q][R]; the
    partner index is a query index)"""
    margin, rng = _check(margin, range)
    c = np.ascontiguousarray(cost, dtype=np.float64)
    e = np.ascontiguousarray(eligible, dtype=np.int32)
    Q, R = c.shape
    ps = np.ascontiguousarray(poses, dtype=np.float64)
    K = ps.shape[0]
    assert ps.shape == (K, Q, R, 4) and e.shape == (Q, R) and K >= 1, (ps.shape, c.shape, e.shape)
    v = np.array(veh, dtype=np.float64)
    out, ptrs = _outs(Q, R)
    lib().oracle_joint_select(Q, R, K, ps.ctypes.data, c.ctypes.data, e.ctypes.data, margin, rng, v.ctypes.data, int(order), *ptrs)
    return out


def select_plans(n_seg, singul, piece_nums, piece_dt, coeffs, cost, eligible, t_call, dt, K, margin, range=None, veh=VEH, order=2):
    """per query a layout padded as the executing table (n_seg [Q], 0: no candidates; singul / piece_nums [Q][max_seg]), per candidate
    piece_dt [Q][R][max_seg] and coeffs [Q][R][row_pieces][6][2]; every candidate starts at t_call, the clocks are t_call + k dt
    -> the dict of select() and poses [K][Q][R][4]"""
    margin, rng = _check(margin, range)
    c = np.ascontiguousarray(cost, dtype=np.float64)
    e = np.ascontiguousarray(eligible, dtype=np.int32)
    Q, R = c.shape
    ns = np.ascontiguousarray(n_seg, dtype=np.int32).reshape(Q)
    sg = np.ascontiguousarray(singul, dtype=np.int32).reshape(Q, -1)
    MS = sg.shape[1]
    pn = np.ascontiguousarray(piece_nums, dtype=np.int32).reshape(Q, MS)
    pd = np.ascontiguousarray(piece_dt, dtype=np.float64).reshape(Q, R, MS)
    co = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(Q, R, -1, 6, 2)
    assert ((0 <= ns) & (ns <= MS)).all() and all(pn[q, :ns[q]].sum() <= co.shape[2] for q in np.arange(Q))
    v = np.array(veh, dtype=np.float64)
    out, ptrs = _outs(Q, R)
    out["poses"] = np.zeros((int(K), Q, R, 4))
    lib().oracle_joint_select_plans(Q, R, MS, co.shape[2], ns.ctypes.data, sg.ctypes.data, pn.ctypes.data, pd.ctypes.data, co.ctypes.data,
                                    c.ctypes.data, e.ctypes.data, float(t_call), float(dt), int(K), margin, rng, v.ctypes.data, int(order), *ptrs,
                                    out["poses"].ctypes.data)
    return out
