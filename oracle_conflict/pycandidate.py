"""ctypes wrapper of the CPU yardstick of the candidate conflict check -- TEST INFRASTRUCTURE (candidate_oracle.cpp, built into
libconflict_oracle.so beside conflict_oracle.cpp).

Only tests/ and scripts/ import this."""
import ctypes as C

import numpy as np

from . import pyconflict as pc

FIELDS, VEH = pc.FIELDS, pc.VEH
_declared = False


def lib():
    global _declared
    L = pc.lib()
    if not _declared:
        cand = [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_double]
        L.oracle_candidate_poses.restype = None
        L.oracle_candidate_poses.argtypes = cand + [C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.oracle_candidate_conflicts.restype = None
        L.oracle_candidate_conflicts.argtypes = (cand + [C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                                         C.c_void_p, C.c_int] + [C.c_void_p] * 6)
        _declared = True
    return L


def check_args(t_start, t0, dt, K, margin=0.0, range=None):
    """what dftpav_batch_check_conflicts refuses, without a library call: raises ValueError; returns (margin, range) as floats, range =
    margin when None.  A negative margin is legal: nothing conflicts."""
    t_start, t0, dt, margin = float(t_start), float(t0), float(dt), float(margin)
    rng = margin if range is None else float(range)
    if int(K) != K or K < 1 or K > pc.MAX_SAMPLES:
        raise ValueError("K must be in [1, %d]" % pc.MAX_SAMPLES)
    if not (dt > 0.0) or not np.isfinite(dt):
        raise ValueError("dt must be positive and finite")
    if not np.isfinite(t0) or not np.isfinite(t_start):
        raise ValueError("t0 and t_start must be finite")
    if margin != margin:
        raise ValueError("margin must be a number")
    if not np.isfinite(rng) or rng < margin:
        raise ValueError("range must be finite and >= margin")
    return margin, rng


def _batch(singul, piece_nums, piece_dt, coeffs):
    sg = np.ascontiguousarray(singul, dtype=np.int32).reshape(-1)
    pn = np.ascontiguousarray(piece_nums, dtype=np.int32).reshape(-1)
    M = sg.shape[0]
    dt = np.ascontiguousarray(piece_dt, dtype=np.float64).reshape(-1, M)
    B = dt.shape[0]
    co = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(B, -1, 6, 2)
    assert pn.shape == (M,) and co.shape[1] == int(pn.sum()), (pn, co.shape)
    keep = (sg, pn, dt, co)
    return keep, [B, M, co.shape[1]] + [a.ctypes.data for a in keep]


def poses(singul, piece_nums, piece_dt, coeffs, t_start, t0, dt, K, veh=VEH, order=2):
    """B candidates of one layout (singul / piece_nums [M], piece_dt [B][M], coeffs [B][sum piece_nums][6][2]) started at t_start
    -> poses [K][B][4] = cx, cy, cs, sn at the clocks t0 + k dt"""
    check_args(t_start, t0, dt, K)
    keep, args = _batch(singul, piece_nums, piece_dt, coeffs)
    v = np.array(veh, dtype=np.float64)
    out = np.zeros((int(K), args[0], 4))
    lib().oracle_candidate_poses(*args, float(t_start), float(t0), float(dt), int(K), v.ctypes.data, int(order), out.ctypes.data)
    return out


def conflicts(singul, piece_nums, piece_dt, coeffs, t_start, table, t0, dt, K, margin=0.0, range=None, own=None, veh=VEH, order=2):
    """the candidates against `table` = the six table arguments of pyconflict.conflicts (n_seg, singul, piece_nums, coeff_dt, coeffs,
    t_start of every slot) -> dict(min_sep, sep_sample, sep_partner, conflict_sample, conflict_partner [B]); own [B] or None"""
    margin, rng = check_args(t_start, t0, dt, K, margin, range)
    keep, args = _batch(singul, piece_nums, piece_dt, coeffs)
    tkeep, targs = pc._table(*table)
    B = args[0]
    ow = None
    if own is not None:
        ow = np.ascontiguousarray(own, dtype=np.int32).reshape(B)
    v = np.array(veh, dtype=np.float64)
    out = dict(min_sep=np.zeros(B), **{k: np.zeros(B, dtype=np.int32) for k in FIELDS[1:]})
    lib().oracle_candidate_conflicts(*args, float(t_start), *targs, float(t0), float(dt), int(K), margin, rng, v.ctypes.data, int(order),
                                     ow.ctypes.data if ow is not None else None, *[out[k].ctypes.data for k in FIELDS])
    return out
