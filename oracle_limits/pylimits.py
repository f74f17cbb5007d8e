"""ctypes loader of the CPU restatement of the kinematic-limits check -- TEST INFRASTRUCTURE (limits_oracle.cpp).

Only tests/ and scripts/ import this."""
import ctypes as C
import os

import numpy as np

from oracle_shared.loader import Loader


QUANTITIES = ("vel", "acc", "latacc", "cur", "steer")
LIMIT_FIELDS = ("max_forward_vel", "max_backward_vel", "max_forward_acc", "max_backward_acc", "max_forward_cur", "max_backward_cur",
                "max_latacc", "max_steer")


def _declare(L):
    L.oracle_limits.restype = None
    L.oracle_limits.argtypes = [C.c_int] * 3 + [C.c_void_p] * 5 + [C.c_double, C.c_double, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + \
        [C.c_int, C.c_void_p, C.c_void_p]


_load = Loader(os.path.dirname(os.path.abspath(__file__)), "liblimits_oracle.so",
               ("limits_oracle.cpp", "../oracle_shared/ref_objects.h", "../oracle/step_trig.h", "../dftpav_amd/csrc/cr_trig.h"), _declare)
build, lib = _load.build, _load.lib


def limits_vector(limits):
    """a dict / object with the fields of dftpav_limits, or a sequence of its 8 values -> float64 [8]"""
    if isinstance(limits, dict):
        return np.array([limits[f] for f in LIMIT_FIELDS], dtype=np.float64)
    if hasattr(limits, "max_forward_vel"):
        return np.array([getattr(limits, f) for f in LIMIT_FIELDS], dtype=np.float64)
    v = np.ascontiguousarray(limits, dtype=np.float64).reshape(-1)
    assert v.shape[0] == 8
    return v


def check_table(n_seg, singul, piece_nums, coeff_dt, coeffs, check_dt, limits, wheel_base=2.85, order=2, max_samples=0):
    """n plans padded as the executing table: n_seg [n], singul / piece_nums / coeff_dt [n][max_seg], coeffs [n][row_pieces][6][2].
    -> dict(max_abs, arg, violated [n][5], feasible [n], n_samples [n], samples [n][max_samples][8] (t, segment, local t, the five
    quantities signed))"""
    i32 = np.int32
    n_seg = np.ascontiguousarray(n_seg, dtype=i32).reshape(-1)
    n = n_seg.shape[0]
    singul = np.ascontiguousarray(singul, dtype=i32).reshape(n, -1)
    max_seg = singul.shape[1]
    piece_nums = np.ascontiguousarray(piece_nums, dtype=i32).reshape(n, max_seg)
    coeff_dt = np.ascontiguousarray(coeff_dt, dtype=np.float64).reshape(n, max_seg)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(n, -1, 6, 2)
    row_pieces = coeffs.shape[1]
    for s in range(n):
        assert 0 <= n_seg[s] <= max_seg and piece_nums[s, :n_seg[s]].sum() <= row_pieces
    lim = limits_vector(limits)
    max_abs = np.zeros((n, 5))
    arg, viol = np.zeros((n, 5), dtype=i32), np.zeros((n, 5), dtype=i32)
    feas, ns = np.zeros(n, dtype=i32), np.zeros(n, dtype=i32)
    samples = np.zeros((n, max(int(max_samples), 1), 8))
    lib().oracle_limits(n, max_seg, row_pieces, n_seg.ctypes.data, singul.ctypes.data, piece_nums.ctypes.data, coeff_dt.ctypes.data,
                        coeffs.ctypes.data, float(check_dt), float(wheel_base), lim.ctypes.data, int(order), max_abs.ctypes.data,
                        arg.ctypes.data, viol.ctypes.data, feas.ctypes.data, int(max_samples), samples.ctypes.data if max_samples else None,
                        ns.ctypes.data)
    return dict(max_abs=max_abs, arg=arg, violated=viol, feasible=feas, n_samples=ns, samples=samples[:, :int(max_samples)])


def check_batch(singuls, piece_nums, coeffs, piece_dt, check_dt, limits, **kw):
    """B trajectories of one layout (singuls / piece_nums [M]), coeffs [B][Ntot][6][2], piece_dt [B][M], as dftpav_batch_coeffs"""
    piece_dt = np.ascontiguousarray(piece_dt, dtype=np.float64)
    B, M = piece_dt.shape
    return check_table(np.full(B, M), np.tile(np.asarray(singuls), (B, 1)), np.tile(np.asarray(piece_nums), (B, 1)), piece_dt, coeffs,
                       check_dt, limits, **kw)
