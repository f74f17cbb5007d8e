"""ctypes loader of the CPU yardstick of the conflict check between executing plans -- TEST INFRASTRUCTURE (conflict_oracle.cpp).

Only tests/ and scripts/ import this."""
import ctypes as C
import os

import numpy as np

from oracle_shared.loader import Loader


FIELDS = ("min_sep", "sep_sample", "sep_partner", "conflict_sample", "conflict_partner")
VEH = (1.90, 4.88, 1.015)     # veh_width, veh_length, veh_d_cr of the default parameters
MAX_SAMPLES = 4096            # DFTPAV_CONFLICT_MAX_SAMPLES


def _declare(L):
    table = [C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_double, C.c_double, C.c_int]
    L.oracle_conflict_poses.restype = None
    L.oracle_conflict_poses.argtypes = table + [C.c_void_p, C.c_int, C.c_void_p]
    L.oracle_conflicts.restype = None
    L.oracle_conflicts.argtypes = table + [C.c_double, C.c_double, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    L.oracle_conflict_sep.restype = C.c_double
    L.oracle_conflict_sep.argtypes = [C.c_void_p] * 3


_load = Loader(os.path.dirname(os.path.abspath(__file__)), "libconflict_oracle.so",
               ("conflict_oracle.cpp", "candidate_oracle.cpp", "../oracle_shared/ref_objects.h", "../oracle/step_trig.h", "../dftpav_amd/csrc/cr_trig.h"), _declare)
build, lib = _load.build, _load.lib


def check_args(t0, dt, K, margin=0.0, range=None):
    """what dftpav_planner_check_conflicts refuses, without a library call: raises ValueError; returns (margin, range) as floats,
    range = margin when None"""
    t0, dt, margin = float(t0), float(dt), float(margin)
    rng = margin if range is None else float(range)
    if int(K) != K or K < 1 or K > MAX_SAMPLES:
        raise ValueError("K must be in [1, %d]" % MAX_SAMPLES)
    if not (dt > 0.0) or not np.isfinite(dt):
        raise ValueError("dt must be positive and finite")
    if not np.isfinite(t0):
        raise ValueError("t0 must be finite")
    if not (margin >= 0.0):
        raise ValueError("margin must be >= 0")
    if not np.isfinite(rng) or rng < margin:
        raise ValueError("range must be finite and >= margin")
    return margin, rng


def _table(n_seg, singul, piece_nums, coeff_dt, coeffs, t_start):
    i32 = np.int32
    n_seg = np.ascontiguousarray(n_seg, dtype=i32).reshape(-1)
    n = n_seg.shape[0]
    singul = np.ascontiguousarray(singul, dtype=i32).reshape(n, -1)
    max_seg = singul.shape[1]
    piece_nums = np.ascontiguousarray(piece_nums, dtype=i32).reshape(n, max_seg)
    coeff_dt = np.ascontiguousarray(coeff_dt, dtype=np.float64).reshape(n, max_seg)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(n, -1, 6, 2)
    t_start = np.ascontiguousarray(t_start, dtype=np.float64).reshape(n)
    row_pieces = coeffs.shape[1]
    for s in range(n):
        assert 0 <= n_seg[s] <= max_seg and piece_nums[s, :n_seg[s]].sum() <= row_pieces
    keep = (n_seg, singul, piece_nums, coeff_dt, coeffs, t_start)
    return keep, [n, max_seg, row_pieces] + [a.ctypes.data for a in keep]


def poses(n_seg, singul, piece_nums, coeff_dt, coeffs, t_start, t0, dt, K, veh=VEH, order=2):
    """n plans padded as the executing table (n_seg / t_start [n], singul / piece_nums / coeff_dt [n][max_seg], coeffs
    [n][row_pieces][6][2]) -> poses [K][n][4] = cx, cy, cs, sn at the clocks t0 + k dt; NaN rows for empty slots"""
    check_args(t0, dt, K)
    keep, args = _table(n_seg, singul, piece_nums, coeff_dt, coeffs, t_start)
    v = np.array(veh, dtype=np.float64)
    out = np.zeros((int(K), args[0], 4))
    lib().oracle_conflict_poses(*args, float(t0), float(dt), int(K), v.ctypes.data, int(order), out.ctypes.data)
    return out


def conflicts(n_seg, singul, piece_nums, coeff_dt, coeffs, t_start, t0, dt, K, margin=0.0, range=None, veh=VEH, order=2):
    """-> dict(min_sep, sep_sample, sep_partner, conflict_sample, conflict_partner [n], examined, inside: the pair-samples of two
    occupied slots, and those of them inside the broad phase)"""
    margin, rng = check_args(t0, dt, K, margin, range)
    keep, args = _table(n_seg, singul, piece_nums, coeff_dt, coeffs, t_start)
    n = args[0]
    v = np.array(veh, dtype=np.float64)
    out = dict(min_sep=np.zeros(n), **{k: np.zeros(n, dtype=np.int32) for k in FIELDS[1:]})
    counts = np.zeros(2, dtype=np.int64)
    lib().oracle_conflicts(*args, float(t0), float(dt), int(K), margin, rng, v.ctypes.data, int(order),
                           *[out[k].ctypes.data for k in FIELDS], counts.ctypes.data)
    out["examined"], out["inside"] = int(counts[0]), int(counts[1])
    return out


def from_executing(rows):
    """the table arguments of poses / conflicts from a list of capi.Planner.executing(slot) dicts"""
    return ([e["n_seg"] for e in rows], [e["singul"] for e in rows], [e["piece_nums"] for e in rows], [e["coeff_dt"] for e in rows],
            np.array([e["coeffs"] for e in rows]), [e["start_time"][0] for e in rows])


def sep(pose_a, pose_b, veh=VEH):
    """the separation of two poses (cx, cy, cs, sn): 0.0 when the boxes overlap"""
    a, b, v = (np.ascontiguousarray(x, dtype=np.float64) for x in (pose_a, pose_b, veh))
    return float(lib().oracle_conflict_sep(a.ctypes.data, b.ctypes.data, v.ctypes.data))
