"""ctypes loader of the CPU yardstick of the distance field and the clearance check -- TEST INFRASTRUCTURE (clearance_oracle.cpp).

Only tests/ and scripts/ import this."""
import ctypes as C
import os

import numpy as np

from oracle_shared.loader import Loader


FAR = 2147483647
FIELDS = ("min_d2", "arg", "clearance")
VEH = (1.90, 4.88, 1.015)     # veh_width, veh_length, veh_d_cr of the default parameters


def _declare(L):
    for f in (L.oracle_field, L.oracle_field_brute):
        f.restype = None
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.oracle_clearance.restype = None
    L.oracle_clearance.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_double] * 3 + [C.c_int] * 3 + [C.c_void_p] * 5 + \
        [C.c_double, C.c_void_p, C.c_double, C.c_int] + [C.c_void_p] * 4


_load = Loader(os.path.dirname(os.path.abspath(__file__)), "libclearance_oracle.so",
               ("clearance_oracle.cpp", "../oracle_shared/ref_objects.h", "../oracle/step_trig.h", "../dftpav_amd/csrc/cr_trig.h"), _declare)
build, lib = _load.build, _load.lib


def _field(fn, grid):
    g = np.ascontiguousarray(grid, dtype=np.uint8)
    assert g.ndim == 2
    out = np.zeros(g.shape, dtype=np.int32)
    fn(g.ctypes.data, g.shape[1], g.shape[0], out.ctypes.data)
    return out


def field(grid):
    """uint8 [size_y][size_x], 80 = occupied -> int32 [size_y][size_x] squared cell distance to the nearest occupied cell (FAR: none)"""
    return _field(lib().oracle_field, grid)


def field_brute(grid):
    """the same by the definition: every cell against every occupied cell"""
    return _field(lib().oracle_field_brute, grid)


def check_table(grid, resolution, origin, n_seg, singul, piece_nums, coeff_dt, coeffs, check_dt, veh=VEH, vertex_res=0.1, order=2):
    """n plans padded as the executing table: n_seg [n], singul / piece_nums / coeff_dt [n][max_seg], coeffs [n][row_pieces][6][2].
    -> dict(min_d2, arg, clearance, n_samples [n])"""
    i32 = np.int32
    g = np.ascontiguousarray(grid, dtype=np.uint8)
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
    v = np.array(veh, dtype=np.float64)
    d2, arg, ns = np.zeros(n, dtype=i32), np.zeros(n, dtype=i32), np.zeros(n, dtype=i32)
    m = np.zeros(n)
    lib().oracle_clearance(g.ctypes.data, g.shape[1], g.shape[0], float(resolution), float(origin[0]), float(origin[1]), n, max_seg,
                           row_pieces, n_seg.ctypes.data, singul.ctypes.data, piece_nums.ctypes.data, coeff_dt.ctypes.data,
                           coeffs.ctypes.data, float(check_dt), v.ctypes.data, float(vertex_res), int(order), d2.ctypes.data,
                           arg.ctypes.data, m.ctypes.data, ns.ctypes.data)
    return dict(min_d2=d2, arg=arg, clearance=m, n_samples=ns)


def check_batch(grid, resolution, origin, singuls, piece_nums, coeffs, piece_dt, check_dt, **kw):
    """B trajectories of one layout (singuls / piece_nums [M]), coeffs [B][Ntot][6][2], piece_dt [B][M], as dftpav_batch_coeffs"""
    piece_dt = np.ascontiguousarray(piece_dt, dtype=np.float64)
    B, M = piece_dt.shape
    return check_table(grid, resolution, origin, np.full(B, M), np.tile(np.asarray(singuls), (B, 1)), np.tile(np.asarray(piece_nums), (B, 1)),
                       piece_dt, coeffs, check_dt, **kw)
