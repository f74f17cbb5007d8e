"""The CPU yardstick of the conflict trigger (dftpav_planner_check_yield, the trigger of dftpav_replan_tick) -- TEST INFRASTRUCTURE.

Plain Python, no build step of its own.  Three steps:
  1. the poses are pyconflict.poses(..., order=2) (the debug hook's form takes the caller's poses instead);
  2. the separation of a pair at a sample is pyconflict.sep, the C++ oracle's, which the device matches bit for bit;
  3. the broad phase, can_yield, precedes and the two lexicographic minima are the explicit triple loop of rows() below.
It shares no code with the kernels.  Only tests/ and scripts/ import this."""
import builtins
import math

import numpy as np

from . import pyconflict as pc

FIELDS = ("yield", "yield_sample", "yield_partner")


def check_args(t_now, t0, dt, K, margin=0.0, range=None):
    """what dftpav_planner_check_yield refuses, without a library call: raises ValueError; returns (margin, range) as floats"""
    if not np.isfinite(float(t_now)):
        raise ValueError("t_now must be finite")
    return pc.check_args(t0, dt, K, margin, range)


def end_times(n_seg, piece_nums, coeff_dt, t_start):
    """the end of every slot's last segment as an installation or an adoption at t_start chains the times: per segment d = its piece
    duration summed piece by piece, end_time = start_time + d, the next segment starts at that end -> [n] (0.0 for an empty slot)"""
    n_seg = np.asarray(n_seg, dtype=np.int64).reshape(-1)
    n = n_seg.shape[0]
    pn = np.asarray(piece_nums, dtype=np.int64).reshape(n, -1)
    dtv = np.asarray(coeff_dt, dtype=np.float64).reshape(n, -1)
    ts = np.asarray(t_start, dtype=np.float64).reshape(n)
    out = np.zeros(n)
    for s in range(n):
        world = float(ts[s])
        for e in range(int(n_seg[s])):
            d = 0.0
            for _ in range(int(pn[s, e])):
                d += float(dtv[s, e])
            world = world + d
        out[s] = world if n_seg[s] > 0 else 0.0
    return out


def can_yield(n_seg, end_time, t_now):
    """the slot holds a plan and !(t_now > the end of its last segment)"""
    return [bool(m > 0 and not (float(t_now) > float(e))) for m, e in zip(np.asarray(n_seg).reshape(-1), np.asarray(end_time).reshape(-1))]


def rows(poses, yields, margin, range=None, veh=pc.VEH, occupied=None, stats=None):
    """poses [K][S][4] = cx, cy, cs, sn, yields [S] = can_yield of every slot -> dict(yield, yield_sample, yield_partner [S]).
    occupied [S]: None takes the slots whose row at k = 0 is finite.  stats: a dict that receives `inside` (the ordered pair-samples of
    two occupied slots inside the broad phase) and `narrow` (those of them whose partner precedes the slot)."""
    margin = float(margin)
    rng = margin if range is None else float(range)
    range = builtins.range       # (the argument keeps the entry points' name)
    P = np.ascontiguousarray(poses, dtype=np.float64)
    K, S = P.shape[0], P.shape[1]
    W, L = float(veh[0]), float(veh[1])
    rad = math.sqrt(0.25 * L * L + 0.25 * W * W)
    R = rng + 2.0 * rad
    reach2 = R * R
    if occupied is None:
        occupied = [bool(np.isfinite(P[0, s]).all()) for s in range(S)]
    yl = [bool(y) and bool(o) for y, o in zip(yields, occupied)]
    cx, cy = P[:, :, 0].tolist(), P[:, :, 1].tolist()
    finite = np.isfinite(P).all(axis=2).tolist()
    out = {k: np.full(S, 0 if k == "yield" else -1, dtype=np.int32) for k in FIELDS}
    inside = narrow = 0
    for i in range(S):
        if not occupied[i]:
            continue
        best = None
        for k in range(K):
            if not finite[k][i]:
                continue
            for j in range(S):
                if j == i or not occupied[j] or not finite[k][j]:
                    continue
                dx, dy = cx[k][i] - cx[k][j], cy[k][i] - cy[k][j]
                d2 = dx * dx + dy * dy
                if not (d2 <= reach2):
                    continue
                inside += 1
                precedes = (not yl[j]) or j < i
                if not precedes:
                    continue
                narrow += 1
                if best is None and pc.sep(P[k, i], P[k, j], veh) <= margin:
                    best = (k, j)       # rising (k, j): the first is the lexicographic minimum
        if best is not None:
            out["yield_sample"][i], out["yield_partner"][i] = best
            out["yield"][i] = 1 if yl[i] else 0
    if stats is not None:
        stats["inside"], stats["narrow"] = inside, narrow
    return out


def check_yield(n_seg, singul, piece_nums, coeff_dt, coeffs, t_start, t_now, t0, dt, K, margin=0.0, range=None, veh=pc.VEH, order=2,
                end_time=None, stats=None):
    """dftpav_planner_check_yield of the table (the arguments of pyconflict.poses).  end_time [n]: the ends the table holds (None: chained
    from t_start by end_times)"""
    margin, rng = check_args(t_now, t0, dt, K, margin, range)
    P = pc.poses(n_seg, singul, piece_nums, coeff_dt, coeffs, t_start, t0, dt, K, veh=veh, order=order)
    ns = np.asarray(n_seg).reshape(-1)
    if end_time is None:
        end_time = end_times(ns, piece_nums, coeff_dt, t_start)
    return rows(P, can_yield(ns, end_time, t_now), margin, rng, veh=veh, occupied=[bool(m > 0) for m in ns], stats=stats)
