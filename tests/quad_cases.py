"""Shared by the tests of the QUAD shapes (not a test module): scenes with other than four half-planes per point, the layouts of
tests/test_gpu_quadm_instances.py, the plan read-out, and the count of active terms per (piece, point) from the restatement's
coefficients."""
import ctypes as C

import numpy as np

from dftpav_amd import scenarios as sc

KEYS = ("final_cost", "x", "status", "iters", "evals", "hist_sum", "success")


def plan_readout(hiplib, s, p, B=None):
    """what dftpav_debug_reference_plan reports for the scenario (or for B trajectories of its layout) on a 256-CU device under the
    DFTPAV_REF_* variables set now: [supported, kind (0 TEAM, 1 WAVE, 3 QUAD, 5 QUAD for several segments), threads, workgroups per
    CU, persistent workgroups, slice, LDS bytes, width of the sequential sums]"""
    fn = hiplib.lib().dftpav_debug_reference_plan
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 8)()
    assert fn(C.byref(s.layout.c_struct()), C.byref(p), 0, int(B or s.B), 256, out) == 0
    return [int(v) for v in out]


def quadm_instance(s):
    """the instance of ref4m_kernel<FAST, TAIL> a scenario's plan of kind 5 launches: launch_solver_quad picks FAST = (H == 4 &&
    help_eps == 0), reference_order_plan TAIL = 1 when n == 33 and 16 otherwise"""
    return "<%s, %d>" % ("true" if s.layout.H == 4 and s.help_eps == 0.0 else "false", 1 if s.layout.n_vars == 33 else 16)


def extra_planes(base, H):
    """the scenario `base` (H = 4 rectangles) with H half-planes per point: the extra ones are copies of the first ones pulled 0.2 m
    inwards (so that they are the active ones), their normals un-normalised"""
    cor = np.zeros((base.B, base.n_points, H, 4))
    cor[:, :, :4] = base.corridor
    for k in range(4, H):
        cor[:, :, k] = base.corridor[:, :, k % 4]
        cor[:, :, k, 2:] -= (0.2 + 0.05 * (k - 4)) * base.corridor[:, :, k % 4, :2]
        cor[:, :, k, :2] *= 3.0
    lay = type(base.layout)(base.layout.piece_nums, base.layout.singuls, H=H)
    return sc.Scenario("planes_%d" % H, lay, base.K, base.Kd, base.B, base.ini_states, base.fin_states, base.inner_pts, base.init_Ts,
                       np.ascontiguousarray(cor), base.t_now, base.help_eps)


def three_planes(base):
    """the scenario `base` (H = 4 rectangles) without its fourth half-plane: a corridor open on one side"""
    lay = type(base.layout)(base.layout.piece_nums, base.layout.singuls, H=3)
    return sc.Scenario("planes_3", lay, base.K, base.Kd, base.B, base.ini_states, base.fin_states, base.inner_pts, base.init_Ts,
                       np.ascontiguousarray(base.corridor[:, :, :3]), base.t_now, base.help_eps)


def gear_scene(case, B, seed, K=5, Kd=7):
    """`case` = piece counts joined by '-' ("5-4-6"): that many gear segments, forward first, directions alternating"""
    pieces = [int(t) for t in case.split("-")]
    return sc.make_scenario(pieces, [1 if i % 2 == 0 else -1 for i in range(len(pieces))], K, Kd, B, seed=seed, n_obs=30)


def active_terms(oracle, p, s, b, x, order=0):
    """[pieces of the trajectory][Kmax + 1] active terms per (piece, point) of trajectory b at x, from the restatement's coefficients:
    the activation tests of addPVAGradCost2CT (oracle/dftpav_oracle.c: violaPos / violaVel / violaAcc / violaCurL / violaCurR > 0)
    segment by segment -- a segment's own limits (by its singul), its own piece duration dt[segment], its end pieces with Kd points,
    its corridor points counted from the segment's first; and the oracle's (corridor cost, feasibility cost) there."""
    o = oracle.OracleProblem(p, s, b, order=order)
    o.eval(x)
    terms = o.cost_terms()
    c, dt = o.coeffs()
    H = s.layout.H
    K, Kd = p.traj_resolution, p.des_traj_resolution
    W, Lg, dcr = p.veh_width + 2 * p.half_margin, p.veh_length + 2 * p.half_margin, p.veh_d_cr
    le = [(dcr + Lg / 2, W / 2), (dcr + Lg / 2, -W / 2), (dcr - Lg / 2, -W / 2), (dcr - Lg / 2, W / 2), (dcr + Lg / 2, W / 2)]
    cor = np.array(s.corridor[b], dtype=np.float64)
    cor[:, :, :2] /= np.linalg.norm(cor[:, :, :2], axis=2, keepdims=True)
    out = np.zeros((s.layout.n_pieces, max(K, Kd) + 1), dtype=np.int64)
    piece0, pid = 0, -1
    for seg, (N, sg) in enumerate(zip(s.layout.piece_nums, s.layout.singuls)):
        fwd = sg > 0
        vmax, amax, cmax = ((p.max_forward_vel, p.max_forward_acc, p.max_forward_cur) if fwd else
                            (p.max_backward_vel, p.max_backward_acc, p.max_backward_cur))
        for i in range(N):
            ci = c[piece0 + i]
            Ki = Kd if i in (0, N - 1) else K
            step, s1 = dt[seg] / Ki, 0.0
            for j in range(Ki + 1):
                b0 = np.array([1.0, s1, s1 ** 2, s1 ** 3, s1 ** 4, s1 ** 5])
                b1 = np.array([0.0, 1.0, 2 * s1, 3 * s1 ** 2, 4 * s1 ** 3, 5 * s1 ** 4])
                b2 = np.array([0.0, 0.0, 2.0, 6 * s1, 12 * s1 ** 2, 20 * s1 ** 3])
                s1 += step
                pid += 1
                sig, ds, dds = b0 @ ci, b1 @ ci, b2 @ ci
                v = float(np.hypot(ds[0], ds[1]))
                if v < 1e-4 or (i == 0 and j == 0) or (i == N - 1 and j == Ki):
                    continue
                zh1 = float(dds @ ds)
                zh3 = float(dds[1] * ds[0] - dds[0] * ds[1])
                cur = zh3 / (v * v + s.help_eps) ** 1.5
                n = int(v * v - vmax * vmax > 0) + int(zh1 * zh1 / (v * v) - amax * amax > 0) + int(cur - cmax > 0) + int(-cur - cmax > 0)
                R = sg * np.array([[ds[0], -ds[1]], [ds[1], ds[0]]]) / v
                for lx, ly in le:
                    bpt = sig + R @ np.array([lx, ly])
                    for k in range(H):
                        col = cor[pid, k]
                        n += int(col[0] * (bpt[0] - col[2]) + col[1] * (bpt[1] - col[3]) > 0)
                out[piece0 + i, j] = n
        piece0 += N
    return out, (terms[2], terms[4])
