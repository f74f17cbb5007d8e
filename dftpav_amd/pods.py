"""ctypes mirrors of the plain-C PODs declared in include/dftpav_hip.h.

Field order and types must match the header exactly; tests/test_abi.py checks
sizeof/offsets against the compiled library (dftpav_abi_sizeof_*).
"""
import ctypes as C

import numpy as np

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)
c_ll_p = C.POINTER(C.c_longlong)


class Params(C.Structure):
    """dftpav_params (include/dftpav_hip.h) == OptCfg + VehicleParam + lbfgs_parameter_t."""
    _fields_ = [
        ("traj_resolution", C.c_int),
        ("des_traj_resolution", C.c_int),
        ("wei_obs", C.c_double),
        ("wei_surround", C.c_double),
        ("wei_feas", C.c_double),
        ("wei_sqrvar", C.c_double),
        ("wei_time", C.c_double),
        ("surround_clearance", C.c_double),
        ("half_margin", C.c_double),
        ("max_forward_vel", C.c_double),
        ("max_forward_acc", C.c_double),
        ("max_forward_cur", C.c_double),
        ("max_backward_vel", C.c_double),
        ("max_backward_acc", C.c_double),
        ("max_backward_cur", C.c_double),
        ("max_latacc", C.c_double),
        ("max_phidot", C.c_double),
        ("gear_opt", C.c_int),
        ("non_sinv", C.c_double),
        ("mini_T", C.c_double),
        ("fail_cost", C.c_double),
        ("veh_width", C.c_double),
        ("veh_length", C.c_double),
        ("veh_wheel_base", C.c_double),
        ("veh_d_cr", C.c_double),
        ("lbfgs_mem_size", C.c_int),
        ("lbfgs_past", C.c_int),
        ("lbfgs_delta", C.c_double),
        ("lbfgs_g_epsilon", C.c_double),
        ("lbfgs_max_iterations", C.c_int),
        ("lbfgs_max_linesearch", C.c_int),
        ("lbfgs_min_step", C.c_double),
        ("lbfgs_max_step", C.c_double),
        ("lbfgs_f_dec_coeff", C.c_double),
        ("lbfgs_s_curv_coeff", C.c_double),
        ("lbfgs_cautious_factor", C.c_double),
        ("lbfgs_machine_prec", C.c_double),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Surround(C.Structure):
    _fields_ = [
        ("S", C.c_int),
        ("piece_offsets", c_int_p),
        ("durations", c_double_p),
        ("coeffs", c_double_p),
        ("total_duration", c_double_p),
        ("start_time", c_double_p),
    ]


class Layout(C.Structure):
    _fields_ = [
        ("M", C.c_int),
        ("piece_nums", c_int_p),
        ("singuls", c_int_p),
        ("H", C.c_int),
    ]


class BatchData(C.Structure):
    _fields_ = [
        ("ini_states", c_double_p),
        ("fin_states", c_double_p),
        ("inner_pts", c_double_p),
        ("init_Ts", c_double_p),
        ("corridor", c_double_p),
        ("t_now", C.c_double),
        ("help_eps", C.c_double),
    ]


def dptr(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_double_p)


def iptr(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_int_p)


def llptr(a):
    assert a.dtype == np.int64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_ll_p)


class SurroundSet:
    """Owner of the arrays behind a dftpav_surround (keeps numpy buffers alive)."""

    def __init__(self, piece_offsets, durations, coeffs, total_duration, start_time):
        self.piece_offsets = np.ascontiguousarray(piece_offsets, dtype=np.int32)
        self.durations = np.ascontiguousarray(durations, dtype=np.float64)
        self.coeffs = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(-1, 12)
        self.total_duration = np.ascontiguousarray(total_duration, dtype=np.float64)
        self.start_time = np.ascontiguousarray(start_time, dtype=np.float64)
        self.S = len(self.total_duration)
        assert self.piece_offsets.shape == (self.S + 1,)
        assert self.durations.shape[0] == self.piece_offsets[-1] == self.coeffs.shape[0]

    def c_struct(self):
        s = Surround()
        s.S = self.S
        s.piece_offsets = iptr(self.piece_offsets)
        s.durations = dptr(self.durations)
        s.coeffs = dptr(self.coeffs)
        s.total_duration = dptr(self.total_duration)
        s.start_time = dptr(self.start_time)
        return s


class LayoutSpec:
    """Owner of a dftpav_layout."""

    def __init__(self, piece_nums, singuls, H=4):
        self.piece_nums = np.ascontiguousarray(piece_nums, dtype=np.int32)
        self.singuls = np.ascontiguousarray(singuls, dtype=np.int32)
        self.M = len(self.piece_nums)
        self.H = int(H)
        assert self.singuls.shape == (self.M,)

    @property
    def n_vars(self):
        M = self.M
        return int(2 * np.sum(self.piece_nums - 1) + M + 3 * (M - 1))

    @property
    def n_inner(self):
        return int(2 * np.sum(self.piece_nums - 1))

    @property
    def n_pieces(self):
        return int(np.sum(self.piece_nums))

    def n_points(self, K, Kd):
        return int(sum((int(N) - 2) * (K + 1) + 2 * (Kd + 1) for N in self.piece_nums))

    def c_struct(self):
        l = Layout()
        l.M = self.M
        l.piece_nums = iptr(self.piece_nums)
        l.singuls = iptr(self.singuls)
        l.H = self.H
        return l


class FrontendParams(C.Structure):
    """dftpav_frontend_params (include/dftpav_hip.h), defaults of minco_config.pb.txt:66-67,76-80."""
    _fields_ = [("max_forward_vel", C.c_double), ("max_forward_acc", C.c_double), ("max_backward_vel", C.c_double),
                ("max_backward_acc", C.c_double), ("non_siguav", C.c_double), ("wheel_base", C.c_double),
                ("piece_duration", C.c_double), ("traj_res", C.c_int), ("dense_traj_res", C.c_int)]

    @classmethod
    def default(cls, K=16, Kd=32):
        return cls(5.0, 8.0, 2.0, 4.0, 0.2, 2.85, 1.0, K, Kd)


class FrontendOutC(C.Structure):
    _fields_ = [("max_seg", C.c_int), ("max_pieces", C.c_int), ("max_states", C.c_int), ("n_seg", C.c_void_p),
                ("singul", C.c_void_p), ("piece_nums", C.c_void_p), ("piece_dt", C.c_void_p), ("ini_states", C.c_void_p),
                ("fin_states", C.c_void_p), ("inner_pts", C.c_void_p), ("n_states", C.c_void_p), ("states", C.c_void_p)]


class FrontendOut:
    """Owner of the padded output arrays of dftpav_frontend_resample."""

    def __init__(self, n_hyp, max_seg=8, max_pieces=64, max_states=2304):
        self.n_seg = np.zeros(n_hyp, dtype=np.int32)
        self.singul = np.zeros((n_hyp, max_seg), dtype=np.int32)
        self.piece_nums = np.zeros((n_hyp, max_seg), dtype=np.int32)
        self.piece_dt = np.zeros((n_hyp, max_seg))
        self.ini_states = np.zeros((n_hyp, max_seg, 6))
        self.fin_states = np.zeros((n_hyp, max_seg, 6))
        self.inner_pts = np.zeros((n_hyp, max_seg, max_pieces - 1, 2))
        self.n_states = np.zeros((n_hyp, max_seg), dtype=np.int32)
        self.states = np.zeros((n_hyp, max_seg, max_states, 3))
        self.c = FrontendOutC(max_seg, max_pieces, max_states, *[a.ctypes.data for a in (
            self.n_seg, self.singul, self.piece_nums, self.piece_dt, self.ini_states, self.fin_states, self.inner_pts,
            self.n_states, self.states)])

    def arrays(self):
        return dict(n_seg=self.n_seg, singul=self.singul, piece_nums=self.piece_nums, piece_dt=self.piece_dt,
                    ini_states=self.ini_states, fin_states=self.fin_states, inner_pts=self.inner_pts, n_states=self.n_states,
                    states=self.states)


class SearchParams(C.Structure):
    """dftpav_search_params (include/dftpav_hip.h): the map_cfg / opt_cfg values of KinoAstar::init (kino_astar.cpp:372-442),
    defaults of minco_config.pb.txt:13-59,81 and the vehicle of semantics.h with the search's +0.2 m margin."""
    _fields_ = [("map_size_x", C.c_double), ("map_size_y", C.c_double), ("map_resl", C.c_double),
                ("phi_grid_resolution", C.c_double), ("lambda_heu", C.c_double), ("tie_breaker", C.c_double),
                ("allocate_num", C.c_int), ("check_num", C.c_int), ("step_arc", C.c_double), ("max_frontend_cur", C.c_double),
                ("checkl", C.c_double), ("traj_forward_penalty", C.c_double), ("traj_back_penalty", C.c_double),
                ("traj_gear_switch_penalty", C.c_double), ("traj_steer_penalty", C.c_double),
                ("traj_steer_change_penalty", C.c_double), ("veh_width", C.c_double), ("veh_length", C.c_double),
                ("veh_d_cr", C.c_double), ("wheel_base", C.c_double), ("vertex_res", C.c_double), ("max_iters", C.c_int),
                ("use3d", C.c_int), ("retry_2d", C.c_int)]

    @classmethod
    def default(cls):
        return cls(1000.0, 1000.0, 0.3, 0.3, 5.0, 1.0 + 1.0 / 10000, 100000, 5, 0.9, 1.0, 0.2, 1.0, 2.5, 15.0, 0.5, 0.0,
                   1.90 + 0.2, 4.88 + 0.2, 1.015, 2.85, 0.1, 20000, 1, 1)

    def copy(self, **kw):
        c = type(self)()
        C.pointer(c)[0] = self
        for k, v in kw.items():
            setattr(c, k, v)
        return c


class SearchOutC(C.Structure):
    _fields_ = [("max_nodes", C.c_int), ("max_path", C.c_int)] + [(n, C.c_void_p) for n in (
        "status", "shot_success", "used_3d", "budget_hit", "iters", "nodes_used", "n_nodes", "nodes", "path_len", "paths")]


class SearchOut:
    """Owner of the padded output arrays of dftpav_kino_search (and of the oracle's restatement)."""
    INTS = ("status", "shot_success", "used_3d", "budget_hit", "iters", "nodes_used", "n_nodes")

    def __init__(self, n, max_nodes=512, max_path=4096):
        self.a = {k: np.zeros(n, dtype=np.int32) for k in self.INTS}
        self.a["nodes"] = np.zeros((n, max_nodes, 6))
        self.a["path_len"] = np.zeros(n, dtype=np.int32)
        self.a["paths"] = np.zeros((n, max_path, 3))
        self.c = SearchOutC(max_nodes, max_path, *[self.a[k].ctypes.data for k in self.INTS + ("nodes", "path_len", "paths")])

    def arrays(self):
        return dict(self.a)


class PlanParams(C.Structure):
    """dftpav_plan_params (include/dftpav_hip.h): the parameters of every stage of dftpav_plan_queries."""
    _fields_ = [("search", SearchParams), ("frontend", FrontendParams), ("sigma", C.c_double), ("dur_lo", C.c_double),
                ("dur_hi", C.c_double), ("seed", C.c_ulonglong), ("check_dt", C.c_double), ("vertex_res", C.c_double),
                ("max_seg", C.c_int), ("max_pieces", C.c_int), ("max_path", C.c_int)]


MAX_PLAN_VARS = 256             # DFTPAV_PLAN_MAX_VARS


class PlanOutC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "plan_status", "n_seg", "singul", "piece_nums", "piece_dt", "winner", "final_cost", "iters", "x", "coeffs", "coeff_dt",
        "r_final_cost", "r_status", "r_success", "r_iters", "r_evals", "r_collision", "r_first_sample", "search_status",
        "search_iters", "search_path_len")]


class PlanOut:
    """Owner of the output arrays of dftpav_plan_queries: Q queries, R restarts, padded to max_seg / max_pieces."""

    def __init__(self, Q, R, max_seg=8, max_pieces=64):
        i32 = np.int32
        a = dict(plan_status=np.zeros(Q, i32), n_seg=np.zeros(Q, i32), singul=np.zeros((Q, max_seg), i32),
                 piece_nums=np.zeros((Q, max_seg), i32), piece_dt=np.zeros((Q, max_seg)), winner=np.zeros(Q, i32),
                 final_cost=np.zeros(Q), iters=np.zeros(Q, i32), x=np.zeros((Q, MAX_PLAN_VARS)),
                 coeffs=np.zeros((Q, max_seg * max_pieces, 6, 2)), coeff_dt=np.zeros((Q, max_seg)), r_final_cost=np.zeros((Q, R)),
                 r_status=np.zeros((Q, R), i32), r_success=np.zeros((Q, R), i32), r_iters=np.zeros((Q, R), i32),
                 r_evals=np.zeros((Q, R), i32), r_collision=np.zeros((Q, R), i32), r_first_sample=np.zeros((Q, R), i32),
                 search_status=np.zeros(Q, i32), search_iters=np.zeros(Q, i32), search_path_len=np.zeros(Q, i32))
        self.a = a
        self.c = PlanOutC(*[a[n].ctypes.data for n, _ in PlanOutC._fields_])

    def arrays(self):
        return dict(self.a)


class ReplanOutC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "occupied", "complete", "exe_index", "is_close_turnpoint", "is_near", "target_moved", "collision", "first_sample", "replan",
        "desired", "start_state", "start_ctrl")]


class ReplanOut:
    """Owner of the output arrays of dftpav_replan_check (dftpav_replan_out): one row per slot."""
    INTS = ("occupied", "complete", "exe_index", "is_close_turnpoint", "is_near", "target_moved", "collision", "first_sample", "replan")

    def __init__(self, slots):
        a = {k: np.zeros(slots, dtype=np.int32) for k in self.INTS}
        a.update(desired=np.zeros((slots, 8)), start_state=np.zeros((slots, 4)), start_ctrl=np.zeros((slots, 2)))
        self.a = a
        self.c = ReplanOutC(*[a[n].ctypes.data for n, _ in ReplanOutC._fields_])

    def arrays(self):
        return dict(self.a)
