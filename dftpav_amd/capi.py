"""ctypes binding of libdftpav_hip.so (the C-ABI of include/dftpav_hip.h).

This is the Python host side used by tests and bench.py; the mirror of the
reference's class interface lives in optimizer.py.  The library is built
in-tree by dftpav_amd/csrc/Makefile; if it is missing this module raises — there
is no fallback path.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from .pods import (BatchData, Layout, Params, Surround, c_double_p, c_int_p, c_ll_p, dptr, iptr, llptr)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DFTPAV_LIB") or os.path.join(_HERE, "libdftpav_hip.so")  # DFTPAV_LIB: an experimental build (scripts/build_variant.sh)
_LIB = None

OK = 0
ORDER_DEVICE, ORDER_REFERENCE = 0, 1
E_INVALID, E_MINI_T, E_ONE_PIECE, E_NO_DEVICE, E_HIP, E_UNSUPPORTED, E_COMM = -1, -2, -3, -4, -5, -6, -7
PUBLISH_CHUNK, PUBLISH_MAX_TICKS = 256, 4096   # DFTPAV_PUBLISH_CHUNK, DFTPAV_PUBLISH_MAX_TICKS
CONFLICT_MAX_SAMPLES = 4096   # DFTPAV_CONFLICT_MAX_SAMPLES
RENDER_MAX_VERTS = 64   # DFTPAV_RENDER_MAX_VERTS
# plan_status of dftpav_plan_queries (DFTPAV_PLAN_*); search status (DFTPAV_SEARCH_*)
PLAN_OK, PLAN_NO_PATH, PLAN_TOO_MANY_SEGMENTS, PLAN_LAYOUT_UNSUPPORTED, PLAN_NO_VALID_RESTART, PLAN_ARRIVED = 0, 1, 2, 3, 4, 5
SEARCH_REACH_END, SEARCH_NO_PATH = 2, 3
# columns of dftpav_batch_cost_terms (DFTPAV_TERM_*)
DIST_FAR = 2147483647   # DFTPAV_DIST_FAR
FIELD_UNREACHED = 2147483647   # DFTPAV_FIELD_UNREACHED
TERM_SMOOTH, TERM_TIME, TERM_CORRIDOR, TERM_SURROUND, TERM_FEAS, COST_TERMS = 0, 1, 2, 3, 4, 5

# every symbol include/dftpav_hip.h declares
EXPORTS = [
    "dftpav_default_params", "dftpav_num_vars", "dftpav_num_points", "dftpav_create", "dftpav_destroy",
    "dftpav_last_error", "dftpav_set_surround", "dftpav_batch_create", "dftpav_batch_destroy",
    "dftpav_batch_upload", "dftpav_batch_get_x0", "dftpav_batch_eval", "dftpav_batch_solve_async",
    "dftpav_batch_sync", "dftpav_batch_results", "dftpav_batch_pack_results", "dftpav_batch_records", "dftpav_batch_coeffs", "dftpav_batch_last_solve_ms",
    "dftpav_solve_batch", "dftpav_stream", "dftpav_set_grid_map", "dftpav_corridor_rectangles",
    "dftpav_corridor_last_ms", "dftpav_batch_corridor_from_states", "dftpav_batch_validate",
    "dftpav_fit_surround", "dftpav_get_surround", "dftpav_frontend_resample",
    "dftpav_sample_restarts", "dftpav_batch_corridor_from_hypotheses", "dftpav_batch_sample_states",
    "dftpav_reeds_shepp_shots", "dftpav_mark", "dftpav_marks_elapsed_ms", "dftpav_batch_set_hand_over", "dftpav_batch_solve_chained", "dftpav_batch_finish", "dftpav_wire_size", "dftpav_wire_pack", "dftpav_wire_info", "dftpav_wire_unpack", "dftpav_set_surround_wire",
    "dftpav_batch_trace", "dftpav_batch_get_trace", "dftpav_plan_cycle", "dftpav_plan_cycle_fetch", "dftpav_batch_create_shaped",
    "dftpav_batch_set_order", "dftpav_batch_get_order", "dftpav_batch_trace_range", "dftpav_batch_get_trace_of",
    "dftpav_comm_available", "dftpav_comm_unique_id", "dftpav_comm_create", "dftpav_comm_destroy", "dftpav_comm_share", "dftpav_comm_layout", "dftpav_batch_allgather_results",
    "dftpav_default_search_params", "dftpav_kino_search", "dftpav_debug_search_slots", "dftpav_debug_validation_table",
    "dftpav_default_plan_params", "dftpav_planner_create", "dftpav_planner_destroy", "dftpav_plan_queries", "dftpav_planner_info",
    "dftpav_plan_group_layouts", "dftpav_debug_plan_select",
    "dftpav_planner_install", "dftpav_planner_adopt", "dftpav_planner_set_history", "dftpav_planner_clear", "dftpav_planner_executing",
    "dftpav_planner_padding",
    "dftpav_replan_check", "dftpav_replan_tick", "dftpav_replan_last_ms",
    "dftpav_planner_publish", "dftpav_planner_publisher_state", "dftpav_planner_set_ctrl_history", "dftpav_publish_last_ms",
    "dftpav_default_limits", "dftpav_batch_check_limits", "dftpav_planner_check_limits", "dftpav_planner_set_limit_filter",
    "dftpav_planner_last_limits", "dftpav_limits_last_ms",
    "dftpav_batch_cost_terms", "dftpav_planner_set_penalty_filter", "dftpav_planner_last_cost_terms", "dftpav_debug_penalty_gate",
    "dftpav_grid_distance_field", "dftpav_batch_check_clearance", "dftpav_planner_check_clearance", "dftpav_planner_set_clearance_filter",
    "dftpav_planner_last_clearance", "dftpav_clearance_last_ms",
    "dftpav_default_goal_field_params", "dftpav_set_search_heuristic", "dftpav_grid_goal_field", "dftpav_goal_field_last_ms",
    "dftpav_goal_window", "dftpav_set_search_heuristic_window", "dftpav_grid_goal_field_windowed",
    "dftpav_default_rs_heuristic_params", "dftpav_set_search_rs_heuristic", "dftpav_rs_table", "dftpav_rs_table_last_ms",
    "dftpav_planner_check_conflicts", "dftpav_planner_sample_poses", "dftpav_conflicts_last_ms",
    "dftpav_batch_check_conflicts", "dftpav_batch_sample_poses", "dftpav_batch_conflicts_last_ms",
    "dftpav_planner_set_conflict_filter", "dftpav_planner_set_own_slots", "dftpav_planner_last_conflicts",
    "dftpav_planner_set_joint_selection", "dftpav_planner_last_joint", "dftpav_joint_last_ms", "dftpav_debug_joint_select",
    "dftpav_planner_check_yield", "dftpav_planner_set_conflict_trigger", "dftpav_planner_last_trigger", "dftpav_trigger_last_ms",
    "dftpav_debug_conflict_trigger",
    "dftpav_grid_stamp_poses", "dftpav_planner_stamp_slots", "dftpav_grid_clear_stamps", "dftpav_grid_read_cells", "dftpav_stamp_last_ms",
    "dftpav_grid_render", "dftpav_grid_origin_centred", "dftpav_render_last_ms",
]


def comm_unique_id():
    """the 128-byte id of a new RCCL communicator (ncclGetUniqueId through the C-ABI): rank 0 makes it, the host hands it round"""
    fn = lib().dftpav_comm_unique_id
    fn.argtypes = [C.c_void_p]
    buf = np.zeros(128, dtype=np.uint8)
    rc = fn(buf.ctypes.data_as(C.c_void_p))
    if rc != OK:
        raise DftpavError(rc, "comm_unique_id: RCCL is not loadable")
    return buf


def comm_available():
    """is RCCL loadable behind the C-ABI?  (dftpav_comm_available: dlopen only -- no bootstrap root is started)"""
    fn = lib().dftpav_comm_available
    fn.argtypes = []
    fn.restype = C.c_int
    return bool(fn())


def comm_layout(global_B, nranks, rank):
    """(first, count, block) of dftpav_comm_layout"""
    fn = lib().dftpav_comm_layout
    fn.argtypes = [C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p]
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = fn(int(global_B), int(nranks), int(rank), C.byref(a), C.byref(b), C.byref(c))
    if rc != OK:
        raise DftpavError(rc, "comm_layout")
    return a.value, b.value, c.value


class DftpavError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("dftpav error %d %s" % (code, msg))
        self.code = code


def build(force=False):
    """Compile libdftpav_hip.so for gfx950 (hipcc cross-compiles without a GPU).  Always goes through make: the
    Makefile tracks every source and header, so a stale library cannot pass for a fresh one.  The build is serialised
    with a file lock: several ranks of one job (the gloo / RCCL tests, torchrun) call this at the same moment, and two
    makes rewriting the same objects could leave one of them loading a half-written library."""
    src_dir = os.path.join(_HERE, "csrc")
    if os.environ.get("DFTPAV_LIB"):   # a prebuilt library was named: nothing of the tree is built or cleaned
        return LIB_PATH
    import fcntl
    with open(os.path.join(src_dir, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force:
                subprocess.check_call(["make", "-C", src_dir, "-s", "clean"])
            if os.path.exists("/opt/rocm/bin/hipcc") or not os.path.exists(LIB_PATH):
                subprocess.check_call(["make", "-C", src_dir, "-s"])
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libdftpav_hip.so is not built (run python -c 'import __graft_entry__ as g; g.build()'); "
                              "there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.dftpav_default_params.argtypes = [C.POINTER(Params)]
        L.dftpav_default_params.restype = None
        L.dftpav_num_vars.argtypes = [C.POINTER(Layout)]
        L.dftpav_num_points.argtypes = [C.POINTER(Params), C.POINTER(Layout)]
        L.dftpav_create.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(vp)]
        L.dftpav_destroy.argtypes = [vp]
        L.dftpav_destroy.restype = None
        L.dftpav_last_error.argtypes = [vp]
        L.dftpav_last_error.restype = C.c_char_p
        L.dftpav_set_surround.argtypes = [vp, C.POINTER(Surround)]
        L.dftpav_batch_create.argtypes = [vp, C.POINTER(Layout), C.c_int, C.POINTER(vp)]
        L.dftpav_batch_destroy.argtypes = [vp]
        L.dftpav_batch_destroy.restype = None
        L.dftpav_batch_upload.argtypes = [vp, C.POINTER(BatchData)]
        L.dftpav_batch_get_x0.argtypes = [vp, c_double_p]
        L.dftpav_batch_eval.argtypes = [vp, c_double_p, c_double_p, c_double_p]
        L.dftpav_batch_solve_async.argtypes = [vp]
        L.dftpav_batch_sync.argtypes = [vp]
        L.dftpav_batch_results.argtypes = [vp, c_double_p, c_double_p, c_int_p, c_int_p, c_int_p, c_int_p, c_ll_p,
                                           c_double_p]
        L.dftpav_batch_pack_results.argtypes = [vp, vp]
        L.dftpav_batch_records.argtypes = [vp, vp]
        L.dftpav_batch_coeffs.argtypes = [vp, c_double_p, c_double_p]
        L.dftpav_batch_last_solve_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.dftpav_solve_batch.argtypes = [vp, C.POINTER(Layout), C.c_int, C.POINTER(BatchData), c_double_p,
                                         c_double_p, c_int_p, c_int_p, c_int_p, c_int_p]
        L.dftpav_stream.argtypes = [vp]
        L.dftpav_stream.restype = vp
        for nm in ("params", "layout", "batch_data", "surround"):
            getattr(L, "dftpav_abi_sizeof_" + nm).restype = C.c_int
        _LIB = L
    return _LIB


def default_params():
    p = Params()
    lib().dftpav_default_params(C.byref(p))
    return p


class Limits(C.Structure):
    """dftpav_limits: every limit > 0; +inf switches a test off"""
    _fields_ = [(k, C.c_double) for k in ("max_forward_vel", "max_backward_vel", "max_forward_acc", "max_backward_acc",
                                          "max_forward_cur", "max_backward_cur", "max_latacc", "max_steer")]


class _LimitsOutC(C.Structure):
    _fields_ = [("max_abs", C.c_void_p), ("arg", C.c_void_p), ("violated", C.c_void_p), ("feasible", C.c_void_p)]


class LimitsOut:
    """the caller-allocated arrays of dftpav_limits_out for `shape` rows: max_abs / arg / violated [shape][5] (velocity, longitudinal
    acceleration, lateral acceleration, curvature, steer), feasible [shape]"""

    def __init__(self, *shape):
        self.a = dict(max_abs=np.zeros(shape + (5,)), arg=np.zeros(shape + (5,), dtype=np.int32),
                      violated=np.zeros(shape + (5,), dtype=np.int32), feasible=np.zeros(shape, dtype=np.int32))
        self.c = _LimitsOutC(*[self.a[k].ctypes.data for k in ("max_abs", "arg", "violated", "feasible")])

    def arrays(self):
        return self.a


class PenaltyCaps(C.Structure):
    """dftpav_penalty_caps: the most a solved restart may keep of each penalty sum; +inf: not judged"""
    _fields_ = [("corridor", C.c_double), ("surround", C.c_double), ("feasibility", C.c_double)]

    def __init__(self, corridor=float("inf"), surround=float("inf"), feasibility=float("inf")):
        super().__init__(float(corridor), float(surround), float(feasibility))


class _ClearanceOutC(C.Structure):
    _fields_ = [("min_d2", C.c_void_p), ("arg", C.c_void_p), ("clearance", C.c_void_p)]


class ClearanceOut:
    """the caller-allocated arrays of dftpav_clearance_out for `shape` rows: min_d2 (squared cell distance, DIST_FAR: none), arg (the
    first sample where it is reached, -1: none), clearance (metres, +inf: none)"""

    def __init__(self, *shape):
        self.a = dict(min_d2=np.zeros(shape, dtype=np.int32), arg=np.zeros(shape, dtype=np.int32), clearance=np.zeros(shape))
        self.c = _ClearanceOutC(*[self.a[k].ctypes.data for k in ("min_d2", "arg", "clearance")])

    def arrays(self):
        return self.a


class _ConflictOutC(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("min_sep", "sep_sample", "sep_partner", "conflict_sample", "conflict_partner")]


class ConflictOut:
    """the caller-allocated arrays of dftpav_conflict_out for `shape` rows: min_sep (metres, 0.0: the footprints overlap, +inf: no
    partner inside the broad phase), sep_sample / sep_partner (where and with whom it is reached), conflict_sample /
    conflict_partner (the first sample with a separation <= margin and the partner there); -1: none"""
    KEYS = ("min_sep", "sep_sample", "sep_partner", "conflict_sample", "conflict_partner")

    def __init__(self, *shape):
        self.a = dict(min_sep=np.zeros(shape), **{k: np.zeros(shape, dtype=np.int32) for k in self.KEYS[1:]})
        self.c = _ConflictOutC(*[self.a[k].ctypes.data for k in self.KEYS])

    def arrays(self):
        return self.a


def conflict_args(t0, dt, K, margin=0.0, range=None):
    """the arguments of dftpav_planner_check_conflicts / _sample_poses as the library takes them, (t0, dt, K, margin, range) with
    range = margin when None; what the library would refuse raises DftpavError(E_INVALID) here, before any library call"""
    t0, dt, margin = float(t0), float(dt), float(margin)
    range = margin if range is None else float(range)
    ok = int(K) == K and 1 <= K <= CONFLICT_MAX_SAMPLES and dt > 0.0 and np.isfinite(dt) and np.isfinite(t0)
    ok = ok and margin >= 0.0 and np.isfinite(range) and range >= margin
    if not ok:
        raise DftpavError(E_INVALID, "conflicts: K in [1, %d], dt > 0, t0 finite, margin >= 0, range finite and >= margin" % CONFLICT_MAX_SAMPLES)
    return t0, dt, int(K), margin, range


class _YieldOutC(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("yield", "yield_sample", "yield_partner")]


class YieldOut:
    """the caller-allocated arrays of dftpav_yield_out for `shape` rows: yield (1: the slot gives way), yield_sample / yield_partner
    (the first sample at which it comes within the margin of a slot that precedes it, and that slot); -1: none"""
    KEYS = ("yield", "yield_sample", "yield_partner")

    def __init__(self, *shape):
        self.a = {k: np.zeros(shape, dtype=np.int32) for k in self.KEYS}
        self.c = _YieldOutC(*[self.a[k].ctypes.data for k in self.KEYS])

    def arrays(self):
        return self.a


def yield_args(t_now, t0, dt, K, margin=0.0, range=None):
    """the arguments of dftpav_planner_check_yield as the library takes them, (t_now, t0, dt, K, margin, range) with range = margin
    when None; what the library would refuse raises DftpavError(E_INVALID) here, before any library call"""
    t_now = float(t_now)
    if not np.isfinite(t_now):
        raise DftpavError(E_INVALID, "yield: t_now finite")
    return (t_now,) + conflict_args(t0, dt, K, margin, range)


def candidate_conflict_args(t_start, t0, dt, K, margin=0.0, range=None):
    """the arguments of dftpav_batch_check_conflicts / _sample_poses as the library takes them, (t_start, t0, dt, K, margin, range)
    with range = margin when None; what the library would refuse raises DftpavError(E_INVALID) here, before any library call.  A
    negative margin is legal (nothing conflicts)."""
    t_start, t0, dt, margin = float(t_start), float(t0), float(dt), float(margin)
    range = margin if range is None else float(range)
    ok = int(K) == K and 1 <= K <= CONFLICT_MAX_SAMPLES and dt > 0.0 and np.isfinite(dt) and np.isfinite(t0) and np.isfinite(t_start)
    ok = ok and margin == margin and np.isfinite(range) and range >= margin
    if not ok:
        raise DftpavError(E_INVALID, "candidate conflicts: K in [1, %d], dt > 0, t0 and t_start finite, margin a number, range finite and >= margin"
                          % CONFLICT_MAX_SAMPLES)
    return t_start, t0, dt, int(K), margin, range


class GoalFieldParams(C.Structure):
    """dftpav_goal_field_params: the search heuristic of dftpav_set_search_heuristic"""
    _fields_ = [("enabled", C.c_int), ("inflate_radius", C.c_double), ("scale", C.c_double)]


def default_goal_field_params():
    """dftpav_default_goal_field_params: off, no inflation, scale 1 / sqrt(1.16)"""
    gp = GoalFieldParams()
    fn = lib().dftpav_default_goal_field_params
    fn.argtypes = [C.c_void_p]
    fn.restype = None
    fn(C.byref(gp))
    return gp


def goal_window(size_x, size_y, resolution, origin, start_xy, goal_xy, margin):
    """dftpav_goal_window, pure host code: the window (X0, Y0, WX, WY) in cells of the goal field of a (start, goal) pair on a grid
    of size_x x size_y cells -- the box of the two cells grown by ceil(margin / resolution), clipped to the grid and snapped outwards
    to the field's tiles of 64 x 32 -- or None for a goal outside the grid (no field)"""
    m = GridMap(None, int(size_x), int(size_y), float(resolution), float(origin[0]), float(origin[1]))
    st, go = (C.c_double * 2)(*[float(v) for v in start_xy[:2]]), (C.c_double * 2)(*[float(v) for v in goal_xy[:2]])
    win = (C.c_int * 4)()
    fn = lib().dftpav_goal_window
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    rc = fn(C.byref(m), st, go, float(margin), win)
    if rc < 0:
        raise DftpavError(rc, "goal_window")
    return tuple(int(v) for v in win) if rc else None


class RsHeuristicParams(C.Structure):
    """dftpav_rs_heuristic_params: the Reeds-Shepp term of the search heuristic (dftpav_set_search_rs_heuristic) and its table"""
    _fields_ = [("enabled", C.c_int), ("n_yaw", C.c_int), ("extent", C.c_double), ("cell", C.c_double), ("scale", C.c_double)]


def default_rs_heuristic_params():
    """dftpav_default_rs_heuristic_params: off, 72 headings, 15 m, cells of 0.25 m, scale 1"""
    gp = RsHeuristicParams()
    fn = lib().dftpav_default_rs_heuristic_params
    fn.argtypes = [C.c_void_p]
    fn.restype = None
    fn(C.byref(gp))
    return gp


def _rs_params(enabled, n_yaw, extent, cell, scale):
    gp = default_rs_heuristic_params()
    gp.enabled = int(bool(enabled))
    for k, v in (("n_yaw", n_yaw), ("extent", extent), ("cell", cell), ("scale", scale)):
        if v is not None:
            setattr(gp, k, int(v) if k == "n_yaw" else float(v))
    return gp


def default_limits(params=None):
    """dftpav_default_limits: the parameters' limits (minco_config.pb.txt:83-91); max_steer = +inf"""
    params = params if params is not None else default_params()
    l = Limits()
    fn = lib().dftpav_default_limits
    fn.restype = None
    fn.argtypes = [C.POINTER(Params), C.POINTER(Limits)]
    fn(C.byref(params), C.byref(l))
    return l


class Handle:
    """dftpav_handle: one HIP stream + the optimiser constants (== a PolyTrajOptimizer after setParam)."""

    def __init__(self, params=None, device=0):
        self.params = params if params is not None else default_params()
        self._map_shape = None   # (size_y, size_x) of the installed grid map
        self._h = C.c_void_p()
        rc = lib().dftpav_create(C.byref(self.params), device, C.byref(self._h))
        if rc != OK:
            self._h = None
            raise DftpavError(rc, "dftpav_create (no usable HIP device?)" if rc == E_NO_DEVICE else "dftpav_create")
        self._sur_keep = None

    def _check(self, rc, what):
        if rc != OK:
            msg = lib().dftpav_last_error(self._h)
            raise DftpavError(rc, "%s: %s" % (what, msg.decode() if msg else ""))

    def set_surround(self, surround_set):
        if surround_set is None:
            self._check(lib().dftpav_set_surround(self._h, None), "set_surround")
            self._sur_keep = None
            return
        s = surround_set.c_struct()
        self._check(lib().dftpav_set_surround(self._h, C.byref(s)), "set_surround")
        self._sur_keep = surround_set

    def reeds_shepp_shots(self, from_, to, max_cur=1.0, checkl=0.2, max_samples=512, vertex_res=0.1, check_collision=False):
        """KinoAstar::computeShotTraj / is_shot_sucess on the device for n pose pairs (x, y, yaw): dict(length, type, seg,
        samples [n][max_samples][3], n_samples, collides or None)."""
        f = np.ascontiguousarray(from_, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(to, dtype=np.float64).reshape(-1, 3)
        n = f.shape[0]
        out = dict(length=np.zeros(n), type=np.zeros(n, dtype=np.int32), seg=np.zeros((n, 5)),
                   samples=np.zeros((n, int(max_samples), 3)), n_samples=np.zeros(n, dtype=np.int32),
                   collides=np.zeros(n, dtype=np.int32) if check_collision else None)
        fn = lib().dftpav_reeds_shepp_shots
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double] + [C.c_void_p] * 6
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._check(fn(self._h, ptr(f), ptr(t), n, float(max_cur), float(checkl), int(max_samples), float(vertex_res),
                       ptr(out["length"]), ptr(out["type"]), ptr(out["seg"]), ptr(out["samples"]), ptr(out["n_samples"]),
                       ptr(out["collides"])), "reeds_shepp_shots")
        return out

    def kino_search(self, start_states, end_states, start_ctrl=None, sp=None, max_nodes=512, max_path=4096):
        """getKinoPath (KinoAstar::search with its 2D retry) + getKinoNode up to SampleTraj on the device for n queries on the
        installed grid map: dict(status, shot_success, used_3d, budget_hit, iters, nodes_used, n_nodes, nodes [n][max_nodes][6],
        path_len, paths [n][max_path][3]) -- paths / path_len are what frontend_resample takes."""
        from .pods import SearchOut, SearchParams
        st = np.ascontiguousarray(start_states, dtype=np.float64).reshape(-1, 4)
        en = np.ascontiguousarray(end_states, dtype=np.float64).reshape(-1, 4)
        n = st.shape[0]
        ct = np.ascontiguousarray(start_ctrl if start_ctrl is not None else np.zeros((n, 2)), dtype=np.float64).reshape(-1, 2)
        sp = sp if sp is not None else SearchParams.default()
        out = SearchOut(n, max_nodes, max_path)
        fn = lib().dftpav_kino_search
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self._check(fn(self._h, C.byref(sp), st.ctypes.data_as(C.c_void_p), ct.ctypes.data_as(C.c_void_p),
                       en.ctypes.data_as(C.c_void_p), n, C.byref(out.c)), "kino_search")
        return out.arrays()

    def comm_create(self, nranks, rank, unique_id):
        """ncclCommInitRank on this handle's device, collectively (dftpav_comm_create); unique_id: the 128 bytes of comm_unique_id()
        of rank 0, distributed by the host."""
        fn = lib().dftpav_comm_create
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        buf = np.ascontiguousarray(unique_id, dtype=np.uint8)
        assert buf.size == 128
        self._check(fn(self._h, int(nranks), int(rank), buf.ctypes.data_as(C.c_void_p)), "comm_create")

    def comm_share(self, owner):
        """this handle uses `owner`'s communicator (dftpav_comm_share): one communicator per rank for several streams"""
        fn = lib().dftpav_comm_share
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self._check(fn(self._h, owner._h), "comm_share")

    def comm_destroy(self):
        fn = lib().dftpav_comm_destroy
        fn.argtypes = [C.c_void_p]
        self._check(fn(self._h), "comm_destroy")

    def mark(self, slot=0):
        """Records one of the handle's two marker events on its stream (dftpav_mark)."""
        fn = lib().dftpav_mark
        fn.argtypes = [C.c_void_p, C.c_int]
        self._check(fn(self._h, int(slot)), "mark")

    def elapsed_since(self, other, other_slot=0, slot=1):
        """Device time in ms from marker `other_slot` of handle `other` to marker `slot` of this handle."""
        fn = lib().dftpav_marks_elapsed_ms
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        ms = C.c_float(0.0)
        self._check(fn(other._h, int(other_slot), self._h, int(slot), C.byref(ms)), "marks_elapsed_ms")
        return float(ms.value)

    def set_surround_wire(self, blobs):
        """Installs serialised trajectories (wire_pack) as the moving obstacles; each blob becomes one obstacle."""
        self._sur_keep = None
        fn = lib().dftpav_set_surround_wire
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        S = len(blobs)
        if S == 0:
            self._check(fn(self._h, None, None, 0), "set_surround_wire")
            return
        keep = [C.create_string_buffer(bytes(bl), len(bl)) for bl in blobs]
        ptrs = (C.c_void_p * S)(*[C.cast(k, C.c_void_p) for k in keep])
        sizes = (C.c_size_t * S)(*[len(bl) for bl in blobs])
        self._check(fn(self._h, ptrs, sizes, S), "set_surround_wire")

    def frontend_resample(self, paths, path_len, start_states, end_states, start_ctrl, fparams=None, **caps):
        """getKinoNode (from SampleTraj on) + the resampling of RunMINCOParking on the device; returns the dict of padded
        arrays of pods.FrontendOut."""
        from .pods import FrontendParams, FrontendOut
        P = np.ascontiguousarray(paths, dtype=np.float64)
        n_hyp, max_path = P.shape[0], P.shape[1]
        pl = np.ascontiguousarray(path_len, dtype=np.int32)
        ss = np.ascontiguousarray(start_states, dtype=np.float64)
        es = np.ascontiguousarray(end_states, dtype=np.float64)
        sc_ = np.ascontiguousarray(start_ctrl, dtype=np.float64)
        fp = fparams if fparams is not None else FrontendParams.default()
        out = FrontendOut(n_hyp, **caps)
        fn = lib().dftpav_frontend_resample
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                       C.c_void_p]
        self._check(fn(self._h, C.byref(fp), P.ctypes.data_as(C.c_void_p), pl.ctypes.data_as(C.c_void_p), max_path,
                       ss.ctypes.data_as(C.c_void_p), es.ctypes.data_as(C.c_void_p), sc_.ctypes.data_as(C.c_void_p), n_hyp,
                       C.byref(out.c)), "frontend_resample")
        return out.arrays()

    def sample_restarts(self, inner, durs, n_restarts, sigma=0.3, lo=0.8, hi=1.25, seed=0):
        """Seeded restarts of hypotheses on the device: inner [n_hyp][n_inner], durs [n_hyp][M] ->
        (inner [n_hyp * n_restarts][n_inner], durs [n_hyp * n_restarts][M])."""
        a = np.ascontiguousarray(inner, dtype=np.float64)
        d = np.ascontiguousarray(durs, dtype=np.float64)
        n_hyp, n_inner, M = a.shape[0], a.shape[1], d.shape[1]
        oi = np.zeros((n_hyp * n_restarts, n_inner))
        od = np.zeros((n_hyp * n_restarts, M))
        fn = lib().dftpav_sample_restarts
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                       C.c_ulonglong, C.c_void_p, C.c_void_p]
        self._check(fn(self._h, a.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), n_hyp, n_restarts, n_inner, M,
                       float(sigma), float(lo), float(hi), int(seed), oi.ctypes.data_as(C.c_void_p),
                       od.ctypes.data_as(C.c_void_p)), "sample_restarts")
        return oi, od

    def fit_surround(self, states):
        """ConverSurroundTrajFromPoints + setSurroundTrajs on the device: states [S][n][7] (x, y, angle, velocity,
        acceleration, curvature, time_stamp)."""
        st = np.ascontiguousarray(states, dtype=np.float64)
        S, n = (st.shape[0], st.shape[1]) if st.size else (0, 0)
        fn = lib().dftpav_fit_surround
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        self._check(fn(self._h, st.ctypes.data_as(C.c_void_p), S, n), "fit_surround")
        self._sur_keep = None

    def get_surround(self):
        """The installed moving obstacles as dict(offsets, durations, coeffs [np][12], total, start)."""
        fn = lib().dftpav_get_surround
        fn.argtypes = [C.c_void_p] + [C.c_void_p] * 7
        S, npc = C.c_int(0), C.c_int(0)
        self._check(fn(self._h, C.byref(S), C.byref(npc), None, None, None, None, None), "get_surround")
        out = dict(offsets=np.zeros(S.value + 1, dtype=np.int32), durations=np.zeros(npc.value), coeffs=np.zeros((npc.value, 12)),
                   total=np.zeros(S.value), start=np.zeros(S.value))
        if S.value:
            self._check(fn(self._h, None, None, out["offsets"].ctypes.data_as(C.c_void_p), out["durations"].ctypes.data_as(C.c_void_p),
                           out["coeffs"].ctypes.data_as(C.c_void_p), out["total"].ctypes.data_as(C.c_void_p),
                           out["start"].ctypes.data_as(C.c_void_p)), "get_surround")
        return out

    def set_grid_map(self, grid, resolution, origin):
        """Obstacle map of the corridor generator: uint8 [size_y][size_x], 80 = occupied (dftpav_grid_map)."""
        g = np.ascontiguousarray(grid, dtype=np.uint8)
        m = GridMap(g.ctypes.data_as(C.c_void_p), g.shape[1], g.shape[0], float(resolution), float(origin[0]), float(origin[1]))
        fn = lib().dftpav_set_grid_map
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self._check(fn(self._h, C.byref(m)), "set_grid_map")
        self._map_shape = g.shape

    def corridor_rectangles(self, states):
        """getRectangleConst on the device: states [n][3] (x, y, yaw) -> [n][4][4] columns (n_x, n_y, p_x, p_y)."""
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 3)
        out = np.zeros((st.shape[0], 4, 4), dtype=np.float64)
        fn = lib().dftpav_corridor_rectangles
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self._check(fn(self._h, st.ctypes.data_as(C.c_void_p), st.shape[0], out.ctypes.data_as(C.c_void_p)), "corridor_rectangles")
        return out

    def distance_field(self, fetch=True):
        """dftpav_grid_distance_field: int32 [size_y][size_x], the squared distance in cells of every cell of the installed map to its
        nearest occupied cell (DIST_FAR on a map without one); built on the device when the map changed.  fetch=False: build only"""
        fn = lib().dftpav_grid_distance_field
        fn.argtypes = [C.c_void_p, C.c_void_p]
        if not fetch:
            self._check(fn(self._h, None), "grid_distance_field")
            return None
        if self._map_shape is None:
            raise DftpavError(E_INVALID, "grid_distance_field: no map")
        out = np.zeros(self._map_shape, dtype=np.int32)
        self._check(fn(self._h, out.ctypes.data_as(C.c_void_p)), "grid_distance_field")
        return out

    def clearance_last_ms(self):
        """dftpav_clearance_last_ms: device ms of (the last field build, the last clearance kernel of a check_clearance call)"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        fn = lib().dftpav_clearance_last_ms
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        self._check(fn(self._h, C.byref(a), C.byref(b)), "clearance_last_ms")
        return float(a.value), float(b.value)

    def batch_conflicts_last_ms(self):
        """dftpav_batch_conflicts_last_ms: device ms of (the pose kernel, the pair kernel) of the last Batch.check_conflicts /
        Batch.sample_poses on this handle; 0.0 for what has not run"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        fn = lib().dftpav_batch_conflicts_last_ms
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(fn(self._h, C.byref(a), C.byref(b)), "batch_conflicts_last_ms")
        return float(a.value), float(b.value)

    def joint_last_ms(self):
        """dftpav_joint_last_ms: device ms of (the pose kernels, the pair kernel, the greedy and row kernels) of the last plan() with
        joint selection or debug_joint_select (which runs no pose kernel); 0.0 for what has not run"""
        a, b, c = C.c_float(0.0), C.c_float(0.0), C.c_float(0.0)
        fn = lib().dftpav_joint_last_ms
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(fn(self._h, C.byref(a), C.byref(b), C.byref(c)), "joint_last_ms")
        return float(a.value), float(b.value), float(c.value)

    def trigger_last_ms(self):
        """dftpav_trigger_last_ms: device ms of (the pose kernel, the pair and reduce kernels) of the last check_yield, tick with the
        conflict trigger on or debug_conflict_trigger (which runs no pose kernel); 0.0 for what has not run"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        fn = lib().dftpav_trigger_last_ms
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(fn(self._h, C.byref(a), C.byref(b)), "trigger_last_ms")
        return float(a.value), float(b.value)

    def conflicts_last_ms(self):
        """dftpav_conflicts_last_ms: device ms of (the pose kernel, the pair and reduce kernels) of the last check_conflicts /
        sample_poses call of a planner of this handle; 0.0 for what has not run"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        fn = lib().dftpav_conflicts_last_ms
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        self._check(fn(self._h, C.byref(a), C.byref(b)), "conflicts_last_ms")
        return float(a.value), float(b.value)

    # ---- the stamps: vehicle footprints written into the installed map on the device
    def stamp_poses(self, poses, inflate=0.0):
        """dftpav_grid_stamp_poses: boxes [n][4] = cx, cy, cs, sn (rows of Planner.sample_poses) become occupied cells of the
        working map, the vehicle's box grown by `inflate` on every side"""
        b = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4)
        fn = lib().dftpav_grid_stamp_poses
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double]
        self._check(fn(self._h, b.ctypes.data_as(C.c_void_p), b.shape[0], float(inflate)), "grid_stamp_poses")

    def clear_stamps(self):
        """dftpav_grid_clear_stamps: the working map is the uploaded one again"""
        fn = lib().dftpav_grid_clear_stamps
        fn.argtypes = [C.c_void_p]
        self._check(fn(self._h), "grid_clear_stamps")

    def read_cells(self):
        """dftpav_grid_read_cells: (the working map uint8 [size_y][size_x], the cells that are 80 in it and not in the uploaded map)"""
        if self._map_shape is None:
            raise DftpavError(E_INVALID, "grid_read_cells: no map")
        out, n = np.zeros(self._map_shape, dtype=np.uint8), C.c_int(-1)
        fn = lib().dftpav_grid_read_cells
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(fn(self._h, out.ctypes.data_as(C.c_void_p), C.byref(n)), "grid_read_cells")
        return out, n.value

    def stamp_last_ms(self):
        """dftpav_stamp_last_ms: device ms of (the pose kernel, the box kernel) of the last stamp call; 0.0 for what has not run"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        fn = lib().dftpav_stamp_last_ms
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        self._check(fn(self._h, C.byref(a), C.byref(b)), "stamp_last_ms")
        return float(a.value), float(b.value)

    # ---- the rendered map: the grid map made on the device from an obstacle set
    def render_map(self, size_x, size_y, resolution, origin, background=127, poly_xy=None, poly_off=None, circles=None, points=None):
        """dftpav_grid_render: the map of size_x x size_y cells at `origin`, wiped to `background`, with the polygons (poly_xy [n][2],
        poly_off [n_poly + 1]), circles [n][3] = cx, cy, radius and points [n][2] of the obstacle set as cells of 80, becomes the
        handle's map as set_grid_map would install it"""
        obs = obstacle_set(poly_xy, poly_off, circles, points)
        fn = lib().dftpav_grid_render
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_ubyte, C.c_void_p]
        self._check(fn(self._h, int(size_x), int(size_y), float(resolution), float(origin[0]), float(origin[1]), int(background),
                       C.byref(obs)), "grid_render")
        self._map_shape = (int(size_y), int(size_x))

    def render_last_ms(self):
        """dftpav_render_last_ms: device ms of the kernels of the last render_map"""
        a = C.c_float(0.0)
        fn = lib().dftpav_render_last_ms
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(fn(self._h, C.byref(a)), "render_last_ms")
        return float(a.value)

    def goal_field(self, goals_xy, inflate_radius=0.0, fetch=True):
        """dftpav_grid_goal_field: for goals [n][2] (x, y) on the installed map, (field int32 [n][size_y][size_x], n_reached [n]): the
        cost of the cheapest 8-connected path (5 axial, 7 diagonal) between every cell and the goal's cell round cells within
        inflate_radius of an occupied one; FIELD_UNREACHED where there is none.  fetch=False: build only, n_reached alone"""
        xy = np.ascontiguousarray(goals_xy, dtype=np.float64).reshape(-1, 2)
        n = xy.shape[0]
        fn = lib().dftpav_grid_goal_field
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        reached = np.zeros(n, dtype=np.int32)
        field = np.zeros((n,) + tuple(self._map_shape), dtype=np.int32) if fetch and self._map_shape is not None else None
        self._check(fn(self._h, xy.ctypes.data_as(C.c_void_p), n, float(inflate_radius),
                       field.ctypes.data_as(C.c_void_p) if field is not None else None, reached.ctypes.data_as(C.c_void_p)), "grid_goal_field")
        return (field, reached) if fetch else reached

    def set_search_heuristic(self, enabled=True, inflate_radius=0.0, scale=None):
        """dftpav_set_search_heuristic: kino_search, Planner.plan and Planner.tick search with max(getHeu, the goal field's cost-to-go)
        when enabled; off (the default state of a handle) they do what they do without this call.  scale None: 1 / sqrt(1.16)"""
        gp = default_goal_field_params()
        gp.enabled, gp.inflate_radius = int(bool(enabled)), float(inflate_radius)
        if scale is not None:
            gp.scale = float(scale)
        fn = lib().dftpav_set_search_heuristic
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self._check(fn(self._h, C.byref(gp)), "set_search_heuristic")

    def set_search_heuristic_window(self, margin):
        """dftpav_set_search_heuristic_window: with set_search_heuristic on, every query's goal field is limited to goal_window of its
        own start and goal with this margin in metres; margin < 0 (the default state of a handle): whole-map fields"""
        fn = lib().dftpav_set_search_heuristic_window
        fn.argtypes = [C.c_void_p, C.c_double]
        self._check(fn(self._h, float(margin)), "set_search_heuristic_window")

    def goal_field_windowed(self, starts_xy, goals_xy, inflate_radius=0.0, margin=0.0, fetch=True):
        """dftpav_grid_goal_field_windowed: for starts and goals [n][2] (x, y) on the installed map, (windows int32 [n][4] (X0, Y0, WX,
        WY), a list of n fields int32 [WY][WX], n_reached [n]): goal_field of the map cropped to each pair's window, blocked by the
        whole map's inflation.  A goal outside the grid has the window (0, 0, 0, 0) and a field of shape (0, 0).  fetch=False: build
        only, (windows, n_reached)"""
        st = np.ascontiguousarray(starts_xy, dtype=np.float64).reshape(-1, 2)
        xy = np.ascontiguousarray(goals_xy, dtype=np.float64).reshape(-1, 2)
        if st.shape != xy.shape:
            raise DftpavError(E_INVALID, "goal_field_windowed: as many starts as goals")
        n = xy.shape[0]
        fn = lib().dftpav_grid_goal_field_windowed
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        win, off, reached = np.zeros((n, 4), dtype=np.int32), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
        head = (self._h, st.ctypes.data_as(C.c_void_p), xy.ctypes.data_as(C.c_void_p), n, float(inflate_radius), float(margin),
                win.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p))
        if not fetch:
            self._check(fn(*head, None, reached.ctypes.data_as(C.c_void_p)), "grid_goal_field_windowed")
            return win, reached
        self._check(fn(*head, None, None), "grid_goal_field_windowed")          # the sizes
        sizes = win[:, 2].astype(np.int64) * win[:, 3]
        packed = np.zeros(max(1, int(sizes.sum())), dtype=np.int32)
        self._check(fn(*head, packed.ctypes.data_as(C.c_void_p), reached.ctypes.data_as(C.c_void_p)), "grid_goal_field_windowed")
        fields = [packed[off[q]:off[q] + sizes[q]].reshape(win[q, 3], win[q, 2]) for q in range(n)]
        return win, fields, reached

    def set_search_rs_heuristic(self, enabled=True, n_yaw=None, extent=None, cell=None, scale=None):
        """dftpav_set_search_rs_heuristic: kino_search, Planner.plan and Planner.tick also take the maximum with scale * the
        Reeds-Shepp length to the goal, read from the handle's table, when enabled; off (the default state of a handle) they do what
        they do without this call.  None: the default of dftpav_default_rs_heuristic_params"""
        gp = _rs_params(enabled, n_yaw, extent, cell, scale)
        fn = lib().dftpav_set_search_rs_heuristic
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self._check(fn(self._h, C.byref(gp)), "set_search_rs_heuristic")

    def rs_table(self, max_cur=None, n_yaw=None, extent=None, cell=None, fetch=True):
        """dftpav_rs_table: the Reeds-Shepp cost-to-go table double [n_yaw][n][n] of rho = 1 / max_cur (None: the default search
        parameters' max_frontend_cur) and the given geometry; fetch=False: its shape (n_yaw, n, n) alone, nothing built"""
        gp = _rs_params(False, n_yaw, extent, cell, None)
        if max_cur is None:
            from .pods import SearchParams
            max_cur = SearchParams.default().max_frontend_cur
        fn = lib().dftpav_rs_table
        fn.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        dims = (C.c_int * 3)()
        self._check(fn(self._h, float(max_cur), C.byref(gp), None, dims), "rs_table")
        shape = tuple(int(v) for v in dims)
        if not fetch:
            return shape
        out = np.zeros(shape, dtype=np.float64)
        self._check(fn(self._h, float(max_cur), C.byref(gp), out.ctypes.data_as(C.c_void_p), dims), "rs_table")
        return out

    def rs_table_last_ms(self):
        """dftpav_rs_table_last_ms: (device ms of the handle's last table build, tables built over the handle's life)"""
        ms, nb = C.c_float(0.0), C.c_int(0)
        fn = lib().dftpav_rs_table_last_ms
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        self._check(fn(self._h, C.byref(ms), C.byref(nb)), "rs_table_last_ms")
        return float(ms.value), int(nb.value)

    def goal_field_last_ms(self):
        """dftpav_goal_field_last_ms: device ms of the goal-field builds of the last call that built any"""
        ms = C.c_float(0.0)
        fn = lib().dftpav_goal_field_last_ms
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(fn(self._h, C.byref(ms)), "goal_field_last_ms")
        return float(ms.value)

    def limits_last_ms(self):
        """device time in ms of the last limits kernel of a check_limits call"""
        ms = C.c_float(0.0)
        fn = lib().dftpav_limits_last_ms
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(fn(self._h, C.byref(ms)), "limits_last_ms")
        return float(ms.value)

    def corridor_last_ms(self):
        ms = C.c_float(0.0)
        fn = lib().dftpav_corridor_last_ms
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(fn(self._h, C.byref(ms)), "corridor_last_ms")
        return float(ms.value)

    def close(self):
        if self._h:
            lib().dftpav_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_plan_params():
    """dftpav_default_plan_params: pods.PlanParams filled from the defaults of the stages"""
    from .pods import PlanParams
    pp = PlanParams()
    fn = lib().dftpav_default_plan_params
    fn.argtypes = [C.c_void_p]
    fn.restype = None
    fn(C.byref(pp))
    return pp


def plan_group_layouts(search_status, n_seg, singul, piece_nums):
    """dftpav_plan_group_layouts (host only): per-query tables (singul / piece_nums [Q][max_seg]) ->
    dict(group [Q], group_first [n_groups], plan_status [Q])"""
    st = np.ascontiguousarray(search_status, dtype=np.int32)
    ns = np.ascontiguousarray(n_seg, dtype=np.int32)
    Q = st.shape[0]
    sg = np.ascontiguousarray(singul, dtype=np.int32)
    pn = np.ascontiguousarray(piece_nums, dtype=np.int32)
    assert sg.ndim == 2 and sg.shape[0] == Q and pn.shape == sg.shape and ns.shape == (Q,)
    max_seg = max(1, sg.shape[1])
    group, first, status = np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.int32)
    ng = C.c_int(-1)
    fn = lib().dftpav_plan_group_layouts
    fn.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 8
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = fn(Q, max_seg, ptr(st), ptr(ns), ptr(sg), ptr(pn), ptr(group), ptr(first), C.byref(ng), ptr(status))
    if rc != OK:
        raise DftpavError(rc, "plan_group_layouts")
    return dict(group=group, group_first=first[:ng.value].copy(), plan_status=status)


class Planner:
    """dftpav_planner: a batch of start / goal queries to their plans on a handle's map (dftpav_plan_queries); owns the device work
    buffers and one batch per layout met so far."""

    def __init__(self, handle, max_queries, n_restarts):
        self.handle = handle
        self.max_queries, self.n_restarts = int(max_queries), int(n_restarts)
        self._p = C.c_void_p()
        fn = lib().dftpav_planner_create
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        rc = fn(handle._h if handle is not None else None, self.max_queries, self.n_restarts, C.byref(self._p))
        if rc != OK:
            self._p = None
            raise DftpavError(rc, "planner_create")

    def plan(self, start_states, end_states, start_ctrl=None, pp=None, t_now=0.0):
        """-> the dict of pods.PlanOut: plan_status, the layout found, winner and its final_cost / iters / x / coeffs / coeff_dt per
        query; r_* per (query, restart); search_status / search_iters / search_path_len"""
        from .pods import PlanOut
        st = np.ascontiguousarray(start_states, dtype=np.float64).reshape(-1, 4)
        en = np.ascontiguousarray(end_states, dtype=np.float64).reshape(-1, 4)
        Q = st.shape[0]
        ct = np.ascontiguousarray(start_ctrl if start_ctrl is not None else np.zeros((Q, 2)), dtype=np.float64).reshape(-1, 2)
        pp = pp if pp is not None else default_plan_params()
        out = PlanOut(Q, self.n_restarts, pp.max_seg, pp.max_pieces)
        fn = lib().dftpav_plan_queries
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
        self.handle._check(fn(self._p, C.byref(pp), st.ctypes.data_as(C.c_void_p), ct.ctypes.data_as(C.c_void_p),
                              en.ctypes.data_as(C.c_void_p), Q, float(t_now), C.byref(out.c)), "plan_queries")
        return out.arrays()

    def info(self):
        """dict(n_batches, group_sizes of the last call, stage_ms = device time of its search, resampling, groups, all)"""
        nb, ng = C.c_int(0), C.c_int(0)
        sizes = np.zeros(self.max_queries, dtype=np.int32)
        ms = np.zeros(4, dtype=np.float32)
        fn = lib().dftpav_planner_info
        fn.argtypes = [C.c_void_p] * 5
        self.handle._check(fn(self._p, C.byref(nb), C.byref(ng), sizes.ctypes.data_as(C.c_void_p), ms.ctypes.data_as(C.c_void_p)),
                           "planner_info")
        return dict(n_batches=nb.value, group_sizes=sizes[:ng.value].copy(), stage_ms=ms.astype(np.float64))

    # ---- the replan loop: the executing table (one slot per query of max_queries), its check and the tick
    @staticmethod
    def _ip(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def install(self, slots, n_seg, singul, piece_nums, coeff_dt, coeffs, end_states, t_start=0.0):
        """dftpav_planner_install: plans from host arrays padded as pods.PlanOut (singul / piece_nums / coeff_dt [n][max_seg],
        coeffs [n][max_seg * max_pieces][6][2], end_states [n][4]) become the executing plans of `slots`"""
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        n = sl.shape[0]
        ns = np.ascontiguousarray(n_seg, dtype=np.int32).reshape(n)
        sg = np.ascontiguousarray(singul, dtype=np.int32).reshape(n, -1)
        pn = np.ascontiguousarray(piece_nums, dtype=np.int32).reshape(n, -1)
        dt = np.ascontiguousarray(coeff_dt, dtype=np.float64).reshape(n, -1)
        co = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(n, -1, 6, 2)
        en = np.ascontiguousarray(end_states, dtype=np.float64).reshape(n, 4)
        max_seg = sg.shape[1]
        assert pn.shape == sg.shape == dt.shape and max_seg >= 1 and co.shape[1] % max_seg == 0
        fn = lib().dftpav_planner_install
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_double]
        self.handle._check(fn(self._p, n, self._ip(sl), max_seg, co.shape[1] // max_seg, self._ip(ns), self._ip(sg), self._ip(pn), self._ip(dt),
                              self._ip(co), self._ip(en), float(t_start)), "planner_install")

    def adopt(self, queries, slots, t_start=0.0, pp=None):
        """dftpav_planner_adopt: the winners of the last plan() become the executing plans of `slots`; -> adopted [n] (0: the query
        had no winner, its slot is untouched).  pp is not read (the library knows that plan()'s padding)."""
        q = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        assert q.shape == sl.shape
        ad = np.zeros(q.shape[0], dtype=np.int32)
        fn = lib().dftpav_planner_adopt
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
        self.handle._check(fn(self._p, q.shape[0], self._ip(q), self._ip(sl), float(t_start), self._ip(ad)), "planner_adopt")
        return ad

    def set_history(self, slots, stamps, angles):
        """dftpav_planner_set_history: the previous desired state (time stamp, angle) of the singularity filter of `slots`"""
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        ts = np.ascontiguousarray(stamps, dtype=np.float64).reshape(-1)
        an = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
        assert sl.shape == ts.shape == an.shape
        fn = lib().dftpav_planner_set_history
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, sl.shape[0], self._ip(sl), self._ip(ts), self._ip(an)), "planner_set_history")

    def clear(self, slots):
        """dftpav_planner_clear: empties `slots`"""
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        fn = lib().dftpav_planner_clear
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self.handle._check(fn(self._p, sl.shape[0], self._ip(sl)), "planner_clear")

    def padding(self):
        """dftpav_planner_padding: (max_seg, max_pieces) of the executing table, (0, 0) before it was filled once"""
        ms, mp = C.c_int(0), C.c_int(0)
        fn = lib().dftpav_planner_padding
        fn.argtypes = [C.c_void_p] * 3
        self.handle._check(fn(self._p, C.byref(ms), C.byref(mp)), "planner_padding")
        return ms.value, mp.value

    def executing(self, slot):
        """dftpav_planner_executing: dict(n_seg, singul, piece_nums, coeff_dt, coeffs, duration, start_time, end_time, end_state,
        hist (time stamp, angle), have_hist) of a slot; n_seg 0: empty.  The arrays have the table's padding (padding())."""
        ms, mp = self.padding()
        i32 = np.int32
        a = dict(n_seg=np.zeros(1, i32), singul=np.zeros(ms, i32), piece_nums=np.zeros(ms, i32), coeff_dt=np.zeros(ms),
                 coeffs=np.zeros((ms * mp, 6, 2)), duration=np.zeros(ms), start_time=np.zeros(ms), end_time=np.zeros(ms),
                 end_state=np.zeros(4), hist=np.zeros(2), have_hist=np.zeros(1, i32))
        fn = lib().dftpav_planner_executing
        fn.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 11
        self.handle._check(fn(self._p, int(slot), *[self._ip(a[k]) for k in (
            "n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "duration", "start_time", "end_time", "end_state", "hist", "have_hist")]),
            "planner_executing")
        a["n_seg"], a["have_hist"] = int(a["n_seg"][0]), int(a["have_hist"][0])
        return a

    def _slot_rows(self, a, width):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == (self.max_queries, width), a.shape
        return a

    def check(self, t_now, budget=0.5, end_states=None, ego_states=None, check_dt=0.05, vertex_res=0.1):
        """dftpav_replan_check: completion, CheckReplan and Replan's desired state of every slot at clock t_now -> the dict of
        pods.ReplanOut.  end_states [slots][4] (None: the stored goals), ego_states [slots][6] x, y, angle, v, steer, acc (None)."""
        from .pods import ReplanOut
        en, eg = self._slot_rows(end_states, 4), self._slot_rows(ego_states, 6)
        out = ReplanOut(self.max_queries)
        fn = lib().dftpav_replan_check
        fn.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
        self.handle._check(fn(self._p, float(t_now), float(budget), self._ip(en), self._ip(eg), float(check_dt), float(vertex_res),
                              C.byref(out.c)), "replan_check")
        return out.arrays()

    def tick(self, t_now, budget=0.5, end_states=None, ego_states=None, pp=None):
        """dftpav_replan_tick: the check, then one plan() of the flagged slots from their desired states at t_now + budget, the
        winners adopted into their slots -> dict(check = the dict of pods.ReplanOut, query_slot [n_queries], plan = the dict of
        pods.PlanOut indexed by query)"""
        from .pods import PlanOut, ReplanOut
        en, eg = self._slot_rows(end_states, 4), self._slot_rows(ego_states, 6)
        pp = pp if pp is not None else default_plan_params()
        S = self.max_queries
        chk, po = ReplanOut(S), PlanOut(S, self.n_restarts, pp.max_seg, pp.max_pieces)
        qslot, nq = np.zeros(S, dtype=np.int32), C.c_int(0)
        fn = lib().dftpav_replan_tick
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double] + [C.c_void_p] * 6
        self.handle._check(fn(self._p, C.byref(pp), float(t_now), float(budget), self._ip(en), self._ip(eg), C.byref(chk.c),
                              self._ip(qslot), C.byref(nq), C.byref(po.c)), "replan_tick")
        n = nq.value
        return dict(check=chk.arrays(), query_slot=qslot[:n].copy(), plan={k: v[:n].copy() for k, v in po.arrays().items()})

    def replan_last_ms(self):
        """dftpav_replan_last_ms: (device ms of the last check kernel, of the last tick from its check to its adoption)"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        fn = lib().dftpav_replan_last_ms
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, C.byref(a), C.byref(b)), "replan_last_ms")
        return float(a.value), float(b.value)

    # ---- the publisher: the 100 Hz half of the server's loop (PublishData), K ticks for every slot in one call
    def publish(self, clocks, want_states=True, want_published=True):
        """dftpav_planner_publish: K publisher ticks at `clocks` [K], in order -> dict(states [K][slots][8] = time_stamp, x, y, angle,
        curvature, velocity, acceleration, steer (zero rows where nothing is published), published [K][slots] = 0 / 1 / 2 (the
        angle replaced by the filter)); an output not wanted is None"""
        t = np.ascontiguousarray(clocks, dtype=np.float64).reshape(-1)
        K, S = t.shape[0], self.max_queries
        st = np.zeros((K, S, 8)) if want_states else None
        pb = np.zeros((K, S), dtype=np.int32) if want_published else None
        fn = lib().dftpav_planner_publish
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, K, self._ip(t), self._ip(st), self._ip(pb)), "planner_publish")
        return dict(states=st, published=pb)

    def publisher_state(self, slot):
        """dftpav_planner_publisher_state: dict(exe_index, hist (time stamp, angle), have_hist) of a slot"""
        e, hv = C.c_int(0), C.c_int(0)
        hist = np.zeros(2)
        fn = lib().dftpav_planner_publisher_state
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, int(slot), C.byref(e), self._ip(hist), C.byref(hv)), "planner_publisher_state")
        return dict(exe_index=e.value, hist=hist, have_hist=hv.value)

    def set_ctrl_history(self, slots, stamps, angles):
        """dftpav_planner_set_ctrl_history: the back of the control history (time stamp, angle) of `slots`"""
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        ts = np.ascontiguousarray(stamps, dtype=np.float64).reshape(-1)
        an = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
        assert sl.shape == ts.shape == an.shape
        fn = lib().dftpav_planner_set_ctrl_history
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, sl.shape[0], self._ip(sl), self._ip(ts), self._ip(an)), "planner_set_ctrl_history")

    # ---- solved plans against the kinematic limits
    def check_limits(self, check_dt=0.05, limits=None):
        """dftpav_planner_check_limits: a row per slot of the executing table -> dict(max_abs, arg, violated [slots][5], feasible
        [slots]); empty slots: zero rows, arg -1"""
        limits = limits if limits is not None else default_limits(self.handle.params)
        out = LimitsOut(self.max_queries)
        fn = lib().dftpav_planner_check_limits
        fn.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, float(check_dt), C.byref(limits), C.byref(out.c)), "planner_check_limits")
        return out.arrays()

    def set_limit_filter(self, limits=None, check_dt=0.05):
        """dftpav_planner_set_limit_filter: None switches the filter off (the default)"""
        fn = lib().dftpav_planner_set_limit_filter
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
        self.handle._check(fn(self._p, C.byref(limits) if limits is not None else None, float(check_dt)), "planner_set_limit_filter")

    def last_limits(self, Q):
        """dftpav_planner_last_limits: the rows [Q][R] of the last plan() of Q queries that ran with the filter on"""
        out = LimitsOut(int(Q), self.n_restarts)
        fn = lib().dftpav_planner_last_limits
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, C.byref(out.c)), "planner_last_limits")
        return out.arrays()

    # ---- the residual penalties of solved plans
    def set_penalty_filter(self, caps=None):
        """dftpav_planner_set_penalty_filter: None switches the filter off (the default)"""
        fn = lib().dftpav_planner_set_penalty_filter
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, C.byref(caps) if caps is not None else None), "planner_set_penalty_filter")

    def last_cost_terms(self, Q):
        """dftpav_planner_last_cost_terms: (r_terms [Q][R][5], r_rejected [Q][R]) of the last plan() of Q queries that ran with the
        penalty filter on"""
        terms = np.zeros((int(Q), self.n_restarts, COST_TERMS))
        rej = np.zeros((int(Q), self.n_restarts), dtype=np.int32)
        fn = lib().dftpav_planner_last_cost_terms
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, terms.ctypes.data_as(C.c_void_p), rej.ctypes.data_as(C.c_void_p)), "planner_last_cost_terms")
        return terms, rej

    # ---- solved plans' clearance from the map's occupied cells
    def check_clearance(self, check_dt=0.05):
        """dftpav_planner_check_clearance: a row per slot of the executing table -> dict(min_d2, arg, clearance [slots]); empty slots:
        DIST_FAR, -1, +inf"""
        out = ClearanceOut(self.max_queries)
        fn = lib().dftpav_planner_check_clearance
        fn.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        self.handle._check(fn(self._p, float(check_dt), C.byref(out.c)), "planner_check_clearance")
        return out.arrays()

    def set_clearance_filter(self, min_clearance=None, check_dt=0.05):
        """dftpav_planner_set_clearance_filter: None (or a negative value) switches the filter off (the default)"""
        fn = lib().dftpav_planner_set_clearance_filter
        fn.argtypes = [C.c_void_p, C.c_double, C.c_double]
        self.handle._check(fn(self._p, -1.0 if min_clearance is None else float(min_clearance), float(check_dt)), "planner_set_clearance_filter")

    def last_clearance(self, Q):
        """dftpav_planner_last_clearance: the rows [Q][R] of the last plan() of Q queries that ran with the filter on"""
        out = ClearanceOut(int(Q), self.n_restarts)
        fn = lib().dftpav_planner_last_clearance
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, C.byref(out.c)), "planner_last_clearance")
        return out.arrays()

    # ---- footprint conflicts between the executing plans, slot against slot
    def check_conflicts(self, t0, dt, K, margin=0.0, range=None):
        """dftpav_planner_check_conflicts at the clocks t0 + k dt, k < K: a row per slot -> dict(min_sep, sep_sample, sep_partner,
        conflict_sample, conflict_partner [slots]); a slot that is empty or has no partner inside the broad phase: +inf, -1, -1, -1,
        -1.  range None: margin"""
        t0, dt, K, margin, range = conflict_args(t0, dt, K, margin, range)
        out = ConflictOut(self.max_queries)
        fn = lib().dftpav_planner_check_conflicts
        fn.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p]
        self.handle._check(fn(self._p, t0, dt, K, margin, range, C.byref(out.c)), "planner_check_conflicts")
        return out.arrays()

    def sample_poses(self, t0, dt, K):
        """dftpav_planner_sample_poses: the pose half of check_conflicts alone -> [K][slots][4] = the footprint's centre cx, cy and
        the heading's cosine and sine; NaN rows for empty slots"""
        t0, dt, K, _, _ = conflict_args(t0, dt, K)
        out = np.zeros((K, self.max_queries, 4))
        fn = lib().dftpav_planner_sample_poses
        fn.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p]
        self.handle._check(fn(self._p, t0, dt, K, self._ip(out)), "planner_sample_poses")
        return out

    # ---- the conflict trigger: which of two executing plans that meet gives way
    def check_yield(self, t_now, t0, dt, K, margin=0.0, range=None):
        """dftpav_planner_check_yield at the clocks t0 + k dt, k < K, with the completion test at t_now: a row per slot ->
        dict(yield, yield_sample, yield_partner [slots]); 0, -1, -1 for a slot that is empty or meets nobody that precedes it.
        range None: margin"""
        t_now, t0, dt, K, margin, range = yield_args(t_now, t0, dt, K, margin, range)
        out = YieldOut(self.max_queries)
        fn = lib().dftpav_planner_check_yield
        fn.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p]
        self.handle._check(fn(self._p, t_now, t0, dt, K, margin, range, C.byref(out.c)), "planner_check_yield")
        return out.arrays()

    def set_conflict_trigger(self, margin=None, range=None, dt=0.1, K=50):
        """dftpav_planner_set_conflict_trigger: tick() also replans the slot without precedence of two executing plans that come
        within `margin` of one another at one of the K clocks t_now + budget + k dt; None (or a negative margin) switches the trigger
        off (the default).  range None: margin.  Keep margin at or below the conflict filter's."""
        fn = lib().dftpav_planner_set_conflict_trigger
        fn.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int]
        m = -1.0 if margin is None else float(margin)
        self.handle._check(fn(self._p, m, m if range is None else float(range), float(dt), int(K)), "planner_set_conflict_trigger")

    def last_trigger(self):
        """dftpav_planner_last_trigger: the rows [slots] of the last tick(), if it ran with the conflict trigger on"""
        out = YieldOut(self.max_queries)
        fn = lib().dftpav_planner_last_trigger
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, C.byref(out.c)), "planner_last_trigger")
        return out.arrays()

    # ---- candidate plans against the executing table: the conflict filter
    def set_conflict_filter(self, margin=None, range=None, dt=0.1, K=50):
        """dftpav_planner_set_conflict_filter: a restart that comes within `margin` of an executing plan at one of the K clocks
        t_now + k dt cannot win; None (or a negative margin) switches the filter off (the default).  range None: margin"""
        fn = lib().dftpav_planner_set_conflict_filter
        fn.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int]
        m = -1.0 if margin is None else float(margin)
        self.handle._check(fn(self._p, m, m if range is None else float(range), float(dt), int(K)), "planner_set_conflict_filter")

    def set_own_slots(self, own):
        """dftpav_planner_set_own_slots: per query of the NEXT plan() the slot its plan would replace (-1: none); consumed by that call"""
        ow = np.ascontiguousarray(own, dtype=np.int32).reshape(-1)
        fn = lib().dftpav_planner_set_own_slots
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self.handle._check(fn(self._p, self._ip(ow), ow.shape[0]), "planner_set_own_slots")

    def last_conflicts(self, Q):
        """dftpav_planner_last_conflicts: the rows [Q][R] of the last plan() of Q queries that ran with the conflict filter on"""
        out = ConflictOut(int(Q), self.n_restarts)
        fn = lib().dftpav_planner_last_conflicts
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, C.byref(out.c)), "planner_last_conflicts")
        return out.arrays()

    # ---- joint selection: the candidates of one call against each other
    def set_joint_selection(self, on=True):
        """dftpav_planner_set_joint_selection: with the conflict filter on, the restarts of one plan() are also tested against the
        winners of the queries in front of their own (call order is priority); off by default"""
        fn = lib().dftpav_planner_set_joint_selection
        fn.argtypes = [C.c_void_p, C.c_int]
        self.handle._check(fn(self._p, 1 if on else 0), "planner_set_joint_selection")

    def last_joint(self, Q):
        """dftpav_planner_last_joint: the rows [Q][R] of the last plan() of Q queries that ran with joint selection (the partner
        index is a query index), and blocked [Q][R]"""
        out = ConflictOut(int(Q), self.n_restarts)
        blocked = np.zeros((int(Q), self.n_restarts), dtype=np.int32)
        fn = lib().dftpav_planner_last_joint
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, C.byref(out.c), self._ip(blocked)), "planner_last_joint")
        return dict(out.arrays(), blocked=blocked)

    def stamp_slots(self, t0, dt, K, inflate=0.0, select=None):
        """dftpav_planner_stamp_slots: the footprints of the selected slots (select [slots], 0: not this one; None: every occupied
        slot) at the clocks t0 + k dt, k < K -- the rows of sample_poses -- become occupied cells of the handle's working map"""
        sel = None
        if select is not None:
            sel = np.ascontiguousarray(np.asarray(select) != 0, dtype=np.uint8).reshape(-1)
            if sel.shape[0] != self.max_queries:
                raise DftpavError(E_INVALID, "planner_stamp_slots: select has a byte per slot")
        fn = lib().dftpav_planner_stamp_slots
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double]
        self.handle._check(fn(self._p, self._ip(sel), float(t0), float(dt), int(K), float(inflate)), "planner_stamp_slots")

    def publish_last_ms(self):
        """dftpav_publish_last_ms: device ms of the last publish kernel (0.0 before the first)"""
        a = C.c_float(0.0)
        fn = lib().dftpav_publish_last_ms
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._p, C.byref(a)), "publish_last_ms")
        return float(a.value)

    def close(self):
        if self._p:
            fn = lib().dftpav_planner_destroy
            fn.argtypes = [C.c_void_p]
            fn.restype = None
            fn(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_joint_select(handle, poses, cost, eligible, margin, range=None):
    """dftpav_debug_joint_select: the pair, greedy and row kernels of joint selection on poses [K][Q][R][4] = cx, cy, cs, sn, cost and
    eligible [Q][R] -> dict(winner [Q], blocked [Q][R], min_sep, sep_sample, sep_partner, conflict_sample, conflict_partner [Q][R])"""
    c = np.ascontiguousarray(cost, dtype=np.float64)
    e = np.ascontiguousarray(eligible, dtype=np.int32)
    Q, R = c.shape
    ps = np.ascontiguousarray(poses, dtype=np.float64)
    K = ps.shape[0]
    if ps.shape != (K, Q, R, 4) or e.shape != (Q, R):
        raise DftpavError(E_INVALID, "debug_joint_select: poses [K][Q][R][4], cost and eligible [Q][R]")
    w = np.zeros(Q, dtype=np.int32)
    b = np.zeros((Q, R), dtype=np.int32)
    out = ConflictOut(Q, R)
    fn = lib().dftpav_debug_joint_select
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                   C.c_void_p]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    m = float(margin)
    handle._check(fn(handle._h, Q, R, K, ptr(ps), ptr(c), ptr(e), m, m if range is None else float(range), ptr(w), ptr(b), C.byref(out.c)),
                  "debug_joint_select")
    return dict(out.arrays(), winner=w, blocked=b)


def debug_conflict_trigger(handle, poses, can_yield, margin, range=None):
    """dftpav_debug_conflict_trigger: the pair and reduce kernels of the conflict trigger on poses [K][S][4] = cx, cy, cs, sn (a NaN row
    at k = 0: an empty slot) and can_yield [S] -> dict(yield, yield_sample, yield_partner [S])"""
    ps = np.ascontiguousarray(poses, dtype=np.float64)
    cy = np.ascontiguousarray(can_yield, dtype=np.int32).reshape(-1)
    if ps.ndim != 3 or ps.shape[2] != 4 or ps.shape[1] != cy.shape[0]:
        raise DftpavError(E_INVALID, "debug_conflict_trigger: poses [K][S][4], can_yield [S]")
    K, S = ps.shape[0], ps.shape[1]
    out = YieldOut(S)
    fn = lib().dftpav_debug_conflict_trigger
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
    m = float(margin)
    handle._check(fn(handle._h, S, K, ps.ctypes.data_as(C.c_void_p), cy.ctypes.data_as(C.c_void_p), m, m if range is None else float(range),
                     C.byref(out.c)), "debug_conflict_trigger")
    return out.arrays()


def debug_plan_select(handle, cost, success, collision):
    """dftpav_debug_plan_select: the selection kernel on [n_query][n_restarts] arrays -> winner [n_query]"""
    c = np.ascontiguousarray(cost, dtype=np.float64)
    s = np.ascontiguousarray(success, dtype=np.int32)
    k = np.ascontiguousarray(collision, dtype=np.int32)
    nq, R = c.shape
    w = np.zeros(nq, dtype=np.int32)
    fn = lib().dftpav_debug_plan_select
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    handle._check(fn(handle._h, nq, R, ptr(c), ptr(s), ptr(k), ptr(w)), "debug_plan_select")
    return w


def debug_penalty_gate(handle, terms, caps, flags_in):
    """dftpav_debug_penalty_gate: the gate kernel on terms [n][5] and flags_in [n] -> (flags_out [n], rejected [n])"""
    t = np.ascontiguousarray(terms, dtype=np.float64).reshape(-1, COST_TERMS)
    fi = np.ascontiguousarray(flags_in, dtype=np.int32).reshape(-1)
    n = t.shape[0]
    assert fi.shape[0] == n
    fo, rj = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    fn = lib().dftpav_debug_penalty_gate
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    handle._check(fn(handle._h, n, ptr(t), C.byref(caps), ptr(fi), ptr(fo), ptr(rj)), "debug_penalty_gate")
    return fo, rj


def debug_validation_table(params, check_dt, vertex_res, max_spacings=0):
    """dftpav_debug_validation_table (host only): (return code, sample times [n_t], spacings [n_v]) of the collision re-check's tables;
    the arrays are None unless the code is OK"""
    out = np.zeros(8192)
    n_t, n_v = C.c_int(0), C.c_int(0)
    fn = lib().dftpav_debug_validation_table
    fn.argtypes = [C.POINTER(Params), C.c_double, C.c_double, C.c_int, C.c_void_p, c_int_p, c_int_p]
    rc = fn(C.byref(params), float(check_dt), float(vertex_res), int(max_spacings), out.ctypes.data_as(C.c_void_p), C.byref(n_t), C.byref(n_v))
    if rc != OK:
        return rc, None, None
    return rc, out[:n_t.value].copy(), out[n_t.value:n_t.value + n_v.value].copy()


class ObstacleSet(C.Structure):
    """dftpav_obstacle_set (include/dftpav_hip.h)."""
    _fields_ = [("n_poly", C.c_int), ("poly_off", C.c_void_p), ("poly_xy", C.c_void_p), ("n_circle", C.c_int), ("circles", C.c_void_p),
                ("n_point", C.c_int), ("points", C.c_void_p)]


def obstacle_set(poly_xy=None, poly_off=None, circles=None, points=None):
    """a dftpav_obstacle_set over contiguous copies of the arrays (kept alive by the structure); None: none of that kind"""
    o = ObstacleSet()
    keep = []

    def arr(a, dtype, cols):
        if a is None:
            return None, 0
        a = np.ascontiguousarray(a, dtype=dtype)
        a = a.reshape(-1, cols) if cols else a.reshape(-1)
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p), a.shape[0]

    o.poly_xy, _ = arr(poly_xy, np.float64, 2)
    o.poly_off, n_off = arr(poly_off, np.int32, 0)
    o.n_poly = max(n_off - 1, 0)
    o.circles, o.n_circle = arr(circles, np.float64, 3)
    o.points, o.n_point = arr(points, np.float64, 2)
    o._keep = keep
    return o


def origin_centred(ego_x, ego_y, extent_x, extent_y):
    """dftpav_grid_origin_centred (host only): the origin (x, y) of a grid of that extent in metres centred on the ego vehicle,
    round(ego - extent / 2) as DataRenderer::GetObstacleMap aligns it"""
    out = (C.c_double * 2)()
    fn = lib().dftpav_grid_origin_centred
    fn.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]
    rc = fn(float(ego_x), float(ego_y), float(extent_x), float(extent_y), out)
    if rc != OK:
        raise DftpavError(rc, "grid_origin_centred")
    return float(out[0]), float(out[1])


class GridMap(C.Structure):
    """dftpav_grid_map (include/dftpav_hip.h)."""
    _fields_ = [("cells", C.c_void_p), ("size_x", C.c_int), ("size_y", C.c_int), ("resolution", C.c_double),
                ("origin_x", C.c_double), ("origin_y", C.c_double)]


class Batch:
    """dftpav_batch: B trajectories of one layout, resident in HBM."""

    def __init__(self, handle, layout_spec, B, residency=-1):
        """residency: -1 by B (dftpav_batch_create); 0 / 1 / 2 = one / two / four workgroups per CU (dftpav_batch_create_shaped)"""
        self.handle = handle
        self.layout = layout_spec
        self.B = B
        self.n = layout_spec.n_vars
        self._b = C.c_void_p()
        lay = layout_spec.c_struct()
        if residency < 0:
            rc = lib().dftpav_batch_create(handle._h, C.byref(lay), B, C.byref(self._b))
        else:
            fn = lib().dftpav_batch_create_shaped
            fn.argtypes = [C.c_void_p, C.POINTER(Layout), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
            rc = fn(handle._h, C.byref(lay), B, int(residency), C.byref(self._b))
        if rc != OK:
            self._b = None
            handle._check(rc, "batch_create")

    def set_order(self, order):
        """ORDER_DEVICE (default, the throughput kernels) or ORDER_REFERENCE: every sum in the order PolyTrajOptimizer
        executes it, whole solves bit-equal to OptimizeTrajectory's (dftpav_batch_set_order)."""
        fn = lib().dftpav_batch_set_order
        fn.argtypes = [C.c_void_p, C.c_int]
        self.handle._check(fn(self._b, int(order)), "batch_set_order")

    def upload(self, scen_or_data, with_corridor=True):
        """with_corridor=False: everything but the half-planes (they come from corridor_from_states)."""
        d = scen_or_data.batch_data() if hasattr(scen_or_data, "batch_data") else scen_or_data
        self._keep = scen_or_data
        if not with_corridor:
            d.corridor = None
        rc = lib().dftpav_batch_upload(self._b, C.byref(d))
        self.handle._check(rc, "batch_upload")

    def validate(self, sample_dt=0.05, vertex_res=0.1):
        """Collision re-check of the solved trajectories against the handle's grid map (CheckReplan,
        traj_server_ros.cpp:385-397): returns (collision [B], first_sample [B])."""
        col = np.zeros(self.B, dtype=np.int32)
        first = np.zeros(self.B, dtype=np.int32)
        fn = lib().dftpav_batch_validate
        fn.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._b, float(sample_dt), float(vertex_res), col.ctypes.data_as(C.c_void_p),
                              first.ctypes.data_as(C.c_void_p)), "batch_validate")
        return col, first

    def check_limits(self, check_dt=0.05, limits=None):
        """dftpav_batch_check_limits: the solved trajectories against the kinematic limits over CheckReplan's samples -> dict(max_abs,
        arg, violated [B][5] (velocity, longitudinal / lateral acceleration, curvature, steer), feasible [B])"""
        limits = limits if limits is not None else default_limits(self.handle.params)
        out = LimitsOut(self.B)
        fn = lib().dftpav_batch_check_limits
        fn.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._b, float(check_dt), C.byref(limits), C.byref(out.c)), "batch_check_limits")
        return out.arrays()

    def check_clearance(self, check_dt=0.05):
        """dftpav_batch_check_clearance: how close the outline of each solved trajectory comes to the map's occupied cells over
        CheckReplan's samples -> dict(min_d2, arg, clearance [B])"""
        out = ClearanceOut(self.B)
        fn = lib().dftpav_batch_check_clearance
        fn.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        self.handle._check(fn(self._b, float(check_dt), C.byref(out.c)), "batch_check_clearance")
        return out.arrays()

    def sample_states(self, t0=0.0, sample_dt=0.01, n_samples=None, filter_singularity=True):
        """Trajectory::GetState over the grid t0 + k * sample_dt for every solved trajectory, played back as the
        server does (traj_server_ros.cpp:244-259): returns (states [B][n_samples][8] = time_stamp, x, y, angle,
        curvature, velocity, acceleration, steer; n_valid [B])."""
        if n_samples is None:
            _, dts = self.coeffs()
            total = float(np.max(np.sum(dts * self.layout.piece_nums[None, :], axis=1)))
            n_samples = int(np.ceil((total - t0) / sample_dt)) + 1
        st = np.zeros((self.B, int(n_samples), 8))
        nv = np.zeros(self.B, dtype=np.int32)
        fn = lib().dftpav_batch_sample_states
        fn.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._b, float(t0), float(sample_dt), int(n_samples), int(bool(filter_singularity)),
                              st.ctypes.data_as(C.c_void_p), nv.ctypes.data_as(C.c_void_p)), "batch_sample_states")
        return st, nv

    def corridor_from_states(self, states, n_restarts=1):
        """getRectangleConst for every constraint point, on the device, straight into the solver's layout: states
        [B / n_restarts][Npts][3] (x, y, yaw), the restarts of a hypothesis sharing its corridor; needs Handle.set_grid_map."""
        st = np.ascontiguousarray(states, dtype=np.float64)
        assert st.shape[0] * n_restarts == self.B and st.shape[-1] == 3
        fn = lib().dftpav_batch_corridor_from_hypotheses
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self.handle._check(fn(self._b, st.ctypes.data_as(C.c_void_p), int(n_restarts)), "batch_corridor_from_hypotheses")

    def x0(self):
        x = np.zeros((self.B, self.n))
        self.handle._check(lib().dftpav_batch_get_x0(self._b, dptr(x)), "get_x0")
        return x

    def eval(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.B, self.n)
        f = np.zeros(self.B)
        g = np.zeros((self.B, self.n))
        self.handle._check(lib().dftpav_batch_eval(self._b, dptr(x), dptr(f), dptr(g)), "batch_eval")
        return f, g

    def cost_terms(self, x=None):
        """dftpav_batch_cost_terms (reference order): the cost of eval(x) term by term -> (terms [B][5], seg_terms [B][M][5]);
        x None: at the solution of the last solve"""
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.B, self.n)
        terms = np.zeros((self.B, COST_TERMS))
        seg = np.zeros((self.B, self.layout.M, COST_TERMS))
        fn = lib().dftpav_batch_cost_terms
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        self.handle._check(fn(self._b, ptr(x) if x is not None else None, ptr(terms), ptr(seg)), "batch_cost_terms")
        return terms, seg

    def solve_async(self):
        self.handle._check(lib().dftpav_batch_solve_async(self._b), "solve_async")

    def sync(self):
        self.handle._check(lib().dftpav_batch_sync(self._b), "sync")

    def last_solve_ms(self):
        ms = C.c_float(0)
        self.handle._check(lib().dftpav_batch_last_solve_ms(self._b, C.byref(ms)), "last_solve_ms")
        return ms.value

    def results(self):
        B, n = self.B, self.n
        r = dict(x=np.zeros((B, n)), final_cost=np.zeros(B), status=np.zeros(B, dtype=np.int32),
                 success=np.zeros(B, dtype=np.int32), iters=np.zeros(B, dtype=np.int32),
                 evals=np.zeros(B, dtype=np.int32), hist_sum=np.zeros(B, dtype=np.int64), latency_us=np.zeros(B))
        rc = lib().dftpav_batch_results(self._b, dptr(r["x"]), dptr(r["final_cost"]), iptr(r["status"]),
                                        iptr(r["success"]), iptr(r["iters"]), iptr(r["evals"]), llptr(r["hist_sum"]),
                                        dptr(r["latency_us"]))
        self.handle._check(rc, "results")
        return r

    def solve(self):
        self.solve_async()
        return self.results()

    def solve_chained(self, prev=None):
        """Throughput mode for a stream of equally shaped batches (dftpav_batch_solve_chained): this batch's last
        trajectories stay suspended for the next chained solve, `prev`'s are taken over and finished here."""
        fn = lib().dftpav_batch_solve_chained
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._b, prev._b if prev is not None else None), "solve_chained")

    def set_hand_over(self, hand_over):
        """End game of a scheduled solve (dftpav_batch_set_hand_over): 0 keeps every trajectory in the queue launch."""
        fn = lib().dftpav_batch_set_hand_over
        fn.argtypes = [C.c_void_p, C.c_int]
        self.handle._check(fn(self._b, int(hand_over)), "set_hand_over")

    def finish(self):
        fn = lib().dftpav_batch_finish
        fn.argtypes = [C.c_void_p]
        self.handle._check(fn(self._b), "finish")

    def plan_cycle(self, scen, states, n_restarts=1, check_dt=0.05, vertex_res=0.1, t0=0.0, state_dt=0.01, n_samples=100,
                   filter_singularity=True):
        """dftpav_plan_cycle: upload, corridor from the map, solve, collision re-check and read-out enqueued in one call."""
        d = scen.batch_data() if hasattr(scen, "batch_data") else scen
        st = np.ascontiguousarray(states, dtype=np.float64)
        fn = lib().dftpav_plan_cycle
        fn.argtypes = [C.c_void_p, C.POINTER(BatchData), C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                       C.c_int]
        self._pc_keep = (d, st)
        self._pc_n = int(n_samples)
        self.handle._check(fn(self._b, C.byref(d), st.ctypes.data_as(C.c_void_p), int(n_restarts), float(check_dt), float(vertex_res),
                              float(t0), float(state_dt), int(n_samples), int(bool(filter_singularity))), "plan_cycle")

    def plan_cycle_fetch(self):
        """-> dict(x, final_cost, status, success, iters, collision, first_sample, states [B][n_samples][8], n_valid)"""
        B, n = self.B, self.layout.n_vars
        r = dict(x=np.zeros((B, n)), final_cost=np.zeros(B), status=np.zeros(B, dtype=np.int32), success=np.zeros(B, dtype=np.int32),
                 iters=np.zeros(B, dtype=np.int32), collision=np.zeros(B, dtype=np.int32), first_sample=np.zeros(B, dtype=np.int32),
                 states=np.zeros((B, self._pc_n, 8)), n_valid=np.zeros(B, dtype=np.int32))
        fn = lib().dftpav_plan_cycle_fetch
        fn.argtypes = [C.c_void_p, c_double_p, c_double_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_double_p, c_int_p]
        self.handle._check(fn(self._b, dptr(r["x"]), dptr(r["final_cost"]), iptr(r["status"]), iptr(r["success"]), iptr(r["iters"]),
                              iptr(r["collision"]), iptr(r["first_sample"]), dptr(r["states"]), iptr(r["n_valid"])), "plan_cycle_fetch")
        return r

    def trace(self, traj, max_evals=4096, count=1):
        """Record every evaluation of trajectories traj .. traj + count - 1 during the following solves
        (dftpav_batch_trace_range); max_evals = 0 switches it off."""
        fn = lib().dftpav_batch_trace_range
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        self.handle._check(fn(self._b, int(traj), int(count), int(max_evals)), "batch_trace")
        self._trace_cap, self._trace_first = int(max_evals), int(traj)

    def get_trace(self, traj=None):
        """-> dict(x [E][n], g [E][n], d [E][n], f [E], stp [E], k [E], count [E]) of a traced trajectory (default: the first)"""
        fn = lib().dftpav_batch_get_trace_of
        fn.argtypes = [C.c_void_p, C.c_int, c_double_p, c_int_p]
        n = self.layout.n_vars
        rows = np.zeros((self._trace_cap, 3 * n + 4))
        cnt = C.c_int(0)
        self.handle._check(fn(self._b, self._trace_first if traj is None else int(traj), dptr(rows), C.byref(cnt)), "batch_get_trace")
        r = rows[:cnt.value]
        return dict(x=r[:, :n].copy(), g=r[:, n:2 * n].copy(), d=r[:, 2 * n:3 * n].copy(), f=r[:, 3 * n].copy(),
                    stp=r[:, 3 * n + 1].copy(), k=r[:, 3 * n + 2].astype(np.int64), count=r[:, 3 * n + 3].astype(np.int64))

    def profile(self, enable=True):
        """Debug: switch the in-kernel phase profiler (thread 0 shader-clock deltas) on or off."""
        fn = lib().dftpav_debug_profile
        fn.argtypes = [C.c_void_p, C.c_int, c_ll_p]
        self.handle._check(fn(self._b, int(enable), None), "profile")

    def read_profile(self):
        fn = lib().dftpav_debug_profile
        fn.argtypes = [C.c_void_p, C.c_int, c_ll_p]
        out = np.zeros((self.B, 12), dtype=np.int64)
        self.handle._check(fn(self._b, 1, llptr(out)), "read_profile")
        return out

    def allgather_results(self, global_B, device_ptr):
        """packs this rank's 16-byte records and all-gathers them over RCCL into device memory of nranks * block * 16 bytes
        (dftpav_batch_allgather_results; asynchronous on the handle's stream)"""
        fn = lib().dftpav_batch_allgather_results
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self.handle._check(fn(self._b, int(global_B), C.c_void_p(device_ptr)), "batch_allgather_results")

    def records(self):
        """the 16-byte result records of the last solve, uint8 [B][16] on the host (waits for the solve; one DMA copy)"""
        out = np.zeros((self.B, 16), dtype=np.uint8)
        self.handle._check(lib().dftpav_batch_records(self._b, out.ctypes.data_as(C.c_void_p)), "records")
        return out

    def pack_results(self, device_ptr):
        """16-byte {f64 cost, i32 status, i32 iters} records into device memory (async on the handle's stream)."""
        self.handle._check(lib().dftpav_batch_pack_results(self._b, C.c_void_p(device_ptr)), "pack_results")

    # ---- the batch's trajectories as candidates against a planner's executing table
    def check_conflicts(self, planner, t_start, t0, dt, K, margin=0.0, range=None, own=None):
        """dftpav_batch_check_conflicts: every trajectory, were it adopted at t_start, against the occupied slots of `planner` at the
        clocks t0 + k dt, k < K -> dict(min_sep, sep_sample, sep_partner, conflict_sample, conflict_partner [B]); own [B]: the slot
        each would replace (-1 or None: none), which takes no part.  Nothing within the broad phase: +inf, -1, -1, -1, -1"""
        t_start, t0, dt, K, margin, range = candidate_conflict_args(t_start, t0, dt, K, margin, range)
        ow = None
        if own is not None:
            ow = np.ascontiguousarray(own, dtype=np.int32).reshape(-1)
            if ow.shape[0] != self.B:
                raise DftpavError(E_INVALID, "batch_check_conflicts: own has an entry per trajectory")
        out = ConflictOut(self.B)
        fn = lib().dftpav_batch_check_conflicts
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._b, planner._p, t_start, t0, dt, K, margin, range,
                              ow.ctypes.data_as(C.c_void_p) if ow is not None else None, C.byref(out.c)), "batch_check_conflicts")
        return out.arrays()

    def sample_poses(self, t_start, t0, dt, K):
        """dftpav_batch_sample_poses: the pose half of check_conflicts alone -> [K][B][4] = the footprint's centre cx, cy and the
        heading's cosine and sine of every trajectory started at t_start"""
        t_start, t0, dt, K, _, _ = candidate_conflict_args(t_start, t0, dt, K)
        out = np.zeros((K, self.B, 4))
        fn = lib().dftpav_batch_sample_poses
        fn.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p]
        self.handle._check(fn(self._b, t_start, t0, dt, K, out.ctypes.data_as(C.c_void_p)), "batch_sample_poses")
        return out

    def set_coeffs(self, coeffs, piece_dt):
        """test hook dftpav_debug_batch_set_coeffs: the steps after a solve run on these coefficients [B][Ntot][6][2] and piece
        durations [B][M] instead of a solution's"""
        co = np.ascontiguousarray(coeffs, dtype=np.float64)
        dt = np.ascontiguousarray(piece_dt, dtype=np.float64)
        assert co.shape == (self.B, self.layout.n_pieces, 6, 2) and dt.shape == (self.B, self.layout.M)
        fn = lib().dftpav_debug_batch_set_coeffs
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self.handle._check(fn(self._b, co.ctypes.data_as(C.c_void_p), dt.ctypes.data_as(C.c_void_p)), "debug_batch_set_coeffs")

    def coeffs(self):
        c = np.zeros((self.B, self.layout.n_pieces, 6, 2))
        dt = np.zeros((self.B, self.layout.M))
        self.handle._check(lib().dftpav_batch_coeffs(self._b, dptr(c), dptr(dt)), "coeffs")
        return c, dt

    def close(self):
        if self._b:
            lib().dftpav_batch_destroy(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- serialised trajectories ("DPTJ" v1, include/dftpav_hip.h): pure host code, no device needed
def wire_size(piece_nums):
    pn = np.ascontiguousarray(piece_nums, dtype=np.int32)
    fn = lib().dftpav_wire_size
    fn.restype = C.c_size_t
    fn.argtypes = [C.c_int, C.c_void_p]
    return int(fn(len(pn), pn.ctypes.data_as(C.c_void_p)))


def wire_pack(layout, coeffs, piece_dt, drone_id=0, traj_id=0, start_time=0.0):
    """One trajectory (coeffs [Ntot][6][2], piece_dt [M] as Batch.coeffs returns them per trajectory) -> bytes."""
    co = np.ascontiguousarray(coeffs, dtype=np.float64)
    dt = np.ascontiguousarray(piece_dt, dtype=np.float64)
    assert co.shape == (layout.n_pieces, 6, 2) and dt.shape == (layout.M,)
    cap = wire_size(layout.piece_nums)
    buf = C.create_string_buffer(cap)
    wr = C.c_size_t(0)
    fn = lib().dftpav_wire_pack
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p]
    ls = layout.c_struct()
    rc = fn(C.byref(ls), co.ctypes.data_as(C.c_void_p), dt.ctypes.data_as(C.c_void_p), int(drone_id), int(traj_id),
            float(start_time), buf, cap, C.byref(wr))
    if rc != 0:
        raise DftpavError(rc, "wire_pack")
    return buf.raw[:wr.value]


def wire_unpack(blob):
    """bytes -> dict(drone_id, traj_id, start_time, singuls, piece_nums, seg_start, seg_duration, durations [np],
    coeffs [np][12] in CoefficientMat order x5,y5,...,x0,y0)."""
    blob = bytes(blob)
    did, tid, M, npc = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    st = C.c_double(0.0)
    fi = lib().dftpav_wire_info
    fi.argtypes = [C.c_char_p, C.c_size_t] + [C.c_void_p] * 5
    rc = fi(blob, len(blob), C.byref(did), C.byref(tid), C.byref(st), C.byref(M), C.byref(npc))
    if rc != 0:
        raise DftpavError(rc, "wire_info")
    out = dict(drone_id=did.value, traj_id=tid.value, start_time=st.value, singuls=np.zeros(M.value, dtype=np.int32),
               piece_nums=np.zeros(M.value, dtype=np.int32), seg_start=np.zeros(M.value), seg_duration=np.zeros(M.value),
               durations=np.zeros(npc.value), coeffs=np.zeros((npc.value, 12)))
    fu = lib().dftpav_wire_unpack
    fu.argtypes = [C.c_char_p, C.c_size_t] + [C.c_void_p] * 6
    rc = fu(blob, len(blob), *[out[k].ctypes.data_as(C.c_void_p)
                               for k in ("singuls", "piece_nums", "seg_start", "seg_duration", "durations", "coeffs")])
    if rc != 0:
        raise DftpavError(rc, "wire_unpack")
    return out
