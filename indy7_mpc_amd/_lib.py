"""ctypes binding of libindy7mpc.so (the C-ABI in include/indy7_mpc.h).

The library is built in-tree by ``__graft_entry__.build()`` into ``indy7_mpc_amd/lib/``.
There is no CPU fallback: if the library or a gfx950 device is missing every entry point
raises :class:`I7MError`.

One HIP runtime per process: torch-ROCm bundles its own ``libamdhip64.so`` (SONAME
``libamdhip64.so.7``, the same SONAME as /opt/rocm's).  If torch is importable we import it
*before* dlopen-ing our library so the dynamic loader binds our NEEDED entry to the runtime
torch already mapped, instead of mapping a second HIP runtime into the process.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
LIB_PATH = os.environ.get("I7M_LIB", os.path.join(LIB_DIR, "libindy7mpc.so"))  # I7M_LIB: A/B builds

ABI_VERSION = 12  # I7M_ABI_VERSION of include/indy7_mpc.h this binding's SIGNATURES follow
NJ, NX, NU = 6, 12, 6
MAX_SQP = 8
MAX_N = 64
LIN_STRIDE, COST_STRIDE = 114, 10

(I7M_K_LIN, I7M_K_RICCATI, I7M_K_LINESEARCH, I7M_K_RICCATI_BOX, I7M_K_IPM, I7M_K_IPM_FUSED, I7M_K_SQP_FUSED,
 I7M_K_LINESEARCH_TAIL, I7M_K_ADMM, I7M_K_ADMM_PREP) = range(10)
I7M_K_COUNT = 10
KERNEL_NAMES = ("k_linearize", "k_riccati", "k_linesearch", "k_riccati_box", "k_ipm", "k_ipm_fused", "k_sqp_fused",
                "k_linesearch_tail", "k_admm_iter", "k_admm_prep")


class I7MError(RuntimeError):
    pass


class i7m_model(C.Structure):
    _fields_ = [
        ("placement_R", (C.c_double * 9) * 6),
        ("placement_t", (C.c_double * 3) * 6),
        ("mass", C.c_double * 6),
        ("com", (C.c_double * 3) * 6),
        ("inertia", (C.c_double * 6) * 6),
        ("gravity", C.c_double * 3),
        ("q_lower", C.c_double * 6),
        ("q_upper", C.c_double * 6),
        ("v_limit", C.c_double * 6),
        ("effort_limit", C.c_double * 6),
    ]


class i7m_config(C.Structure):
    _fields_ = [
        ("N", C.c_int32),
        ("regularize", C.c_int32),
        ("dt", C.c_double),
        ("dQ_cost", C.c_double),
        ("R_cost", C.c_double),
        ("QN_cost", C.c_double),
        ("eps", C.c_double),
        ("mu", C.c_double),
        ("step_tol", C.c_double),
        ("max_sqp_iters", C.c_int32),
        ("max_batch", C.c_int32),
        ("device_id", C.c_int32),
        ("qp_mode", C.c_int32),
        ("model", i7m_model),
        ("box_mask", C.c_int32),
        ("box_max_iters", C.c_int32),
        ("box_tol", C.c_double),
        ("pipeline", C.c_int32),
        ("h2h_chunks", C.c_int32),
        ("admm_rho", C.c_double),
        ("admm_sigma", C.c_double),
        ("admm_alpha", C.c_double),
        ("admm_eps_abs", C.c_double),
        ("admm_eps_rel", C.c_double),
        ("admm_max_iter", C.c_int32),
        ("admm_check_termination", C.c_int32),
        ("admm_scaling", C.c_int32),
        ("admm_check_dualgap", C.c_int32),
        ("admm_adaptive_rho_interval", C.c_int32),
        ("precision", C.c_int32),
        ("admm_adaptive_rho_tolerance", C.c_double),
    ]


QP_DIRECT, QP_BOX, QP_ADMM = 0, 1, 2
PREC_F64, PREC_F32 = 0, 1  # i7m_config.precision (only PREC_F64 is built)
ADMM_RESET_RHO, ADMM_RESET_DUAL, ADMM_RESET_PRIMAL, ADMM_RESET_ALL = 1, 2, 4, 7
# OSQP's settings as i7m_config_default sets them (oracle/osqp_admm.py DEFAULTS)
ADMM_DEFAULTS = dict(rho=0.1, sigma=1e-6, alpha=1.6, eps_abs=1e-3, eps_rel=1e-3, max_iter=4000, check_termination=25,
                     scaling=10, check_dualgap=True, adaptive_rho_interval=0, adaptive_rho_tolerance=5.0)
PIPE_AUTO, PIPE_SPLIT, PIPE_FUSED, PIPE_FUSED_ITER = 0, 1, 2, 3
WRENCH_LOCAL, WRENCH_WORLD = 0, 1
CONTROL_NEW, CONTROL_PREV, CONTROL_POLICY = 0, 1, 2  # i7m_multirate_opts.control_from
_CONTROLS = {"new": CONTROL_NEW, "prev": CONTROL_PREV, "policy": CONTROL_POLICY, CONTROL_NEW: CONTROL_NEW,
             CONTROL_PREV: CONTROL_PREV, CONTROL_POLICY: CONTROL_POLICY}
MULTIRATE_MAX_SUB = 66  # i7m_plan.h
_FRAMES = {"local": WRENCH_LOCAL, "world": WRENCH_WORLD, WRENCH_LOCAL: WRENCH_LOCAL, WRENCH_WORLD: WRENCH_WORLD}
BOX_Q, BOX_V, BOX_U = 1, 2, 4


class i7m_problem_stats(C.Structure):
    _fields_ = [
        ("qp_iters", C.c_int32),
        ("n_alphas", C.c_int32),
        ("n_steps", C.c_int32),
        ("pad", C.c_int32),
        ("alphas", C.c_double * MAX_SQP),
        ("stepsizes", C.c_double * MAX_SQP),
    ]


STATS_DTYPE = np.dtype(
    [("qp_iters", "<i4"), ("n_alphas", "<i4"), ("n_steps", "<i4"), ("pad", "<i4"),
     ("alphas", "<f8", (MAX_SQP,)), ("stepsizes", "<f8", (MAX_SQP,))]
)
assert STATS_DTYPE.itemsize == C.sizeof(i7m_problem_stats)

class i7m_sampled_opts(C.Structure):
    _fields_ = [
        ("sim_dt", C.c_double),
        ("decay", C.c_double),
        ("frame", C.c_int32),
        ("reset_what", C.c_int32),
        ("keep_best", C.c_int32),
        ("n_actual", C.c_int32),
    ]


class i7m_sampled_multirate_opts(C.Structure):
    _fields_ = i7m_sampled_opts._fields_ + [
        ("shift_warm_start", C.c_int32),
        ("control_from", C.c_int32),
    ]


class i7m_multirate_opts(C.Structure):
    _fields_ = [
        ("sim_dt", C.c_double),
        ("goal_radius", C.c_double),
        ("control_from", C.c_int32),
        ("reset_what", C.c_int32),
    ]


_DP = C.POINTER(C.c_double)
_IP32 = C.POINTER(C.c_int32)
_H = C.c_void_p

# (name, restype, argtypes) — every symbol declared in include/indy7_mpc.h
SIGNATURES = [
    ("i7m_last_error", C.c_char_p, []),
    ("i7m_version", C.c_char_p, []),
    ("i7m_abi_version", C.c_int, []),
    ("i7m_config_default", C.c_int, [C.POINTER(i7m_config)]),
    ("i7m_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("i7m_create", C.c_int, [C.POINTER(i7m_config), C.POINTER(_H)]),
    ("i7m_destroy", None, [_H]),
    ("i7m_set_stream", C.c_int, [_H, C.c_void_p]),
    ("i7m_synchronize", C.c_int, [_H]),
    ("i7m_set_external_wrench", C.c_int, [_H, C.c_int32, _DP, C.c_int32]),
    ("i7m_solve", C.c_int, [_H, C.c_int32, _DP, _DP, _DP, C.c_int32, _DP, C.c_void_p]),
    ("i7m_solve_device", C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p]),
    ("i7m_qp", C.c_int, [_H, C.c_int32, _DP, _DP, _DP, C.c_int32, _DP]),
    ("i7m_qp_value", C.c_int, [_H, C.c_int32, _DP, _DP, _DP, C.c_int32, _DP]),
    ("i7m_qp_policy", C.c_int, [_H, C.c_int32, _DP, _DP, _DP, C.c_int32, C.c_int32, _DP, _DP]),
    ("i7m_get_box_stats", C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _DP]),
    ("i7m_admm_reset", C.c_int, [_H, C.c_int32, C.c_int32]),
    ("i7m_get_admm_stats", C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), _DP]),
    ("i7m_get_admm_state", C.c_int, [_H, C.c_int32, _DP, _DP, _DP, _DP, _DP]),
    ("i7m_get_admm_status", C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32)]),
    ("i7m_get_admm_dual", C.c_int, [_H, C.c_int32, _DP]),
    ("i7m_linearize", C.c_int, [_H, C.c_int32, _DP, _DP, C.c_int32, _DP, _DP]),
    ("i7m_merit", C.c_int, [_H, C.c_int32, _DP, _DP, _DP, C.c_int32, _DP]),
    ("i7m_linesearch", C.c_int, [_H, C.c_int32, _DP, _DP, _DP, C.c_int32, _DP]),
    ("i7m_eepos", C.c_int, [_H, C.c_int32, _DP, _DP, _DP]),
    ("i7m_aba", C.c_int, [_H, C.c_int32, _DP, _DP, _DP, _DP, C.c_int32, _DP]),
    ("i7m_aba_derivatives", C.c_int, [_H, C.c_int32, _DP, _DP, _DP, _DP, _DP, _DP, _DP]),
    ("i7m_rk4", C.c_int, [_H, C.c_int32, _DP, _DP, _DP, C.c_double, _DP, C.c_int32, _DP, _DP]),
    ("i7m_mpc_run", C.c_int, [_H, C.c_int32, _DP, _DP, C.c_int32, C.c_int32, _DP, _DP, _DP, _DP]),
    ("i7m_multirate_opts_default", C.c_int, [C.POINTER(i7m_multirate_opts)]),
    ("i7m_multirate_substeps", C.c_int, [C.c_double, C.c_double, C.c_int32, C.c_int32, _IP32]),
    ("i7m_multirate_knots", C.c_int, [C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, _IP32]),
    ("i7m_mpc_run_multirate", C.c_int, [_H, C.c_int32, _DP, _DP, C.c_int32, C.c_int32, C.POINTER(i7m_multirate_opts),
                                        _DP, _DP, _DP, _DP, _DP, _DP]),
    ("i7m_sampled_opts_default", C.c_int, [C.POINTER(i7m_sampled_opts)]),
    ("i7m_mpc_run_sampled", C.c_int, [_H, C.c_int32, C.c_int32, _DP, _DP, C.c_int32, C.c_int32, _DP, _DP, _DP,
                                      C.POINTER(i7m_sampled_opts), _DP, _IP32, _DP, _DP, _DP, _DP, _DP]),
    ("i7m_mpc_run_tracking", C.c_int, [_H, C.c_int32, C.c_int32, _DP, _DP, C.c_int32, C.c_int32, _IP32, _IP32, C.c_int32,
                                       _DP, _DP, _DP, C.POINTER(i7m_sampled_opts), _DP, _IP32, _DP, _DP, _DP, _DP, _DP,
                                       _DP]),
    ("i7m_sampled_multirate_opts_default", C.c_int, [C.POINTER(i7m_sampled_multirate_opts)]),
    ("i7m_mpc_run_sampled_multirate", C.c_int, [_H, C.c_int32, C.c_int32, _DP, _DP, C.c_int32, C.c_int32, _DP, _DP, _DP,
                                                C.POINTER(i7m_sampled_multirate_opts), _DP, _IP32, _DP, _DP, _DP, _DP,
                                                _DP, _DP, _DP]),
    ("i7m_mpc_run_tracking_multirate", C.c_int, [_H, C.c_int32, C.c_int32, _DP, _DP, C.c_int32, C.c_int32, _IP32,
                                                 C.c_int32, _DP, _DP, _DP, C.POINTER(i7m_sampled_multirate_opts), _DP,
                                                 _IP32, _DP, _DP, _DP, _DP, _IP32, _DP, _DP, _DP, _DP]),
    ("i7m_ctrl_begin", C.c_int, [_H, C.c_int32, C.c_int32, _DP, _DP, C.c_int32, C.c_int32, _IP32, _DP,
                                 C.POINTER(i7m_sampled_opts), _DP]),
    ("i7m_ctrl_step", C.c_int, [_H, _DP, C.c_double, C.c_int32, _DP, _DP, _IP32, _DP, _DP, _DP]),
    ("i7m_ctrl_end", C.c_int, [_H, _DP, _DP]),
    ("i7m_ctrl_set_policy", C.c_int, [_H, C.c_int32]),
    ("i7m_ctrl_get_policy", C.c_int, [_H, _DP, _DP]),
    ("i7m_ctrl_set_applied", C.c_int, [_H, _DP]),
    ("i7m_set_timing", C.c_int, [_H, C.c_int]),
    ("i7m_get_kernel_times", C.c_int, [_H, _DP, C.POINTER(C.c_int32), C.c_int32]),
    ("i7m_reset_kernel_times", C.c_int, [_H]),
    ("i7m_reset", C.c_int, [_H]),
]

_lib = None
_lock = threading.Lock()


def load(path: str = LIB_PATH):
    """dlopen libindy7mpc.so (once).  Raises I7MError if it is missing."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise I7MError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        try:  # share torch's HIP runtime if torch is present (see module docstring)
            import torch  # noqa: F401
        except Exception:
            pass
        lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
        for name, res, args in SIGNATURES:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.i7m_abi_version() != ABI_VERSION:
            raise I7MError(f"{path} has C-ABI revision {lib.i7m_abi_version()}, this binding expects {ABI_VERSION}")
        _lib = lib
        return lib


def _check(rc: int):
    if rc != 0:
        msg = _lib.i7m_last_error().decode(errors="replace")
        raise I7MError(f"libindy7mpc error {rc}: {msg}")


def version() -> str:
    """i7m_version(): build kind and the sha256 prefix of the sources it was compiled from
    (__graft_entry__.src_hash)."""
    return load().i7m_version().decode()


def device_count() -> int:
    lib = load()
    n = C.c_int(0)
    rc = lib.i7m_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def _f64(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ptr(a):
    """float64 array, or None for a null pointer"""
    return None if a is None else a.ctypes.data_as(_DP)


def _iptr(a):
    """int32 array, or None"""
    return None if a is None else a.ctypes.data_as(_IP32)


def multirate_schedule(dt, sim_dt, num_steps, N=None, knots=False):
    """The plant's sub-steps of a multi-rate run (i7m_plan.h multirate_schedule, the same double
    arithmetic in the same order: the reference's inner while-loop, src/gato_mpc_batch.py:171-199):
    (sub_start (num_steps + 1,) int32, sub_dt (S,), shift (num_steps,) int32).  Step i owns sub-steps
    [sub_start[i], sub_start[i + 1]) and completes shift[i] knots.  The float residues are kept
    (dt 0.01, sim_dt 0.001: step 9 is [0.001, 8.67e-19]).  ValueError for what the library refuses:
    sim_dt not finite or not positive, more than MULTIRATE_MAX_SUB sub-steps in a step and, with N
    given, a step that completes more than N - 1 knots.  knots=True appends sub_knot (S,) int32
    (i7m_multirate_knots): the knots its step had completed when the sub-step began, the knot whose
    control and gain drive it under control_from="policy"."""
    dt, sim_dt = float(dt), float(sim_dt)
    if not np.isfinite(sim_dt) or not sim_dt > 0.0:
        raise ValueError("sim_dt must be finite and > 0")
    sub_start, sub_dt, shift, sub_knot = [0], [], [], []
    acc = 0.0  # carried over all steps
    for i in range(int(num_steps)):
        rem, sh, n = sim_dt, 0, 0
        while rem > 0.0:
            n += 1
            if n > MULTIRATE_MAX_SUB:
                raise ValueError(f"sim_dt = {sim_dt} needs more than {MULTIRATE_MAX_SUB} plant sub-steps in step {i}")
            ts = min(rem, dt - acc)
            acc += ts
            rem -= ts
            sub_dt.append(ts)
            sub_knot.append(sh)
            if abs(acc - dt) < 1e-10:
                sh += 1
                acc = 0.0
        if N is not None and sh > N - 1:
            raise ValueError(f"sim_dt = {sim_dt} completes more than N - 1 = {N - 1} knots in step {i}")
        shift.append(sh)
        sub_start.append(len(sub_dt))
    out = (np.array(sub_start, dtype=np.int32), np.array(sub_dt, dtype=np.float64), np.array(shift, dtype=np.int32))
    return out + (np.array(sub_knot, dtype=np.int32),) if knots else out


def multirate_knots(dt, sim_dt, N, num_steps, control_from="policy"):
    """i7m_multirate_knots (pure host): the library's knot index per plant sub-step, (S,) int32; raises
    I7MError for what i7m_mpc_run_multirate refuses of sim_dt under that control_from."""
    lib = load()
    n_sub = C.c_int32(0)
    _check(lib.i7m_multirate_substeps(float(dt), float(sim_dt), int(N), int(num_steps), C.byref(n_sub)))
    kn = np.zeros(n_sub.value, dtype=np.int32)
    _check(lib.i7m_multirate_knots(float(dt), float(sim_dt), int(N), int(num_steps), _CONTROLS[control_from], _iptr(kn)))
    return kn


class Handle:
    """One device handle (= one OSQPSolver-like solver state on one GPU)."""

    def __init__(self, model, N=32, dt=0.01, dQ_cost=0.01, R_cost=1e-5, QN_cost=100.0, regularize=True, eps=1.0,
                 max_batch=1, device_id=0, mu=10.0, step_tol=1e-3, max_sqp_iters=2, qp_mode=QP_DIRECT,
                 box_mask=BOX_Q | BOX_V | BOX_U, box_max_iters=30, box_tol=1e-8, pipeline=PIPE_AUTO, h2h_chunks=0,
                 admm=None):
        """admm: OSQP settings for qp_mode=QP_ADMM (keys of ADMM_DEFAULTS; missing keys keep the
        defaults)."""
        lib = load()
        cfg = i7m_config()
        _check(lib.i7m_config_default(C.byref(cfg)))
        cfg.N, cfg.dt, cfg.dQ_cost, cfg.R_cost, cfg.QN_cost = int(N), float(dt), float(dQ_cost), float(R_cost), float(QN_cost)
        cfg.regularize, cfg.eps, cfg.mu, cfg.step_tol = int(bool(regularize)), float(eps), float(mu), float(step_tol)
        cfg.max_sqp_iters, cfg.max_batch, cfg.device_id = int(max_sqp_iters), int(max_batch), int(device_id)
        cfg.qp_mode, cfg.box_mask, cfg.box_max_iters, cfg.box_tol = int(qp_mode), int(box_mask), int(box_max_iters), float(box_tol)
        cfg.pipeline = int(pipeline)
        cfg.h2h_chunks = int(h2h_chunks)
        if admm:
            unknown = set(admm) - set(ADMM_DEFAULTS)
            if unknown:
                raise ValueError(f"unknown ADMM settings {sorted(unknown)}")
            for k, v in admm.items():
                f = "admm_" + k
                setattr(cfg, f, type(getattr(cfg, f))(v) if not isinstance(v, bool) else int(v))
        packed = np.ascontiguousarray(model.packed(), dtype=np.float64)
        assert packed.nbytes == C.sizeof(i7m_model), (packed.nbytes, C.sizeof(i7m_model))
        C.memmove(C.byref(cfg.model), packed.ctypes.data, packed.nbytes)
        h = _H()
        _check(lib.i7m_create(C.byref(cfg), C.byref(h)))
        self._lib, self._h, self.cfg = lib, h, cfg
        self.N, self.T, self.max_batch = int(N), 18 * int(N) - 6, int(max_batch)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.i7m_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- batched entry points (numpy in / numpy out) -------------------------------------
    def _batch(self, xu, goals, xcur=None):
        xu = _f64(xu)
        if xu.ndim == 1:
            xu = xu[None]
        B = xu.shape[0]
        if xu.shape[1] != self.T:
            raise ValueError(f"XU must have {self.T} columns, got {xu.shape[1]}")
        goals = _f64(goals)
        if goals.ndim == 1:
            goals = goals[None]
        if goals.shape[0] != B:
            raise ValueError("goals batch mismatch")
        stride = goals.shape[1] // self.N
        if stride not in (3, 6) or goals.shape[1] != stride * self.N:
            raise ValueError(f"goals must have 3N or 6N columns (N={self.N}), got {goals.shape[1]}")
        out = [xu, goals, B, stride]
        if xcur is not None:
            xc = _f64(xcur)
            if xc.ndim == 1:
                xc = xc[None]
            if xc.shape != (B, NX):
                raise ValueError(f"xcur must be ({B}, 12)")
            out.append(xc)
        return out

    def solve(self, xcur, goals, xu, out=None, stats=None):
        """out / stats: optional preallocated (B, T) float64 / (B,) STATS_DTYPE arrays (e.g. views
        of pinned host memory, which the chunked host-to-host path can copy asynchronously)."""
        xu, goals, B, stride, xc = self._batch(xu, goals, xcur)
        if out is None:
            out = np.empty_like(xu)
        elif out.shape != xu.shape or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array shaped like XU")
        st = np.zeros(B, dtype=STATS_DTYPE) if stats is None else stats
        if st.shape != (B,) or st.dtype != STATS_DTYPE:
            raise ValueError("stats must be a (B,) STATS_DTYPE array")
        _check(self._lib.i7m_solve(self._h, B, _ptr(xu), _ptr(xc), _ptr(goals), stride, _ptr(out),
                                   st.ctypes.data_as(C.c_void_p)))
        return out, st

    def solve_device(self, B, d_xu_in, d_xcur, d_goals, goal_stride, d_xu_out, d_stats=None):
        """Device pointers (ints, e.g. torch ``data_ptr()``); async on the handle's stream."""
        _check(self._lib.i7m_solve_device(self._h, int(B), C.c_void_p(d_xu_in), C.c_void_p(d_xcur),
                                          C.c_void_p(d_goals), int(goal_stride), C.c_void_p(d_xu_out),
                                          C.c_void_p(d_stats) if d_stats else None))

    def qp(self, xu, xcur, goals):
        xu, goals, B, stride, xc = self._batch(xu, goals, xcur)
        sol = np.empty_like(xu)
        _check(self._lib.i7m_qp(self._h, B, _ptr(xu), _ptr(xc), _ptr(goals), stride, _ptr(sol)))
        return sol

    def qp_value(self, xu, xcur, goals):
        """The QP's cost-to-go at the first knot, V~_0 (B, 13, 13) (i7m_qp_value): [[Vxx, vx], [vx', c]]
        in the homogeneous coordinates [x_0; 1], as the Riccati recursion ends with it."""
        xu, goals, B, stride, xc = self._batch(xu, goals, xcur)
        V = np.empty((B, 13, 13))
        _check(self._lib.i7m_qp_value(self._h, B, _ptr(xu), _ptr(xc), _ptr(goals), stride, _ptr(V)))
        return V

    def qp_policy(self, xu, xcur, goals, n_k, want_sol=False):
        """The QP's feedback policy (i7m_qp_policy): K (B, n_k, 6, 13), K[b, k, :, :12] the gain K_k and
        K[b, k, :, 12] the feedforward of the exact QP linearised at xu with x_0 = xcur, whose
        minimiser satisfies u_k = K~_k [x_k; 1].  want_sol: also the minimiser (B, T), i7m_qp's buffer.
        I7M_QP_DIRECT and I7M_QP_ADMM handles (the carried OSQP state is left untouched)."""
        xu, goals, B, stride, xc = self._batch(xu, goals, xcur)
        n_k = int(n_k)
        K = np.empty((B, max(n_k, 0), NU, NX + 1))
        sol = np.empty_like(xu) if want_sol else None
        _check(self._lib.i7m_qp_policy(self._h, B, _ptr(xu), _ptr(xc), _ptr(goals), stride, n_k, _ptr(K), _ptr(sol)))
        return (K, sol) if want_sol else K

    def box_stats(self, B):
        """Interior-point record of the last QP (box mode): (iters, converged, mu), each (B,)."""
        it = np.zeros(B, dtype=np.int32)
        cv = np.zeros(B, dtype=np.int32)
        mu = np.zeros(B)
        ip = C.POINTER(C.c_int32)
        _check(self._lib.i7m_get_box_stats(self._h, int(B), it.ctypes.data_as(ip), cv.ctypes.data_as(ip), _ptr(mu)))
        return it, cv.astype(bool), mu

    def admm_reset(self, B=None, what=ADMM_RESET_ALL):
        """I7M_QP_ADMM: start the OSQP state of problems [0, B) afresh (what: ADMM_RESET_* bits;
        RHO = batch_sqp resetRho, DUAL = resetLambda, ALL = a new OSQP object)."""
        _check(self._lib.i7m_admm_reset(self._h, int(self.max_batch if B is None else B), int(what)))

    def admm_stats(self, B, with_status=False):
        """I7M_QP_ADMM: (OSQP iterations per SQP iteration of the last solve (B, 8), -1 = none;
        rho (B,)); with_status also OSQP's status per SQP iteration (B, 8): 1 solved, 2 solved inaccurate, 0 maximum
        iterations reached, -1 no QP."""
        it = np.zeros((B, MAX_SQP), dtype=np.int32)
        rho = np.zeros(B)
        _check(self._lib.i7m_get_admm_stats(self._h, int(B), it.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(rho)))
        if not with_status:
            return it, rho
        stat = np.zeros((B, MAX_SQP), dtype=np.int32)
        _check(self._lib.i7m_get_admm_status(self._h, int(B), stat.ctypes.data_as(C.POINTER(C.c_int32))))
        return it, rho, stat

    def admm_dual(self, B):
        """I7M_QP_ADMM: each problem's last QP's dual y, unscaled as OSQP returns it (B, 12N)."""
        y = np.empty((B, 12 * self.N))
        _check(self._lib.i7m_get_admm_dual(self._h, int(B), _ptr(y)))
        return y

    def admm_state(self, B):
        """I7M_QP_ADMM: the carried OSQP state (scaled x (B, T), z, y (B, 12N), previous q (B, T),
        rho (B,))."""
        m = 12 * self.N
        x, q = np.empty((B, self.T)), np.empty((B, self.T))
        z, y = np.empty((B, m)), np.empty((B, m))
        rho = np.empty(B)
        _check(self._lib.i7m_get_admm_state(self._h, int(B), _ptr(x), _ptr(z), _ptr(y), _ptr(q), _ptr(rho)))
        return x, z, y, q, rho

    def linearize(self, xu, goals):
        xu, goals, B, stride = self._batch(xu, goals)
        lin = np.empty((B, self.N - 1, LIN_STRIDE))
        cost = np.empty((B, self.N, COST_STRIDE))
        _check(self._lib.i7m_linearize(self._h, B, _ptr(xu), _ptr(goals), stride, _ptr(lin), _ptr(cost)))
        return lin, cost

    def merit(self, xu, xu_ref, goals):
        xu, goals, B, stride = self._batch(xu, goals)
        xr = _f64(xu_ref).reshape(B, self.T)
        out = np.empty((B, 5))
        _check(self._lib.i7m_merit(self._h, B, _ptr(xu), _ptr(xr), _ptr(goals), stride, _ptr(out)))
        return out

    def linesearch(self, xu, xu_full, goals):
        xu, goals, B, stride = self._batch(xu, goals)
        xf = _f64(xu_full).reshape(B, self.T)
        out = np.empty(B)
        _check(self._lib.i7m_linesearch(self._h, B, _ptr(xu), _ptr(xf), _ptr(goals), stride, _ptr(out)))
        return out

    # ---- query hooks ---------------------------------------------------------------------
    def eepos(self, q, jacobian=False):
        q = _f64(q).reshape(-1, NJ)
        n = q.shape[0]
        p = np.empty((n, 3))
        J = np.empty((n, 3, NJ)) if jacobian else None
        _check(self._lib.i7m_eepos(self._h, n, _ptr(q), _ptr(p), _ptr(J)))
        return (p, J) if jacobian else p

    def aba(self, q, v, tau, fext=None, frame="local"):
        """fext (n, 6) joint-6 wrench, in joint 6's frame ("local") or the world frame ("world",
        converted at q by oMi[6].actInv)."""
        q, v, tau = (_f64(x).reshape(-1, NJ) for x in (q, v, tau))
        n = q.shape[0]
        a = np.empty((n, NJ))
        f = _f64(fext).reshape(n, 6) if fext is not None else None
        _check(self._lib.i7m_aba(self._h, n, _ptr(q), _ptr(v), _ptr(tau), _ptr(f), _FRAMES[frame], _ptr(a)))
        return a

    def aba_derivatives(self, q, v, tau):
        q, v, tau = (_f64(x).reshape(-1, NJ) for x in (q, v, tau))
        n = q.shape[0]
        dq, dv, Mi = (np.empty((n, NJ, NJ)) for _ in range(3))
        a = np.empty((n, NJ))
        _check(self._lib.i7m_aba_derivatives(self._h, n, _ptr(q), _ptr(v), _ptr(tau), _ptr(dq), _ptr(dv), _ptr(Mi),
                                             _ptr(a)))
        return dq, dv, Mi, a

    def rk4(self, q, v, u, dt, fext=None, frame="local"):
        """utils.rk4 per row; a "world" wrench is converted once at the start q (the reference's
        host plant, src/gato_mpc_batch_sample.py:270-279)."""
        q, v, u = (_f64(x).reshape(-1, NJ) for x in (q, v, u))
        n = q.shape[0]
        qo, vo = np.empty((n, NJ)), np.empty((n, NJ))
        f = _f64(fext).reshape(n, 6) if fext is not None else None
        _check(self._lib.i7m_rk4(self._h, n, _ptr(q), _ptr(v), _ptr(u), float(dt), _ptr(f), _FRAMES[frame], _ptr(qo),
                                 _ptr(vo)))
        return qo, vo

    def mpc_run(self, xstart, endpoints, num_steps):
        """Closed-loop MPC of B instances on the device (i7m_mpc_run): returns (dists
        (num_steps, B), q (num_steps, B, 6), xcur (B, 12), XU (B, T))."""
        xs = _f64(xstart).reshape(-1, NX)
        ep = _f64(endpoints).reshape(-1, 3)
        B = xs.shape[0]
        d = np.empty((num_steps, B))
        q = np.empty((num_steps, B, NJ))
        xc = np.empty((B, NX))
        xu = np.empty((B, self.T))
        _check(self._lib.i7m_mpc_run(self._h, B, _ptr(xs), _ptr(ep), ep.shape[0], int(num_steps), _ptr(d), _ptr(q),
                                     _ptr(xc), _ptr(xu)))
        return d, q, xc, xu

    def mpc_run_multirate(self, xstart, endpoints, num_steps, sim_dt=0.001, goal_radius=0.1, control_from="new",
                          reset_what=ADMM_RESET_ALL):
        """Multi-rate closed loop of B instances on the device (i7m_mpc_run_multirate): the plant
        advances sim_dt per solve against the knot grid dt, split at knot boundaries, the warm start
        shifted by the knots each step completes.  control_from "new" (MPC_GATO_Batch), "prev"
        (MPC_GATO) or "policy" (the solve's controls under its own Riccati feedback gains, u = u_j +
        K_j (x - x_j) per plant sub-step; no counterpart in the reference).  Returns a dict: dist (num_steps, B), q and u (num_steps, B, 6), xpath (S, B, 6)
        one q per plant sub-step, xcur (B, 12), xu (B, T), and the schedule the library ran, from
        i7m_multirate_substeps and the same arithmetic here: sub_start (num_steps + 1,), shift
        (num_steps,) (step i wrote xpath[sub_start[i]:sub_start[i + 1]]).  NaN from an instance's stop on."""
        xs = _f64(xstart).reshape(-1, NX)
        ep = _f64(endpoints).reshape(-1, 3)
        B, num_steps = xs.shape[0], int(num_steps)
        o = i7m_multirate_opts()
        _check(self._lib.i7m_multirate_opts_default(C.byref(o)))
        o.sim_dt, o.goal_radius = float(sim_dt), float(goal_radius)
        o.control_from, o.reset_what = _CONTROLS[control_from], int(reset_what)
        n_sub = C.c_int32(0)
        _check(self._lib.i7m_multirate_substeps(self.cfg.dt, o.sim_dt, self.N, num_steps, C.byref(n_sub)))
        sub_start, _, shift = multirate_schedule(self.cfg.dt, o.sim_dt, num_steps, self.N)
        if sub_start[-1] != n_sub.value:
            raise I7MError(f"the library plans {n_sub.value} sub-steps, this binding {sub_start[-1]}")
        out = dict(dist=np.empty((num_steps, B)), q=np.empty((num_steps, B, NJ)), u=np.empty((num_steps, B, NU)),
                   xpath=np.empty((n_sub.value, B, NJ)), xcur=np.empty((B, NX)), xu=np.empty((B, self.T)),
                   sub_start=sub_start, shift=shift)
        _check(self._lib.i7m_mpc_run_multirate(self._h, B, _ptr(xs), _ptr(ep), ep.shape[0], num_steps, C.byref(o),
                                               _ptr(out["dist"]), _ptr(out["q"]), _ptr(out["u"]), _ptr(out["xpath"]),
                                               _ptr(out["xcur"]), _ptr(out["xu"])))
        return out

    # ---- the sampled-wrench family: what its three entry points parse the same way -------------
    @staticmethod
    def _hypotheses(fhyp, G):
        """fhyp as (G * H, 6) and H."""
        fh = _f64(fhyp).reshape(-1, 6)
        if G < 1 or fh.shape[0] % G:
            raise ValueError(f"fhyp has {fh.shape[0]} rows, not a multiple of the {G} groups")
        return fh, fh.shape[0] // G

    @staticmethod
    def _reference(ref):
        """ref as a 2-D array: its extents are L and the stride."""
        rf = _f64(ref)
        if rf.ndim != 2:
            raise ValueError("ref must be (L, 3) or (L, 6)")
        return rf

    @staticmethod
    def _phases(ref_phase, G):
        """The groups' phases as a (G,) int32 array, or None."""
        if ref_phase is None:
            return None
        rp = np.ascontiguousarray(ref_phase, dtype=np.int32).reshape(-1)
        if rp.shape[0] != G:
            raise ValueError(f"ref_phase must be ({G},)")
        return rp

    def _opts(self, frame, reset_what, keep_best, decay, sim_dt=None, n_actual=None):
        """The options struct: the library's defaults, then the caller's."""
        o = i7m_sampled_opts()
        _check(self._lib.i7m_sampled_opts_default(C.byref(o)))
        o.decay, o.frame, o.reset_what, o.keep_best = float(decay), _FRAMES[frame], int(reset_what), int(bool(keep_best))
        if sim_dt is not None:
            o.sim_dt, o.n_actual = float(sim_dt), int(n_actual)
        return o

    def _sampled_inputs(self, xstart, num_steps, fhyp, f_actual, noise, sim_dt, frame, reset_what, keep_best, decay):
        """The arguments mpc_run_sampled and mpc_run_tracking share, as contiguous arrays and the
        options struct: (xs, G, fh, H, fa, noise or None, opts)."""
        xs = _f64(xstart).reshape(-1, NX)
        G = xs.shape[0]
        fh, Hn = self._hypotheses(fhyp, G)
        fa = _f64(f_actual)
        if fa.size == G * 6:
            fa = fa.reshape(1, G, 6)
        elif fa.size == num_steps * G * 6:
            fa = fa.reshape(num_steps, G, 6)
        else:
            raise ValueError(f"f_actual must be ({G}, 6) or ({num_steps}, {G}, 6)")
        nz = None
        if noise is not None:
            nz = _f64(noise)
            if nz.size != num_steps * G * Hn * 3:
                raise ValueError(f"noise must be ({num_steps}, {G * Hn}, 3)")
        return xs, G, fh, Hn, fa, nz, self._opts(frame, reset_what, keep_best, decay, sim_dt, fa.shape[0])

    def _multirate_opts(self, o, shift_warm_start, control_from="new"):
        """The multi-rate options struct from the family's (same fields first), the shift flag and
        the plant's control ("new", "policy", or the C value: the library refuses the others)."""
        m = i7m_sampled_multirate_opts()
        _check(self._lib.i7m_sampled_multirate_opts_default(C.byref(m)))
        for f, _ in i7m_sampled_opts._fields_:
            setattr(m, f, getattr(o, f))
        m.shift_warm_start = int(shift_warm_start)
        m.control_from = int(_CONTROLS.get(control_from, control_from))
        return m

    def _multirate_plan(self, sim_dt, num_steps):
        """(n_sub, sub_start, shift) of a run: the library's count (i7m_multirate_substeps, which
        raises for what the library refuses) and this binding's schedule, which must agree."""
        n_sub = C.c_int32(0)
        _check(self._lib.i7m_multirate_substeps(self.cfg.dt, float(sim_dt), self.N, int(num_steps), C.byref(n_sub)))
        sub_start, _, shift = multirate_schedule(self.cfg.dt, sim_dt, num_steps, self.N)
        if sub_start[-1] != n_sub.value:
            raise I7MError(f"the library plans {n_sub.value} sub-steps, this binding {sub_start[-1]}")
        return n_sub.value, sub_start, shift

    def _run_family(self, xstart, num_steps, fhyp, f_actual, noise, sim_dt, frame, reset_what, keep_best, decay,
                    endpoints=None, ref=None, ref_phase=None, ref_offset=None, shift_warm_start=None,
                    control_from="new"):
        """The four loops of the family behind one marshalling: the goal source is `endpoints`, or
        `ref` with `ref_phase` and (single-rate plant) `ref_offset`; the plant is multi-rate where
        shift_warm_start is given.  The returned dict holds the entry point's outputs in the order of
        its C arguments, then a multi-rate run's schedule."""
        track, multi = ref is not None, shift_warm_start is not None
        if track:
            rf = self._reference(ref)
        else:
            ep = _f64(endpoints).reshape(-1, 3)
        xs, G, fh, Hn, fa, nz, o = self._sampled_inputs(xstart, num_steps, fhyp, f_actual, noise, sim_dt, frame,
                                                         reset_what, keep_best, decay)
        if track:
            rp = self._phases(ref_phase, G)
            goal = [_ptr(rf), *rf.shape, _iptr(rp)] + ([] if multi else [_iptr(ref_offset)])
        else:
            goal = [_ptr(ep), ep.shape[0]]
        out = {"err" if track else "dist": np.empty((num_steps, G)), "best": np.empty((num_steps, G), dtype=np.int32),
               "q": np.empty((num_steps, G, NJ))}
        if multi:
            o = self._multirate_opts(o, shift_warm_start, control_from)
            n_sub, sub_start, shift = self._multirate_plan(sim_dt, num_steps)
            out.update(u=np.empty((num_steps, G, NU)), xpath=np.empty((n_sub, G, NJ)))
        if track:
            out["ee"] = np.empty((num_steps, G, 3))
        if track and multi:
            out["off"] = np.empty(num_steps, dtype=np.int32)
        out.update(fbest=np.empty((num_steps, G, 6)), xcur=np.empty((G, NX)), xu_best=np.empty((G, self.T)),
                   fhyp=np.empty((G * Hn, 6)))
        fn = getattr(self._lib, "i7m_mpc_run_" + ("tracking" if track else "sampled") + ("_multirate" if multi else ""))
        _check(fn(self._h, G, Hn, _ptr(xs), *goal, num_steps, _ptr(fh), _ptr(fa), _ptr(nz), C.byref(o),
                  *[(_iptr if v.dtype == np.int32 else _ptr)(v) for v in out.values()]))
        if multi:
            out.update(sub_start=sub_start, shift=shift)
        return out

    def mpc_run_sampled(self, xstart, endpoints, num_steps, fhyp, f_actual, noise=None, sim_dt=0.001, frame="world",
                        reset_what=ADMM_RESET_ALL, keep_best=False, decay=1.0):
        """Sampled-wrench closed loop of G controllers with H hypotheses each on the device
        (i7m_mpc_run_sampled): xstart (G, 12), endpoints (E, 3), fhyp (G * H, 6) with group g owning
        rows [g H, (g + 1) H), f_actual (G, 6) held for the run or (num_steps, G, 6), noise
        (num_steps, G * H, 3) or None (no resampling).  Returns a dict: dist (num_steps, G), best
        (num_steps, G) int32, q and fbest (num_steps, G, 6), xcur (G, 12), xu_best (G, T), fhyp
        (G * H, 6) the final hypotheses (also left set on the handle, in `frame`)."""
        return self._run_family(xstart, int(num_steps), fhyp, f_actual, noise, sim_dt, frame, reset_what, keep_best, decay,
                                endpoints=endpoints)

    def mpc_run_tracking(self, xstart, ref, ref_offset, fhyp, f_actual, ref_phase=None, noise=None, sim_dt=0.01,
                         frame="world", reset_what=ADMM_RESET_ALL, keep_best=False, decay=1.0):
        """The sampled-wrench closed loop tracking a reference trajectory (i7m_mpc_run_tracking):
        ref (L, 3) or (L, 6) (the first three of each point read), ref_offset (num_steps,) the
        window's offset at every step, ref_phase (G,) the groups' start points on the reference or
        None; the rest as mpc_run_sampled.  At step i every row of group g is solved against
        ref[min(phase[g] + ref_offset[i] + k, L - 1)], k = 0 .. N-1.  Returns a dict: err
        (num_steps, G) the distance of the EE to the window's first point, best, q, ee
        (num_steps, G, 3), fbest, xcur, xu_best, fhyp."""
        ro = np.ascontiguousarray(ref_offset, dtype=np.int32).reshape(-1)
        return self._run_family(xstart, ro.shape[0], fhyp, f_actual, noise, sim_dt, frame, reset_what, keep_best, decay,
                                ref=ref, ref_phase=ref_phase, ref_offset=ro)

    def mpc_run_sampled_multirate(self, xstart, endpoints, num_steps, fhyp, f_actual, noise=None, sim_dt=0.001,
                                  frame="world", reset_what=ADMM_RESET_ALL, keep_best=False, decay=1.0,
                                  shift_warm_start=0, control_from="new"):
        """mpc_run_sampled with a multi-rate plant (i7m_mpc_run_sampled_multirate): sim_dt is not
        bounded by dt, a plant step is split at knot boundaries, the hypotheses are scored by one rk4
        step of the whole sim_dt.  shift_warm_start=1 shifts the rows' warm start by the knots a step
        completes.  Returns mpc_run_sampled's dict plus u (num_steps, G, 6) the control applied at
        each step, xpath (n_sub, G, 6) one q per plant sub-step, and the schedule: sub_start
        (num_steps + 1,), shift (num_steps,).
        control_from="policy": the plant runs under the winner's feedback policy, u_j + K_j (x - x_j)
        per sub-step, and the hypotheses are scored by replaying the step under the recorded controls;
        u stays the nominal first control."""
        return self._run_family(xstart, int(num_steps), fhyp, f_actual, noise, sim_dt, frame, reset_what, keep_best, decay,
                                endpoints=endpoints, shift_warm_start=shift_warm_start, control_from=control_from)

    def mpc_run_tracking_multirate(self, xstart, ref, num_steps, fhyp, f_actual, ref_phase=None, noise=None,
                                   sim_dt=0.02, frame="world", reset_what=ADMM_RESET_ALL, keep_best=False, decay=1.0,
                                   shift_warm_start=0, control_from="new"):
        """mpc_run_tracking with a multi-rate plant (i7m_mpc_run_tracking_multirate): the window's
        offset at step i is the number of knots the plant has completed by then (the notebook's
        eepos_offset), computed by the library.  Returns mpc_run_tracking's dict plus u, xpath, off
        (num_steps,) int32 those offsets, sub_start and shift.  control_from as
        mpc_run_sampled_multirate's."""
        return self._run_family(xstart, int(num_steps), fhyp, f_actual, noise, sim_dt, frame, reset_what, keep_best, decay,
                                ref=ref, ref_phase=ref_phase, shift_warm_start=shift_warm_start, control_from=control_from)

    # ---- the controller session (i7m_ctrl_begin / _step / _end) ----------------------------
    def ctrl_begin(self, ref, fhyp, x0=None, groups=None, ref_phase=None, frame="world", reset_what=ADMM_RESET_ALL,
                   keep_best=False, decay=1.0):
        """Open a controller session (i7m_ctrl_begin): G controllers of H hypotheses tracking ref
        (L, 3) or (L, 6) from measured states.  x0 (G, 12): the start states, remembered as x_last
        with the returned control as u_last; x0 None: the controller's constructor (rows at the
        zero state, the first step scores from x_last = x_meas, u_last = 0), G = `groups` (default
        1).  fhyp (G * H, 6), ref_phase (G,) or None.  Returns u (G, 6), the initial solve's control."""
        rf = self._reference(ref)
        xs = None if x0 is None else _f64(x0).reshape(-1, NX)
        G = int(groups) if groups is not None else (1 if xs is None else xs.shape[0])
        if xs is not None and xs.shape[0] != G:
            raise ValueError(f"x0 must be ({G}, 12)")
        fh, Hn = self._hypotheses(fhyp, G)
        rp = self._phases(ref_phase, G)
        o = self._opts(frame, reset_what, keep_best, decay)
        u = np.empty((G, NU))
        _check(self._lib.i7m_ctrl_begin(self._h, G, Hn, _ptr(xs), _ptr(rf), *rf.shape,
                                        _iptr(rp), _ptr(fh), C.byref(o), _ptr(u)))
        self._ctrl = (G, Hn)
        self._ctrl_nk = 0
        return u

    def ctrl_step(self, x_meas, elapsed, ref_offset, noise=None):
        """One controller step on the measured states x_meas (G, 12) (i7m_ctrl_step): elapsed the
        time since the previous measurement, ref_offset the window's offset, noise (G * H, 3) or
        None (no resampling this step).  Returns a dict: u (G, 6) the controls to apply, best (G,)
        int32, fbest (G, 6), err (G,) the tracking error, ee (G, 3)."""
        G, Hn = getattr(self, "_ctrl", None) or (np.size(x_meas) // NX, 0)
        xm = _f64(x_meas).reshape(G, NX)
        nz = None
        if noise is not None:
            nz = _f64(noise)
            if nz.size != G * Hn * 3:
                raise ValueError(f"noise must be ({G * Hn}, 3)")
        out = dict(u=np.empty((G, NU)), best=np.empty(G, dtype=np.int32), fbest=np.empty((G, 6)), err=np.empty(G),
                   ee=np.empty((G, 3)))
        _check(self._lib.i7m_ctrl_step(self._h, _ptr(xm), float(elapsed), int(ref_offset), _ptr(nz), _ptr(out["u"]),
                                       _iptr(out["best"]), _ptr(out["fbest"]), _ptr(out["err"]), _ptr(out["ee"])))
        return out

    def ctrl_set_policy(self, n_k):
        """Turn the session's policy on for the first n_k stages (i7m_ctrl_set_policy; 0: off)."""
        _check(self._lib.i7m_ctrl_set_policy(self._h, int(n_k)))
        self._ctrl_nk = int(n_k)

    def ctrl_get_policy(self):
        """The winner's policy of the last step (i7m_ctrl_get_policy).  Returns (K (G, n_k, 6, 13) =
        [K_k | kff_k], xu_ref (G, n_k, 18) = [x_k, u_k] of XU_best)."""
        G, _ = getattr(self, "_ctrl", None) or (0, 0)
        n_k = getattr(self, "_ctrl_nk", 0) if getattr(self, "_ctrl", None) else 0
        K, xu = np.empty((G, n_k, NU, NX + 1)), np.empty((G, n_k, NX + NU))
        _check(self._lib.i7m_ctrl_get_policy(self._h, _ptr(K), _ptr(xu)))
        return K, xu

    def ctrl_set_applied(self, u_applied):
        """Report the time-average torque (G, 6) applied since the last measurement
        (i7m_ctrl_set_applied): it replaces u_last for the next step's scoring only."""
        G, _ = getattr(self, "_ctrl", None) or (np.size(u_applied) // NU, 0)
        ua = None if u_applied is None else _f64(u_applied).reshape(G, NU)
        _check(self._lib.i7m_ctrl_set_applied(self._h, _ptr(ua)))

    def ctrl_end(self):
        """Close the session (i7m_ctrl_end).  Returns a dict: xu_best (G, T) the final XU_best, fhyp
        (G * H, 6) the final hypotheses (left set on the handle)."""
        G, Hn = getattr(self, "_ctrl", None) or (0, 0)
        out = dict(xu_best=np.empty((G, self.T)), fhyp=np.empty((G * Hn, 6)))
        _check(self._lib.i7m_ctrl_end(self._h, _ptr(out["xu_best"]), _ptr(out["fhyp"])))
        self._ctrl = None
        self._ctrl_nk = 0
        return out

    # ---- timing --------------------------------------------------------------------------
    def set_stream(self, stream_ptr: int):
        _check(self._lib.i7m_set_stream(self._h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def set_external_wrench(self, fext, frame="local"):
        """(B, 6) joint-6 wrench per problem ([f; n]; frame "local" = joint 6's frame, "world" =
        world frame about the origin, converted per configuration), or None to clear."""
        if fext is None:
            _check(self._lib.i7m_set_external_wrench(self._h, 0, None, 0))
            return
        f = _f64(fext).reshape(-1, 6)
        _check(self._lib.i7m_set_external_wrench(self._h, f.shape[0], _ptr(f), _FRAMES[frame]))

    def synchronize(self):
        _check(self._lib.i7m_synchronize(self._h))

    def set_timing(self, on: bool):
        _check(self._lib.i7m_set_timing(self._h, int(bool(on))))

    def kernel_times(self):
        ms = (C.c_double * I7M_K_COUNT)()
        cnt = (C.c_int32 * I7M_K_COUNT)()
        _check(self._lib.i7m_get_kernel_times(self._h, ms, cnt, I7M_K_COUNT))
        return {KERNEL_NAMES[i]: (ms[i], cnt[i]) for i in range(I7M_K_COUNT) if cnt[i] > 0}

    def reset_kernel_times(self):
        _check(self._lib.i7m_reset_kernel_times(self._h))

    def reset(self):
        """i7m_reset: back to the post-create solver state (ADMM mode: every problem's OSQP state
        afresh; drops captured graphs and timing sums; the external wrench is kept)."""
        _check(self._lib.i7m_reset(self._h))
