"""The off-default solver settings that tests/test_settings_oracle.py (port against the numpy
restatement, CPU) and tests/test_gpu_settings.py (device against the port and the numpy oracle)
run, and the helpers both share: one list of cases, one rule for step_tol, one numpy loop.

OSQP settings are keyed as oracle/cpu.py::admm_cfg, _lib.ADMM_DEFAULTS and oracle/osqp_admm.py
DEFAULTS key them (the same names); SQP settings as oracle/cpu.py::_cfg keys them (max_iters, mu,
step_tol) — `handle_kw` renames them for _lib.Handle.
"""
import numpy as np

from oracle.osqp_ref import OSQPSolverRef, SQPRef

# OSQP's status strings (oracle/osqp_admm.py) as i7m_get_admm_status's codes
STATUS_CODE = {"solved": 1, "solved_inaccurate": 2, "max_iter_reached": 0}

# (id, OSQP settings).  adapt: an adaptation interval (10) that is no multiple of the check interval
# (25), so that most adaptations run at an iteration without a termination check; rho starts at
# 0.005 and the tolerance band is 2 so that rho moves.
OSQP_CASES = [
    ("sigma_alpha_rho", dict(sigma=1e-4, alpha=1.2, rho=1.0)),
    ("scaling0", dict(scaling=0)),
    ("scaling3", dict(scaling=3)),
    ("check1", dict(check_termination=1)),
    ("check7", dict(check_termination=7)),
    ("check0", dict(check_termination=0, max_iter=60)),
    ("no_gap", dict(check_dualgap=False)),
    ("eps_rel0", dict(eps_rel=0.0, eps_abs=1e-5)),
    ("eps_abs0", dict(eps_abs=0.0, eps_rel=1e-2)),
    ("adapt", dict(rho=0.005, adaptive_rho_interval=10, adaptive_rho_tolerance=2.0)),
]

# (id, SQP settings); the default step_tol (1e-3) stops nothing on these draws (steps are 50-200:
# XU holds torques), so every problem runs max_iters QPs
SQP_CASES = [
    ("sqp1", dict(max_iters=1)),
    ("sqp5", dict(max_iters=5)),
    ("sqp8", dict(max_iters=8, step_tol=1e-9)),
    ("mu1", dict(mu=1.0, max_iters=4)),
    ("mu1000", dict(mu=1000.0, max_iters=4)),
]

# (id, box settings as oracle/cpu.py::box_cfg keys them)
BOX_CASES = [
    ("mask1", dict(mask=1)),
    ("mask2", dict(mask=2)),
    ("mask3", dict(mask=3)),
    ("mask4", dict(mask=4)),
    ("mask5", dict(mask=5)),
    ("mask6", dict(mask=6)),
    ("max_iters4", dict(max_iters=4)),
    ("max_iters1", dict(max_iters=1)),
    ("tol1e-4", dict(tol=1e-4)),
]


def ids(cases):
    return [c[0] for c in cases]


def handle_kw(sqp_kw):
    """oracle/cpu.py::_cfg's names -> _lib.Handle's."""
    return {{"max_iters": "max_sqp_iters"}.get(k, k): v for k, v in sqp_kw.items()}


def step_gap(steps, tol):
    """The smallest relative distance of any step length (NaN = no step) to tol."""
    s = np.asarray(steps, float)
    s = s[~np.isnan(s)]
    return float(np.min(np.abs(s - tol) / s))


def choose_step_tol(steps):
    """A step tolerance that stops some problems early and that no rounding can flip: the median
    step length of SQP iterations 2-5 of a run with step_tol = 0 (`steps`: its (B, 8) step lengths,
    NaN = none), moved up until no step length of that run is within 1 % of it."""
    tol = float(np.nanmedian(steps[:, 2:6]))
    while step_gap(steps, tol) < 0.01:
        tol *= 1.003
    return tol


def numpy_solves(xcur, goals, xu, N, solver_kw, sqp_kw, calls=1):
    """Every problem through SQPRef on its own OSQPSolverRef(N=N, **solver_kw), `calls` consecutive
    solves (each from the previous one's output and, in "osqp" mode, OSQP state).  Returns one dict
    per call: xu (B, T), qp_iters (B,), alphas (list of lists), and in "osqp" mode its / status
    (lists of lists: OSQP's iterations and status code per QP) and rho (B,); in "box" mode ipm
    (list of lists of (iterations, converged) per QP)."""
    B = xu.shape[0]
    res = [dict(xu=np.empty_like(xu), qp_iters=np.zeros(B, int), alphas=[], its=[], status=[], rho=np.zeros(B), ipm=[])
           for _ in range(calls)]
    for b in range(B):
        s = OSQPSolverRef(N=N, **solver_kw)
        ipm = []
        if s.qp == "box":
            inner = s.setup_and_solve_qp

            def rec(*a, _inner=inner, _s=s, _ipm=ipm):
                r = _inner(*a)
                _ipm.append((_s.last_ipm.iters, bool(_s.last_ipm.converged)))
                return r

            s.setup_and_solve_qp = rec
        sq = SQPRef(s, **sqp_kw)
        x = xu[b].copy()
        na = nh = ni = 0
        for r in res:
            x = sq.sqp(xcur[b], goals[b], x.copy())
            r["xu"][b] = x
            r["qp_iters"][b] = sq.stats["qp_iters"]["values"][-1]
            al = sq.stats["linesearch_alphas"]["values"]
            r["alphas"].append([float(a) for a in al[na:]])
            na = len(al)
            if s.qp == "osqp":
                h = s.osqp.history[nh:]
                nh = len(s.osqp.history)
                r["its"].append([e[0] for e in h])
                r["status"].append([STATUS_CODE[e[5]] for e in h])
                r["rho"][b] = s.osqp.rho
            r["ipm"].append(ipm[ni:])
            ni = len(ipm)
    return res


def rel(a, b):
    """Per-problem relative 2-norm error (tests/test_gpu_admm.py's metric)."""
    return np.linalg.norm(a - b, axis=-1) / np.maximum(np.linalg.norm(b, axis=-1), 1e-300)


def box_relerr(a, b):
    """tests/test_gpu_box.py::_relerr."""
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())
