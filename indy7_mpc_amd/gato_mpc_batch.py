"""Drop-in for the reference's ``src/gato_mpc_batch.py``: ``GATO_Batch`` (the batched solver
wrapper, :8-58) and ``MPC_GATO_Batch`` (the multi-rate closed loop, :60-221).  The loop runs on the
device (``i7m_mpc_run_multirate``): per MPC step a reset, a solve and one kernel that tests the goal,
integrates the plant over ``sim_dt`` split at the knot boundaries of ``dt`` and shifts the warm
start by the knots completed.  No host round trip per step.

What the loop keeps from the reference: the plant advances ``sim_dt`` per solve (0.001 s against
10 ms knots: ten solves per knot); a time accumulator carries the position inside the knot from
step to step; the warm start moves only when a knot completes, and until then stays the older
trajectory while the NEW one drives the plant (:185); the goal test comes after the solve; an
instance stops at its last endpoint and nowhere else; the float residues of the accumulator (step 9
of 0.001 / 0.01 is [0.001, 8.67e-19], the second a real rk4 call and a real path entry).

What differs, on purpose:
  * :213 with no knot completed (its slice ``:-(0) or len(XU_batch)`` ends at ``batch_size`` and
    copies row 0's first ``batch_size`` warm-start entries over every row's) is not reproduced;
  * ``solve_times`` is the device loop's mean time per step (the reference times each solve on the
    host), as ``MPC_GATO_Batch_Sample`` reports it;
  * the QP is OSQP's iteration on the formulation of src/osqp_solver.py in fp64 (``qp_mode="admm"``,
    reset before every solve like the reference's ``solver.reset()``), or exact (``"direct"``): the
    reference's external CUDA solver is absent;
  * nothing is printed, and the per-step "trajectories equal" scan of :125-134 is not run:
    ``run_mpc``'s rows are identical inputs through independent problems, bitwise equal by
    construction (tests/test_gpu_multirate_mpc.py).
"""
from __future__ import annotations

import time

import numpy as np

from . import _lib, _sampling
from .bindings import batch_sqp
from .model import default_model

LOG_EVERY = 0.05  # the reference logs where abs((i * sim_dt) % 0.05) < 1e-10 (:149)


def logged_steps(num_steps, sim_dt):
    """The steps the reference logs statistics at: its own float test (src/gato_mpc_batch.py:149),
    kept as is (with sim_dt = 0.001 it misses some multiples of 0.05 and that is its behaviour)."""
    return np.array([i for i in range(num_steps) if abs((i * sim_dt) % LOG_EVERY) < 1e-10], dtype=int)


class GATO_Batch:
    """The reference's solver wrapper (:8-58) over ``bindings.batch_sqp``: ``solve`` appends to
    the reference's stats keys."""

    def __init__(self, N=32, dt=0.01, batch_size=4, stats=None, model=None, qp_mode="admm", device_id=0):
        if batch_size not in _sampling.SIZES:
            raise ValueError(f"Batch size {batch_size} not supported")
        self.N, self.dt, self.batch_size = int(N), float(dt), int(batch_size)
        self.solver = getattr(batch_sqp, f"SQPSolverfloat_{batch_size}")(model=model, device_id=device_id, qp_mode=qp_mode)
        self.stats = stats or {
            "solve_time": {"values": [], "unit": "us", "multiplier": 1},
            "sqp_iters": {"values": [], "unit": "", "multiplier": 1},
            "pcg_iters": {"values": [], "unit": "", "multiplier": 1},
            "step_size": {"values": [], "unit": "", "multiplier": 1},
        }

    def solve(self, xcur_batch, eepos_goals_batch, XU_batch):
        """xcur (B, 12), goals (B, 6 N) or (B, 3 N), XU (B, 18 N - 6) -> the new XU (B, 18 N - 6)."""
        result = self.solver.solve(XU_batch, self.dt, xcur_batch, eepos_goals_batch)
        self.stats["solve_time"]["values"].append(result["solve_time_us"])
        self.stats["sqp_iters"]["values"].append(result["sqp_iterations"])
        for rec in result["pcg_stats"]:
            self.stats["pcg_iters"]["values"].append(rec["pcg_iterations"])
        for rec in result["line_search_stats"]:
            self.stats["step_size"]["values"].append(rec["step_size"])
        return result["xu_trajectory"]

    def reset(self):
        self.solver.reset()

    def get_stats(self):
        return self.stats


class MPC_GATO_Batch:
    """``run_mpc`` as the reference's (:76-217); ``run_mpc_instances`` for distinct start states."""

    # what MPC_GATO (gato_mpc.py) changes: the goal radius and whose control drives the plant
    GOAL_RADIUS = 0.1
    CONTROL_FROM = "new"

    def __init__(self, model=None, N=32, dt=0.01, batch_size=4, qp_mode="admm", device_id=0, feedback=False):
        """feedback=True: the plant runs under the solve's own Riccati feedback policy, u = u_j + K_j
        (x - x_j) per plant sub-step (``I7M_CONTROL_POLICY``), where the reference holds knot 0's
        control until the next solve; the default is the reference's behaviour."""
        self.feedback = bool(feedback)
        self.qp_mode = _sampling.qp_mode_of(batch_size, qp_mode)
        self.model = model or default_model()
        self.N, self.dt, self.batch_size = int(N), float(dt), int(batch_size)
        self.device_id = device_id
        self.xpath = []
        self.nq = self.nv = self.nu = 6
        self.nx = 12
        self._solver_args = dict(N=self.N, dt=self.dt, batch_size=self.batch_size, model=self.model, qp_mode=qp_mode,
                                 device_id=device_id)
        self._solver = None
        self._h = None
        self._cap = 0

    @property
    def solver(self):
        """The reference's ``self.solver`` (a GATO_Batch), built on first use: the closed loop itself
        runs on a handle of its own."""
        if self._solver is None:
            self._solver = GATO_Batch(**self._solver_args)
        return self._solver

    def _handle(self, rows):
        if self._h is None or self._cap < rows:
            self._h = _lib.Handle(self.model, N=self.N, dt=self.dt, max_batch=rows, device_id=self.device_id,
                                  qp_mode=self.qp_mode)
            self._cap = rows
        return self._h

    def run_mpc_instances(self, xstarts, endpoints, sim_dt=0.001, sim_time=5):
        """B independent instances, one per row of xstarts (B, 12).  Returns (xpaths, stats): a list
        of B q-paths (one q per plant sub-step, up to the instance's stop), and the reference's
        stats keys with a (logged steps, B) layout: goal_distances (logged, B), control_inputs
        (logged, B, 6), NaN where an instance had stopped."""
        xs = np.asarray(xstarts, float).reshape(-1, 12)
        B = xs.shape[0]
        num_steps = int(sim_time / sim_dt)
        h = self._handle(B)
        t0 = time.perf_counter()
        r = h.mpc_run_multirate(xs, endpoints, num_steps, sim_dt=sim_dt, goal_radius=self.GOAL_RADIUS,
                                control_from="policy" if self.feedback else self.CONTROL_FROM,
                                reset_what=_lib.ADMM_RESET_ALL)
        per_step = (time.perf_counter() - t0) / max(num_steps, 1)
        ran = np.isfinite(r["xpath"][:, :, 0])  # an instance's path ends with the step before its stop
        xpaths = [[q for q in r["xpath"][ran[:, b], b]] for b in range(B)]
        log = logged_steps(num_steps, sim_dt)
        stats = {
            "solve_times": [round(per_step, 5)] * len(log),  # the device loop's mean time per step
            "goal_distances": np.round(r["dist"][log], 5),
            "control_inputs": np.round(r["u"][log], 5),
        }
        self.last = r
        return xpaths, stats

    def run_mpc(self, xstart, endpoints, sim_dt=0.001, sim_time=5):
        """The reference's run_mpc: batch_size identical rows (:84-99), and row 0's (xpath, stats)
        (:136-143): xpath one q per plant sub-step up to the stop, the stats logged at the
        reference's steps up to and including the step it stopped at."""
        rows = np.tile(np.asarray(xstart, float).reshape(1, 12), (self.batch_size, 1))
        return self._row0(*self.run_mpc_instances(rows, endpoints, sim_dt, sim_time))

    def _row0(self, xpaths, st):
        """(xpath, stats) of instance 0, as the reference returns them."""
        self.xpath += xpaths[0]
        keep = np.isfinite(st["goal_distances"][:, 0])
        stats = {
            "solve_times": [t for t, k in zip(st["solve_times"], keep) if k],
            "goal_distances": [float(d) for d in st["goal_distances"][keep, 0]],
            "control_inputs": [u for u in st["control_inputs"][keep, 0]],
        }
        return self.xpath, stats
