"""Drop-in for the reference's ``src/gato_mpc.py``: ``GATO`` (the one-problem solver wrapper, :8-37)
and ``MPC_GATO`` (:40-154), the multi-rate closed loop of ``gato_mpc_batch.py`` with one instance
and three constants of its own: the plant advances a fixed ``sim_dt = 0.02`` per solve (:76: two
10 ms knots, so the warm start shifts by two every step), the goal radius is ``1e-2`` (:106,113) and
the plant is driven by the PREVIOUS trajectory's first control (:126), not the new one's.  The loop
runs on the device (``i7m_mpc_run_multirate`` with ``I7M_CONTROL_PREV``).

What differs from the reference is what ``indy7_mpc_amd.gato_mpc_batch`` lists (solve_times, the
QP, no printing); src/gato_mpc.py has no counterpart of src/gato_mpc_batch.py:213.
"""
from __future__ import annotations

import numpy as np

from .gato_mpc_batch import GATO_Batch, MPC_GATO_Batch

SIM_DT = 0.02  # src/gato_mpc.py:76


class GATO(GATO_Batch):
    def __init__(self, N=32, dt=0.01, stats=None, model=None, qp_mode="admm", device_id=0):
        super().__init__(N, dt, 1, stats, model=model, qp_mode=qp_mode, device_id=device_id)


class MPC_GATO(MPC_GATO_Batch):
    GOAL_RADIUS = 1e-2
    CONTROL_FROM = "prev"

    def __init__(self, model=None, N=32, dt=0.01, qp_mode="admm", device_id=0, feedback=False):
        super().__init__(model, N, dt, 1, qp_mode, device_id, feedback)

    @property
    def solver(self):
        if self._solver is None:
            args = {k: v for k, v in self._solver_args.items() if k != "batch_size"}
            self._solver = GATO(**args)
        return self._solver

    def run_mpc_instances(self, xstarts, endpoints, sim_time=5):
        return super().run_mpc_instances(xstarts, endpoints, SIM_DT, sim_time)

    def run_mpc(self, xstart, endpoints, sim_time=5):
        """The reference's run_mpc (:53-150): (xpath, stats), xpath one q per plant sub-step."""
        return self._row0(*self.run_mpc_instances(np.asarray(xstart, float).reshape(1, 12), endpoints, sim_time))
