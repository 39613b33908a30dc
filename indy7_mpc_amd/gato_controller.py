"""Drop-in for the reference's ``gato_controller.py``: ``GATO_Controller`` without ROS.  The deployed
controller (gato_controller.py:144-250) gets a joint state from a robot or a simulator at wall-clock
intervals, slides the goal window along the reference trajectory, solves ``batch_size`` wrench
hypotheses, scores them against the measurement over the elapsed time, resamples them and returns
one torque vector.  Here ``step(x_curr)`` is ``joint_callback`` and the whole step is one call into
the library (``i7m_ctrl_step``): one copy in, two small kernels around the solve, one copy out.

    ctrl = GATO_Controller(ref_traj, batch_size=16, N=64, dt=0.01, f_ext_std=10.0, f_ext_resample_std=2.0)
    u = ctrl.step(x_curr)        # in the joint-state callback; publish u as the effort command

What differs from the reference, on purpose:
  * no ROS node, publishers or timers: the caller owns the transport and calls ``step``;
    ``f_ext_actual`` and its clipped random walk (:236-239) belong to the simulator, not here;
  * the hypotheses and the resampling noise come from ``numpy.random.default_rng(seed)`` with the
    reference's shapes and zeroing (torques 0, row 0 zero, :77-83; (batch_size, 6) normals per step
    with the torques dropped), as ``MPC_GATO_Batch_Sample`` draws them; the reference's global
    ``np.random`` draw order is not reproduced;
  * the EE position is the model's forward kinematics of the measured q, where the controller
    reads it from the simulator's message (``msg.effort[0:3]``, :203);
  * ties go to the lowest index, the device's rule, where the controller's ``<=`` (:115) takes the
    highest; tied hypotheses are identical rows, so the trajectories are the same;
  * a window that runs past the end of the reference holds its last point (the controller's slice
    would come up short there);
  * ``solve_times`` are the wall-clock seconds of the whole step, not the solver's own microseconds;
  * everything is fp64 (the reference's batch_sqp solves in float);
  * ``groups`` > 1 runs that many independent controllers on one handle, one state row each, all on
    one clock; ``step`` then takes (groups, 12) and returns (groups, 6).
"""
from __future__ import annotations

import time

import numpy as np

from . import _lib, _sampling
from .model import default_model


class GATO_Controller:
    def __init__(self, ref_traj=None, batch_size=1, N=32, dt=0.01, f_ext_std=0.0, f_ext_resample_std=0.0, model=None,
                 seed=None, qp_mode="admm", groups=1, device_id=0, policy_knots=0):
        if ref_traj is None:
            raise ValueError("ref_traj must be provided")
        mode = _sampling.qp_mode_of(batch_size, qp_mode)
        self.ref_traj = ref = _sampling.reference_points(ref_traj)
        self.ref_traj_offset = 0
        self.batch_size, self.N, self.dt, self.groups = int(batch_size), int(N), float(dt), int(groups)
        self.nu, self.nx = 6, 12
        self.config = f"dt:{self.dt}_batch_size:{self.batch_size}_N:{self.N}_f_ext_std:{f_ext_std}"
        self.rng = np.random.default_rng(seed)
        self.f_ext_batch = _sampling.initial_hypotheses(self.rng, self.batch_size, f_ext_std)
        self.f_ext_resample_std = float(f_ext_resample_std)
        self.resample_f_ext = self.f_ext_resample_std > 0.0  # :85
        self._h = _lib.Handle(model or default_model(), N=self.N, dt=self.dt, max_batch=self.groups * self.batch_size,
                              device_id=device_id, qp_mode=mode)
        # :174-185: the window at offset 0, the zero state, one solve, XU_best = row 0; x_last unset
        self._h.ctrl_begin(ref, np.tile(self.f_ext_batch, (self.groups, 1)), x0=None, groups=self.groups, frame="world",
                           reset_what=_lib.ADMM_RESET_ALL, keep_best=True, decay=0.97)
        self._open = True
        # the winner's feedback policy for a torque loop faster than the solver (policy(), control())
        self.policy_knots = int(policy_knots)
        self._policy = None
        if self.policy_knots:
            self._h.ctrl_set_policy(self.policy_knots)
        # stats (:188-193), one entry per step
        self.dts, self.tracking_errors, self.ee_positions, self.ee_ref_positions = [], [], [], []
        self.joint_positions, self.solve_times, self.best_ids, self.f_ext_best = [], [], [], []
        self.last_time = time.time()

    def step(self, x_curr, elapsed_time=None, u_applied=None):
        """joint_callback (:201-250) on the measured state x_curr (12,) (or (groups, 12)):
        elapsed_time seconds since the previous state, None = the wall clock since the previous
        call (:209-211).  u_applied (6,) (or (groups, 6)): the time-average torque a caller that
        applies control() itself has applied since the previous state; the hypotheses are scored
        against it instead of the last returned torque.  Returns u_curr (6,) (or (groups, 6)), the
        torques to command."""
        now = time.time()
        elapsed = now - self.last_time if elapsed_time is None else float(elapsed_time)
        x = np.asarray(x_curr, float).reshape(self.groups, self.nx)
        offset = int(self.ref_traj_offset + elapsed / self.dt)  # :214-215
        noise = None
        if self.resample_f_ext:
            noise = _sampling.resampling_noise(self.rng, self.f_ext_resample_std, self.groups * self.batch_size)
        t0 = time.perf_counter()
        if u_applied is not None:
            self._h.ctrl_set_applied(np.asarray(u_applied, float).reshape(self.groups, self.nu))
        r = self._h.ctrl_step(x, elapsed, offset, noise=noise)
        self._policy = None
        solve_time = time.perf_counter() - t0
        # a refused step (a non-finite state, a clock that did not advance) changes nothing above
        self.last_time = now
        self.ref_traj_offset += elapsed / self.dt
        self.dts.append(elapsed)
        one = self.groups == 1
        first = self.ref_traj[min(offset, len(self.ref_traj) - 1), :3]
        self.tracking_errors.append(r["err"][0] if one else r["err"])
        self.ee_positions.append(r["ee"][0] if one else r["ee"])
        self.ee_ref_positions.append(first)
        self.joint_positions.append(x[0, :6].copy() if one else x[:, :6].copy())
        self.solve_times.append(solve_time)
        self.best_ids.append(int(r["best"][0]) if one else r["best"])
        self.f_ext_best.append(r["fbest"][0] if one else r["fbest"])
        return r["u"][0] if one else r["u"]

    def policy(self):
        """The winner's feedback policy of the last step (policy_knots > 0): a dict of K
        (G, n_k, 6, 12), kff (G, n_k, 6), x_ref (G, n_k, 12) and u_ref (G, n_k, 6), knot k at time
        k dt after the measurement the step was given."""
        if self._policy is None:
            K, xu = self._h.ctrl_get_policy()
            self._policy = {"K": K[..., :12].copy(), "kff": K[..., 12].copy(), "x_ref": xu[..., :12].copy(),
                            "u_ref": xu[..., 12:].copy()}
        return self._policy

    def control(self, x, t):
        """The torque a loop faster than the solver applies at state x (12,) (or (groups, 12)), t
        seconds after the last step's measurement: u_ref[j] + K[j] (x - x_ref[j]) with
        j = min(int(t / dt), n_k - 1).  Plain numpy on the last step's policy."""
        p = self.policy()
        j = min(int(t / self.dt), self.policy_knots - 1)
        dx = np.asarray(x, float).reshape(self.groups, self.nx) - p["x_ref"][:, j]
        u = p["u_ref"][:, j] + np.einsum("grc,gc->gr", p["K"][:, j], dx)
        return u[0] if self.groups == 1 else u

    def get_stats(self):
        return {k: getattr(self, k) for k in ("dts", "tracking_errors", "ee_positions", "ee_ref_positions",
                                              "joint_positions", "solve_times", "best_ids", "f_ext_best")}

    def close(self):
        """End the session: f_ext_batch becomes the final hypotheses (group 0's), XU_best the final
        trajectories.  The handle stays, so a later ``step`` is refused by the library."""
        if self._open:
            end = self._h.ctrl_end()
            self.f_ext_batch = end["fhyp"][:self.batch_size].copy()
            self.XU_best = end["xu_best"]
            self._open = False
