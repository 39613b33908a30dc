"""Drop-in for the reference's ``src/gato_mpc_batch_sample.py``: ``MPC_GATO_Batch_Sample``, the
closed loop that estimates the external force by solving ``batch_size`` wrench hypotheses every
control step and keeping the trajectory whose one-step prediction best matches the measured state
(src/gato_mpc_batch_sample.py:74-300, with the controller's selection / resampling rule,
gato_controller.py:109-129).  The whole loop runs on the device (``i7m_mpc_run_sampled``): no
host round trip per step.

What differs from the reference, on purpose:
  * the hypotheses and the resampling noise come from ``numpy.random.default_rng(seed)``, drawn
    up front with the reference's shapes and zeroing (torques 0, row 0 zero, :37-40,291-297); the
    reference's global ``np.random`` draw order is not reproduced;
  * the actual force is ``constant_f_ext`` for the whole run (zero if None), a WORLD-frame force
    like the hypotheses; the reference random-walks it every step (:244-250) and applies it to the
    plant as a joint-6 LOCAL force (:96-102) while it scores the hypotheses as world-frame ones;
  * with ``sim_dt <= dt``, one rk4 step of ``sim_dt`` per control step (``i7m_mpc_run_sampled``: the
    reference's split at a knot boundary, :170-187, is left out there, and with it the float-residue
    sub-step of 8.67e-19 s that the reference takes at every tenth step of sim_dt = 0.001);
    with ``sim_dt > dt`` the plant step is split at the knot boundaries as the reference does
    (``i7m_mpc_run_sampled_multirate``), xpath holds one q per plant sub-step and
    ``control_inputs`` one control per logged step;
  * ``resample_f_ext=True`` perturbs every row but row 0 (:291-298: keep_best = 0, decay = 1);
    pass ``keep_best=True, decay=0.97`` for the controller's rule (gato_controller.py:120-129).

``run_tracking`` / ``run_tracking_groups`` are the deployed controller's loop
(``GATO_Controller.joint_callback``, gato_controller.py:201-250: the N-knot goal window slides along
a reference trajectory, ``i7m_mpc_run_tracking``).  What differs from ``GATO_Controller``:
  * the plant is the device's rk4 step of ``sim_dt``, not MuJoCo at wall-clock intervals, so the
    window's offset follows the schedule floor((i + 1) sim_dt / dt) (or the caller's); for a plant
    outside the device use ``indy7_mpc_amd.gato_controller.GATO_Controller`` (one step per call on
    the measured state);
  * the first step scores the hypotheses with the initial solve's control, where the controller
    starts from u_last = 0 (:206);
  * ties go to the lowest index, the device's rule, where the controller's ``<=`` (:115) takes the
    highest; tied hypotheses are identical rows, so the trajectories are the same;
  * the actual force is the caller's schedule (``f_actual``), not the controller's clipped random
    walk (:236-239).

``run_mpc_fig8`` / ``run_fig8_groups`` are ``run_mpc_fig8`` of the reference's
notebooks/gato_mpc_indy7_fig8.ipynb (``i7m_mpc_run_tracking_multirate``): the figure-8 tracking run
under an unknown force, the plant stepped ``sim_dt`` per solve against the knot grid.  Kept: the
split of a plant step at a knot boundary with its float residues, knot 0's control on every
sub-step, the goal window advancing by the knots the plant completed (``eepos_offset``), no
warm-start shift, the reset before every solve, the one-step scoring over the whole ``sim_dt``, the
logging rule ``abs((i * sim_dt) % 0.05) < 1e-5`` with one control per logged step, the end of the
run at the first step whose offset reaches ``L - 6 N`` (that step's plant is still in the path).
What differs, besides the draws and the force schedule above:
  * the actual force is a WORLD-frame force converted to joint 6's frame at every step's start
    state, as src/gato_mpc_batch_sample.py:151-161 does; the notebook passes the world force as a
    local one (its actInv is commented out);
  * ties go to the lowest index, where the notebook's ``<=`` takes the highest; tied hypotheses are
    identical rows;
  * the notebook's resampling keeps f_best in row 1; here ``keep_best`` keeps it in the winning row
    (gato_controller.py:120-129).
"""
from __future__ import annotations

import time
from fractions import Fraction

import numpy as np

from . import _lib, _sampling
from .model import default_model


def tracking_schedule(sim_dt, sim_time, dt):
    """(num_steps, offsets) of a tracking run: floor(sim_time / sim_dt) control steps, and at step i
    the window has slid by floor((i + 1) sim_dt / dt) points (gato_controller.py:214-215 with a
    constant elapsed time of sim_dt).  In exact rational arithmetic on the decimal values the
    floats print as, so that 0.001 / 0.01 is 1 / 10 and the window moves at steps 9, 19, ...:
    accumulated floats would move it a step late or early."""
    sim_dt, sim_time, dt = (Fraction(repr(float(v))) for v in (sim_dt, sim_time, dt))
    num_steps = int(sim_time / sim_dt)
    return num_steps, np.array([int((i + 1) * sim_dt / dt) for i in range(num_steps)], dtype=np.int32)


def logged_steps(num_steps, sim_dt):
    """The steps the reference logs: abs((i * sim_dt) % 0.05) < 1e-5 (:236), in its float arithmetic."""
    return np.array([i for i in range(num_steps) if abs((i * sim_dt) % 0.05) < 1e-5], dtype=int)


def fig8_steps(dt, sim_dt, sim_time, N, L):
    """(num_steps, full) of a figure-8 run over a reference of L points: full = the steps that reach
    their solve (offset < L - 6 N, the notebook's bound), num_steps = full plus the step whose plant
    still runs before the notebook breaks, int(sim_time / sim_dt) at most."""
    most = int(sim_time / sim_dt)
    off = np.cumsum(_lib.multirate_schedule(dt, sim_dt, most, N)[2])
    over = np.flatnonzero(off >= L - 6 * N)
    full = int(over[0]) if len(over) else most
    return min(full + 1, most), full


def _controls_after(r):
    """(num_steps, G, 6) the control chosen by each step's solve and selection, XU_best[12:18] after
    step i, which the reference logs (:240): it is the control the next step applies, and the last
    step's is the final XU_best's."""
    return np.concatenate([r["u"][1:], r["xu_best"][None, :, 12:18]], axis=0) if len(r["u"]) else r["u"]


class MPC_GATO_Batch_Sample:
    def __init__(self, model=None, N=32, dt=0.01, batch_size=4, constant_f_ext=None, resample_f_ext=False,
                 f_ext_std=1.0, f_ext_resample_std=2.0, seed=None, qp_mode="admm", keep_best=False, decay=1.0,
                 device_id=0):
        self.qp_mode = _sampling.qp_mode_of(batch_size, qp_mode)
        self.model = model or default_model()
        self.N, self.dt, self.batch_size = int(N), float(dt), int(batch_size)
        self.device_id = device_id
        self.resample_f_ext = bool(resample_f_ext)
        self.f_ext_resample_std = float(f_ext_resample_std)
        self.keep_best, self.decay = bool(keep_best), float(decay)
        self.rng = np.random.default_rng(seed)
        self.f_ext_batch = _sampling.initial_hypotheses(self.rng, self.batch_size, f_ext_std)
        self.actual_f_ext = np.zeros(6)
        if constant_f_ext is not None:
            self.actual_f_ext[:3] = np.asarray(constant_f_ext, float).reshape(-1)[:3]
        self.xpath = []
        self._h = None
        self._cap = 0

    def _handle(self, rows):
        if self._h is None or self._cap < rows:
            self._h = _lib.Handle(self.model, N=self.N, dt=self.dt, max_batch=rows, device_id=self.device_id,
                                  qp_mode=self.qp_mode)
            self._cap = rows
        return self._h

    def _run_inputs(self, G, num_steps, f_actual):
        """What both loops start from: the actual wrenches as (G, 6) or the caller's schedule, the
        run's resampling noise (or None) and the handle."""
        fa = np.tile(self.actual_f_ext, (G, 1)) if f_actual is None else np.asarray(f_actual, float)
        if fa.size == 6:
            fa = np.tile(fa.reshape(6), (G, 1))
        noise = None
        if self.resample_f_ext:
            noise = _sampling.resampling_noise(self.rng, self.f_ext_resample_std, num_steps, G * self.batch_size)
        return fa, noise, self._handle(G * self.batch_size)

    def run_mpc_groups(self, xstarts, endpoints, sim_dt=0.001, sim_time=5, f_actual=None, feedback=False):
        """G independent controllers, one per row of xstarts (G, 12), each with this object's
        hypotheses and its own resampling noise.  f_actual: (6,), (G, 6) or (num_steps, G, 6)
        world-frame wrenches (default: constant_f_ext for every group).  Returns (xpaths, stats): a
        list of G q-paths, and the reference's stats keys with a (logged steps, G) layout, plus
        'best_ids' and 'f_ext_best' (every step).  feedback=True: the plant runs under the winner's
        feedback policy (control_from="policy"), through the multi-rate loop whatever sim_dt is."""
        xs = np.asarray(xstarts, float).reshape(-1, 12)
        G, H = xs.shape[0], self.batch_size
        num_steps = int(sim_time / sim_dt)
        fa, noise, h = self._run_inputs(G, num_steps, f_actual)
        if sim_dt > self.dt or feedback:
            return self._run_mpc_groups_multirate(h, xs, endpoints, num_steps, fa, noise, sim_dt, feedback)
        t0 = time.perf_counter()
        r = h.mpc_run_sampled(xs, endpoints, num_steps, np.tile(self.f_ext_batch, (G, 1)), fa, noise=noise,
                              sim_dt=sim_dt, frame="world", reset_what=_lib.ADMM_RESET_ALL, keep_best=self.keep_best,
                              decay=self.decay)
        per_step = (time.perf_counter() - t0) / max(num_steps, 1)
        self.f_ext_batch = r["fhyp"][:H].copy()
        ran = np.isfinite(r["q"][:, :, 0])  # a group's path ends with the step it stopped at
        xpaths = [[q for q in r["q"][ran[:, g], g]] for g in range(G)]
        every = max(int(round(0.05 / sim_dt)), 1)  # the reference logs every 0.05 s, :236-242
        log = np.arange(0, num_steps, every)
        stats = {
            "solve_times": [round(per_step, 5)] * len(log),  # the device loop's mean time per step
            "goal_distances": np.round(r["dist"][log], 5),
            # the controls stay on the device between steps: only the final one is returned
            "control_inputs": [np.round(r["xu_best"][:, 12:18], 5)],
            "best_ids": r["best"],
            "f_ext_best": r["fbest"],
        }
        self.last = r
        return xpaths, stats

    def _run_mpc_groups_multirate(self, h, xs, endpoints, num_steps, fa, noise, sim_dt, feedback=False):
        """run_mpc_groups with sim_dt > dt (i7m_mpc_run_sampled_multirate): the paths hold one q per
        plant sub-step, control_inputs (logged, G, 6) one control per logged step."""
        G, H = xs.shape[0], self.batch_size
        t0 = time.perf_counter()
        r = h.mpc_run_sampled_multirate(xs, endpoints, num_steps, np.tile(self.f_ext_batch, (G, 1)), fa, noise=noise,
                                        sim_dt=sim_dt, frame="world", reset_what=_lib.ADMM_RESET_ALL,
                                        keep_best=self.keep_best, decay=self.decay,
                                        control_from="policy" if feedback else "new")
        per_step = (time.perf_counter() - t0) / max(num_steps, 1)
        self.f_ext_batch = r["fhyp"][:H].copy()
        ran = np.isfinite(r["xpath"][:, :, 0])  # a group's path ends with the step it stopped at
        xpaths = [[q for q in r["xpath"][ran[:, g], g]] for g in range(G)]
        log = logged_steps(num_steps, sim_dt)
        stats = {
            "solve_times": [round(per_step, 5)] * len(log),  # the device loop's mean time per step
            "goal_distances": np.round(r["dist"][log], 5),
            "control_inputs": np.round(_controls_after(r)[log], 5),
            "best_ids": r["best"],
            "f_ext_best": r["fbest"],
        }
        self.last = r
        return xpaths, stats

    def run_fig8_groups(self, xstarts, fig8_traj, sim_dt=0.001, sim_time=5, f_actual=None, ref_phase=None,
                        feedback=False):
        """G independent controllers on the notebook's figure-8 run (i7m_mpc_run_tracking_multirate),
        one per row of xstarts (G, 12), group g starting at point ref_phase[g] of the reference
        (default 0).  fig8_traj: flat with six entries per point (as the notebook's figure8 builds
        it), or (L, 3) / (L, 6).  The run has int(sim_time / sim_dt) steps at most and ends with the
        first step whose window offset reaches L - 6 N (the notebook's bound): that step's plant is in
        the paths, and it is not logged.  Returns (xpaths, stats): a list of G q-paths, one q per
        plant sub-step, and the notebook's stats keys with a (logged steps, G) layout
        (goal_distances (logged, G), control_inputs (logged, G, 6)) plus 'best_ids', 'f_ext_best'
        and 'offsets' (every step).  feedback=True: the plant runs under the winner's feedback policy
        (control_from="policy"); control_inputs stay the nominal controls."""
        xs = np.asarray(xstarts, float).reshape(-1, 12)
        G, H = xs.shape[0], self.batch_size
        ref = _sampling.reference_points(fig8_traj)
        num_steps, full = fig8_steps(self.dt, sim_dt, sim_time, self.N, ref.shape[0])
        fa, noise, h = self._run_inputs(G, num_steps, f_actual)
        phase = None if ref_phase is None else np.asarray(ref_phase, dtype=np.int32).reshape(G)
        t0 = time.perf_counter()
        r = h.mpc_run_tracking_multirate(xs, ref, num_steps, np.tile(self.f_ext_batch, (G, 1)), fa, ref_phase=phase,
                                         noise=noise, sim_dt=sim_dt, frame="world", reset_what=_lib.ADMM_RESET_ALL,
                                         keep_best=self.keep_best, decay=self.decay,
                                         control_from="policy" if feedback else "new")
        per_step = (time.perf_counter() - t0) / max(num_steps, 1)
        self.f_ext_batch = r["fhyp"][:H].copy()
        xpaths = [[q for q in r["xpath"][:, g]] for g in range(G)]
        log = logged_steps(full, sim_dt)  # the step the run ends at breaks before the notebook logs it
        stats = {
            "solve_times": [round(per_step, 5)] * len(log),  # the device loop's mean time per step
            "goal_distances": np.round(r["err"][log], 5),
            "control_inputs": np.round(_controls_after(r)[log], 5),
            "best_ids": r["best"],
            "f_ext_best": r["fbest"],
            "offsets": r["off"],
        }
        self.last = r
        return xpaths, stats

    def run_mpc_fig8(self, xstart, fig8_traj, sim_dt=0.001, sim_time=5, feedback=False):
        """One controller, as the notebook's run_mpc_fig8: (xpath, stats), xpath one q per plant
        sub-step, the stats logged where abs((i * sim_dt) % 0.05) < 1e-5."""
        xpaths, st = self.run_fig8_groups(np.asarray(xstart, float).reshape(1, 12), fig8_traj, sim_dt, sim_time,
                                          feedback=feedback)
        self.xpath += xpaths[0]
        stats = {
            "solve_times": st["solve_times"],
            "goal_distances": [float(d) for d in st["goal_distances"][:, 0]],
            "control_inputs": [u for u in st["control_inputs"][:, 0]],
            "best_ids": st["best_ids"][:, 0],
            "f_ext_best": st["f_ext_best"][:, 0],
            "offsets": st["offsets"],
        }
        return self.xpath, stats

    def run_tracking_groups(self, xstarts, ref_traj, sim_dt=0.01, sim_time=5, f_actual=None, ref_phase=None,
                            ref_offset=None):
        """G independent controllers tracking ref_traj (i7m_mpc_run_tracking), one per row of xstarts
        (G, 12), group g starting at point ref_phase[g] of the reference (default 0).  ref_traj: flat
        with six entries per point (as utils.figure8 builds it), or (L, 3) / (L, 6).  ref_offset
        (num_steps,): the window's offset at every step; default floor((i + 1) sim_dt / dt).
        f_actual as run_mpc_groups'.  Returns the controller's stats (tracking_errors
        (num_steps, G), ee_positions and ee_ref_positions (num_steps, G, 3), joint_positions
        (num_steps, G, 6), solve_times) plus 'best_ids' and 'f_ext_best'."""
        xs = np.asarray(xstarts, float).reshape(-1, 12)
        G, H = xs.shape[0], self.batch_size
        ref = _sampling.reference_points(ref_traj)
        if ref_offset is None:
            num_steps, ref_offset = tracking_schedule(sim_dt, sim_time, self.dt)
        ref_offset = np.asarray(ref_offset, dtype=np.int32).reshape(-1)
        num_steps = len(ref_offset)
        phase = np.zeros(G, np.int32) if ref_phase is None else np.asarray(ref_phase, dtype=np.int32).reshape(G)
        fa, noise, h = self._run_inputs(G, num_steps, f_actual)
        t0 = time.perf_counter()
        r = h.mpc_run_tracking(xs, ref, ref_offset, np.tile(self.f_ext_batch, (G, 1)), fa, ref_phase=phase, noise=noise,
                               sim_dt=sim_dt, frame="world", reset_what=_lib.ADMM_RESET_ALL, keep_best=self.keep_best,
                               decay=self.decay)
        per_step = (time.perf_counter() - t0) / max(num_steps, 1)
        self.f_ext_batch = r["fhyp"][:H].copy()
        first = np.minimum(phase[None, :].astype(np.int64) + ref_offset[:, None], ref.shape[0] - 1)
        self.last = r
        return {
            "tracking_errors": r["err"],
            "ee_positions": r["ee"],
            "ee_ref_positions": ref[first, :3],
            "joint_positions": r["q"],
            "solve_times": [round(per_step, 5)] * num_steps,  # the device loop's mean time per step
            "best_ids": r["best"],
            "f_ext_best": r["fbest"],
        }

    def run_tracking(self, xstart, ref_traj, sim_dt=0.01, sim_time=5, f_actual=None):
        """One controller tracking ref_traj, as the deployed GATO_Controller does between two joint
        states (gato_controller.py:201-250): the stats of run_tracking_groups with one entry per
        control step (no group axis)."""
        st = self.run_tracking_groups(np.asarray(xstart, float).reshape(1, 12), ref_traj, sim_dt, sim_time, f_actual)
        return {k: (v if k == "solve_times" else v[:, 0]) for k, v in st.items()}

    def run_mpc(self, xstart, endpoints, sim_dt=0.001, sim_time=5, feedback=False):
        """One controller, as the reference's run_mpc (src/gato_mpc_batch_sample.py:106-252):
        (xpath, stats), xpath one q per control step (sim_dt > dt: per plant sub-step) until the
        final goal is reached."""
        xpaths, st = self.run_mpc_groups(np.asarray(xstart, float).reshape(1, 12), endpoints, sim_dt, sim_time,
                                         feedback=feedback)
        self.xpath += xpaths[0]
        if sim_dt > self.dt or feedback:
            keep = np.isfinite(st["goal_distances"][:, 0])
            controls = [u for u in st["control_inputs"][keep, 0]]
        else:
            controls = [st["control_inputs"][0][0]]
        stats = {
            "solve_times": st["solve_times"],
            "goal_distances": [float(d) for d in st["goal_distances"][:, 0] if np.isfinite(d)],
            "control_inputs": controls,
            "best_ids": st["best_ids"][:, 0],
            "f_ext_best": st["f_ext_best"][:, 0],
        }
        return self.xpath, stats
