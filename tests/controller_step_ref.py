"""Helper (not collected): the controller session of include/indy7_mpc.h (i7m_ctrl_begin /
i7m_ctrl_step) in numpy — GATO_Controller's constructor and joint_callback (reference
gato_controller.py:174-185,201-250) over G groups of H wrench hypotheses, on a state measured outside
the controller — on the C++ port's SQP (oracle.cpu.solve / solve_admm with fext_frame="world" or
"local"), oracle.rbd.rk4 and oracle.rbd.eepos, with the scoring and resampling of
tests/sampled_mpc_ref.py and the window of tests/tracking_mpc_ref.py.

The measurements are an input: a recorded sequence (steps, G, 12), or a plant callable
measure(i, u_prev) -> (G, 12) that is handed the control the controller returned last (the initial
solve's at i = 0).  HostPlant is the tests' plant: oracle.rbd.rk4 under a constant world wrench.
Like the other helpers it returns, per step and group, the two smallest scoring errors (err2).
"""
import numpy as np

from oracle import cpu, rbd
from sampled_mpc_ref import resample, score
from tracking_mpc_ref import window

ELAPSED = np.array([0.010, 0.008, 0.012, 0.010, 0.009, 0.011])


def schedule(steps, dt=0.01):
    """(elapsed, ref_offset) of the parity cases: the uneven clock cycling through ELAPSED and the
    controller's offset rule int(sum of elapsed / dt) (gato_controller.py:214-215)."""
    el = ELAPSED[np.arange(steps) % len(ELAPSED)]
    return el, (np.cumsum(el) / dt).astype(int)


class HostPlant:
    """The robot outside the controller: G states advanced by one oracle.rbd.rk4 step of `elapsed`
    under the control handed in and the constant world wrench f_actual (G, 6).  With hold_first the
    first measurement is the start state itself (the x0 = NULL form: the controller has seen no
    state yet, so nothing was applied)."""

    def __init__(self, xstart, f_actual, elapsed, hold_first=False):
        self.x = np.array(xstart, float).reshape(-1, 12)
        self.f = np.asarray(f_actual, float).reshape(-1, 6)
        self.elapsed, self.hold_first = np.asarray(elapsed, float), hold_first

    def __call__(self, i, u):
        if i == 0 and self.hold_first:
            return self.x.copy()
        for g in range(len(self.x)):
            qn, vn = rbd.rk4(self.x[g, :6], self.x[g, 6:], u[g], float(self.elapsed[i]), fext6_world=self.f[g])
            self.x[g] = np.concatenate([qn, vn])
        return self.x.copy()


def run_ctrl_ref(N, G, H, ref, fhyp, elapsed, ref_offset, measure, x0=None, ref_phase=None, noise=None, frame="world",
                 qp_mode="direct", reset_all=True, keep_best=False, decay=1.0, dt=0.01):
    """measure: (steps, G, 12) measurements or a callable measure(i, u_prev).  x0 (G, 12): the
    session's first form (x_last = x0, u_last = the initial control); None: the controller's
    constructor (zero state, the first step scores from x_last = x_meas, u_last = 0).  noise
    (steps, G H, 3) or None.  Returns u0 (G, 6) and, per step, u (steps, G, 6), best, fbest, err, ee,
    x_meas, err2 (steps, G, 2); and the final xu_best and fhyp."""
    B, T = G * H, 18 * N - 6
    ref = np.asarray(ref, float)
    elapsed = np.asarray(elapsed, float).reshape(-1)
    ref_offset = np.asarray(ref_offset, int).reshape(-1)
    steps = len(elapsed)
    phase = np.zeros(G, int) if ref_phase is None else np.asarray(ref_phase, int).reshape(G)
    fh = np.array(fhyp, float).reshape(B, 6)
    state = [cpu.AdmmState(B, N)]

    def sqp(xs, goals, XU):
        if qp_mode == "admm":
            if reset_all:
                state[0] = cpu.AdmmState(B, N)
            return cpu.solve_admm(xs, goals, XU, N, state[0], fext=fh, fext_frame=frame, dt=dt)[0]
        return cpu.solve(xs, goals, XU, N, fext=fh, fext_frame=frame, dt=dt)[0]

    # gato_controller.py:174-185
    start = np.zeros((G, 12)) if x0 is None else np.asarray(x0, float).reshape(G, 12)
    goals = np.repeat(np.stack([window(ref, phase[g], 0, N) for g in range(G)]), H, axis=0)
    xs = np.repeat(start, H, axis=0)
    XU = np.zeros((B, T))
    XU[:, :12] = xs
    xu_best = sqp(xs, goals, XU)[::H].copy()
    u_prev = xu_best[:, 12:18].copy()
    x_last, u_last = (None, None) if x0 is None else (start.copy(), u_prev.copy())
    out = dict(u0=u_prev.copy(), u=np.empty((steps, G, 6)), best=np.empty((steps, G), np.int32),
               fbest=np.empty((steps, G, 6)), err=np.empty((steps, G)), ee=np.empty((steps, G, 3)),
               x_meas=np.empty((steps, G, 12)), err2=np.empty((steps, G, 2)))
    for i in range(steps):
        xm = np.array(measure(i, u_prev) if callable(measure) else measure[i], float).reshape(G, 12)
        out["x_meas"][i] = xm
        if x_last is None:  # :205-206
            x_last, u_last = xm.copy(), np.zeros((G, 6))
        best = np.zeros(G, int)
        for g in range(G):
            r = slice(g * H, (g + 1) * H)
            goals[r] = window(ref, phase[g], ref_offset[i], N)
            xs[r] = xm[g]
            XU[r, :12] = xm[g]
            XU[r, 12:] = xu_best[g, 12:]
            out["ee"][i, g] = rbd.eepos(xm[g, :6])
            out["err"][i, g] = np.linalg.norm(out["ee"][i, g] - goals[g * H, :3])
            err, best[g] = score(x_last[g], u_last[g], xm[g], fh[r], float(elapsed[i]), frame)
            e = np.sort(np.where(np.isnan(err), np.inf, err))
            out["err2"][i, g] = [e[0], e[1] if H > 1 else np.inf]
        XU_new = sqp(xs, goals, XU)
        for g in range(G):
            r = slice(g * H, (g + 1) * H)
            out["best"][i, g] = best[g]
            out["fbest"][i, g] = fh[g * H + best[g]]
            xu_best[g] = XU_new[g * H + best[g]]
            if noise is not None:
                fh[r] = resample(fh[r], best[g], np.asarray(noise, float).reshape(steps, B, 3)[i, r], keep_best, decay)
        u_prev = xu_best[:, 12:18].copy()
        out["u"][i] = u_prev
        x_last, u_last = xm.copy(), u_prev.copy()
    out.update(xu_best=xu_best, fhyp=fh)
    return out
