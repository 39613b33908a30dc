"""Helper (not collected): the reference-tracking closed loop of include/indy7_mpc.h's
i7m_mpc_run_tracking in numpy — the deployed controller's loop (GATO_Controller.joint_callback,
reference gato_controller.py:201-250) over G groups of H wrench hypotheses — on the C++ port's SQP
(oracle.cpu.solve / solve_admm with fext_frame), oracle.rbd.rk4 and oracle.rbd.eepos, with the
scoring and resampling of tests/sampled_mpc_ref.py.  It is run_sampled_ref with the goal source
replaced: at step i every row of group g is solved against the window
ref[min(phase[g] + ref_offset[i] + k, L - 1)], k = 0 .. N-1, the error is measured against the
window's first point, and no group ever stops.  Like that helper it returns, per step and group,
the two smallest scoring errors (err2).
"""
import numpy as np

from oracle import cpu, rbd
from sampled_mpc_ref import resample, score


def make_tracking_case(G, H, seed, sigma=10.0):
    """The parity tests' inputs: random start states, hypotheses N(0, sigma) newtons on the force
    with zero torque and row 0 of every group zero, the actual wrench of group g = its hypothesis
    (g + 1) mod H.  Returns (xstart, fhyp, f_actual, k) with k (G,) those indices."""
    rng = np.random.default_rng(seed)
    xstart = np.concatenate([rng.uniform(-1, 1, (G, 6)), rng.uniform(-0.5, 0.5, (G, 6))], axis=1)
    fhyp = np.zeros((G, H, 6))
    fhyp[:, :, :3] = rng.normal(0, sigma, (G, H, 3))
    fhyp[:, 0] = 0.0
    k = (np.arange(G) + 1) % H
    return xstart, fhyp.reshape(G * H, 6), fhyp[np.arange(G), k].copy(), k


def window(ref, ph, off, N):
    """(3 N,) the N-knot goal window at phase ph and offset off, held at the last point."""
    idx = np.minimum(ph + off + np.arange(N), len(ref) - 1)
    return ref[idx, :3].reshape(-1)


def run_tracking_ref(N, G, H, xstart, ref, ref_offset, fhyp, f_actual, ref_phase=None, noise=None, sim_dt=0.01,
                     frame="world", qp_mode="direct", reset_all=True, keep_best=False, decay=1.0, dt=0.01):
    """ref (L, 3) or (L, 6); ref_offset (num_steps,) ints; ref_phase (G,) ints or None.  qp_mode
    "direct" (cpu.solve) or "admm" (cpu.solve_admm; reset_all: a fresh AdmmState before every solve
    = I7M_ADMM_RESET_ALL, else the state is carried).  Returns the device's outputs (err, best, q,
    ee, fbest, xcur, xu_best, fhyp) and err2 (num_steps, G, 2)."""
    B, T = G * H, 18 * N - 6
    xstart = np.asarray(xstart, float).reshape(G, 12)
    ref = np.asarray(ref, float)
    ref_offset = np.asarray(ref_offset, int).reshape(-1)
    num_steps = len(ref_offset)
    phase = np.zeros(G, int) if ref_phase is None else np.asarray(ref_phase, int).reshape(G)
    fh = np.array(fhyp, float).reshape(B, 6)
    fa = np.asarray(f_actual, float).reshape(-1, G, 6)
    state = [cpu.AdmmState(B, N)]

    def sqp(xs, goals, XU):
        if qp_mode == "admm":
            if reset_all:
                state[0] = cpu.AdmmState(B, N)
            return cpu.solve_admm(xs, goals, XU, N, state[0], fext=fh, fext_frame=frame, dt=dt)[0]
        return cpu.solve(xs, goals, XU, N, fext=fh, fext_frame=frame, dt=dt)[0]

    goals = np.repeat(np.stack([window(ref, phase[g], 0, N) for g in range(G)]), H, axis=0)
    xcur = xstart.copy()
    xs = np.repeat(xstart, H, axis=0)
    XU = np.zeros((B, T))
    XU[:, :12] = xs
    XU_new = sqp(xs, goals, XU)
    xu_best = XU_new[::H].copy()
    out = dict(err=np.full((num_steps, G), np.nan), best=np.full((num_steps, G), -1, np.int32),
               q=np.full((num_steps, G, 6), np.nan), ee=np.full((num_steps, G, 3), np.nan),
               fbest=np.full((num_steps, G, 6), np.nan), err2=np.full((num_steps, G, 2), np.nan))
    for i in range(num_steps):
        x_last, u_last = xcur.copy(), xu_best[:, 12:18].copy()
        for g in range(G):
            f = fa[i if len(fa) > 1 else 0, g]
            if frame == "world":
                qn, vn = rbd.rk4(x_last[g, :6], x_last[g, 6:], u_last[g], sim_dt, fext6_world=f)
            else:
                qn, vn = rbd.rk4(x_last[g, :6], x_last[g, 6:], u_last[g], sim_dt,
                                 fext=rbd.fext_list(x_last[g, :6], f, "local"))
            xcur[g] = np.concatenate([qn, vn])
            out["q"][i, g] = qn
            r = slice(g * H, (g + 1) * H)
            xs[r] = xcur[g]
            XU[r, :12] = xcur[g]
            XU[r, 12:] = xu_best[g, 12:]
            goals[r] = window(ref, phase[g], ref_offset[i], N)
            out["ee"][i, g] = rbd.eepos(xcur[g, :6])
            out["err"][i, g] = np.linalg.norm(out["ee"][i, g] - goals[g * H, :3])
        XU_new = sqp(xs, goals, XU)
        for g in range(G):
            r = slice(g * H, (g + 1) * H)
            err, best = score(x_last[g], u_last[g], xcur[g], fh[r], sim_dt, frame)
            e = np.sort(np.where(np.isnan(err), np.inf, err))
            out["err2"][i, g] = [e[0], e[1] if H > 1 else np.inf]
            out["best"][i, g] = best
            out["fbest"][i, g] = fh[g * H + best]
            xu_best[g] = XU_new[g * H + best]
            if noise is not None:
                fh[r] = resample(fh[r], best, np.asarray(noise, float).reshape(num_steps, B, 3)[i, r], keep_best, decay)
    out.update(xcur=xcur, xu_best=xu_best, fhyp=fh)
    return out
