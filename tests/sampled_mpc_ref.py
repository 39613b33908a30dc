"""Helper (not collected): the sampled-wrench closed loop of include/indy7_mpc.h's
i7m_mpc_run_sampled in numpy — MPC_GATO_Batch_Sample.run_mpc (reference
src/gato_mpc_batch_sample.py:106-300) with the controller's selection / resampling rule
(gato_controller.py:109-129) — on the C++ port's SQP (oracle.cpu.solve / solve_admm with
fext_frame), oracle.rbd.rk4 and oracle.rbd.eepos.  G groups of H hypotheses, group g owning rows
[g H, (g + 1) H).  Besides the device's outputs it returns, per step and group, the two smallest
scoring errors (err2): the argmin is discrete, so a parity test must know how far from a tie it is.
"""
import numpy as np

from oracle import cpu, rbd

GOAL_RADIUS = 0.095


def make_case(G, H, seed, sigma=10.0):
    """The parity tests' inputs: random start states, two distant endpoints, hypotheses N(0, sigma)
    newtons on the force with zero torque and row 0 of every group zero
    (src/gato_mpc_batch_sample.py:37-40), the actual wrench of group g = its hypothesis
    (g + 1) mod H.  Returns (xstart, endpoints, fhyp, f_actual, k) with k (G,) those indices."""
    rng = np.random.default_rng(seed)
    xstart = np.concatenate([rng.uniform(-1, 1, (G, 6)), rng.uniform(-0.5, 0.5, (G, 6))], axis=1)
    endpoints = np.array([rbd.eepos(np.full(6, 0.3)), rbd.eepos(np.full(6, 0.9))])
    fhyp = np.zeros((G, H, 6))
    fhyp[:, :, :3] = rng.normal(0, sigma, (G, H, 3))
    fhyp[:, 0] = 0.0
    k = (np.arange(G) + 1) % H
    f_actual = fhyp[np.arange(G), k].copy()
    return xstart, endpoints, fhyp.reshape(G * H, 6), f_actual, k


def resample(rows, best, noise, keep_best, decay):
    """gato_controller.py:120-129's order on one group's (H, 6) hypotheses; returns the new rows."""
    f_best = rows[best].copy()
    out = np.tile(f_best, (rows.shape[0], 1))
    out[:, :3] += noise
    if keep_best:
        out[best] = f_best
    out[:, 3:] = 0.0
    out[0] = 0.0
    return out * decay


def score(x_last, u_last, xcur, rows, sim_dt, frame):
    """Errors (H,) of every hypothesis's one-step prediction and the winner: the lowest index
    among the minima (`<`, src/gato_mpc_batch_sample.py:287); a NaN never wins, all NaN -> 0."""
    err = np.empty(len(rows))
    for j, f in enumerate(rows):
        if frame == "world":
            qn, vn = rbd.rk4(x_last[:6], x_last[6:], u_last, sim_dt, fext6_world=f)
        else:
            qn, vn = rbd.rk4(x_last[:6], x_last[6:], u_last, sim_dt, fext=rbd.fext_list(x_last[:6], f, "local"))
        err[j] = np.linalg.norm(np.concatenate([qn, vn]) - xcur)
    best, best_err = 0, np.inf
    for j, e in enumerate(err):
        if e < best_err:
            best, best_err = j, e
    return err, best


def run_sampled_ref(N, G, H, xstart, endpoints, num_steps, fhyp, f_actual, noise=None, sim_dt=0.001, frame="world",
                    qp_mode="direct", reset_all=True, keep_best=False, decay=1.0, dt=0.01):
    """qp_mode "direct" (cpu.solve) or "admm" (cpu.solve_admm; reset_all: a fresh AdmmState before
    every solve = I7M_ADMM_RESET_ALL, else the state is carried).  Returns a dict with the device's
    outputs (dist, best, q, fbest, xcur, xu_best, fhyp) and err2 (num_steps, G, 2)."""
    B, T = G * H, 18 * N - 6
    xstart = np.asarray(xstart, float).reshape(G, 12)
    endpoints = np.asarray(endpoints, float).reshape(-1, 3)
    fh = np.array(fhyp, float).reshape(B, 6)
    fa = np.asarray(f_actual, float).reshape(-1, G, 6)
    state = [cpu.AdmmState(B, N)]

    def sqp(xs, goals, XU):
        if qp_mode == "admm":
            if reset_all:
                state[0] = cpu.AdmmState(B, N)
            return cpu.solve_admm(xs, goals, XU, N, state[0], fext=fh, fext_frame=frame, dt=dt)[0]
        return cpu.solve(xs, goals, XU, N, fext=fh, fext_frame=frame, dt=dt)[0]

    goal_idx = np.zeros(G, int)
    alive = np.ones(G, bool)
    goals = np.tile(endpoints[0], (B, N))
    xcur = xstart.copy()
    xs = np.repeat(xstart, H, axis=0)
    XU = np.zeros((B, T))
    XU[:, :12] = xs
    XU_new = sqp(xs, goals, XU)
    xu_best = XU_new[::H].copy()
    out = dict(dist=np.full((num_steps, G), np.nan), best=np.full((num_steps, G), -1, np.int32),
               q=np.full((num_steps, G, 6), np.nan), fbest=np.full((num_steps, G, 6), np.nan),
               err2=np.full((num_steps, G, 2), np.nan))
    for i in range(num_steps):
        x_last, u_last = xcur.copy(), xu_best[:, 12:18].copy()
        run = alive.copy()  # the groups that select at this step
        for g in np.flatnonzero(alive):
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
            d = np.linalg.norm(rbd.eepos(xcur[g, :6]) - goals[g * H, :3])
            out["dist"][i, g] = d
            if d < GOAL_RADIUS:
                if goal_idx[g] < len(endpoints) - 1:
                    goal_idx[g] += 1
                    goals[r] = np.tile(endpoints[goal_idx[g]], N)
                else:
                    alive[g] = run[g] = False
        XU_new = sqp(xs, goals, XU)
        for g in np.flatnonzero(run):
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
