"""Helper (not collected): the multi-rate closed loop of include/indy7_mpc.h's
i7m_mpc_run_multirate in numpy — MPC_GATO_Batch.run_mpc (reference src/gato_mpc_batch.py:76-217) and,
with control "prev", MPC_GATO.run_mpc (src/gato_mpc.py:53-150) — on the C++ port's SQP
(oracle.cpu.solve / solve_admm), oracle.rbd.rk4 and oracle.rbd.eepos, B independent instances.
Besides the device's outputs it returns, per step and instance, the margin |d - radius|: the goal
switch and the stop are discrete, so a parity test must know how far from the radius every
distance is.
"""
import numpy as np

from oracle import cpu, rbd

from indy7_mpc_amd._lib import multirate_schedule


def make_case():
    """The tests' four instances and two endpoints: row 0 at q = 0.31 (within 0.1 of endpoint 0, so
    it switches at step 0, and within 0.1 of endpoint 1, so it stops at step 1), rows 1 and 3
    random, row 2 at q = 0.6."""
    rng = np.random.default_rng(8)
    xs = np.zeros((4, 12))
    xs[0, :6] = 0.31
    xs[1, :6] = rng.uniform(-1, 1, 6)
    xs[1, 6:] = rng.uniform(-0.5, 0.5, 6)
    xs[2, :6] = 0.6
    xs[3, :6] = rng.uniform(-1, 1, 6)
    xs[3, 6:] = rng.uniform(-0.5, 0.5, 6)
    endpoints = np.array([rbd.eepos(np.full(6, 0.3)), rbd.eepos(np.full(6, 0.33))])
    return xs, endpoints


def run_multirate_ref(N, xstart, endpoints, num_steps, dt=0.01, sim_dt=0.001, radius=0.1, control="new",
                      qp_mode="direct", reset_all=True):
    """qp_mode "direct" (cpu.solve) or "admm" (cpu.solve_admm; reset_all: a fresh AdmmState before
    every solve = I7M_ADMM_RESET_ALL, else the state is carried).  Returns a dict with the device's
    outputs (dist, q, u, xpath, xcur, xu, sub_start, shift), u0 (B, 6) the initial solve's first
    control and margin (num_steps, B)."""
    xstart = np.asarray(xstart, float).reshape(-1, 12)
    endpoints = np.asarray(endpoints, float).reshape(-1, 3)
    B, T = xstart.shape[0], 18 * N - 6
    sub_start, sub_dt, shift = multirate_schedule(dt, sim_dt, num_steps, N)
    state = [cpu.AdmmState(B, N)]

    def sqp(xs, goals, XU):
        if qp_mode == "admm":
            if reset_all:
                state[0] = cpu.AdmmState(B, N)
            return cpu.solve_admm(xs, goals, XU, N, state[0], dt=dt)[0]
        return cpu.solve(xs, goals, XU, N, dt=dt)[0]

    goal_idx = np.zeros(B, int)
    alive = np.ones(B, bool)
    goals = np.tile(endpoints[0], (B, N))
    xcur = xstart.copy()
    XU = np.zeros((B, T))
    XU[:, :12] = xcur
    XU = np.array(sqp(xcur, goals, XU))
    out = dict(dist=np.full((num_steps, B), np.nan), q=np.full((num_steps, B, 6), np.nan),
               u=np.full((num_steps, B, 6), np.nan), xpath=np.full((sub_start[-1], B, 6), np.nan),
               margin=np.full((num_steps, B), np.nan), u0=XU[:, 12:18].copy(), sub_start=sub_start, shift=shift)
    for i in range(num_steps):
        xu_new = sqp(xcur, goals, XU)  # against the goal before this step's switch
        for b in np.flatnonzero(alive):
            d = np.linalg.norm(rbd.eepos(xcur[b, :6]) - goals[b, :3])
            out["dist"][i, b] = d
            out["margin"][i, b] = abs(d - radius)
            out["u"][i, b] = XU[b, 12:18]
            if d < radius:
                if goal_idx[b] < len(endpoints) - 1:
                    goal_idx[b] += 1
                    goals[b] = np.tile(endpoints[goal_idx[b]], N)
                else:
                    alive[b] = False
                    continue
            u = (xu_new if control == "new" else XU)[b, 12:18].copy()  # knot 0's: the accumulator stays below dt
            q, v = xcur[b, :6].copy(), xcur[b, 6:].copy()
            for s in range(sub_start[i], sub_start[i + 1]):
                q, v = rbd.rk4(q, v, u, sub_dt[s])
                out["xpath"][s, b] = q
            xcur[b] = np.concatenate([q, v])
            out["q"][i, b] = q
            if shift[i] > 0:
                XU[b, :T - 18 * shift[i]] = xu_new[b, 18 * shift[i]:]
            XU[b, :12] = xcur[b]
            XU[b, -12:] = [1.0] * 6 + [0.0] * 6
    out.update(xcur=xcur, xu=XU)
    return out
