"""Helper (not collected): the multi-rate sampled-wrench closed loops of include/indy7_mpc.h's
i7m_mpc_run_sampled_multirate / i7m_mpc_run_tracking_multirate in numpy — MPC_GATO_Batch_Sample's
loop with its inner plant loop (reference src/gato_mpc_batch_sample.py:163-193) and run_mpc_fig8 of
notebooks/gato_mpc_indy7_fig8.ipynb — on the C++ port's SQP (oracle.cpu.solve / solve_admm with
fext_frame), oracle.rbd.rk4 and oracle.rbd.eepos, with score / resample of tests/sampled_mpc_ref.py,
window of tests/tracking_mpc_ref.py and the schedule of indy7_mpc_amd._lib.multirate_schedule.

Per step the actual wrench is converted to joint 6's frame once, at x_last's q
(rbd.fext_list(q, f, "world")), and held over the step's sub-steps; the hypotheses are scored by ONE
rk4 step of the whole sim_dt.  Besides the device's outputs it returns err2 (the two smallest
scoring errors per step and group) and, in endpoint mode, margin = |d - 0.095|.
"""
import numpy as np

from oracle import cpu, rbd
from sampled_mpc_ref import GOAL_RADIUS, resample, score
from tracking_mpc_ref import window

from indy7_mpc_amd._lib import multirate_schedule


def run_sampled_multirate_ref(N, G, H, xstart, num_steps, fhyp, f_actual, endpoints=None, ref=None, ref_phase=None,
                              noise=None, sim_dt=0.02, frame="world", qp_mode="direct", reset_all=True, keep_best=False,
                              decay=1.0, dt=0.01, shift_warm_start=0, ref_offset=None):
    """Endpoint mode (endpoints (E, 3)) or tracking mode (ref (L, 3) or (L, 6), ref_phase (G,) or
    None).  ref_offset: the window's offsets (num_steps,) instead of the knots completed (the
    self-test against run_tracking_ref uses it).  qp_mode "direct" or "admm" (reset_all: a fresh
    AdmmState before every solve).  Returns dist (endpoints) or err, ee, off (tracking), best, q, u,
    xpath, fbest, xcur, xu_best, fhyp, sub_start, shift, err2 and margin."""
    B, T = G * H, 18 * N - 6
    track = ref is not None
    xstart = np.asarray(xstart, float).reshape(G, 12)
    fh = np.array(fhyp, float).reshape(B, 6)
    fa = np.asarray(f_actual, float).reshape(-1, G, 6)
    sub_start, sub_dt, shift = multirate_schedule(dt, sim_dt, num_steps, N)
    off = np.cumsum(shift) if ref_offset is None else np.asarray(ref_offset, int).reshape(-1)
    state = [cpu.AdmmState(B, N)]

    def sqp(xs, goals, XU):
        if qp_mode == "admm":
            if reset_all:
                state[0] = cpu.AdmmState(B, N)
            return cpu.solve_admm(xs, goals, XU, N, state[0], fext=fh, fext_frame=frame, dt=dt)[0]
        return cpu.solve(xs, goals, XU, N, fext=fh, fext_frame=frame, dt=dt)[0]

    if track:
        ref = np.asarray(ref, float)
        phase = np.zeros(G, int) if ref_phase is None else np.asarray(ref_phase, int).reshape(G)
        goals = np.repeat(np.stack([window(ref, phase[g], 0, N) for g in range(G)]), H, axis=0)
    else:
        endpoints = np.asarray(endpoints, float).reshape(-1, 3)
        goals = np.tile(endpoints[0], (B, N))
    goal_idx = np.zeros(G, int)
    alive = np.ones(G, bool)
    xcur = xstart.copy()
    xs = np.repeat(xstart, H, axis=0)
    XU = np.zeros((B, T))
    XU[:, :12] = xs
    XU_new = sqp(xs, goals, XU)
    xu_best = XU_new[::H].copy()
    out = dict(dist=np.full((num_steps, G), np.nan), best=np.full((num_steps, G), -1, np.int32),
               q=np.full((num_steps, G, 6), np.nan), u=np.full((num_steps, G, 6), np.nan),
               xpath=np.full((sub_start[-1], G, 6), np.nan), ee=np.full((num_steps, G, 3), np.nan),
               fbest=np.full((num_steps, G, 6), np.nan), err2=np.full((num_steps, G, 2), np.nan),
               margin=np.full((num_steps, G), np.nan), sub_start=sub_start, shift=shift,
               off=np.asarray(off[:num_steps], np.int32))
    for i in range(num_steps):
        x_last, u_last = xcur.copy(), xu_best[:, 12:18].copy()
        run = alive.copy()  # the groups that select at this step
        for g in np.flatnonzero(alive):
            f = fa[i if len(fa) > 1 else 0, g]
            held = rbd.fext_list(x_last[g, :6], f, frame)  # converted once, at x_last's q
            q, v = x_last[g, :6].copy(), x_last[g, 6:].copy()
            out["u"][i, g] = u_last[g]
            for s in range(sub_start[i], sub_start[i + 1]):
                q, v = rbd.rk4(q, v, u_last[g], sub_dt[s], fext=held)
                out["xpath"][s, g] = q
            xcur[g] = np.concatenate([q, v])
            out["q"][i, g] = q
            r = slice(g * H, (g + 1) * H)
            xs[r] = xcur[g]
            XU[r, :12] = xcur[g]
            XU[r, 12:] = xu_best[g, 12:]
            sh = 18 * int(shift[i]) if shift_warm_start else 0
            if sh > 0 and T - sh > 12:
                XU[r, 12:T - sh] = xu_best[g, 12 + sh:]
            ee = rbd.eepos(xcur[g, :6])
            if track:
                goals[r] = window(ref, phase[g], off[i], N)
                out["ee"][i, g] = ee
                out["dist"][i, g] = np.linalg.norm(ee - goals[g * H, :3])
                continue
            d = np.linalg.norm(ee - goals[g * H, :3])
            out["dist"][i, g] = d
            out["margin"][i, g] = abs(d - GOAL_RADIUS)
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
    if track:
        out["err"] = out.pop("dist")
    out.update(xcur=xcur, xu_best=xu_best, fhyp=fh)
    return out
