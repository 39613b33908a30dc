"""Helper (not collected): the multi-rate sampled-wrench closed loops under the winner's feedback
policy (i7m_sampled_multirate_opts.control_from = I7M_CONTROL_POLICY; csrc/i7m_mpc_sampled_policy.h)
in numpy.  It is tests/sampled_multirate_ref.py's loop, copied, with the plant and the score changed:

  plant   sub-step s of a step begins at plant state x with j = the knots the step has completed and
          is driven by u_s = XU_best[g].u_j + K_j (x - XU_best[g].x_j).  K_j comes from
          policy_ref.riccati_gains (float64) on the blocks of OSQPSolverRef(N, dt, fext6 = the selected
          row's wrench as the solve used it, fext_frame = frame), linearised at that row's solve
          result with x_0 = the row's state: the blocks policy_ref.qp_blocks builds without a wrench.
  score   hypothesis h replays the step: from x_last the same sub-steps of the same lengths under the
          RECORDED controls u_s, wrench row h converted once at x_last's q; err_h = |replay - xcur|.

`gains`: "riccati" (above), or "zero" (K = 0: sub-step s is driven by XU_best[g].u_j alone).
Besides run_sampled_multirate_ref's outputs it returns jmax, the highest knot index a sub-step began
in.  policy_cases() are the inputs the GPU parity tests use; tests/test_sampled_policy_ref_self.py
vets them on this loop alone.
"""
import functools

import numpy as np
from scipy.sparse import diags

from indy7_mpc_amd._lib import multirate_schedule
from indy7_mpc_amd.utils import figure8
from oracle import cpu, rbd
from oracle.osqp_ref import OSQPSolverRef
from policy_ref import NU, NX, riccati_gains
from sampled_mpc_ref import GOAL_RADIUS, make_case, resample
from tracking_mpc_ref import make_tracking_case, window


def qp_blocks_wrench(xu, xs, goals, N, fext6, frame, dt=0.01):
    """policy_ref.qp_blocks with the row's joint-6 wrench in the dynamics: the stage blocks of the QP
    linearised at xu with x_0 row xs."""
    s = OSQPSolverRef(N=N, dt=dt, fext6=fext6, fext_frame=frame)
    s.update_constraint_matrix(np.asarray(xu, float), np.asarray(xs, float))
    s.update_cost_matrix(np.asarray(xu, float), np.asarray(goals, float).reshape(3 * N))
    P, Am = s.matrices()
    Pf = (P + P.T - diags(P.diagonal())).toarray()
    Ad = Am.toarray()
    out = dict(A=np.zeros((N - 1, NX, NX)), B=np.zeros((N - 1, NX, NU)), c=np.zeros((N - 1, NX)), Q=np.zeros((N, NX, NX)),
               q=np.zeros((N, NX)), R=np.zeros((N - 1, NU, NU)), r=np.zeros((N - 1, NU)), solver=s)
    for k in range(N):
        o = 18 * k
        out["Q"][k] = Pf[o:o + NX, o:o + NX]
        out["q"][k] = s.g[o:o + NX]
        if k < N - 1:
            rows = slice(NX * (k + 1), NX * (k + 2))
            out["A"][k] = Ad[rows, o:o + NX]
            out["B"][k] = Ad[rows, o + NX:o + 18]
            out["c"][k] = -s.l[rows]
            out["R"][k] = Pf[o + NX:o + 18, o + NX:o + 18]
            out["r"][k] = s.g[o + NX:o + 18]
            assert not Pf[o:o + NX, o + NX:o + 18].any()  # no state-control cross term
    return out


def replay_score(x_last, us, sub_dt, xcur, rows, frame):
    """Errors (H,) of every hypothesis's replay of the step (the sub-steps sub_dt under the recorded
    controls us, its wrench converted once at x_last's q) and the winner: the lowest index among the
    minima; a NaN never wins, all NaN -> 0."""
    err = np.empty(len(rows))
    for h, f in enumerate(rows):
        held = rbd.fext_list(x_last[:6], f, frame)
        q, v = x_last[:6].copy(), x_last[6:].copy()
        for u, ts in zip(us, sub_dt):
            q, v = rbd.rk4(q, v, u, ts, fext=held)
        err[h] = np.linalg.norm(np.concatenate([q, v]) - xcur)
    best, best_err = 0, np.inf
    for h, e in enumerate(err):
        if e < best_err:
            best, best_err = h, e
    return err, best


def run_sampled_policy_ref(N, G, H, xstart, num_steps, fhyp, f_actual, endpoints=None, ref=None, ref_phase=None,
                           noise=None, sim_dt=0.02, frame="world", qp_mode="direct", reset_all=True, keep_best=False,
                           decay=1.0, dt=0.01, shift_warm_start=0, gains="riccati"):
    """Endpoint mode (endpoints (E, 3)) or tracking mode (ref (L, 3) or (L, 6), ref_phase (G,) or
    None), as run_sampled_multirate_ref.  Returns dist (endpoints) or err, ee, off (tracking), best,
    q, u, xpath, fbest, xcur, xu_best, fhyp, sub_start, shift, err2, margin and jmax."""
    B, T = G * H, 18 * N - 6
    track = ref is not None
    xstart = np.asarray(xstart, float).reshape(G, 12)
    fh = np.array(fhyp, float).reshape(B, 6)
    fa = np.asarray(f_actual, float).reshape(-1, G, 6)
    sub_start, sub_dt, shift, knot = multirate_schedule(dt, sim_dt, num_steps, N, knots=True)
    off = np.cumsum(shift)
    state = [cpu.AdmmState(B, N)]

    def sqp(xs, goals, XU):
        if qp_mode == "admm":
            if reset_all:
                state[0] = cpu.AdmmState(B, N)
            return cpu.solve_admm(xs, goals, XU, N, state[0], fext=fh, fext_frame=frame, dt=dt)[0]
        return cpu.solve(xs, goals, XU, N, fext=fh, fext_frame=frame, dt=dt)[0]

    def gains_of(XU_new, xs, goals, row):
        """K (N - 1, 6, 12) of row `row` of the solve just run (its wrench fh[row], before any resample)"""
        if gains == "zero":
            return np.zeros((N - 1, NU, NX))
        return riccati_gains(qp_blocks_wrench(XU_new[row], xs[row], goals[row], N, fh[row].copy(), frame, dt))[:, :, :NX]

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
    K = [gains_of(XU_new, xs, goals, g * H) for g in range(G)]  # the initial solve's row 0
    out = dict(dist=np.full((num_steps, G), np.nan), best=np.full((num_steps, G), -1, np.int32),
               q=np.full((num_steps, G, 6), np.nan), u=np.full((num_steps, G, 6), np.nan),
               xpath=np.full((sub_start[-1], G, 6), np.nan), ee=np.full((num_steps, G, 3), np.nan),
               fbest=np.full((num_steps, G, 6), np.nan), err2=np.full((num_steps, G, 2), np.nan),
               margin=np.full((num_steps, G), np.nan), sub_start=sub_start, shift=shift,
               off=np.asarray(off[:num_steps], np.int32), jmax=np.zeros((), int))
    for i in range(num_steps):
        x_last = xcur.copy()
        us = {}
        run = alive.copy()  # the groups that select at this step
        steps = range(sub_start[i], sub_start[i + 1])
        for g in np.flatnonzero(alive):
            f = fa[i if len(fa) > 1 else 0, g]
            held = rbd.fext_list(x_last[g, :6], f, frame)  # converted once, at x_last's q
            q, v = x_last[g, :6].copy(), x_last[g, 6:].copy()
            out["u"][i, g] = xu_best[g, 12:18]
            us[g] = []
            for s in steps:
                j = int(knot[s])
                out["jmax"][...] = max(int(out["jmax"]), j)
                u = xu_best[g, 18 * j + 12:18 * j + 18] + K[g][j] @ (np.concatenate([q, v]) - xu_best[g, 18 * j:18 * j + 12])
                us[g].append(u)
                q, v = rbd.rk4(q, v, u, sub_dt[s], fext=held)
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
            err, best = replay_score(x_last[g], us[g], sub_dt[steps.start:steps.stop], xcur[g], fh[r], frame)
            e = np.sort(np.where(np.isnan(err), np.inf, err))
            out["err2"][i, g] = [e[0], e[1] if H > 1 else np.inf]
            out["best"][i, g] = best
            out["fbest"][i, g] = fh[g * H + best]
            xu_best[g] = XU_new[g * H + best]
            K[g] = gains_of(XU_new, xs, goals, g * H + best)  # before the resample: the wrench the solve used
            if noise is not None:
                fh[r] = resample(fh[r], best, np.asarray(noise, float).reshape(num_steps, B, 3)[i, r], keep_best, decay)
    if track:
        out["err"] = out.pop("dist")
    out.update(xcur=xcur, xu_best=xu_best, fhyp=fh)
    return out


# ---- the parity tests' inputs (tests/test_gpu_sampled_policy.py), vetted by the CPU self-test ----------

G, H, N = 2, 4, 8
SHAPES = [(0.025, 6), (0.001, 12)]  # (sim_dt, steps): j up to 2 within a step; step 9's residue sub-step
REF = figure8(0.5, 0.55, [0, 0.4, 0.45], period=1.0, dt=0.01, cycles=3).reshape(-1, 6)
REF.setflags(write=False)
PHASES = (3, 40)
RESAMPLE = dict(keep_best=True, decay=0.97)
NOISE_STD = 6.0


@functools.lru_cache(maxsize=None)
def policy_case(source, sim_dt):
    """dict of the loop's inputs for a goal source and a shape.  Endpoints: group 0 starts at rest at
    q = 0.31, within the radius of both endpoints eepos(0.3), eepos(0.33): it switches at step 0 and
    stops at step 1; group 1 runs on.  Tracking: make_tracking_case on the figure 8.  The actual wrench
    of group g is its hypothesis (g + 1) mod H; resampling noise N(0, NOISE_STD) newtons, kept best."""
    steps = dict(SHAPES)[sim_dt]
    noise = np.random.default_rng(11).normal(0, NOISE_STD, (steps, G * H, 3))
    if source == "endpoints":
        xs, _, fhyp, fact, k = make_case(G, H, seed=1)
        xs = xs.copy()
        xs[0] = 0.0
        xs[0, :6] = 0.31
        ends = np.array([rbd.eepos(np.full(6, 0.3)), rbd.eepos(np.full(6, 0.33))])
        c = dict(xstart=xs, fhyp=fhyp, f_actual=fact, endpoints=ends, k=k)
    else:
        xs, fhyp, fact, k = make_tracking_case(G, H, seed=3)
        c = dict(xstart=xs, fhyp=fhyp, f_actual=fact, ref=REF, ref_phase=PHASES, k=k)
    c.update(num_steps=steps, noise=noise, sim_dt=sim_dt)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def loop_kwargs(c):
    """policy_case's dict as run_sampled_policy_ref's / run_sampled_multirate_ref's keyword arguments"""
    kw = {k: v for k, v in c.items() if k not in ("k", "xstart", "num_steps", "fhyp", "f_actual")}
    kw.update(RESAMPLE)
    return kw


@functools.lru_cache(maxsize=None)
def policy_reference(source, sim_dt, mode):
    """run_sampled_policy_ref on policy_case, computed once and left unchanged"""
    c = policy_case(source, sim_dt)
    r = run_sampled_policy_ref(N, G, H, c["xstart"], c["num_steps"], c["fhyp"], c["f_actual"], qp_mode=mode, **loop_kwargs(c))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r
