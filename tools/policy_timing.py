#!/usr/bin/env python3
"""GPU: what the feedback policy costs and what it does.

cost      i7m_mpc_run_multirate at B x N (default 4096 x 32), sim_dt = 0.02, I7M_QP_DIRECT and
          I7M_QP_ADMM: ms per MPC step with control_from "new" and "policy" in alternating repetitions
          (a call of warm + steps minus a call of warm, over steps, so allocation, copies and the
          initial solve cancel), and the HIP-event sums of k_linearize and k_riccati per step in both:
          their difference is the policy pass; the rest of the wall-clock difference is the policy
          step kernel against the step kernel it replaces.
tracking  an MPC_GATO-shaped run (20 ms per solve, N = 32, goal radius 1e-2) of 64 instances from
          synthetic_batch's start states towards one endpoint: the mean goal distance over the run
          with control_from "prev" (MPC_GATO), "new" and "policy" on the device loop; then the same
          loop composed on the host from the solve, qp_policy and rk4 hooks with the plant under a
          constant world wrench the controller does not know (the device plant has none).

Prints and writes (--out) one JSON object.  One process; run it under `timeout`.  Not a test, and
nothing is asserted: it reports, whatever the sign.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def per_step(run, h, warm, steps):
    t = []
    for n in (warm + steps, warm):
        h.reset()
        t0 = time.perf_counter()
        run(n)
        t.append(time.perf_counter() - t0)
    return 1e3 * (t[0] - t[1]) / steps


def cost(lib, model, B, N, sim_dt, warm, steps, reps, xs, ends):
    res = []
    for mode, name in ((lib.QP_DIRECT, "direct"), (lib.QP_ADMM, "admm")):
        h = lib.Handle(model, N=N, max_batch=B, qp_mode=mode)
        runs = {c: (lambda n, c=c: h.mpc_run_multirate(xs, ends, n, sim_dt=sim_dt, goal_radius=1e-2, control_from=c))
                for c in ("new", "policy")}
        for run in runs.values():
            run(2)  # first-use costs out of the way
        ms = {c: [] for c in runs}
        for _ in range(reps):
            for c, run in runs.items():
                ms[c].append(per_step(run, h, warm, steps))
        kern = {}
        for c, run in runs.items():
            h.reset()
            h.set_timing(True)
            h.reset_kernel_times()
            run(warm + steps)
            kt = h.kernel_times()
            h.set_timing(False)
            # per MPC step of the run; the initial solve's launches are in the sums (1 of warm + steps + 1)
            kern[c] = {k: {"ms_per_step": v[0] / (warm + steps), "launches": int(v[1])} for k, v in kt.items() if v[1]}
        med = {c: float(np.median(v)) for c, v in ms.items()}
        zero = {"ms_per_step": 0.0, "launches": 0}  # (an ADMM solve launches no k_riccati)
        pass_ms = sum(kern["policy"].get(k, zero)["ms_per_step"] - kern["new"].get(k, zero)["ms_per_step"]
                      for k in ("k_linearize", "k_riccati"))
        pass_launches = {k: (kern["policy"].get(k, zero)["launches"] - kern["new"].get(k, zero)["launches"]) / (warm + steps)
                         for k in ("k_linearize", "k_riccati")}
        res.append({"B": B, "N": N, "qp_mode": name, "sim_dt": sim_dt, "warm": warm, "steps": steps, "ms_per_step": ms,
                    "median_ms_per_step": med, "policy_minus_new_ms": med["policy"] - med["new"],
                    "policy_pass_event_ms_per_step": pass_ms, "policy_pass_launches_per_step": pass_launches,
                    "step_kernel_and_launch_remainder_ms": med["policy"] - med["new"] - pass_ms, "kernels": kern})
        print(json.dumps(res[-1]), flush=True)
        h.close()
    return res


def host_run(lib, h, xs, end, steps, sim_dt, control, wrench):
    """The multi-rate loop from the hooks, one endpoint, no goal switch or stop; the plant under a
    constant world wrench (or none).  Returns the distances (steps, B) before each step's plant."""
    N, B, T = h.N, xs.shape[0], h.T
    sub_start, sub_dt, shift, knot = lib.multirate_schedule(h.cfg.dt, sim_dt, steps, N, knots=True)
    admm = h.cfg.qp_mode == lib.QP_ADMM
    goals = np.tile(end, (B, N))
    xcur = xs.copy()
    XU = np.zeros((B, T))
    XU[:, :12] = xcur
    if admm:
        h.admm_reset(B)
    XU = h.solve(xcur, goals, XU)[0]
    f = None if wrench is None else np.tile(wrench, (B, 1))
    dist = np.zeros((steps, B))
    for i in range(steps):
        if admm:
            h.admm_reset(B)
        xu_new = h.solve(xcur, goals, XU)[0]
        K = h.qp_policy(xu_new, xcur, goals, N - 1) if control == "policy" else None
        dist[i] = np.linalg.norm(h.eepos(xcur[:, :6]) - end, axis=1)
        q, v = xcur[:, :6].copy(), xcur[:, 6:].copy()
        for s in range(sub_start[i], sub_start[i + 1]):
            j = knot[s]
            if control == "policy":
                dx = np.hstack([q, v]) - xu_new[:, 18 * j:18 * j + 12]
                u = xu_new[:, 18 * j + 12:18 * j + 18] + np.einsum("bij,bj->bi", K[:, j, :, :12], dx)
            else:
                u = (xu_new if control == "new" else XU)[:, 12:18]
            q, v = h.rk4(q, v, u, sub_dt[s], fext=f, frame="world")
        xcur = np.hstack([q, v])
        if shift[i] > 0:
            XU[:, :T - 18 * shift[i]] = xu_new[:, 18 * shift[i]:]
        XU[:, :12] = xcur
        XU[:, -12:] = [1.0] * 6 + [0.0] * 6
    return dist


def tracking(lib, model, B, N, sim_dt, steps, wrench):
    from oracle.osqp_ref import synthetic_batch

    xs = synthetic_batch(B, N, seed=7)[0]
    res = []
    for mode, name in ((lib.QP_DIRECT, "direct"), (lib.QP_ADMM, "admm")):
        h = lib.Handle(model, N=N, max_batch=B, qp_mode=mode)
        end = h.eepos(np.full((1, 6), 0.3))[0]
        far = end[None]  # one endpoint and radius 0: no switch, no stop, every instance tracks the point
        rec = {"B": B, "N": N, "qp_mode": name, "sim_dt": sim_dt, "steps": steps, "endpoint": end.tolist(),
               "device_loop": {}, "host_loop_no_wrench": {}, "host_loop_unknown_wrench": {}, "wrench_world": list(wrench)}
        for c in ("prev", "new", "policy"):
            r = h.mpc_run_multirate(xs, far, steps, sim_dt=sim_dt, goal_radius=0.0, control_from=c)
            rec["device_loop"][c] = {"mean_goal_distance": float(np.mean(r["dist"])), "final_mean": float(np.mean(r["dist"][-1]))}
            for key, w in (("host_loop_no_wrench", None), ("host_loop_unknown_wrench", np.asarray(wrench, float))):
                d = host_run(lib, h, xs, end, steps, sim_dt, c, w)
                rec[key][c] = {"mean_goal_distance": float(np.mean(d)), "final_mean": float(np.mean(d[-1]))}
        res.append(rec)
        print(json.dumps(rec), flush=True)
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="4096x32", help="BxN of the cost part")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--track-steps", type=int, default=50)
    ap.add_argument("--wrench", default="0,0,-10,0,0,0", help="world wrench on joint 6 the controller does not know")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_timing.json"))
    a = ap.parse_args()
    from indy7_mpc_amd import _lib as lib
    from indy7_mpc_amd.model import default_model
    from multirate_loop_timing import case

    model = default_model()
    q = lib.Handle(model, N=2, max_batch=2)
    ends = q.eepos(np.array([np.full(6, 0.3), np.full(6, 0.9)]))
    B, N = (int(v) for v in a.shape.split("x"))
    out = {"tool": "tools/policy_timing.py", "version": lib.version(),
           "cost": cost(lib, model, B, N, 0.02, a.warm, a.steps, a.reps, case(B, 11, q.eepos, ends), ends),
           "tracking": tracking(lib, model, 64, 32, 0.02, a.track_steps, [float(v) for v in a.wrench.split(",")])}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
