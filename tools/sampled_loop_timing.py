#!/usr/bin/env python3
"""GPU: time the sampled-wrench closed loop (G controllers x H hypotheses) two ways on the same
tree, both in the default ADMM mode with the OSQP state reset before every solve and resampling on:

  device  one i7m_mpc_run_sampled call (csrc/i7m_mpc_sampled.h): no host round trip per step;
  host    the loop the reference drives from Python, one round trip per step through the
          batch_sqp surface: reset() + resetRho(), solve(), sim_forward(), numpy argmin,
          set_external_wrench_batch().  G = 1 uses bindings.batch_sqp.SQPSolverfloat_H itself; for
          G > 1 (batch_sqp stops at 256 rows) the same calls go to one Handle of G H rows, which
          is what batch_sqp wraps (Handle.reset / admm_reset / solve / rk4 / set_external_wrench).

Prints and writes (--out) one JSON object: per shape the wall time per MPC step and
instance-steps/s = G H steps / time of both.  One process, one run per shape after a warm-up run;
run it under `timeout`.  Not a test, and no ratio is asserted: it reports.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def case(G, H, steps, seed, eepos, ends):
    """Start states at least 0.3 from both endpoints (redrawn otherwise): no group reaches a goal
    within the timed steps, so the host loop needs no goal logic to stay comparable."""
    rng = np.random.default_rng(seed)
    xs = np.concatenate([rng.uniform(-1, 1, (G, 6)), rng.uniform(-0.5, 0.5, (G, 6))], axis=1)
    for _ in range(100):
        near = np.linalg.norm(eepos(xs[:, :6])[:, None] - ends[None], axis=2).min(axis=1) < 0.3
        if not near.any():
            break
        xs[near, :6] = rng.uniform(-1, 1, (int(near.sum()), 6))
    fh = np.zeros((G, H, 6))
    fh[:, :, :3] = rng.normal(0, 10.0, (G, H, 3))
    fh[:, 0] = 0.0
    fact = fh[np.arange(G), (np.arange(G) + 1) % H].copy()
    noise = rng.normal(0, 2.0, (steps, G * H, 3))
    return xs, fh.reshape(G * H, 6), fact, noise


def resample(rows, best, noise, H):
    """gato_controller.py:120-129 with keep_best, decay 0.97, per group of H rows."""
    G = rows.shape[0] // H
    r = rows.reshape(G, H, 6)
    fb = r[np.arange(G), best].copy()
    out = np.repeat(fb[:, None], H, axis=1)
    out[:, :, :3] += noise.reshape(G, H, 3)
    out[np.arange(G), best] = fb
    out[:, :, 3:] = 0.0
    out[:, 0] = 0.0
    return (out * 0.97).reshape(G * H, 6)


def host_loop(lib, model, G, H, N, steps, xs, ends, fh, fact, noise, sim_dt):
    """The per-step host round trip.  Returns (seconds for `steps` steps, best (steps, G))."""
    from indy7_mpc_amd.bindings import batch_sqp

    B, T = G * H, 18 * N - 6
    if G == 1:
        s = getattr(batch_sqp, f"SQPSolverfloat_{H}")(model)
        s.set_external_wrench_batch(fh)
        reset = lambda: (s.reset(), s.resetRho())  # noqa: E731
        solve = lambda x, g, xu: s.solve(xu, 0.01, x, g)["xu_trajectory"]  # noqa: E731
        sim = lambda x, u, f: s.sim_forward(x[0], u[0], sim_dt)  # noqa: E731
        set_f = s.set_external_wrench_batch
        goals = np.tile(np.concatenate([ends[0], np.zeros(3)]), (B, N))
        plant = lib.Handle(model, N=2, max_batch=1)
    else:
        h = lib.Handle(model, N=N, max_batch=B, qp_mode=lib.QP_ADMM)
        h.set_external_wrench(fh, "world")
        reset = lambda: (h.reset(), h.admm_reset(what=lib.ADMM_RESET_RHO))  # noqa: E731
        solve = lambda x, g, xu: h.solve(x, g, xu)[0]  # noqa: E731

        def sim(x, u, f):
            qo, vo = h.rk4(np.repeat(x[:, :6], H, 0), np.repeat(x[:, 6:], H, 0), np.repeat(u, H, 0), sim_dt, fext=f,
                           frame="world")
            return np.hstack([qo, vo])

        set_f = lambda f: h.set_external_wrench(f, "world")  # noqa: E731
        goals = np.tile(ends[0], (B, N))
        plant = h
    f = fh.copy()
    xcur = xs.copy()
    xrows = np.repeat(xcur, H, 0)
    XU = np.zeros((B, T))
    XU[:, :12] = xrows
    xu_best = solve(xrows, goals, XU)[::H].copy()
    bests = np.zeros((steps, G), int)
    t0 = time.perf_counter()
    for i in range(steps):
        x_last, u_last = xcur.copy(), xu_best[:, 12:18].copy()
        qo, vo = plant.rk4(x_last[:, :6], x_last[:, 6:], u_last, sim_dt, fext=fact, frame="world")
        xcur = np.hstack([qo, vo])
        xrows = np.repeat(xcur, H, 0)
        XU[:, :12] = xrows
        XU[:, 12:] = np.repeat(xu_best[:, 12:], H, 0)
        reset()
        XU_new = solve(xrows, goals, XU)
        pred = sim(x_last, u_last, f)
        err = np.linalg.norm(pred.reshape(G, H, 12) - xcur[:, None], axis=2)
        best = err.argmin(axis=1)
        bests[i] = best
        xu_best = XU_new[np.arange(G) * H + best]
        f = resample(f, best, noise[i], H)
        set_f(f)
    return time.perf_counter() - t0, bests


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shapes", default="1x16x64,256x16x32", help="GxHxN, comma separated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_loop_timing.json"))
    a = ap.parse_args()
    from indy7_mpc_amd import _lib as lib
    from indy7_mpc_amd.model import default_model

    model = default_model()
    q = lib.Handle(model, N=2, max_batch=2)
    ends = q.eepos(np.array([np.full(6, 0.3), np.full(6, 0.9)]))
    sim_dt, res = 0.01, []
    for shape in a.shapes.split(","):
        G, H, N = (int(v) for v in shape.split("x"))
        xs, fh, fact, noise = case(G, H, a.steps, 11, q.eepos, ends)
        h = lib.Handle(model, N=N, max_batch=G * H, qp_mode=lib.QP_ADMM)
        kw = dict(noise=noise, sim_dt=sim_dt, keep_best=True, decay=0.97)
        h.mpc_run_sampled(xs, ends, 2, fh, fact, noise=noise[:2], sim_dt=sim_dt, keep_best=True, decay=0.97)  # warm-up
        t0 = time.perf_counter()
        r = h.mpc_run_sampled(xs, ends, a.steps, fh, fact, **kw)
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        h.mpc_run_sampled(xs, ends, 0, fh, fact, sim_dt=sim_dt)  # allocation, copies, the initial solve alone
        t_dev0 = time.perf_counter() - t0
        h.close()
        host_loop(lib, model, G, H, N, 2, xs, ends, fh, fact, noise, sim_dt)  # warm-up
        t_host, bests = host_loop(lib, model, G, H, N, a.steps, xs, ends, fh, fact, noise, sim_dt)
        ran = r["best"] >= 0
        res.append({
            "G": G, "H": H, "N": N, "steps": a.steps, "qp_mode": "admm", "reset": "all", "resample": "keep_best, 0.97",
            "device": {"ms_per_step": 1e3 * t_dev / a.steps, "instance_steps_per_s": G * H * a.steps / t_dev,
                       "ms_per_step_without_setup": 1e3 * (t_dev - t_dev0) / a.steps,
                       "note": "whole call: allocation, copies in and out, the initial solve and steps; "
                               "without_setup subtracts a call of 0 steps"},
            "host": {"ms_per_step": 1e3 * t_host / a.steps, "instance_steps_per_s": G * H * a.steps / t_host,
                     "note": "steps only (the initial solve is outside the timed region)"},
            "same_best_fraction": float((r["best"][ran] == bests[ran]).mean()),
            "groups_that_met_a_goal": int((~ran).any(axis=0).sum() + (r["dist"] < 0.095).any(axis=0).sum()),
        })
        print(json.dumps(res[-1]), flush=True)
    out = {"tool": "tools/sampled_loop_timing.py", "version": lib.version(), "results": res}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
