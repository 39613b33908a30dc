#!/usr/bin/env python3
"""GPU: the per-step time of the multi-rate sampled-wrench loop (i7m_mpc_run_sampled_multirate,
k_sampled_multirate_step between two solves) against i7m_mpc_run_sampled (k_sampled_step) in the same
session on the same handle, ADMM mode, at sim_dt = dt: there both loops take one plant step and
solve the same QPs, so the per-step times should be equal within the old entry point's own spread.
sim_dt = 0.02 (two sub-steps per step, which the old loop refuses) is reported beside it, without a
bound.

Per shape `--reps` alternating repetitions; a repetition times a call of warm + steps MPC steps and
a call of warm steps and reports their difference / steps, so allocation, copies and the initial
solve cancel.  The goal is one distant endpoint, so no group switches or stops within the timed
steps (the record counts the groups that did).

Prints and writes (--out) one JSON object.  One process; run it under `timeout`.  Not a test, and
no ratio is asserted: it reports.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def per_step(run, warm, steps):
    """ms per MPC step of run(num_steps): (a call of warm + steps) - (a call of warm), over steps."""
    t = []
    for n in (warm + steps, warm):
        t0 = time.perf_counter()
        run(n)
        t.append(time.perf_counter() - t0)
    return 1e3 * (t[0] - t[1]) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="256x16x32,1x16x64", help="GxHxN, comma separated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_multirate_loop_timing.json"))
    a = ap.parse_args()
    from indy7_mpc_amd import _lib as lib
    from indy7_mpc_amd.model import default_model

    model = default_model()
    q = lib.Handle(model, N=2, max_batch=1)
    ends = q.eepos(np.full((1, 6), 0.9))
    res = []
    for shape in a.shapes.split(","):
        G, H, N = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(11)
        xs = np.concatenate([rng.uniform(-0.3, 0.3, (G, 6)), rng.uniform(-0.2, 0.2, (G, 6))], axis=1)
        fhyp = np.zeros((G, H, 6))
        fhyp[:, :, :3] = rng.normal(0, 5.0, (G, H, 3))
        fhyp[:, 0] = 0.0
        fact = fhyp[:, 1 % H].copy()
        fhyp = fhyp.reshape(G * H, 6)
        h = lib.Handle(model, N=N, max_batch=G * H, qp_mode=lib.QP_ADMM)
        dt = h.cfg.dt
        runs = {
            "sampled": lambda n: h.mpc_run_sampled(xs, ends, n, fhyp, fact, sim_dt=dt),
            "sampled_multirate": lambda n: h.mpc_run_sampled_multirate(xs, ends, n, fhyp, fact, sim_dt=dt),
            "sampled_multirate_0.02": lambda n: h.mpc_run_sampled_multirate(xs, ends, n, fhyp, fact, sim_dt=0.02),
        }
        for run in runs.values():
            run(2)  # first-use costs out of the way
        ms = {k: [] for k in runs}
        for _ in range(a.reps):  # alternating
            for k, run in runs.items():
                ms[k].append(per_step(run, a.warm, a.steps))
        old = runs["sampled"](a.warm + a.steps)
        new = runs["sampled_multirate"](a.warm + a.steps)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
        diff = med["sampled_multirate"] - med["sampled"]
        res.append({
            "G": G, "H": H, "N": N, "qp_mode": "admm", "steps": a.steps, "warm": a.warm,
            "ms_per_step": ms, "median_ms_per_step": med, "spread_ms": spread,
            "multirate_minus_sampled_ms_at_dt": diff,
            "within_the_old_loops_spread": bool(abs(diff) <= spread["sampled"]),
            "same_winners_at_dt": bool(np.array_equal(old["best"], new["best"])),
            "max_abs_q_difference_at_dt": float(np.nanmax(np.abs(old["q"] - new["q"]))),
            "groups_that_met_the_goal": int((~np.isfinite(new["dist"])).any(axis=0).sum() + (new["dist"] < 0.095).any(axis=0).sum()),
            "note": "sampled: i7m_mpc_run_sampled; sampled_multirate: i7m_mpc_run_sampled_multirate at sim_dt = dt "
                    "(one sub-step per step); sampled_multirate_0.02: two sub-steps per step, no bound; reset ALL "
                    "before every solve in all three",
        })
        print(json.dumps(res[-1]), flush=True)
        h.close()
    out = {"tool": "tools/sampled_multirate_loop_timing.py", "version": lib.version(), "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
